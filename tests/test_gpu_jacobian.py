"""The emulator Jacobian and Fisher matrix on the HIP path: ``posterior.mean_jacobian`` (mfgp_*_jacobian),
``posterior.fisher`` and the batched Fisher kernel ``mfgp_mvn_fisher``.

References: tests/_jacobian_oracle.py on the CPU (autograd through the Cholesky form of predict_f, the per-row
diagonal), which tests/test_jacobian_host.py holds against the solve form and the numpy closed form to a tenth of
the bounds used here.  Bounds (tests/_input_grad_oracle's): |J - ref|max <= 1e-9 max(1, |ref|max), Goku
1e-8 |ref|max; Fisher 1e-9 max(1, |F|max) with obs_cov from _sample_oracle.spd at cond 1e3.  mean / var of the
calls carry predict_f's bits; two calls with the same inputs return the same bits."""
import numpy as np
import pytest
import torch

import _input_grad_oracle as G
import _jacobian_oracle as JO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import CholeskyError, PrecomputeCacheType
from multi_fidelity_gpflow_amd.engine import Engine
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64), device="cuda")


def _err(name, got, ref, goku=False):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    lim = JO.bound(ref, goku)
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{name}: err {err:.1e} (|ref|max {np.abs(ref).max() if ref.size else 0.0:.1e}, bound {lim:.1e})")
    assert err <= lim, (name, err)
    return err


def _np3(r):
    return r[0].numpy(), r[1].numpy(), r[2].numpy()


def _jac_checked(name, post, case, goku=False):
    """One mean_jacobian call: J within the bound, mean / var equal to predict_f's bits, a second call bitwise equal,
    and J contracted with an upstream gradient equal to predict_f_vjp's gX within the bound."""
    Xs = case["Xs"]
    mean, var, J = _np3(post.mean_jacobian(Xs))
    _err(name, J, case["chol"], goku)
    pm, pv = post.predict_f(Xs)
    np.testing.assert_array_equal(mean, pm.numpy())
    np.testing.assert_array_equal(var, pv.numpy())
    for a, b in zip(_np3(post.mean_jacobian(Xs)), (mean, var, J)):
        np.testing.assert_array_equal(a, b)
    gm = G.upstream(Xs.shape[0], mean.shape[1], 31)[0]
    gX = post.predict_f_vjp(Xs, gm, None)[2].numpy()
    _err(f"{name} vs predict_f_vjp", np.einsum("scd,sc->sd", J, gm), gX[:, :-1], goku)
    return mean, var, J


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("case", JO.GPR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpr_jacobian_synthetic(case, nb, eng):
    """(n_lf, n_hf, P, D, N*) = (20, 5, 1, 1, 1): one tile, D = P = N* = 1; (70, 9, 3, 3, 33): three row tiles at
    NB = 32 (chunks of one tile, partials summed by the last workgroup), a one-row tail in a second column tile;
    (150, 30, 65, 32, 70): P across a 64-tile, D at the limit (two dimension groups at NB = 32, eight at 64),
    more than 128 rows.  References three ways on the CPU: 1.3e-15, 3.0e-13, 1.0e-14.
    Measured on an MI355X (NB = 32 / 64): 5.3e-15 / 1.8e-15, 2.9e-13 / 3.1e-13, 1.0e-14 / 1.0e-14 (bounds 2.5e-9,
    7.2e-9, 1.8e-9); against predict_f_vjp <= 3.1e-13 (bound 1.1e-8)."""
    c = JO.gpr_synthetic(*case)
    eng.set_tile(nb)
    try:
        post = _model(c["X"], c["Y"], c["prm"]).posterior()
        _jac_checked(f"gpr {case} nb{nb}", post, c)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("which,nb", [("hbs", 32), ("hbs", 64), ("goku", 32)])
def test_gpr_jacobian_datasets(which, nb, eng):
    """HBS (n = 53, P = 49, the 33-row mixed-fidelity Xnew) at both tiles and Goku (n = 1164, P = 64, D = 10, its
    36 test rows; 37 row tiles in chunks) at NB = 32 with the Goku bound 1e-8 |ref|max.  References three ways on
    the CPU: HBS 1.9e-14, Goku 3.1e-12.  Measured on an MI355X: HBS 3.2e-14 (NB = 32) / 1.4e-14 (64), bound 2.2e-9;
    Goku 1.3e-12, bound 3.0e-8 (against predict_f_vjp 3.2e-12, bound 2.6e-7)."""
    c = JO.gpr_dataset(which)
    eng.set_tile(nb)
    try:
        post = _model(c["X"], c["Y"], c["prm"]).posterior()
        _jac_checked(f"{which} nb{nb}", post, c, goku=which == "goku")
    finally:
        eng.set_tile(32)


def test_gpr_jacobian_edge_rows(eng):
    """A training row and an Xnew row with fidelity 0.9999999999999999 (neither 0 nor 1): that Xnew row's Jacobian
    is exactly 0 and the training row contributes nothing (moving it leaves every bit in place); Xnew rows equal
    to training rows (all differences 0 against them) stay within the bound.
    Measured on an MI355X: 3.6e-13 (bound 6.9e-9); the masked rows exactly 0."""
    c = JO.gpr_edge_rows()
    post = _model(c["X"], c["Y"], c["prm"]).posterior()
    mean, var, J = _jac_checked("edge rows", post, c)
    assert np.all(J[5] == 0.0) and np.all(c["chol"][5] == 0.0)
    X2 = c["X"].copy()
    X2[40, :-1] += 0.25
    again = _np3(_model(X2, c["Y"], c["prm"]).posterior().mean_jacobian(c["Xs"]))
    np.testing.assert_array_equal(again[2], J)


def test_jacobian_shapes_views_and_empty_calls(eng):
    """jac is the [N*, P, D] view of the device layout [N*, D, P]; N* = 0 returns empty tensors; a device Xnew."""
    c = JO.gpr_synthetic(*JO.GPR_CASES[1])
    post = _model(c["X"], c["Y"], c["prm"]).posterior()
    mean, var, J = post.mean_jacobian(torch.as_tensor(c["Xs"], device="cuda"))
    ns, p, d = c["chol"].shape
    assert tuple(J.shape) == (ns, p, d) and J.stride() == (d * p, 1, p)
    assert tuple(mean.shape) == (ns, p) and tuple(var.shape) == (ns, p)
    _err("device Xnew", J.numpy(), c["chol"])
    e = post.mean_jacobian(c["Xs"][:0])
    assert tuple(e[0].shape) == (0, p) and tuple(e[1].shape) == (0, p) and tuple(e[2].shape) == (0, p, d)
    f = post.fisher(c["Xs"][:0], obs_var=0.1)
    assert tuple(f.fisher.shape) == (0, d, d) and tuple(f.jacobian.shape) == (0, p, d) and tuple(f.var.shape) == (0, p)


@pytest.mark.parametrize("nb", [32, 64])
def test_svgp_jacobian_eleven_latents(nb, eng):
    """The synthetic latent model with L = 11 latents (mixed in latent order), M = 70 (three row tiles at NB = 32),
    P = 17, D = 5, N* = 33.  References three ways on the CPU: 8.8e-14.
    Measured on an MI355X (NB = 32 / 64): 8.3e-14 / 8.0e-14 (bound 1e-9)."""
    c = JO.svgp_synthetic()
    eng.set_tile(nb)
    try:
        m, Xs2 = G.svgp_synthetic_model()
        np.testing.assert_array_equal(Xs2, c["Xs"])
        _jac_checked(f"svgp L=11 nb{nb}", m.posterior(), c)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_jacobian_hbs(which, eng):
    """The HBS single-bin model (M = 50, L = P = 49, no W: J[s, l, k] = dg_l[s, k]) and the HBS latent model
    (5 latents, M = 30, with W), Xnew of 8 + 33 rows; then q_mu changed: the snapshot's until update_cache(),
    the new parameters' after it (the weights are dropped with the block).  References three ways on the CPU:
    2.7e-13 (single bin), 6.3e-15 (latent).  Measured on an MI355X: single bin 4.6e-13 (bound 2.0e-9), after
    update_cache 5.3e-13; latent 1.7e-14 (bound 1e-9), 1.6e-14."""
    c = JO.svgp_hbs(which)
    m, Wm, Xs = G.svgp_hbs_model(which)
    post = m.posterior()
    assert isinstance(post, M.SVGPPosterior)
    got = _jac_checked(f"svgp hbs {which}", post, c)
    one = _np3(post.mean_jacobian(Xs[:1]))
    _err(f"svgp hbs {which} one row", one[2], c["chol"][:1])
    m.q_mu.assign(m.q_mu.numpy() + 0.25)
    np.testing.assert_array_equal(_np3(post.mean_jacobian(Xs))[2], got[2])
    post.update_cache()
    upd = _np3(post.mean_jacobian(Xs))
    assert np.abs(upd[2] - got[2]).max() > 1e-3
    _err(f"svgp hbs {which} after update_cache", upd[2], JO.svgp_refs(G.svgp_state(m, Wm), Xs)["chol"])


# ---------------------------------------------------------------- the Fisher kernel
def _padded_cov(Cm):
    """obs_cov on the device with ldc = P + 3 and a NaN upper triangle: only the lower one may be read."""
    p = Cm.shape[0]
    buf = torch.full((p, p + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :p] = _dev(np.where(np.tril(np.ones((p, p), dtype=bool)), Cm, np.nan))
    return buf[:, :p]


def _fisher_case(ns, p, d, seed, var_cols=True, obs_var="row"):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((ns, p, d))
    var = rng.uniform(0.05, 0.5, (ns, p) if var_cols else (ns,))
    ov = None if obs_var is None else rng.uniform(0.05, 0.5, (ns, p) if obs_var == "row" else (p,))
    return J, var, ov


def _fisher_call(eng, J, var, ov, oc):
    Jd = _dev(J).transpose(1, 2).contiguous()   # the device layout [ns, D, P]
    F, info = eng.mvn_fisher(Jd, _dev(var), _dev(ov), None if oc is None else _padded_cov(oc))
    return F.cpu().numpy(), info.cpu().numpy()


def _fisher_checked(name, eng, J, var, ov, oc):
    F, info = _fisher_call(eng, J, var, ov, oc)
    assert np.all(info == 0), name
    vfull = var if var.ndim == 2 else np.repeat(var[:, None], J.shape[1], axis=1)
    ref = JO.fisher(J, vfull, ov, oc)
    lim = JO.BOUND * max(1.0, np.abs(ref).max())
    err = np.abs(F - ref).max()
    print(f"{name}: err {err:.1e} (|F|max {np.abs(ref).max():.1e}, bound {lim:.1e})")
    assert err <= lim, (name, err)
    np.testing.assert_array_equal(F, F.transpose(0, 2, 1))   # bitwise symmetric
    return F


DENSE = [(p, d) for p in (1, 3, 17, 64, 65) for d in (1, 10, 32)] + [(128, 15)]


@pytest.mark.parametrize("p,d", DENSE, ids=lambda v: str(v))
def test_fisher_dense_against_oracle(p, d, eng):
    """P below, at and above an 8-column block with D = 1, 10 and the limit 32 (every pair fits: P8 + D <= 104),
    and P = 128 at the largest D that fits (15: the image takes 159.8 of the 160 KiB).  obs_cov with cond 1e3,
    ldc = P + 3, NaN upper triangle; var per output and one per row, obs_var per row, shared and absent.  A row's
    bits are unchanged when the call is repeated on a subset of the rows.
    Measured on an MI355X: <= 4.5e-13 (at P = 128, |F|max 5.5e2, bound 5.5e-7); every F bitwise symmetric."""
    ns = 3
    oc = JO.obs_cov(p, 50 + p)
    for k, (var_cols, obs_var) in enumerate([(True, "row"), (False, "shared"), (True, None)]):
        J, var, ov = _fisher_case(ns, p, d, 1000 * p + 10 * d + k, var_cols, obs_var)
        F = _fisher_checked(f"dense P={p} D={d} form {k}", eng, J, var, ov, oc)
        sub = [2, 0]
        Fs, info = _fisher_call(eng, J[sub], var[sub], ov[sub] if obs_var == "row" else ov, oc)
        np.testing.assert_array_equal(Fs, F[sub])


def test_fisher_dense_is_refused_beyond_the_limit(eng):
    """The first (P, D) beyond the limit, P = 128 with D = 16: ValueError in Python and MFGP_ERR_ARG from the C
    entry, both before any device work (the outputs keep their fill); the diagonal form runs there."""
    ns, p, d = 2, 128, 16
    f64 = dict(dtype=torch.float64, device="cuda")
    J, var, Cm = torch.ones((ns, d, p), **f64), torch.ones((ns, p), **f64), torch.eye(p, **f64)
    with pytest.raises(ValueError, match=r"P8 \+ D <= 143"):
        eng.mvn_fisher(J, var, obs_cov=Cm)
    F = torch.full((ns, d, d), 7.0, **f64)
    info = torch.full((ns,), 7, dtype=torch.int32, device="cuda")
    ws = eng.workspace("mvn_fisher", 256)
    rc = eng.lib.mfgp_mvn_fisher(eng.h, ns, p, d, J.data_ptr(), p, var.data_ptr(), p, 1, None, 0, Cm.data_ptr(), p,
                                 ws.data_ptr(), ws.numel(), F.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and np.all(F.cpu().numpy() == 7.0) and np.all(info.cpu().numpy() == 7)
    out, inf = eng.mvn_fisher(J, var)
    assert np.all(inf.cpu().numpy() == 0)
    np.testing.assert_allclose(out.cpu().numpy(), np.full((ns, d, d), float(p)), rtol=1e-13)


@pytest.mark.parametrize("p,d", [(200, 32), (64, 10), (1, 1)])
def test_fisher_diagonal_form(p, d, eng):
    """No obs_cov, any P (200: four 64-output blocks with a tail; D = 32: 528 pairs, three a thread); var per
    output and one per row, obs_var per row / shared / absent; row subsets keep their bits.
    Measured on an MI355X: <= 4.5e-13 (P = 200, |F|max 1.5e3, bound 1.5e-6)."""
    ns = 5
    for k, (var_cols, obs_var) in enumerate([(True, "row"), (False, "shared"), (True, None)]):
        J, var, ov = _fisher_case(ns, p, d, 77 * p + d + k, var_cols, obs_var)
        F = _fisher_checked(f"diag P={p} D={d} form {k}", eng, J, var, ov, None)
        Fs, _ = _fisher_call(eng, J[3:4], var[3:4], ov[3:4] if obs_var == "row" else ov, None)
        np.testing.assert_array_equal(Fs, F[3:4])


def test_fisher_info_names_the_bad_output(eng):
    """A non-positive total variance (diagonal) / pivot (dense) at output 5 of row 1: info[1] = 6, row 0 untouched."""
    ns, p, d = 2, 9, 3
    J, var, _ = _fisher_case(ns, p, d, 3, True, None)
    var[1, 5] = -1.0
    F, info = _fisher_call(eng, J, var, None, None)
    assert list(info) == [0, 6]
    F0, _ = _fisher_call(eng, J[:1], var[:1], None, None)
    np.testing.assert_array_equal(F0, F[:1])
    Fd, info = _fisher_call(eng, J, var, None, 1e-3 * np.eye(p))
    assert list(info) == [0, 6]


# ---------------------------------------------------------------- posterior.fisher
def _fisher_post(name, post, case, ov, oc):
    res = post.fisher(case["Xs"], obs_cov=None if oc is None else _padded_cov(oc), obs_var=ov)
    assert isinstance(res, M.FisherResult)
    ref = JO.fisher(case["chol"], case["var"], ov, oc)
    lim = JO.BOUND * max(1.0, np.abs(ref).max())
    F = res.fisher.numpy()
    err = np.abs(F - ref).max()
    print(f"{name}: err {err:.1e} (|F|max {np.abs(ref).max():.1e}, bound {lim:.1e})")
    assert err <= lim, (name, err)
    np.testing.assert_array_equal(F, F.transpose(0, 2, 1))
    mean, var, J = _np3(post.mean_jacobian(case["Xs"]))
    np.testing.assert_array_equal(res.mean.numpy(), mean)
    np.testing.assert_array_equal(res.var.numpy(), var)
    np.testing.assert_array_equal(res.jacobian.numpy(), J)
    return res


def test_fisher_gpr_posterior(eng):
    """HBS on the GPR posterior (one variance per row; P = 49, D = 5): dense obs_cov alone, with a shared and a
    per-row obs_var, and the diagonal form; a row subset keeps its bits.
    Measured on an MI355X: dense 2.2e-10 (|F|max 8.9e2, bound 8.9e-7); with obs_var <= 3.0e-12 (bound 1.3e-7);
    diagonal 3.2e-12 (bound 1.5e-7)."""
    c = JO.gpr_dataset("hbs")
    post = _model(c["X"], c["Y"], c["prm"]).posterior()
    ns, p, d = c["chol"].shape
    oc = JO.obs_cov(p, 7)
    rng = np.random.default_rng(8)
    full = _fisher_post("hbs dense", post, c, None, oc)
    _fisher_post("hbs dense + shared obs_var", post, c, rng.uniform(0.05, 0.5, p), oc)
    _fisher_post("hbs dense + per-row obs_var", post, c, rng.uniform(0.05, 0.5, (ns, p)), oc)
    _fisher_post("hbs dense + scalar obs_var", post, c, 0.25, oc)
    _fisher_post("hbs diagonal", post, c, rng.uniform(0.05, 0.5, p), None)
    sub = post.fisher(c["Xs"][4:9], obs_cov=_dev(oc))
    np.testing.assert_array_equal(sub.fisher.numpy(), full.fisher.numpy()[4:9])


def test_fisher_goku(eng):
    """Goku (P = 64, D = 10, dense obs_cov at cond 1e3; |F|max 3.1e4).  Measured on an MI355X: 1.3e-7 (bound 3.1e-5)."""
    c = JO.gpr_dataset("goku")
    post = _model(c["X"], c["Y"], c["prm"]).posterior()
    _fisher_post("goku dense", post, c, None, JO.obs_cov(64, 7))


def test_fisher_svgp_posterior(eng):
    """The synthetic latent model (a variance per output; P = 17, D = 5): dense with per-row obs_var, diagonal.
    Measured on an MI355X: 4.0e-13 (bound 2.7e-9), 3.2e-13 (bound 2.9e-9)."""
    c = JO.svgp_synthetic()
    m, _ = G.svgp_synthetic_model()
    post = m.posterior()
    ns, p, d = c["chol"].shape
    rng = np.random.default_rng(9)
    _fisher_post("svgp dense", post, c, rng.uniform(0.05, 0.5, (ns, p)), JO.obs_cov(p, 11))
    _fisher_post("svgp diagonal", post, c, rng.uniform(0.05, 0.5, p), None)


def test_fisher_nan_row_raises_and_names_it(eng):
    """A NaN input row: CholeskyError naming that row (the call's one host read is info); without it the call succeeds."""
    c = JO.gpr_synthetic(*JO.GPR_CASES[1])
    post = _model(c["X"], c["Y"], c["prm"]).posterior()
    p = c["chol"].shape[1]
    Xs = c["Xs"][:6].copy()
    Xs[4, 0] = np.nan
    for kw in (dict(obs_cov=JO.obs_cov(p, 3)), dict(obs_var=0.1)):
        with pytest.raises(CholeskyError, match="fisher: row 4"):
            post.fisher(Xs, **kw)
        ok = post.fisher(np.delete(Xs, 4, axis=0), **kw)
        assert np.all(np.isfinite(ok.fisher.numpy()))


# ---------------------------------------------------------------- the weights' life cycle
@pytest.mark.parametrize("cache", [PrecomputeCacheType.TENSOR, PrecomputeCacheType.VARIABLE])
def test_weights_follow_update_cache(cache, eng):
    """alpha is kept beside the cache block and dropped by update_cache(): after the model's parameters change,
    mean_jacobian is the snapshot's until update_cache() and the new parameters' after it -- also for a VARIABLE
    cache, which is rewritten in place (the same device block).
    Measured on an MI355X, both cache types: 2.9e-13 before (bound 7.2e-9), 2.6e-13 after (bound 7.4e-9)."""
    c = JO.gpr_synthetic(*JO.GPR_CASES[1])
    X, Y, Xs, prm = c["X"], c["Y"], c["Xs"], c["prm"]
    m = _model(X, Y, prm)
    post = m.posterior(precompute_cache=cache)
    before = _np3(post.mean_jacobian(Xs))
    _err(f"{cache.value} before", before[2], c["chol"])
    block = post.cache.data_ptr()
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.kernel.kernel_L.lengthscales.assign(0.8 * np.asarray(prm.lL))
    for a, b in zip(_np3(post.mean_jacobian(Xs)), before):
        np.testing.assert_array_equal(a, b)
    new = prm.copy()
    new.rho, new.lL = np.full((Y.shape[1], 1), 1.234), 0.8 * np.asarray(prm.lL)
    post.update_cache()
    if cache is PrecomputeCacheType.VARIABLE:
        assert post.cache.data_ptr() == block
    upd = _np3(post.mean_jacobian(Xs))
    assert np.abs(upd[2] - before[2]).max() > 1e-3
    _err(f"{cache.value} after update_cache", upd[2], JO._gpr_refs(X, Y, Xs, new)["chol"])


def test_weights_of_a_conditioned_posterior(eng):
    """A condition_on result starts without weights and builds its own: mean_jacobian matches the oracle of the
    stacked data; the parent's weights and results are untouched.  Measured on an MI355X: 4.7e-13 (bound 5.8e-9)."""
    c = JO.gpr_synthetic(*JO.GPR_CASES[1])
    X, Y, Xs, prm = c["X"], c["Y"], c["Xs"], c["prm"]
    post = _model(X, Y, prm).posterior()
    before = _np3(post.mean_jacobian(Xs))
    rng = np.random.default_rng(12)
    Xadd = np.hstack([rng.random((5, X.shape[1] - 1)), (np.arange(5) % 2)[:, None].astype(float)])
    Yadd = rng.standard_normal((5, Y.shape[1]))
    cond = post.condition_on(Xadd, Yadd)
    assert getattr(cond, "_jac_weights", None) is None
    got = _np3(cond.mean_jacobian(Xs))
    _err("conditioned", got[2], JO._gpr_refs(np.vstack([X, Xadd]), np.vstack([Y, Yadd]), Xs, prm)["chol"])
    assert np.abs(got[2] - before[2]).max() > 1e-6
    for a, b in zip(_np3(post.mean_jacobian(Xs)), before):
        np.testing.assert_array_equal(a, b)
