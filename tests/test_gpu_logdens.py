"""The emulator log-likelihood on the HIP path: ``mfgp_mvn_logpdf`` (the batched density kernel), the fused
``posterior.log_density`` and ``predict_log_density``.

References: tests/_logdens_oracle.py on the CPU, which tests/test_logdens_host.py holds against scipy and torch
autograd to a tenth of the bound used here, 1e-9 max(1, |ref|max) for logp, gmean and gvar each: the forward
bound tests/test_gpu_sample.py derives for a backward-stable Cholesky at n <= 128 and cond <= 1e3.  The
kernel's sum of gvar over the outputs (one variance per row) is P numbers within that bound each: P times it.
grad_X is bitwise predict_f_vjp fed the density's own gradients, and against the CPU VJP fed the oracle's
gradients it is within the VJP's bound plus the density's: the VJP is linear in its upstream, so an upstream
within 1e-9 of its scale moves grad_X by 1e-9 of grad_X's scale."""
import numpy as np
import pytest
import torch

import _input_grad_oracle as G
import _logdens_oracle as LD
import multi_fidelity_gpflow_amd as M
from _sample_oracle import spd
from multi_fidelity_gpflow_amd import CholeskyError, PrecomputeCacheType
from multi_fidelity_gpflow_amd.engine import Engine
from test_gpu_graph import _data as _graph_data, _model as _graph_model, _oracle_params as _graph_params
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


def _padded_cov(Cm):
    """obs_cov on the device with ldc = P + 3 and a NaN upper triangle: only the lower one may be read."""
    p = Cm.shape[0]
    buf = torch.full((p, p + 3), float("nan"), dtype=torch.float64, device="cuda")
    lo = np.where(np.tril(np.ones((p, p), dtype=bool)), Cm, np.nan)
    buf[:, :p] = _dev(lo)
    return buf[:, :p]


def _close(name, got, ref, bound=LD.BOUND, scale=1.0):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, name
    lim = scale * bound * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"{name}: err {err:.1e} (|ref|max {np.abs(ref).max():.1e}, bound {lim:.1e})")
    assert err <= lim, (name, err)


def _call(eng, mean, Y, var, ov, Cm, **kw):
    logp, gm, gv, info = eng.mvn_logpdf(_dev(mean), _dev(Y), _dev(var), _dev(ov), None if Cm is None else _padded_cov(Cm),
                                        **kw)
    c = lambda t: None if t is None else t.cpu().numpy()
    return c(logp), c(gm), c(gv), c(info)


# (per-row Y, var per output, obs_var): shared and per-row Y, var_cs 0 and 1, obs_var absent / shared / per row
FORMS = [(True, True, "row"), (False, False, None), (True, False, "shared"), (False, True, None)]


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("p", [1, 2, 31, 32, 33, 64, 65, 128])
def test_dense_kernel_against_oracle(p, ns, eng):
    """P below, at and above each 8-column block / LDS size step and at the cap; obs_cov with cond <= 1e3,
    ldc = P + 3, NaN upper triangle."""
    for k, (per_row_y, var_cols, obs_var) in enumerate(FORMS):
        mean, Y, var, ov, Cm = LD.case(ns, p, 1000 * p + 10 * ns + k, per_row_y=per_row_y, var_cols=var_cols,
                                       obs_var=obs_var)
        assert np.linalg.cond(Cm) <= 1e3 * (1 + 1e-9)
        ref = LD.logpdf(mean, Y, var, ov, Cm)
        logp, gm, gv, info = _call(eng, mean, Y, var, ov, Cm, grad=True)
        tag = f"P={p} ns={ns} form {k}"
        assert np.all(info == 0), tag
        _close(f"{tag} logp", logp, ref[0])
        _close(f"{tag} gmean", gm, ref[1])
        _close(f"{tag} gvar", gv, ref[2])
        val, none_m, none_v, info = _call(eng, mean, Y, var, ov, Cm)   # the value alone: the same bits, no inverse
        assert none_m is None and none_v is None and np.all(info == 0)
        np.testing.assert_array_equal(val, logp)
        if not var_cols:   # one variance per row: the kernel's own sum over the outputs
            _, gm2, gvs, _ = _call(eng, mean, Y, var, ov, Cm, grad=True, sum_gvar=True)
            np.testing.assert_array_equal(gm2, gm)
            assert gvs.shape == (ns,)
            _close(f"{tag} summed gvar", gvs, ref[2].sum(axis=1), scale=p)


@pytest.mark.parametrize("p", [1, 63, 64, 65, 300])
def test_diagonal_kernel_with_missing_targets(p, eng):
    """No obs_cov, any P: NaN targets in 15 % of the entries and one all-NaN row (logp exactly 0, gradients
    exactly 0); var per output and one per row, obs_var per row and shared."""
    ns = 6
    rng = np.random.default_rng(40 + p)
    for k, (per_row_y, var_cols, obs_var) in enumerate(FORMS[:3]):
        mean, Y = rng.standard_normal((ns, p)), rng.standard_normal((ns, p))
        var = rng.uniform(0.05, 0.5, (ns, p) if var_cols else (ns,))
        ov = None if obs_var is None else rng.uniform(0.05, 0.5, (ns, p) if obs_var == "row" else (p,))
        Y[rng.random((ns, p)) < 0.15] = np.nan
        Y[3] = np.nan
        ref = LD.logpdf(mean, Y, var, ov, None)
        logp, gm, gv, info = _call(eng, mean, Y, var, ov, None, grad=True)
        tag = f"diag P={p} form {k}"
        assert np.all(info == 0), tag
        _close(f"{tag} logp", logp, ref[0])
        _close(f"{tag} gmean", gm, ref[1])
        _close(f"{tag} gvar", gv, ref[2])
        assert logp[3] == 0.0 and np.all(gm[3] == 0.0) and np.all(gv[3] == 0.0)
        assert np.all(gm[np.isnan(Y)] == 0.0) and np.all(gv[np.isnan(Y)] == 0.0)
        if not var_cols:
            _, _, gvs, _ = _call(eng, mean, Y, var, ov, None, grad=True, sum_gvar=True)
            _close(f"{tag} summed gvar", gvs, ref[2].sum(axis=1), scale=p)


def test_dense_form_is_refused_beyond_128_outputs(eng):
    """P = 129 with obs_cov: ValueError in Python and MFGP_ERR_ARG from the C entry, both before any device
    work (the outputs keep their fill); without obs_cov the same P runs."""
    ns, p = 2, 129
    f64 = dict(dtype=torch.float64, device="cuda")
    mean, Y, var, Cm = torch.zeros((ns, p), **f64), torch.zeros(p, **f64), torch.ones((ns, p), **f64), torch.eye(p, **f64)
    with pytest.raises(ValueError, match="P <= 128"):
        eng.mvn_logpdf(mean, Y, var, obs_cov=Cm)
    logp = torch.full((ns,), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((ns,), 7, dtype=torch.int32, device="cuda")
    ws = eng.workspace("mvn_logpdf", 256)
    rc = eng.lib.mfgp_mvn_logpdf(eng.h, ns, p, mean.data_ptr(), p, Y.data_ptr(), 0, var.data_ptr(), p, 1, None, 0,
                                 Cm.data_ptr(), p, ws.data_ptr(), ws.numel(), logp.data_ptr(), None, p, None, p,
                                 info.data_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and np.all(logp.cpu().numpy() == 7.0) and np.all(info.cpu().numpy() == 7)
    out, _, _, inf = eng.mvn_logpdf(mean, Y, var)
    _close("P=129 diagonal", out.cpu().numpy(), LD.logpdf(np.zeros((ns, p)), np.zeros(p), np.ones((ns, p)))[0])
    assert np.all(inf.cpu().numpy() == 0)


@pytest.mark.parametrize("p", [33, 64])
def test_info_names_the_pivot_of_the_bad_row_only(p, eng):
    """A row whose covariance is indefinite (a negative variance at output k: the leading k x k block is still
    positive definite, so pivot k + 1 is the first to fail) and a row whose mean is NaN (its first residual,
    output 1) report in info; every other row keeps its bits.  An indefinite obs_cov fails every row at the
    same pivot.  The diagonal form reports the first non-positive total variance the same way."""
    ns, k = 5, p - 7
    mean, Y, var, ov, Cm = LD.case(ns, p, 77 + p)
    good = _call(eng, mean, Y, var, ov, Cm, grad=True)
    assert np.all(good[3] == 0)
    var2, mean2 = var.copy(), mean.copy()
    var2[1, k] = -50.0
    mean2[3] = np.nan
    bad = _call(eng, mean2, Y, var2, ov, Cm, grad=True)
    assert list(bad[3]) == [0, k + 1, 0, 1, 0]
    for s in (0, 2, 4):
        for a, b in zip(good[:3], bad[:3]):
            np.testing.assert_array_equal(a[s], b[s])
    C2 = Cm.copy()
    C2[k, k] = -50.0
    assert list(_call(eng, mean, Y, var, ov, C2, grad=True)[3]) == [k + 1] * ns
    dgood = _call(eng, mean, Y, var, ov, None, grad=True)
    dbad = _call(eng, mean2, Y, var2, ov, None, grad=True)
    assert list(dgood[3]) == [0] * ns and list(dbad[3]) == [0, k + 1, 0, 1, 0]
    for s in (0, 2, 4):
        for a, b in zip(dgood[:3], dbad[:3]):
            np.testing.assert_array_equal(a[s], b[s])


@pytest.mark.parametrize("dense", [True, False])
def test_row_bits_do_not_depend_on_the_batch(dense, eng):
    """A row evaluated alone equals its bits inside a batch of 9 (three workgroups of the diagonal form, nine
    of the dense one), and a repeated call is bitwise equal."""
    ns, p = 9, 65
    mean, Y, var, ov, Cm = LD.case(ns, p, 5150)
    Cm = Cm if dense else None
    full = _call(eng, mean, Y, var, ov, Cm, grad=True)
    again = _call(eng, mean, Y, var, ov, Cm, grad=True)
    for a, b in zip(full, again):
        np.testing.assert_array_equal(a, b)
    for s in (0, 4, 8):
        one = _call(eng, mean[s:s + 1], Y[s:s + 1], var[s:s + 1], ov[s:s + 1], Cm, grad=True)
        for a, b in zip(one[:3], full[:3]):
            np.testing.assert_array_equal(a[0], b[s])


# ---------------------------------------------------------------- posterior level
def _observation(mean_ref, seed, shared):
    """Y near the CPU mean (one vector for every row, or one per row), obs_cov with cond 1e3 and a shared
    diagonal obs_var."""
    ns, p = mean_ref.shape
    rng = np.random.default_rng(seed)
    Y = (mean_ref[0] if shared else mean_ref) + 0.3 * rng.standard_normal((p,) if shared else (ns, p))
    Cm = 0.2 * spd(p, 1, seed + 1, lam_hi=1.0, lam_lo=1e-3)[0]
    return Y, rng.uniform(0.02, 0.1, (p,)), Cm


def _np(t):
    return None if t is None else t.numpy()


def _check_posterior(name, eng, post, Xs, mean_ref, var_ref, cpu_vjp, seed, shared, svgp, grad=True, vjp_bound=None):
    """log_density on one posterior: mean / var carry predict_f's bits, logp within the bound of the oracle on
    the CPU predict, grad_X bitwise predict_f_vjp fed the density's own gradients and within the summed bound
    of the CPU VJP fed the oracle's, fidelity column exactly 0; the diagonal form (no obs_cov) as well."""
    Y, ov, Cm = _observation(mean_ref, seed, shared)
    for dense in (True, False):
        oc = _padded_cov(Cm) if dense else None
        res = post.log_density(Xs, Y, obs_cov=oc, obs_var=ov, grad=grad)
        assert isinstance(res, M.LogDensityResult)
        pm, pv = post.predict_f(Xs)
        np.testing.assert_array_equal(_np(res.mean), pm.numpy())
        np.testing.assert_array_equal(_np(res.var), pv.numpy())
        assert not res.logp.requires_grad
        ref = LD.logpdf(mean_ref, Y, var_ref, ov, Cm if dense else None)
        tag = f"{name} {'dense' if dense else 'diag'}"
        _close(f"{tag} logp", _np(res.logp), ref[0])
        if not grad:
            assert res.grad_X is None
            continue
        gX = _np(res.grad_X)
        assert gX.shape == Xs.shape and np.all(gX[:, -1] == 0.0)
        # the density's own gradients on the forward's bits, then the VJP call: the same bits
        mean_d = res.mean.as_subclass(torch.Tensor)
        var_d = res.var.as_subclass(torch.Tensor)
        var_d = var_d if svgp else var_d[:, 0].contiguous()
        _, gm, gv, _ = eng.mvn_logpdf(mean_d, _dev(Y), var_d, _dev(ov), oc, grad=True, sum_gvar=not svgp)
        np.testing.assert_array_equal(post.predict_f_vjp(Xs, gm, gv)[2].numpy(), gX)
        want = cpu_vjp(ref[1], ref[2])[2]
        amax = np.abs(want).max()
        bound = (G.BOUND * max(1.0, amax) if vjp_bound is None else vjp_bound * amax) + LD.BOUND * max(1.0, amax)
        err = np.abs(gX - want).max()
        print(f"{tag} grad_X: err {err:.1e} (|ref|max {amax:.1e}, bound {bound:.1e})")
        assert err <= bound, (tag, err)
        again = post.log_density(Xs, Y, obs_cov=oc, obs_var=ov, grad=True)
        np.testing.assert_array_equal(_np(again.grad_X), gX)
        np.testing.assert_array_equal(_np(again.logp), _np(res.logp))


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("case", G.GPR_CASES[1:], ids=lambda c: "-".join(map(str, c)))
def test_gpr_log_density_synthetic(case, nb, eng):
    X, Y, Xs, prm, _, _, ref = G.gpr_synthetic(*case)
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        _check_posterior(f"gpr {case} nb{nb}", eng, post, Xs, ref[0], ref[1],
                         lambda gm, gv: G.gpr_vjp(X, Y, Xs, prm, gm, gv), 11, shared=case[2] > 3, svgp=False)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("nb", [32, 64])
def test_gpr_log_density_conditioned_posterior(nb, eng):
    """condition_on's posterior (a block append under the cached factors) against the CPU refit of the stacked
    rows."""
    X, Y, Xs, prm, _, _, _ = G.gpr_synthetic(*G.GPR_CASES[1])
    eng.set_tile(nb)
    try:
        Xa, Ya = X[-5:], Y[-5:]
        post = _model(X[:-5], Y[:-5], prm).posterior().condition_on(Xa, Ya)
        zero = np.zeros((Xs.shape[0], Y.shape[1]))
        ref = G.gpr_vjp(X, Y, Xs, prm, zero, zero)
        _check_posterior(f"conditioned nb{nb}", eng, post, Xs, ref[0], ref[1],
                         lambda gm, gv: G.gpr_vjp(X, Y, Xs, prm, gm, gv), 12, shared=False, svgp=False)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("nb", [32, 64])
def test_graph_log_density_value_only(nb, eng):
    """The graph model: the value from the cache; grad=True raises as predict_f_vjp does."""
    from oracle import graph_oracle as GO
    m, D = 2, 3
    Xg, Yg = _graph_data(m, D)
    mod = _graph_model(Xg, Yg, m, D, asym=True)
    Xs = Xg[::7].copy()
    mo, vo = GO.predict_f(torch.tensor(Xg), torch.tensor(Yg), torch.tensor(Xs), _graph_params(mod, D),
                          torch.tensor(1e-3, dtype=torch.float64))
    mean_ref = mo.numpy()
    var_ref = np.repeat(vo.numpy()[:, None], Yg.shape[1], axis=1)
    eng.set_tile(nb)
    try:
        post = mod.posterior()
        _check_posterior(f"graph nb{nb}", eng, post, Xs, mean_ref, var_ref, None, 13, shared=True, svgp=False,
                         grad=False)
        with pytest.raises(NotImplementedError, match="graph kernel"):
            post.log_density(Xs, mean_ref[0], grad=True)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("nb", [32, 64])
def test_svgp_log_density_eleven_latents(nb, eng):
    state, Xs, _, _, ref = G.svgp_synthetic()
    eng.set_tile(nb)
    try:
        m, _ = G.svgp_synthetic_model()
        _check_posterior(f"svgp L=11 nb{nb}", eng, m.posterior(), Xs, ref[0], ref[1],
                         lambda gm, gv: G.svgp_vjp(state, Xs, gm, gv), 14, shared=True, svgp=True)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("which", ["gpr", "singlebin", "latent"])
def test_log_density_hbs(which, nb, eng):
    """The HBS models (P = 49): the GPR at its initial parameters on 33 mixed-fidelity rows, the single-bin
    and latent SVGP models on 8 + 33 rows."""
    eng.set_tile(nb)
    try:
        if which == "gpr":
            X, Y, Xs, prm, _, _, ref = G.gpr_dataset("hbs")
            post = _model(X, Y, prm).posterior()
            cpu = lambda gm, gv: G.gpr_vjp(X, Y, Xs, prm, gm, gv)
        else:
            m, Wm, Xs = G.svgp_hbs_model(which)
            state = G.svgp_state(m, Wm)
            zero = np.zeros((Xs.shape[0], m.num_outputs))
            ref = G.svgp_vjp(state, Xs, zero, zero)
            post = m.posterior()
            cpu = lambda gm, gv: G.svgp_vjp(state, Xs, gm, gv)
        _check_posterior(f"hbs {which} nb{nb}", eng, post, Xs, ref[0], ref[1], cpu, 15, shared=True,
                         svgp=which != "gpr")
    finally:
        eng.set_tile(32)


def test_gpr_log_density_goku(eng):
    """Goku (n = 1164, P = 64), its 36 HF test rows as walkers against one data vector; the VJP part of the
    bound is Goku's, 1e-8 |ref|max."""
    X, Y, Xs, prm, _, _, ref = G.gpr_dataset("goku")
    post = _model(X, Y, prm).posterior()
    _check_posterior("goku", eng, post, Xs, ref[0], ref[1], lambda gm, gv: G.gpr_vjp(X, Y, Xs, prm, gm, gv), 16,
                     shared=True, svgp=False, vjp_bound=G.GOKU_BOUND)


def test_log_density_reports_a_bad_row_and_refuses_nocache(eng):
    """One host read, of info: a NaN input row raises CholeskyError naming the row; a NOCACHE posterior raises
    as predict_f_vjp does; an empty Xnew returns empty results."""
    X, Y, Xs, prm, _, _, ref = G.gpr_synthetic(*G.GPR_CASES[1])
    m = _model(X, Y, prm)
    post = m.posterior()
    Yo, ov, Cm = _observation(ref[0], 17, True)
    Xb = Xs.copy()
    Xb[4, 0] = np.nan
    for oc in (Cm, None):
        with pytest.raises(CholeskyError, match="row 4"):
            post.log_density(Xb, Yo, obs_cov=oc, obs_var=ov, grad=True)
    with pytest.raises(NotImplementedError):
        m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE).log_density(Xs, Yo)
    empty = post.log_density(Xs[:0], Yo, obs_cov=Cm, grad=True)
    assert tuple(empty.logp.shape) == (0,) and tuple(empty.grad_X.shape) == (0, Xs.shape[1])
    # obs_var forms: a scalar equals the [P] vector of that value, which equals the [N*, P] block of it
    a = post.log_density(Xs, Yo, obs_cov=Cm, obs_var=0.07, grad=True)
    b = post.log_density(Xs, Yo, obs_cov=Cm, obs_var=np.full(Y.shape[1], 0.07), grad=True)
    c = post.log_density(Xs, Yo, obs_cov=Cm, obs_var=np.full((Xs.shape[0], Y.shape[1]), 0.07), grad=True)
    for r in (b, c):
        np.testing.assert_array_equal(_np(r.logp), _np(a.logp))
        np.testing.assert_array_equal(_np(r.grad_X), _np(a.grad_X))


# ---------------------------------------------------------------- predict_log_density
def _pld_check(name, obj, Xs, Yn, s2, masked=False):
    """predict_log_density of a model or posterior against the oracle on its own predict_f and s2."""
    mean, var = obj.predict_f(Xs)
    p = mean.shape[1]
    Yo = Yn[:, :p]
    ov = np.broadcast_to(s2, (Xs.shape[0], p)) + (Yn[:, p:] ** 2 if Yn.shape[1] == 2 * p else 0.0)
    ref = LD.logpdf(mean.numpy().astype(np.float64), Yo, var.numpy().astype(np.float64), ov, None)[0]
    if not masked:
        ref = np.where(np.isnan(Yo).any(axis=1), np.nan, ref)
    got = obj.predict_log_density((Xs, Yn))
    assert tuple(got.shape) == (Xs.shape[0],) and got.dtype == torch.float64
    got = got.numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    _close(name, got[ok], ref[ok])


def test_predict_log_density_gpr_and_graph(eng):
    """The two GPR models (fp64 and fp32) and their posteriors (cached and NOCACHE): the likelihood variance is
    added; a NaN target gives a NaN row, as GPflow's Gaussian does."""
    X, Y, Xs, prm, _, _, ref = G.gpr_synthetic(*G.GPR_CASES[1])
    rng = np.random.default_rng(18)
    Yn = ref[0] + 0.2 * rng.standard_normal(ref[0].shape)
    m = _model(X, Y, prm)
    for name, obj in (("gpr model", m), ("gpr posterior", m.posterior()),
                      ("gpr nocache", m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE))):
        _pld_check(name, obj, Xs, Yn, prm.noise)
    Ynan = Yn.copy()
    Ynan[2, 1] = np.nan
    _pld_check("gpr NaN target", m, Xs, Ynan, prm.noise)
    D = X.shape[1] - 1
    m32 = M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                 M.SquaredExponential(lengthscales=np.ones(D)), dtype="float32")
    m32.likelihood.variance.assign(1e-2)
    _pld_check("gpr fp32 model", m32, Xs, Yn, 1e-2)
    # a symmetric rho_LF and rows off the training inputs: with an asymmetric one predict_f at a row of LF
    # source >= 1 takes its cross-covariance from the other triangle, and its variance may be negative
    Xg, Yg = _graph_data(2, 3)
    gm = _graph_model(Xg, Yg, 2, 3, asym=False)
    Xgs = Xg[::7].copy()
    Xgs[:, :-1] += 0.05
    Ygn = Yg[::7] + 0.1 * rng.standard_normal(Yg[::7].shape)
    _pld_check("graph model", gm, Xgs, Ygn, 1e-3)
    _pld_check("graph posterior", gm.posterior(), Xgs, Ygn, 1e-3)


def test_predict_log_density_svgp_likelihoods(eng):
    """Single-bin and latent SVGP; HeteroscedasticGaussian with [N*, P] (baseline only) and [N*, 2P] targets
    (baseline + Y_unc^2); MaskedGaussian with one variance per output and NaN targets left out."""
    from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
    P, D = 5, 3
    X, Y, Xs, _ = synthetic_multifidelity(60, 15, D, P, 9, seed=19)
    Xs[:, -1] = np.arange(9) % 2
    rng = np.random.default_rng(20)
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(D))
    Yn = 0.5 * rng.standard_normal((9, P))
    Yunc = rng.uniform(0.1, 0.6, (9, P))

    sb = M.SingleBinSVGP(X, Y, kern(), kern(), P, Z=X[:20].copy())
    G.randomize(sb, 31)
    sb.likelihood.variance.assign(0.3)
    _pld_check("singlebin model", sb, Xs, Yn, 0.3)
    _pld_check("singlebin posterior", sb.posterior(), Xs, Yn, 0.3)

    lat = M.LatentMFCoregionalizationSVGP(X, Y, kern(), kern(), num_latents=3, num_inducing=20, num_outputs=P)
    G.randomize(lat, 32)
    lat.likelihood.variance.assign(0.2)
    _pld_check("latent model", lat, Xs, Yn, 0.2)
    _pld_check("latent posterior", lat.posterior(), Xs, Yn, 0.2)

    het = M.LatentMFCoregionalizationSVGP(X, np.hstack([Y, 0.1 * np.ones_like(Y)]), kern(), kern(), num_latents=3,
                                          num_inducing=20, num_outputs=P, heterosed=True)
    G.randomize(het, 33)
    het.likelihood.variance.assign(np.array([0.15]))
    _pld_check("het model, baseline only", het, Xs, Yn, 0.15)
    _pld_check("het model, [Y | Y_unc]", het, Xs, np.hstack([Yn, Yunc]), 0.15)
    _pld_check("het posterior, [Y | Y_unc]", het.posterior(), Xs, np.hstack([Yn, Yunc]), 0.15)

    Ym = Yn.copy()
    Ym[rng.random(Ym.shape) < 0.3] = np.nan
    Ym[4] = np.nan
    msk = M.SingleBinSVGP(X, Y, kern(), kern(), P, Z=X[:20].copy(), missing_outputs=True)
    G.randomize(msk, 34)
    s2 = rng.uniform(0.1, 0.5, (P,))
    msk.likelihood.variance.assign(s2)
    _pld_check("masked model", msk, Xs, Ym, s2, masked=True)
    _pld_check("masked posterior", msk.posterior(), Xs, Ym, s2, masked=True)
    assert float(msk.predict_log_density((Xs, Ym))[4]) == 0.0
    for obj in (sb, lat.posterior()):
        with pytest.raises(NotImplementedError):
            obj.predict_log_density((Xs, Yn), full_cov=True)
