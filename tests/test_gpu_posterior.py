"""Cached posteriors (``model.posterior()``, posteriors.py) on the HIP path.

The cached ``predict_f`` (mfgp_gpr_posterior_predict / mfgp_svgp_posterior_predict: the product
against the cached inverse factor with K(X, X*) generated in the kernel) against the CPU oracles at
the bounds the model's own predict_f is held to (tests/test_gpu_parity.py: mean 1e-9 max(1, |mean|),
var 1e-9; tests/test_gpu_svgp.py covariance forms: 1e-10 max(1, |ref|)), and against the model's
predict_f at twice that (both sit within the bound of the oracle).  Snapshot semantics, stable
VARIABLE buffers, bitwise repeatability, build-time failure, the graph model and the fp32 refusal."""
import functools
import os

import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType
from multi_fidelity_gpflow_amd.engine import Engine
from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O
from oracle import svgp_oracle as S
from test_gpu_graph import _data as _graph_data, _model as _graph_model, _oracle_params as _graph_oracle_params
from test_gpu_parity import _model, _oracle_params, _params
from test_gpu_svgp import _oracle_state, _randomize

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _check_gpr(name, got, ref, scale=1.0):
    """(mean, var) against (mean, var): mean atol scale 1e-9 max(1, |mean|max), var atol scale 1e-9."""
    mean, var = got[0].numpy(), got[1].numpy()
    mo, vo = np.asarray(ref[0]), np.asarray(ref[1])
    assert mean.shape == mo.shape and var.shape == vo.shape, name
    em, ev = np.abs(mean - mo).max(), np.abs(var - vo).max()
    print(f"{name}: mean err {em:.1e} var err {ev:.1e}")
    assert em <= scale * 1e-9 * max(1.0, np.abs(mo).max()), (name, em)
    assert ev <= scale * 1e-9, (name, ev)


def _mixed33(X, seed):
    """33 rows (one more than a 32-column tile) near training inputs, fidelities 0 and 1 alternating."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(X.shape[0], 33, replace=False)
    Xs = X[idx].copy()
    Xs[:, :-1] += 0.01 * rng.standard_normal((33, X.shape[1] - 1))
    Xs[:, -1] = np.arange(33) % 2
    return Xs


@functools.lru_cache(maxsize=None)
def _gpr_case(which):
    """The dataset's seed-7 parameters, its four X* sets and their oracle predictions (computed once)."""
    from conftest import GOKU_DIR, HBS_DIR
    d = O.load_powerspecs(HBS_DIR if which == "hbs" else GOKU_DIR)
    X, Y = d["X"], d["Y"]
    p = _params(X.shape[1] - 1, Y.shape[1], seed=7)
    hf = d["Xtest"][:1].copy()
    hf[:, -1] = 1.0
    sets = {"one-hf": hf, "xtest": d["Xtest"], "x7": X[::7], "mixed33": _mixed33(X, 3)}
    po = _oracle_params(_model(X, Y, p))
    refs = {k: O.gpr_predict_f(X, Y, Xs, po) for k, Xs in sets.items()}
    cov = O.gpr_predict_f_full_cov(X, Y, d["Xtest"], po)
    return X, Y, p, sets, refs, cov


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("which", ["hbs", "goku"])
def test_gpr_posterior_parity(which, nb, eng):
    X, Y, p, sets, refs, (mo, co) = _gpr_case(which)
    eng.set_tile(nb)
    try:
        m = _model(X, Y, p)
        post = m.posterior()
        assert isinstance(post, M.GPRPosterior)
        for k, Xs in sets.items():
            got = post.predict_f(Xs)
            _check_gpr(f"{which} nb{nb} {k} vs oracle", got, refs[k])
            own = m.predict_f(Xs)
            _check_gpr(f"{which} nb{nb} {k} vs model", got, (own[0].numpy(), own[1].numpy()), scale=2.0)
            again = post.predict_f(Xs)   # fixed-order partial sums: the same bits
            np.testing.assert_array_equal(again[0].numpy(), got[0].numpy())
            np.testing.assert_array_equal(again[1].numpy(), got[1].numpy())
        Xs = sets["xtest"]
        mean, cov = post.predict_f(Xs, full_cov=True)
        assert tuple(cov.shape) == (Y.shape[1], Xs.shape[0], Xs.shape[0])
        np.testing.assert_allclose(mean.numpy(), mo, rtol=0, atol=1e-9 * max(1, np.abs(mo).max()))
        np.testing.assert_allclose(cov.numpy(), co, rtol=0, atol=1e-9)
        _, var = post.predict_f(Xs)
        np.testing.assert_allclose(np.diagonal(cov.numpy()[0]), var.numpy()[:, 0], rtol=0, atol=1e-12)
        with pytest.raises(NotImplementedError):
            post.predict_f(Xs, full_output_cov=True)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("n_lf,n_hf,p", [(20, 5, 1), (70, 9, 3), (60, 20, 65)])
def test_gpr_posterior_small_shapes(n_lf, n_hf, p, eng):
    """n below one 32-tile, n across a tile edge, p across a tile edge (D = 1), X* of 1, 31, 32 and 33
    rows; a fidelity of 0.9999999999999999 is neither 0 nor 1: an exactly zero prediction (quirk C-3)."""
    rng = np.random.default_rng(100 * n_lf + p)
    X = np.vstack([np.hstack([rng.random((n_lf, 1)), np.zeros((n_lf, 1))]),
                   np.hstack([rng.random((n_hf, 1)), np.ones((n_hf, 1))])])
    Y = np.sin(3.0 * X[:, :1] * (1.0 + rng.random((1, p)))) + 0.3 * X[:, 1:]
    prm = _params(1, p, seed=9)
    m = _model(X, Y, prm)
    po = _oracle_params(m)
    post = m.posterior()
    for ns in (1, 31, 32, 33):
        Xs = np.hstack([rng.random((ns, 1)), (np.arange(ns)[:, None] + ns) % 2 * 1.0])
        if ns == 33:
            Xs[5, 1] = 0.9999999999999999
        got = post.predict_f(Xs)
        _check_gpr(f"n={n_lf + n_hf} p={p} ns={ns}", got, O.gpr_predict_f(X, Y, Xs, po))
        if ns == 33:
            assert np.all(got[0].numpy()[5] == 0.0) and np.all(got[1].numpy()[5] == 0.0)


def test_gpr_posterior_snapshot_semantics(eng):
    X, Y, p, sets, refs, _ = _gpr_case("hbs")
    Xs = sets["mixed33"]
    m = _model(X, Y, p)
    post = m.posterior()
    var_post = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    before = post.predict_f(Xs)
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.likelihood.variance.assign(5e-3)
    after = post.predict_f(Xs)
    np.testing.assert_array_equal(after[0].numpy(), before[0].numpy())
    np.testing.assert_array_equal(after[1].numpy(), before[1].numpy())
    fused, own = post.fused_predict_f(Xs), m.predict_f(Xs)
    np.testing.assert_array_equal(fused[0].numpy(), own[0].numpy())
    np.testing.assert_array_equal(fused[1].numpy(), own[1].numpy())
    assert np.abs(own[0].numpy() - before[0].numpy()).max() > 1e-6   # the change does move predict_f
    new_ref = O.gpr_predict_f(X, Y, Xs, _oracle_params(m))
    post.update_cache()
    _check_gpr("after update_cache", post.predict_f(Xs), new_ref)
    # VARIABLE: update_cache rewrites the same device block
    ptr0 = var_post.cache.data_ptr()
    _check_gpr("variable before", var_post.predict_f(Xs), refs["mixed33"])
    var_post.update_cache()
    assert var_post.cache.data_ptr() == ptr0
    _check_gpr("variable after", var_post.predict_f(Xs), new_ref)
    # NOCACHE: predict_f is the fused one
    nc = m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE)
    assert nc.cache is None
    np.testing.assert_array_equal(nc.predict_f(Xs)[0].numpy(), own[0].numpy())


def test_posterior_failure_surfaces_at_build_time(eng, hbs):
    """The non-PD set-up of test_gpu_parity.test_non_pd_reports_info_and_raises: a numerical
    non-PD report (info != 0), raised by posterior(), never by a cached predict_f."""
    bad = _model(hbs["X"], hbs["Y"], _params(5, 49))
    bad.kernel.kernel_L.variance.assign(1e300)    # overflowing trailing updates -> non-finite pivot
    with pytest.raises(M.CholeskyError):
        bad.posterior()
    good = _model(hbs["X"], hbs["Y"], _params(5, 49))
    post = good.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    good.kernel.kernel_L.variance.assign(1e300)
    with pytest.raises(M.CholeskyError):
        post.update_cache()


def test_graph_posterior(eng):
    m, D = 2, 3
    X, Y = _graph_data(m, D)
    rng = np.random.default_rng(9)
    Xs = np.hstack([rng.uniform(0, 1, (35, D)), (np.arange(35)[:, None] % (m + 1)) * 1.0])
    mod = _graph_model(X, Y, m, D, asym=True)
    post = mod.posterior()
    prm = _graph_oracle_params(mod, D)
    noise = torch.tensor(1e-3, dtype=torch.float64)
    mean, var = post.predict_f(Xs)
    mo, vo = GO.predict_f(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), prm, noise)
    np.testing.assert_allclose(mean.numpy(), mo.numpy(), rtol=0, atol=1e-9 * max(1.0, np.abs(mo.numpy()).max()))
    np.testing.assert_allclose(var.numpy()[:, 0], vo.numpy(), rtol=0, atol=1e-9)
    own = mod.predict_f(Xs)
    _check_gpr("graph vs model", (mean, var), (own[0].numpy(), own[1].numpy()), scale=2.0)
    Xt = Xs[Xs[:, -1] == float(m)]
    meanc, cov = post.predict_f(Xt, full_cov=True)
    mo, co = GO.predict_f_full_cov(torch.tensor(X), torch.tensor(Y), torch.tensor(Xt), prm, 1e-3)
    np.testing.assert_allclose(meanc.numpy(), mo.numpy(), rtol=0, atol=1e-9 * max(1.0, np.abs(mo.numpy()).max()))
    np.testing.assert_allclose(cov.numpy()[2], co.numpy(), rtol=0, atol=1e-9)


def _svgp_model(which, hbs):
    X, Y = hbs["X"], hbs["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    if which == "singlebin":
        m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                            M.SquaredExponential(lengthscales=np.ones(D)), P, Z=np.zeros((50, D + 1)))
        _randomize(m, 21)
        return m, None
    m = M.LatentMFCoregionalizationSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                        M.SquaredExponential(lengthscales=np.ones(D)), num_latents=5,
                                        num_inducing=30, num_outputs=P, w_type='diagonal')
    _randomize(m, 22)
    return m, m.kernel.W.numpy()


def _svgp_oracle(m, Wm, Xs):
    lik, m.likelihood = m.likelihood, M.Gaussian()   # _oracle_state reads a scalar noise; predict_f has none
    try:
        Z, kps, q_mu, q_sqrt, W, _ = _oracle_state(m, Wm)
    finally:
        m.likelihood = lik
    gm, gv = S.latent_moments(torch.tensor(Xs), Z, kps, q_mu, q_sqrt)
    if W is None:
        return gm.numpy(), gv.numpy()
    return (gm @ W.T).numpy(), (gv @ (W * W).T).numpy()


def _check_svgp(name, got, ref, scale=1.0):
    for what, g, r in (("mean", got[0], ref[0]), ("var", got[1], ref[1])):
        g, r = np.asarray(g), np.asarray(r)
        assert g.shape == r.shape, (name, what)
        err = np.abs(g - r).max()
        print(f"{name} {what}: err {err:.1e}")
        assert err <= scale * 1e-10 * max(1.0, np.abs(r).max()), (name, what, err)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_posterior(which, hbs, eng):
    m, Wm = _svgp_model(which, hbs)
    Xs = np.vstack([hbs["Xtest"], _mixed33(hbs["X"], 4)])
    post = m.posterior()
    assert isinstance(post, M.SVGPPosterior)
    got = post.predict_f(Xs)
    ref = _svgp_oracle(m, Wm, Xs)
    _check_svgp(f"{which} vs oracle", (got[0].numpy(), got[1].numpy()), ref)
    own = m.predict_f(Xs)
    _check_svgp(f"{which} vs model", (got[0].numpy(), got[1].numpy()), (own[0].numpy(), own[1].numpy()), scale=2.0)
    one = post.predict_f(Xs[:1])
    _check_svgp(f"{which} one row", (one[0].numpy(), one[1].numpy()), (ref[0][:1], ref[1][:1]))
    # covariance forms: the model's entry point on the snapshot's state
    Xc = hbs["Xtest"]
    for fc, foc in ((True, False), (False, True), (True, True)):
        a, b = post.predict_f(Xc, full_cov=fc, full_output_cov=foc), m.predict_f(Xc, full_cov=fc, full_output_cov=foc)
        np.testing.assert_array_equal(a[0].numpy(), b[0].numpy())
        np.testing.assert_array_equal(a[1].numpy(), b[1].numpy())
    # snapshot semantics with q_mu changed
    var_post = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    ptr0 = var_post.cache.data_ptr()
    m.q_mu.assign(m.q_mu.numpy() + 0.25)
    after = post.predict_f(Xs)
    np.testing.assert_array_equal(after[0].numpy(), got[0].numpy())
    np.testing.assert_array_equal(after[1].numpy(), got[1].numpy())
    cov_old = post.predict_f(Xc, full_cov=True)
    assert np.abs(cov_old[0].numpy() - m.predict_f(Xc)[0].numpy()).max() > 1e-3   # still the snapshot's mean
    fused, own = post.fused_predict_f(Xs), m.predict_f(Xs)
    np.testing.assert_array_equal(fused[0].numpy(), own[0].numpy())
    new_ref = _svgp_oracle(m, Wm, Xs)
    var_post.update_cache()
    assert var_post.cache.data_ptr() == ptr0
    upd = var_post.predict_f(Xs)
    _check_svgp(f"{which} after update_cache", (upd[0].numpy(), upd[1].numpy()), new_ref)


def test_svgp_posterior_goku_singlebin(goku, eng):
    """SingleBinSVGP at Goku (M = 300, L = P = 64), the 36 test rows: one batch over 64 latents."""
    X, Y = goku["X"], goku["Y"]
    Zfix = np.load(os.path.join(os.path.dirname(__file__), "golden", "goku_kmeans_z300.npy"))
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(10)),
                        M.SquaredExponential(lengthscales=np.ones(10)), 64, Z=np.zeros((300, 11)))
    m.inducing_variable.assign(Zfix)
    _randomize(m, 23)
    Xs = goku["Xtest"]
    assert Xs.shape[0] == 36
    got = m.posterior().predict_f(Xs)
    _check_svgp("goku singlebin vs oracle", (got[0].numpy(), got[1].numpy()), _svgp_oracle(m, None, Xs))
    own = m.predict_f(Xs)
    _check_svgp("goku singlebin vs model", (got[0].numpy(), got[1].numpy()), (own[0].numpy(), own[1].numpy()),
                scale=2.0)


@pytest.mark.parametrize("lik", ["het", "masked"])
def test_svgp_posterior_other_likelihoods(lik, hbs, eng):
    """The likelihood does not enter predict_f: the het and masked models' posteriors return the
    model's predict_f (to the cached-vs-model bound)."""
    X, Y = hbs["X"], hbs["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    kw = dict(heterosed=True) if lik == "het" else dict(missing_outputs=True)
    Yt = np.hstack([Y, 0.1 * np.ones_like(Y)]) if lik == "het" else Y
    m = M.LatentMFCoregionalizationSVGP(X, Yt, M.SquaredExponential(lengthscales=np.ones(D)),
                                        M.SquaredExponential(lengthscales=np.ones(D)), num_latents=5,
                                        num_inducing=30, num_outputs=P, w_type='diagonal', **kw)
    rng = np.random.default_rng(31)
    m.q_mu.assign(rng.standard_normal(m.q_mu.shape) * 0.3)
    Xs = hbs["Xtest"]
    got, own = m.posterior().predict_f(Xs), m.predict_f(Xs)
    _check_svgp(f"{lik} vs model", (got[0].numpy(), got[1].numpy()), (own[0].numpy(), own[1].numpy()), scale=2.0)
    _check_svgp(f"{lik} vs oracle", (got[0].numpy(), got[1].numpy()), _svgp_oracle(m, m.kernel.W.numpy(), Xs))


# ---------------------------------------------------------------- the schedules of the cached predict
# post_chunk (mfgp_posterior_capi.hip) cuts rows into 8-tile tasks unless batch T Ts >= 256; the shapes below
# reach each side for triangular (GPR) and square (SVGP) rows, more than 8 partials a row, more than
# 8 row groups, a partial last batch of the mixing loop and the graph kernel with several row groups.
# tests/test_posterior_host.py::test_posterior_shapes_reach_their_schedule witnesses on the host that
# the GPR and M = 270 shapes take the schedule named here.  Each case: against the oracle at this
# file's bounds, against the model's predict_f at twice that, two calls bitwise equal, and X*[:1]
# against the first row of the reference.
def _np(pair):
    return pair[0].numpy(), pair[1].numpy()


def _four_ways(check, name, post, model, Xs, ref):
    got = _np(post.predict_f(Xs))
    check(f"{name} vs oracle", got, ref)
    check(f"{name} vs model", got, _np(model.predict_f(Xs)), scale=2.0)
    again = _np(post.predict_f(Xs))
    np.testing.assert_array_equal(again[0], got[0])
    np.testing.assert_array_equal(again[1], got[1])
    check(f"{name} one row", _np(post.predict_f(Xs[:1])), (ref[0][:1], ref[1][:1]))
    return got


def _check_gpr_np(name, got, ref, scale=1.0):
    _check_gpr(name, (torch.as_tensor(got[0]), torch.as_tensor(got[1])), ref, scale)


def _syn_gpr(n_lf, n_hf, d, p, nstar, seed):
    """Synthetic GPR case on the unit cube: lengthscales 0.5-2, noise 1e-2 (cond(K + s2 I) stays below
    ~1e6, so the oracle's own solves are good to a tenth of the 1e-9 bound: see the tests' docstrings),
    X* near nothing in particular with the two fidelities alternating."""
    from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
    X, Y, Xt, _ = synthetic_multifidelity(n_lf, n_hf, d, p, nstar, seed=seed)
    Xt[:, -1] = np.arange(nstar) % 2
    prm = _params(d, p, seed=seed)
    prm.noise = 1e-2
    return X, Y, Xt, prm


@functools.lru_cache(maxsize=None)
def _gpr_whole_rows_case():
    X, Y, Xs, prm = _syn_gpr(400, 100, 3, 3, 512, 500)
    return X, Y, Xs, prm, O.gpr_predict_f(X, Y, Xs, prm)


def test_gpr_posterior_whole_rows(eng):
    """n = 500 (T = 16), X* of 512 rows (Ts = 16): T Ts = 256, whole triangular rows (chunk = T); the
    first 32 of those rows alone (Ts = 1) take 8-tile chunks, and the two schedules agree on them
    within the oracle bound (another association: not bitwise).
    Reference computed two ways on the CPU (the oracle's triangular solves against the explicit
    inverse factor, mean = (L^{-1} K*)^T (L^{-1} Y)): they disagree by 2.5e-12 (mean, |mean| <= 1.9) and
    5.3e-15 (var) at cond(K + s2 I) = 5.7e4: under a tenth of the bounds (1.9e-10, 1e-10).
    Measured on an MI355X: whole rows 2.9e-12 (mean) / 6.2e-15 (var) against the oracle, the chunked 32 rows
    2.1e-12 / 3.6e-15, the two schedules 5.5e-13 / 2.0e-15 apart, the model 4.7e-13 / 4.9e-15, one row 1.2e-12."""
    X, Y, Xs, prm, ref = _gpr_whole_rows_case()
    assert X.shape[0] == 500 and Xs.shape[0] == 512
    m = _model(X, Y, prm)
    post = m.posterior()
    whole = _four_ways(_check_gpr_np, "gpr whole rows", post, m, Xs, ref)
    chunked = _four_ways(_check_gpr_np, "gpr first 32 rows, chunked", post, m, Xs[:32], (ref[0][:32], ref[1][:32]))
    _check_gpr_np("whole rows vs chunked", chunked, (whole[0][:32], whole[1][:32]))


@functools.lru_cache(maxsize=None)
def _gpr_nine_partials_case():
    X, Y, Xs, prm = _syn_gpr(1800, 281, 1, 2, 33, 2081)
    return X, Y, Xs, prm, O.gpr_predict_f(X, Y, Xs, prm)


def test_gpr_posterior_more_than_eight_partials(eng):
    """n = 2081 (T = 66 at NB = 32), X* of 33 rows (Ts = 2: 132 < 256, 8-tile chunks): the row tiles
    64 and 65 have 9 partials, the second pass of post_sum's eight-at-a-time loop; 17 row groups, the
    third pass of post_sum_coherent.
    Reference two ways on the CPU (as in test_gpr_posterior_whole_rows): 6.0e-13 (mean), 8.2e-15 (var) at
    cond(K + s2 I) = 2.4e5.  Measured on an MI355X: 5.9e-13 / 3.1e-15 against the oracle, 3.7e-13 / 9.3e-15
    against the model, one row 3.0e-13 / 2.2e-16."""
    X, Y, Xs, prm, ref = _gpr_nine_partials_case()
    assert X.shape[0] == 2081 and Xs.shape[0] == 33
    m = _model(X, Y, prm)
    _four_ways(_check_gpr_np, "gpr 9 partials", m.posterior(), m, Xs, ref)


def _syn_latent(n_lf, n_hf, L, Mi, seed, nstar):
    from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
    d, P = 5, 6
    X, Y, Xt, _ = synthetic_multifidelity(n_lf, n_hf, d, P, nstar, seed=seed)
    Xt[:, -1] = np.arange(nstar) % 2
    m = M.LatentMFCoregionalizationSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(d)),
                                        M.SquaredExponential(lengthscales=np.ones(d)), num_latents=L,
                                        num_inducing=Mi, num_outputs=P, w_type='diagonal')
    _randomize(m, seed)
    return m, Xt


def test_svgp_posterior_chunked_square_rows(eng):
    """The headline use (a latent emulator with M ~ 300 and a handful of latents asked for a few
    points): L = 3, M = 270 (Tm = 9).  X* of 1 and 33 rows: 3 x 9 x Ts <= 54 < 256, square rows in two
    chunks, tasks (i < 8, second chunk) wholly right of the diagonal (A's partial stays zero, only the C
    product runs) and two partials a row for A and B.  X* of 320 rows: 270 >= 256, whole rows; the
    rows shared by the two schedules agree within the oracle bound.
    Reference two ways on the CPU (the oracle's triangular solve against the explicit inverse of
    chol(K_uu), B = (Lq^T Lm^{-1}) K_uf as the device forms it): 3.0e-13 (mean), 2.4e-14 (var) at
    cond(K_uu) = 1.3e8; a tenth of the bound is 1e-11.  Measured on an MI355X against the oracle: 5.3e-13 /
    3.4e-14 (320 rows), 3.7e-13 / 9.4e-15 (33), 1.8e-14 / 3.5e-15 (1); chunked against whole rows 9.6e-15 /
    8.1e-16; against the model 1.7e-13 / 6.2e-15."""
    m, Xs = _syn_latent(400, 100, 3, 270, 270, 320)
    assert m.inducing_variable.shape[0] == 270
    Wm = m.kernel.W.numpy()
    ref = _svgp_oracle(m, Wm, Xs)
    post = m.posterior()
    whole = _four_ways(_check_svgp, "svgp M=270 whole rows (320)", post, m, Xs, ref)
    for ns in (1, 33):
        part = _four_ways(_check_svgp, f"svgp M=270 chunked ({ns})", post, m, Xs[:ns], (ref[0][:ns], ref[1][:ns]))
        _check_svgp(f"chunked ({ns}) vs whole rows", part, (whole[0][:ns], whole[1][:ns]))


def test_svgp_posterior_more_than_eight_row_groups(eng):
    """SingleBinSVGP with L = P = 2 and M = 1030 (Tm = 33: 9 row groups of 4 tiles, the last of one),
    X* of 5 rows: post_sum_coherent's second pass over the pa / pb / pm strides; rows of 5 chunks.
    The lengthscales are half of _randomize's (0.26-0.68 on the unit cube, cond(K_uu) = 2.9e8): with
    _randomize's own (cond 7.1e8) the reference computed two ways on the CPU (the oracle's triangular
    solve against the explicit inverse of chol(K_uu)) disagreed by 1.5e-11 in the mean, more than a
    tenth of the 1e-10 bound; with these by 9.3e-13 (mean), 2.6e-13 (var).  Measured on an MI355X: 2.6e-12 /
    4.1e-13 against the oracle, 7.6e-13 / 7.7e-14 against the model, one row 1.1e-13 / 3.4e-13."""
    from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
    d, P = 5, 2
    X, Y, Xs, _ = synthetic_multifidelity(900, 200, d, P, 5, seed=1030)
    Xs[:, -1] = np.arange(5) % 2
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(d)),
                        M.SquaredExponential(lengthscales=np.ones(d)), P, Z=np.zeros((1030, d + 1)))
    _randomize(m, 1030)
    for k in m.kernel.kernels:
        k.kernel_L.lengthscales.assign(0.5 * k.kernel_L.lengthscales.numpy())
        k.kernel_delta.lengthscales.assign(0.5 * k.kernel_delta.lengthscales.numpy())
    assert m.inducing_variable.shape[0] == 1030
    _four_ways(_check_svgp, "svgp M=1030", m.posterior(), m, Xs, _svgp_oracle(m, None, Xs))


def test_svgp_posterior_mixing_eleven_latents(eng):
    """Mixing with W and L = 11 latents: k_post_out's l0 loop runs a full batch of 8 and a partial one
    of 3.  M = 40, X* of 33 rows (two column tiles, the second with one row).
    Reference two ways on the CPU: 3.6e-15 (mean), 2.5e-16 (var).  Measured on an MI355X: 5.8e-15 / 6.4e-16
    against the oracle, 3.9e-15 / 3.9e-16 against the model."""
    m, Xs = _syn_latent(150, 40, 11, 40, 11, 33)
    Wm = m.kernel.W.numpy()
    assert Wm.shape == (6, 11) and np.count_nonzero(Wm[:, 8:]) > 0     # the partial batch carries weight
    _four_ways(_check_svgp, "svgp L=11", m.posterior(), m, Xs, _svgp_oracle(m, Wm, Xs))


@functools.lru_cache(maxsize=None)
def _graph_case():
    m, D = 2, 3
    X, Y = _graph_data(m, D, sizes=(150, 100, 40))
    rng = np.random.default_rng(9)
    Xs = np.hstack([rng.uniform(0, 1, (35, D)), (np.arange(35)[:, None] % (m + 1)) * 1.0])
    return m, D, X, Y, Xs


@pytest.mark.parametrize("nb", [32, 64])
def test_graph_posterior_row_groups(nb, eng):
    """The graph kernel (k_post_a's graph_entry branch) at n = 290: T = 10 at NB = 32 (three row
    groups, rows 8 and 9 of two chunks), T = 5 at NB = 64 (three row groups of two); X* of 35 rows over
    the three fidelities; marginal and, on the top-fidelity rows, full_cov.  Bounds: test_graph_posterior's.
    Reference two ways on the CPU (the oracle against the explicit inverse factor, and the mean through
    K^{-1} Y): 7.7e-12 (mean, |mean| <= 2.6), 1.7e-15 (var) at cond 1.5e5.  Measured on an MI355X against the
    oracle: 1.4e-11 / 4.0e-15 at NB = 32, 1.0e-11 / 3.1e-15 at 64 (bound 2.6e-9 / 1e-9); full_cov 1.2e-11 /
    4.0e-15 and 1.1e-11 / 3.3e-15."""
    m, D, X, Y, Xs = _graph_case()
    assert X.shape[0] == 290
    eng.set_tile(nb)
    try:
        mod = _graph_model(X, Y, m, D, asym=True)
        post = mod.posterior()
        prm = _graph_oracle_params(mod, D)
        noise = torch.tensor(1e-3, dtype=torch.float64)
        mo, vo = GO.predict_f(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), prm, noise)
        ref = (mo.numpy(), np.tile(vo.numpy()[:, None], (1, Y.shape[1])))
        _four_ways(_check_gpr_np, f"graph nb{nb}", post, mod, Xs, ref)
        Xt = Xs[Xs[:, -1] == float(m)]
        meanc, cov = post.predict_f(Xt, full_cov=True)
        mo, co = GO.predict_f_full_cov(torch.tensor(X), torch.tensor(Y), torch.tensor(Xt), prm, 1e-3)
        em, ec = np.abs(meanc.numpy() - mo.numpy()).max(), np.abs(cov.numpy()[2] - co.numpy()).max()
        print(f"graph nb{nb} full_cov: mean err {em:.1e} cov err {ec:.1e}")
        assert em <= 1e-9 * max(1.0, np.abs(mo.numpy()).max()) and ec <= 1e-9
        assert tuple(cov.shape) == (Y.shape[1], Xt.shape[0], Xt.shape[0])
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_posterior_tile64(which, eng):
    """test_svgp_posterior at NB = 64 (k_post_a<64> with C, k_post_out<64>'s SVGP tail,
    svgp_factor_run<64>) on synthetic models with M = 70 (two 64-tiles; the HBS models of
    test_svgp_posterior fit one): n = 190, d = 5, P = 6, X* of 8 + 62 rows (two column tiles); the four
    checks, update_cache() on a VARIABLE cache, and the tile-mismatch error of a cache built at another
    tile.  Reference two ways on the CPU: 5.2e-14 (mean), 2.2e-14 (var) single bin; 9.0e-15, 3.5e-16 latent.
    Measured on an MI355X against the oracle: 7.1e-14 / 2.4e-14 single bin, 6.1e-15 / 4.2e-16 latent; after
    update_cache 1.2e-13 / 2.4e-14 and 1.4e-14 / 4.2e-16."""
    from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
    d, P = 5, 6
    X, Y, Xt, _ = synthetic_multifidelity(150, 40, d, P, 8, seed=64)
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(d))
    rng = np.random.default_rng(70)
    Xn = X[rng.choice(X.shape[0], 62, replace=False)].copy()
    Xn[:, -1] = np.arange(62) % 2
    Xs = np.vstack([Xt, Xn])
    eng.set_tile(64)
    try:
        if which == "singlebin":
            m, Wm = M.SingleBinSVGP(X, Y, kern(), kern(), P, Z=np.zeros((70, d + 1))), None
        else:
            m = M.LatentMFCoregionalizationSVGP(X, Y, kern(), kern(), num_latents=3, num_inducing=70, num_outputs=P,
                                                w_type='diagonal')
            Wm = m.kernel.W.numpy()
        _randomize(m, 64)
        post = m.posterior()
        var_post = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
        ref = _svgp_oracle(m, Wm, Xs)
        got = _four_ways(_check_svgp, f"{which} nb64", post, m, Xs, ref)
        # VARIABLE: update_cache rewrites the same block with the new state; the TENSOR snapshot stays
        ptr0 = var_post.cache.data_ptr()
        m.q_mu.assign(m.q_mu.numpy() + 0.25)
        after = _np(post.predict_f(Xs))
        np.testing.assert_array_equal(after[0], got[0])
        np.testing.assert_array_equal(after[1], got[1])
        var_post.update_cache()
        assert var_post.cache.data_ptr() == ptr0
        _check_svgp(f"{which} nb64 after update_cache", _np(var_post.predict_f(Xs)), _svgp_oracle(m, Wm, Xs))
        # the cache is tied to the tile it was built with
        eng.set_tile(32)
        with pytest.raises(M.MFGPError, match="built for tile size 64"):
            post.predict_f(Xs)
        post.update_cache()                       # rebuilt at 32: the new state, the 32-tile kernels
        _check_svgp(f"{which} rebuilt at 32", _np(post.predict_f(Xs)), _svgp_oracle(m, Wm, Xs))
        eng.set_tile(64)
        with pytest.raises(M.MFGPError, match="built for tile size 32"):
            post.predict_f(Xs)
    finally:
        eng.set_tile(32)


def test_fp32_posterior_not_cached(hbs):
    D = hbs["X"].shape[1] - 1
    m = M.MultiFidelityGPModel(hbs["X"], hbs["Y"], M.SquaredExponential(lengthscales=np.ones(D)),
                               M.SquaredExponential(lengthscales=np.ones(D)), dtype="float32")
    with pytest.raises(NotImplementedError, match="float32 path is not cached"):
        m.posterior()
