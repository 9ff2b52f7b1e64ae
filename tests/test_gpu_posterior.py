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


def test_fp32_posterior_not_cached(hbs):
    D = hbs["X"].shape[1] - 1
    m = M.MultiFidelityGPModel(hbs["X"], hbs["Y"], M.SquaredExponential(lengthscales=np.ones(D)),
                               M.SquaredExponential(lengthscales=np.ones(D)), dtype="float32")
    with pytest.raises(NotImplementedError, match="float32 path is not cached"):
        m.posterior()
