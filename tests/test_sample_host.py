"""predict_f_samples, host side: the numpy oracle against an independent formulation and against the
moments it must reproduce, the stride arithmetic of the two uses of mfgp_mvn_sample, and every argument
check that needs no device.  No GPU."""
import numpy as np
import pytest
import scipy.linalg as sla

import _sample_oracle as SO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import engine as E
from multi_fidelity_gpflow_amd.posteriors import GPRPosterior, PrecomputeCacheType, SVGPPosterior


def _moments(n, p, seed):
    rng = np.random.default_rng(seed)
    cov = SO.spd(n, p, seed)
    return rng.standard_normal((n, p)), cov, np.abs(rng.standard_normal((n, p))) + 0.1


def test_oracle_equals_explicit_loops():
    """sample[s, :, p] = mean[:, p] + L_p eps[s, :, p] with scipy's lower factor and loops over s and p; the
    upper triangle of cov is NaN for the oracle (it must read the lower one only)."""
    n, p, S = 7, 3, 4
    mean, cov, var = _moments(n, p, 1)
    eps = np.random.default_rng(2).standard_normal((S, n, p))
    ref = np.empty((S, n, p))
    for q in range(p):
        L = sla.cholesky(cov[q] + SO.JITTER * np.eye(n), lower=True)
        for s in range(S):
            ref[s, :, q] = mean[:, q] + L @ eps[s, :, q]
    poisoned = cov.copy()
    poisoned[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
    got = SO.predict_f_samples(mean, poisoned, eps, num_samples=S)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13)
    one = SO.predict_f_samples(mean, cov, eps[0])
    assert one.shape == (n, p)
    np.testing.assert_array_equal(one, SO.predict_f_samples(mean, cov, eps[:1], num_samples=1)[0])
    marg = SO.predict_f_samples(mean, var, eps, num_samples=S, full_cov=False)
    np.testing.assert_array_equal(marg, mean[None] + np.sqrt(var)[None] * eps)
    with pytest.raises(NotImplementedError):
        SO.predict_f_samples(mean, cov, eps, num_samples=S, full_cov=True, full_output_cov=True)


def test_oracle_moments():
    """20 000 seeded draws at n = 5: the sample mean and covariance sit within 5 standard errors of mean
    and cov + jitter I (se of a mean sqrt(C_ii / N); of a covariance entry sqrt((C_ii C_jj + C_ij^2) / N)).
    An L^T in place of L, or a transposed eps, fails this."""
    n, N = 5, 20000
    mean, cov, _ = _moments(n, 1, 3)
    eps = np.random.default_rng(4).standard_normal((N, n, 1))
    x = SO.predict_f_samples(mean, cov, eps, num_samples=N)[:, :, 0]
    C = cov[0] + SO.JITTER * np.eye(n)
    d = np.diag(C)
    em = np.abs(x.mean(0) - mean[:, 0]) / np.sqrt(d / N)
    xc = x - x.mean(0)
    ec = np.abs(xc.T @ xc / (N - 1) - C) / np.sqrt((np.outer(d, d) + C * C) / N)
    print(f"mean: {em.max():.2f} se, cov: {ec.max():.2f} se")
    assert em.max() <= 5.0 and ec.max() <= 5.0
    assert np.abs(C - C.T).max() == 0.0 and np.abs(C - np.diag(d)).max() > 0.1   # the check can see a transpose


@pytest.mark.parametrize("use", ["gpr", "svgp"])
def test_stride_arithmetic(use):
    """The two uses of mfgp_mvn_sample, emulated element by element through the header's strides on flat
    arrays, against the oracle's [S, N*, P]: GPR batch = 1, ncol = P, rs = P, ss = N* P (one factor for all
    outputs); SVGP batch = P, ncol = 1, bs = 1, rs = P, ss = N* P, mean_bs = 1, mean_rs = P."""
    n, p, S, pad = 6, 4, 3, 2
    rng = np.random.default_rng(5)
    mean = rng.standard_normal((n, p))
    eps = rng.standard_normal((S, n, p))
    ldc = n + pad
    if use == "gpr":
        block = SO.spd(n, 1, 6)
        cov = np.tile(block, (p, 1, 1))
        buf = np.full((1, n, ldc), np.nan)
        buf[0, :, :n] = np.where(np.tri(n, dtype=bool), block[0], np.nan)
        geo = dict(batch=1, ncol=p, sC=0, mean_rs=p, mean_bs=0, rs=p, ss=n * p, bs=0)
    else:
        cov = SO.spd(n, p, 7)
        buf = np.full((p, n, ldc), np.nan)
        buf[:, :, :n] = np.where(np.tri(n, dtype=bool)[None], cov, np.nan)
        geo = dict(batch=p, ncol=1, sC=n * ldc, mean_rs=p, mean_bs=1, rs=p, ss=n * p, bs=1)
    out = SO.emulate_abi(n, geo["batch"], S, geo["ncol"], buf.ravel(), ldc, geo["sC"], SO.JITTER, mean.ravel(),
                         geo["mean_rs"], geo["mean_bs"], eps.ravel(), geo["rs"], geo["ss"], geo["bs"], S * n * p)
    assert not np.isnan(out).any()   # every element of [S, N*, P] is written exactly through these strides
    np.testing.assert_allclose(out.reshape(S, n, p), SO.predict_f_samples(mean, cov, eps, num_samples=S), rtol=0,
                               atol=1e-13)


# ---------------------------------------------------------------- argument checks, no device
def _bare_gpr(cache=PrecomputeCacheType.TENSOR, d=3, p=2):
    post = GPRPosterior.__new__(GPRPosterior)
    post.model, post.cache, post._valid, post._stacked, post._theta = None, None, True, None, None
    post._precompute_cache, post._nlf, post._shape, post._nb = cache, 0, (10, p, d), 32
    return post


def _bare_svgp(d=3, p=2):
    post = SVGPPosterior.__new__(SVGPPosterior)
    post.model, post.cache, post._valid, post._state, post._jitter = None, None, True, None, 1e-6
    post._precompute_cache, post._shape, post._nb = PrecomputeCacheType.TENSOR, (8, p, p, d, False), 32
    return post


def _host_models(d=3, p=2):
    rng = np.random.default_rng(8)
    X = np.hstack([rng.random((12, d)), (np.arange(12)[:, None] % 2) * 1.0])
    Y = rng.standard_normal((12, p))
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(d))
    return [M.MultiFidelityGPModel(X, Y, kern(), kern()),
            M.GraphMultiFidelityGPModel(X, Y, [kern()], kern()),
            M.SingleBinSVGP(X, Y, kern(), kern(), p, Z=np.zeros((5, d + 1))),
            M.LatentMFCoregionalizationSVGP(X, Y, kern(), kern(), num_latents=2, num_inducing=5, num_outputs=p,
                                            w_type='diagonal')]


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def test_argument_checks_come_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    Xs = np.zeros((4, 4))
    for obj in [_bare_gpr(), _bare_svgp()] + _host_models():
        name = type(obj).__name__
        bad = [
            dict(num_samples=0), dict(num_samples=-2), dict(num_samples=2.0), dict(num_samples=True),
            dict(num_samples="3"),
            dict(num_samples=3, eps=np.zeros((2, 4, 2))),     # S disagrees with num_samples
            dict(num_samples=3, eps=np.zeros((3, 5, 2))),     # N*
            dict(num_samples=3, eps=np.zeros((3, 4, 1))),     # P
            dict(num_samples=3, eps=np.zeros((4, 2))),        # one draw's shape with num_samples given
            dict(eps=np.zeros((1, 4, 2))),                    # [S, N*, P] with num_samples=None
            dict(eps=np.zeros((4, 3))),
            dict(eps=[[0.0, 0.0]]),                           # a list of the wrong shape
            dict(num_samples=2, jitter=-1e-9), dict(jitter=float("nan")), dict(jitter="1e-6"),
            dict(num_samples=2, full_cov=False, eps=np.zeros((2, 4, 3))),
        ]
        for kw in bad:
            with pytest.raises(ValueError, match="predict_f_samples"):
                obj.predict_f_samples(Xs, **kw)
        with pytest.raises(ValueError, match="predict_f_samples"):
            obj.predict_f_samples(np.zeros(4), 2)             # Xnew is not 2-D
        with pytest.raises(NotImplementedError, match="both"):
            obj.predict_f_samples(Xs, 2, full_cov=True, full_output_cov=True)
        with pytest.raises(NotImplementedError, match="not built"):
            obj.predict_f_samples(Xs, 2, full_cov=False, full_output_cov=True)
        for kw in (dict(num_samples=2), dict(), dict(num_samples=2, full_cov=False),
                   dict(num_samples=np.int64(2), eps=np.zeros((2, 4, 2)), jitter=0)):
            with pytest.raises(AssertionError, match="device was touched"):   # good arguments reach the device
                obj.predict_f_samples(Xs, **kw)
        print(f"{name}: ok")


def test_float32_model_and_nocache(monkeypatch):
    _no_device(monkeypatch)
    d = 3
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(d))
    X = np.hstack([np.random.default_rng(9).random((6, d)), np.zeros((6, 1))])
    m32 = M.MultiFidelityGPModel(X, X[:, :2], kern(), kern(), dtype="float32")
    with pytest.raises(NotImplementedError, match="float32"):
        m32.predict_f_samples(np.zeros((4, 4)), 2)

    class Model:
        def predict_f_samples(self, *a, **k):
            return ("model", a, k)
    post = _bare_gpr(PrecomputeCacheType.NOCACHE)
    post.model = Model()
    eps = np.zeros((2, 4, 2))
    tag, a, k = post.predict_f_samples(np.zeros((4, 4)), 2, eps=eps, jitter=1e-7)
    assert tag == "model" and a[1:] == (2, True, False) and k["eps"] is eps and k["jitter"] == 1e-7
