"""HeteroscedasticGaussian (LatentMFCoregionalizationSVGP(heterosed=True)): the fp64 restatement
against the KAT-pinned oracle, and the host logic that runs before any device call.  No GPU."""
import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import engine as E
from multi_fidelity_gpflow_amd.svgp import _transform_code
from oracle import svgp_oracle as S

from _het_oracle import het_elbo_t, synthetic_uncertainties


def _state(rng, N, P, D, L, Mi, with_W):
    X = np.hstack([rng.random((N, D)), (rng.random((N, 1)) < 0.3).astype(float)])
    Y = rng.standard_normal((N, P))
    Z = np.hstack([rng.random((Mi, D)), (rng.random((Mi, 1)) < 0.3).astype(float)])
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)   # a python float would make an fp32 tensor
    kps = [dict(vL=t64(0.5 + rng.random()), lL=t64(0.5 + rng.random(D)), vD=t64(0.2 + rng.random()),
                lD=t64(0.5 + rng.random(D)), rho=t64(0.5 + rng.random())) for _ in range(L)]
    q_mu = torch.tensor(rng.standard_normal((Mi, L)) * 0.3)
    q_sqrt = torch.tensor(np.tril(rng.standard_normal((L, Mi, Mi)) * 0.05) + np.eye(Mi)[None] * 0.4)
    W = torch.tensor(rng.standard_normal((P, L)) * 0.4) if with_W else None
    noise = torch.tensor(0.05 + rng.random() * 0.1, dtype=torch.float64)
    return torch.tensor(X), torch.tensor(Y), torch.tensor(Z), kps, q_mu, q_sqrt, W, noise


@pytest.mark.parametrize("with_W", [True, False])
def test_het_oracle_with_zero_uncertainty_is_the_pinned_oracle(with_W):
    """het_elbo_t(U = 0) == oracle.svgp_oracle.elbo_t, value and autograd gradients, 1e-14 relative."""
    P, L = (6, 3) if with_W else (4, 4)
    res = []
    for het in (False, True):
        X, Y, Z, kps, q_mu, q_sqrt, W, noise = _state(np.random.default_rng(7), 23, P, 3, L, 9, with_W)
        leaves = [Z, q_mu, q_sqrt, noise] + ([W] if W is not None else []) + [t for kp in kps for t in kp.values()]
        for t in leaves:
            t.requires_grad_(True)
        if het:
            e, kl, ve = het_elbo_t(X, Y, torch.zeros_like(Y), Z, kps, q_mu, q_sqrt, W, noise, num_data=40)
        else:
            e, kl, ve = S.elbo_t(X, Y, Z, kps, q_mu, q_sqrt, W, noise, num_data=40)
        e.backward()
        res.append((float(e.detach()), float(kl.detach()), float(ve.detach()),
                    [t.grad.numpy().copy() for t in leaves]))
    (e0, kl0, ve0, g0), (e1, kl1, ve1, g1) = res
    for a, b in ((e0, e1), (kl0, kl1), (ve0, ve1)):
        assert abs(a - b) <= 1e-14 * abs(a), (a, b)
    for a, b in zip(g0, g1):
        assert np.abs(a - b).max() <= 1e-14 * max(np.abs(a).max(), 1e-300), (a, b)


def test_synthetic_uncertainties_vary_by_row_and_column():
    U = synthetic_uncertainties((53, 49), 3)
    assert U.min() == 0.0 and 0.1 < (U == 0).mean() < 0.3
    nz = U[U > 0]
    assert nz.min() >= 0.05 and nz.max() <= 0.5
    assert np.ptp(U, axis=0).min() > 0 and np.ptp(U, axis=1).min() > 0


def test_likelihood_transform_shape_and_export():
    lik = M.HeteroscedasticGaussian(np.array([1.0]))
    assert isinstance(lik, M.Gaussian)
    v = lik.variance
    assert v.shape == (1,) and v.trainable
    assert _transform_code(v) == 1                       # plain Softplus: positive() without a lower bound
    assert _transform_code(M.Gaussian().variance) == 2   # Shift(1e-6) o Softplus stays the Gaussian's
    np.testing.assert_array_equal(v.numpy(), [1.0])
    assert M.HeteroscedasticGaussian(0.25).variance.shape == (1,)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def _model(hbs, **kw):
    X, Y = hbs["X"], hbs["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    Y2 = np.hstack([Y, synthetic_uncertainties(Y.shape, 5)])
    m = M.LatentMFCoregionalizationSVGP(X, Y2, M.SquaredExponential(lengthscales=np.ones(D)),
                                        M.SquaredExponential(lengthscales=np.ones(D)), num_latents=3,
                                        num_inducing=8, num_outputs=P, heterosed=True, **kw)
    return m, X, Y, Y2


def test_constructor_builds_the_heteroscedastic_likelihood(hbs, monkeypatch):
    _no_device(monkeypatch)
    m, X, Y, Y2 = _model(hbs, w_type='pca')
    assert isinstance(m.likelihood, M.HeteroscedasticGaussian)
    assert m.likelihood.variance.shape == (1,) and m.likelihood.variance.trainable
    assert m.kernel.W.shape == (Y.shape[1], 3)           # the PCA initialisation saw Y_obs only
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # no NumPy size-1-array-to-scalar deprecation
        assert m._noise() == 1.0
    h = M.LatentMFCoregionalizationSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(5)),
                                        M.SquaredExponential(lengthscales=np.ones(5)), 3, 8, Y.shape[1])
    assert type(h.likelihood) is M.Gaussian and h.likelihood.variance.shape == ()


def test_poisson_is_refused(hbs, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match="NOT FULLY IMPLEMENTED"):
        _model(hbs, loss_type='poisson')


@pytest.mark.parametrize("call", ["elbo", "training_loss", "elbo_and_grad", "optimize"])
def test_targets_must_be_n_by_2p(hbs, monkeypatch, call):
    _no_device(monkeypatch)
    m, X, Y, Y2 = _model(hbs)
    P = Y.shape[1]
    for bad in (Y, Y2[:, :2 * P - 1], Y2[:, 0]):
        with pytest.raises(ValueError, match=rf"\[N, {2 * P}\]"):
            if call == "optimize":
                m.optimize((X, bad), max_iters=2)
            else:
                getattr(m, call)((X, bad))


def test_parameter_dict_round_trip(hbs, monkeypatch, tmp_path):
    _no_device(monkeypatch)
    m, X, Y, Y2 = _model(hbs)
    rng = np.random.default_rng(1)
    m.q_mu.assign(rng.standard_normal(m.q_mu.shape))
    # trained values are forward(u) of arbitrary u: inverse() alone returns to them only to an ulp
    for p in m.parameters:
        if p.transform is not None:
            p.unconstrained_variable = rng.normal(0.3, 1.0, p.shape)
    d = M.parameter_dict(m)
    assert d[".likelihood.variance"].shape == (1,)
    path = str(tmp_path / "het.pkl")
    m.save_model(path)
    k = lambda: M.SquaredExponential(lengthscales=np.ones(5))
    m2 = M.LatentMFCoregionalizationSVGP.load_model(path, X, Y2, k(), k(), 3, 8, Y.shape[1], True, True)
    assert isinstance(m2.likelihood, M.HeteroscedasticGaussian)
    d2 = M.parameter_dict(m2)
    assert d2.keys() == d.keys() and d2[".likelihood.variance"].shape == (1,)
    for k in d:   # bit for bit: a loaded model predicts what the saved one did
        np.testing.assert_array_equal(d2[k], d[k], err_msg=k)
