"""Conditioning the cached GPR posterior on new rows, host side: the block-append identity the device
evaluates against the oracle's own predict functions on the stacked data, and the argument checks of
``GPRPosterior.condition_on`` that need no device.  No GPU."""
import numpy as np
import pytest
import scipy.linalg as sla

import _condition_oracle as CO
from multi_fidelity_gpflow_amd import engine as E
from multi_fidelity_gpflow_amd import posteriors as PS
from multi_fidelity_gpflow_amd.posteriors import GPRPosterior, PrecomputeCacheType

IDENTITY = 1e-12


def _close(name, got, ref, slack=0.0):
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{name}: err {err:.1e} |ref|max {scale:.3g} (reference's own error {slack:.1e})")
    assert err <= IDENTITY * max(1.0, scale) + slack, (name, err, scale, slack)


def _identity(name, X, Y, prm, Xadd, Yadd, Xs, s2, mean_slack=0.0):
    Xst, Yst = np.vstack([X, Xadd]), np.vstack([Y, Yadd])
    Ky = CO.stacked_Ky(Xst, prm, s2)
    cond = np.linalg.cond(Ky)
    print(f"{name}: cond(K_y) {cond:.2e}")
    assert cond < 1e6
    Lo, Zo, _ = CO.append(Ky, X.shape[0], Y, Yadd)
    mean, var, cov = CO.predict_from(Lo, Zo, Xst, Xs, prm)
    rmean, rvar, rcov = CO.stacked(Xst, Yst, Xs, prm, s2)
    if mean_slack:   # the oracle's mean against the same mean by cho_solve from the same matrix
        alt = CO.kernel(Xst, Xs, prm).T @ sla.cho_solve((np.linalg.cholesky(Ky), True), Yst)
        mean_slack *= float(np.abs(alt - rmean).max())
    _close(name + " mean", mean, rmean, mean_slack)
    _close(name + " var", var, rvar)
    _close(name + " cov", cov, rcov)
    return Ky, Lo, Zo


@pytest.mark.parametrize("which,k", [("n25", 1), ("n25", 7), ("n25", 8), ("n79", 32), ("n180", 17), ("hbs", 3)])
def test_append_identity(which, k):
    """L'^{-1} and Z' of the block append predict what the oracle predicts from the stacked data, to
    1e-12 max(1, |ref|max), at cond(K_y) < 1e6."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case(which, k)
    Ky, Lo, Zo = _identity(f"{which}+{k}", X, Y, prm, Xadd, Yadd, Xs, float(prm.noise))
    np.testing.assert_allclose(Lo @ Ky @ Lo.T, np.eye(Ky.shape[0]), rtol=0, atol=1e-9)   # L'^{-1} is the inverse factor


def test_fantasy_identity():
    """Rows observed at the posterior's own mean: zero rows of Z', the unstacked mean, the refit's variance."""
    X, Y, prm, Xadd, _, Xs = CO.case("n79", 32)
    Xst = np.vstack([X, Xadd])
    Ky = CO.stacked_Ky(Xst, prm, float(prm.noise))
    Lo, Zo, mean_add = CO.append(Ky, X.shape[0], Y)
    assert not Zo[X.shape[0]:].any()
    mean, var, _ = CO.predict_from(Lo, Zo, Xst, Xs, prm)
    _close("fantasy mean vs unstacked", mean, CO.stacked(X, Y, Xs, prm)[0])
    _close("fantasy var vs stacked", var, CO.reference("n79", 32)[1])
    _close("fantasy targets", mean_add, CO.stacked(X, Y, Xadd, prm)[0])


@pytest.mark.parametrize("asym", [True, False])
def test_graph_append_identity(asym):
    """The graph kernel at m = 2: the cross block is the lower triangle of graph_K(vstack, vstack), i.e.
    the NEW row is the row argument.  With the asymmetric rho_LF of the graph tests the other argument
    order is another model.  There the factorization of the sorted training rows reads rho_LF[1, 0] only;
    a row of source 0 appended BELOW the source-1 rows reads rho_LF[0, 1] against them, and the stacked
    matrix is then indefinite (asserted: the oracle itself cannot factor it), so the asymmetric case
    appends sources 1 and 2 (HF); the symmetric one cycles 0, 1, 2.

    Bound: 1e-12 max(1, |ref|max) for the variance and the covariance.  The graph tests' model has noise
    1e-3 (cond(K_y) 4.7e4), where the oracle's mean is itself only good to a few 1e-12: recomputed by
    cho_solve from the same matrix it moves by 2e-12 .. 5e-12 (|ref|max 2.8).  The mean is therefore
    held to 1e-12 max(1, |ref|max) plus twice that measured deviation of the reference from itself."""
    from test_gpu_graph import _data, _model, _oracle_params
    m, D = 2, 3
    X, Y = _data(m, D)
    mod = _model(X, Y, m, D, asym=asym)
    prm, s2 = _oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    Xadd, Yadd, Xs = CO.graph_rows(m, D, Y.shape[1], 9, sources=(1, 2) if asym else None)
    Ky, _, _ = _identity(f"graph asym={asym} +9", X, Y, prm, Xadd, Yadd, Xs, s2, mean_slack=2.0)
    if asym:
        n = X.shape[0]
        wrong = CO.kernel(X, Xadd, prm).T   # predict_f's argument order
        assert np.abs(wrong - Ky[n:, :n]).max() > 1e-3
        X0 = CO.graph_rows(m, D, Y.shape[1], 3)[0]   # sources 0, 1, 2
        assert np.linalg.eigvalsh(CO.stacked_Ky(np.vstack([X, X0]), prm, s2))[0] < -1e-3


# ---------------------------------------------------------------- argument checks, no device
def _bare_posterior(cache=PrecomputeCacheType.TENSOR, d=3, p=2):
    """A GPRPosterior with the fields the argument checks read and no device block."""
    post = GPRPosterior.__new__(GPRPosterior)
    post.model, post.cache, post._valid, post._stacked, post._theta = None, None, True, None, None
    post._precompute_cache, post._nlf, post._shape, post._nb = cache, 0, (10, p, d), 32
    return post


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def test_value_errors_come_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    assert PS.MAX_APPEND == 32
    post = _bare_posterior()
    bad_calls = [
        (np.zeros((3, 3)), None),                # D + 1 = 4 columns expected
        (np.zeros(4), None),                     # not 2-D
        (np.zeros((0, 4)), None),                # k = 0
        (np.zeros((33, 4)), None),               # k > 32
        (np.zeros((3, 4)), np.zeros((2, 2))),    # Yadd rows
        (np.zeros((3, 4)), np.zeros((3, 1))),    # Yadd columns
        (np.zeros((3, 4)), np.zeros(3)),         # [k] only when P = 1
        ([[0.0, 0.0, 0.0]], None),               # a list
    ]
    for Xadd, Yadd in bad_calls:
        with pytest.raises(ValueError, match="condition_on"):
            post.condition_on(Xadd, Yadd)
    with pytest.raises(ValueError, match="condition_on"):
        post.fantasize(np.zeros((33, 4)))
    with pytest.raises(AssertionError, match="device was touched"):   # good arguments do reach the device
        _bare_posterior(p=1).condition_on(np.zeros((3, 4)), np.zeros(3))


def test_nocache_and_conditioned_surface(monkeypatch):
    _no_device(monkeypatch)
    post = _bare_posterior(PrecomputeCacheType.NOCACHE)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        post.condition_on(np.zeros((3, 4)), np.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        post.fantasize(np.zeros((3, 4)))
    cond = _bare_posterior()
    cond._stacked = (None, None, None)   # what marks a conditioned posterior
    with pytest.raises(NotImplementedError, match="conditioned"):
        cond.fused_predict_f(np.zeros((2, 4)))
