"""Simulation design from the cached GPR posterior, the parts that need no GPU: the closed form the
device evaluates against one refit per candidate (tests/_design_oracle.py), and the argument checks of
``GPRPosterior.variance_reduction`` / ``select``, which must all come before the device is touched."""
import numpy as np
import pytest
import torch

import _design_oracle as DO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import engine as E
from multi_fidelity_gpflow_amd.posteriors import GPRPosterior, PrecomputeCacheType


@pytest.mark.parametrize("which", ["n25", "n25s", "n79", "n180"])
def test_closed_form_is_the_refit(which):
    """The identity: cov(f_r, f_c)^2 / (var f_c + s2) summed with the weights equals the drop of the
    references' variance after a refit with the candidate appended, to 1e-12 |ref|max."""
    X, Y, prm, Xref, Xcand, w = DO.case(which)
    ref = DO.brute(X, Y, prm, Xref, Xcand, w)
    got = DO.reference(which)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{which}: closed form vs refit {err:.1e} (|ref|max {scale:.3g})")
    assert got.shape == (Xcand.shape[0],) and scale > 0
    assert err <= 1e-12 * scale, (which, err)
    if which == "n79":   # the fidelity-0.5 candidate scores exactly 0 (the refit: up to its other factorization)
        assert got[7] == 0.0 and abs(ref[7]) <= 1e-12 * scale
        w0 = w.copy()
        w0[9] = 0.0      # the fidelity-0.5 reference adds exactly 0: its weight does not matter
        np.testing.assert_array_equal(DO.closed(X, Y, prm, Xref, Xcand, w0), got)


def test_graph_closed_form_is_the_refit():
    """The graph kernel with a symmetric rho_LF (any row order reads the same K): closed form against refits."""
    from test_gpu_graph import _data, _model, _oracle_params
    m, D = 2, 3
    X, Y = _data(m, D)
    mod = _model(X, Y, m, D, asym=False)
    prm, s2 = _oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    Xref, Xcand, w = DO.graph_points(m, D)
    ref, got = DO.brute(X, Y, prm, Xref, Xcand, w, noise=s2), DO.closed(X, Y, prm, Xref, Xcand, w, noise=s2)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"graph: closed form vs refit {err:.1e} (|ref|max {scale:.3g})")
    assert err <= 1e-10 * scale   # a tenth of the GPU bound (cond(K + s2 I) ~ 1e5 at noise 1e-3)
    assert got[4] == 0.0


def test_greedy_margins():
    """The select tests' condition, on the oracle side: every step's best score / cost leads the second
    best by a relative margin >= 1e-6, so a pick cannot hinge on the last bits."""
    for which in ("n25s", "n79", "n180"):
        picks, gain, margin = DO.greedy_reference(which)
        print(f"{which}: picks {picks.tolist()} gain {gain} margins {margin}")
        assert picks.shape == (4,) and np.all(margin >= 1e-6) and np.all(gain > 0)


def _bare_posterior(cache=PrecomputeCacheType.TENSOR, d=3):
    """A GPRPosterior with the fields the argument checks read and no device block."""
    post = GPRPosterior.__new__(GPRPosterior)
    post.model, post.cache, post._valid = None, None, True
    post._precompute_cache, post._nlf, post._shape, post._nb = cache, 0, (10, 2, d), 32
    return post


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def test_value_errors_come_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    post = _bare_posterior()
    Xc, Xr = np.zeros((5, 4)), np.zeros((3, 4))
    bad_calls = [
        (lambda: post.variance_reduction(np.zeros((5, 3)), Xr), r"Xcand has shape \(5, 3\)"),
        (lambda: post.variance_reduction(Xc, np.zeros((3, 5))), r"Xref has shape \(3, 5\)"),
        (lambda: post.variance_reduction(Xc, np.zeros(4)), "Xref has shape"),
        (lambda: post.variance_reduction(Xc, Xr, weights=[1.0, -1e-300, 1.0]), "non-negative"),
        (lambda: post.variance_reduction(Xc, Xr, weights=[1.0, np.nan, 1.0]), "non-negative"),
        (lambda: post.variance_reduction(Xc, Xr, weights=np.ones(5)), r"weights has shape \(5,\)"),
        (lambda: post.variance_reduction(Xc, Xr, weights=np.ones((3, 1))), "weights has shape"),
        (lambda: post.select(Xc, Xr, 2, weights=torch.tensor([1.0, 1.0, -1.0])), "non-negative"),
        (lambda: post.select(Xc, Xr, 2, cost=[1, 1, 0, 1, 1]), "positive"),
        (lambda: post.select(Xc, Xr, 2, cost=[1, 1, -4, 1, 1]), "positive"),
        (lambda: post.select(Xc, Xr, 2, cost=np.ones(3)), r"cost has shape \(3,\)"),
        (lambda: post.select(Xc, Xr, 0), "q must be"),
        (lambda: post.select(Xc, Xr, 33), "q must be"),
        (lambda: post.select(Xc, Xr, 2.0), "q must be"),
        (lambda: post.select(np.zeros((0, 4)), Xr, 1), "no candidate"),
        (lambda: post.select(np.zeros((5, 3)), Xr, 1), "Xcand has shape"),
    ]
    for call, match in bad_calls:
        with pytest.raises(ValueError, match=match):
            call()
    # well-formed arguments do reach the device (zero weights and 32 picks are legal)
    for call in (lambda: post.variance_reduction(Xc, Xr, weights=np.zeros(3)),
                 lambda: post.select(Xc, Xr, 32, cost=np.full(5, 0.5)),
                 lambda: post.variance_reduction(np.zeros((0, 4)), Xr)):
        with pytest.raises(AssertionError, match="device was touched"):
            call()


def test_nocache_and_surface(monkeypatch):
    _no_device(monkeypatch)
    post = _bare_posterior(PrecomputeCacheType.NOCACHE)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        post.variance_reduction(np.zeros((5, 4)), np.zeros((3, 4)))
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        post.select(np.zeros((5, 4)), np.zeros((3, 4)), 2)
    assert M.DesignResult._fields == ("picks", "gain")
    assert not hasattr(M.SVGPPosterior, "variance_reduction") and not hasattr(M.SVGPPosterior, "select")
