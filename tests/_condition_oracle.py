"""fp64 CPU references for conditioning the cached GPR posterior on new rows -- TEST INFRASTRUCTURE ONLY.

  stacked   the oracle's own predict functions on vstack(X, Xadd), vstack(Y, Yadd)
            (oracle.mfgp_oracle.gpr_predict_f / _full_cov; graph models: oracle.graph_oracle).  What a user
            does today: a new model.  THE reference of the GPU tests.
  append    the identity the device evaluates, in numpy from one factorization of the first n rows:
            A = L^{-1} B^T, S = K(Xadd, Xadd) + s2 I - A^T A = L22 L22^T, R = L22^{-1},
            L'^{-1} = [L^{-1} 0 ; -R A^T L^{-1}  R], Z' = [Z ; R (Yadd - A^T Z)] (zeros for a fantasy),
            with the stacked kernel matrix taken as a factorization reads it (its lower triangle).

tests/test_condition_host.py holds the two to 1e-12 max(1, |ref|max).  The cases are built here once and
shared by both test files; nothing here runs the code under test.
"""
import functools

import numpy as np
import scipy.linalg as sla
import torch

import _design_oracle as DO
import _leave_out_oracle as LO
from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O

NSTAR = 40   # seeded test points of every case


def _graph(prm):
    return isinstance(prm, dict)


def kernel(X, X2, prm, jitter=False):
    """K(X, X2) with X as the row argument (graph models: with or without the kernel's own 1e-6 jitter)."""
    if _graph(prm):
        return GO.graph_K(torch.tensor(X), torch.tensor(X2), prm, jitter=jitter).numpy()
    return O.mf_K(X, X2, prm)


def stacked_Ky(Xst, prm, s2):
    """K + s2 I of the stacked rows as its Cholesky reads it: the lower triangle, mirrored."""
    K = kernel(Xst, Xst, prm, jitter=True)
    K = np.tril(K) + np.tril(K, -1).T
    K[np.diag_indices_from(K)] += s2
    return K


def append(Ky, n, Y, Yadd=None):
    """(L'^{-1}, Z', mean at the new rows) by the block identity from the factors of Ky[:n, :n]."""
    k = Ky.shape[0] - n
    L = np.linalg.cholesky(Ky[:n, :n])
    Li = sla.solve_triangular(L, np.eye(n), lower=True)
    Z = Li @ Y
    A = Li @ Ky[n:, :n].T
    R = sla.solve_triangular(np.linalg.cholesky(Ky[n:, n:] - A.T @ A), np.eye(k), lower=True)
    mean = A.T @ Z
    Lo = np.block([[Li, np.zeros((n, k))], [-R @ A.T @ Li, R]])
    Zo = np.vstack([Z, R @ (Yadd - mean) if Yadd is not None else np.zeros_like(mean)])
    return Lo, Zo, mean


def predict_from(Lo, Zo, Xst, Xs, prm):
    """(mean [N*, P], var [N*], cov [N*, N*]) of predict_f from the factors, as the cached predict forms them."""
    A = Lo @ kernel(Xst, Xs, prm)
    Kss = kernel(Xs, Xs, prm, jitter=True)
    kdiag = np.diag(kernel(Xs, Xs, prm))
    return A.T @ Zo, kdiag - np.sum(A * A, axis=0), Kss - A.T @ A


def stacked(Xst, Yst, Xs, prm, s2=None):
    """(mean, var [N*], cov [N*, N*]) of the oracle's predict_f on the stacked data."""
    if _graph(prm):
        t = torch.tensor
        mean, var = GO.predict_f(t(Xst), t(Yst), t(Xs), prm, s2)
        cov = GO.predict_f_full_cov(t(Xst), t(Yst), t(Xs), prm, s2)[1]
        return mean.numpy(), var.numpy().reshape(-1), cov.numpy()
    mean, var = O.gpr_predict_f(Xst, Yst, Xs, prm)
    return mean, var[:, 0], O.gpr_predict_f_full_cov(Xst, Yst, Xs, prm)[1][0]


@functools.lru_cache(maxsize=None)
def case(which, k):
    """(X, Y, prm, Xadd, Yadd, Xs): a leave-out case with k seeded rows to append (fidelities alternating
    from 0, seeded normal targets) and NSTAR seeded test points.  n79 + 32: Xadd[0] carries the inputs of
    training row 12 (a replicate).  hbs: HF rows only.  n64: the first 64 rows of n79 (no padding at
    either tile size)."""
    X, Y, prm = LO._data("n79" if which == "n64" else which)
    if which == "n64":
        X, Y = X[:64], Y[:64]
    D = X.shape[1] - 1
    rng = np.random.default_rng(1000 * X.shape[0] + k)
    Xadd = DO._points(rng, k, D, 0)
    if which == "hbs":
        Xadd[:, -1] = 1.0
    if which == "n79" and k == 32:
        Xadd[0, :-1] = X[12, :-1]
    Yadd = rng.standard_normal((k, Y.shape[1]))
    return X, Y, prm, Xadd, Yadd, DO._points(rng, NSTAR, D, 0)


@functools.lru_cache(maxsize=None)
def reference(which, k, fantasy=False):
    """`stacked` of one case at its test points, computed once (read-only for its users).  fantasy: the
    new rows' targets are the unstacked oracle's mean at Xadd."""
    X, Y, prm, Xadd, Yadd, Xs = case(which, k)
    if fantasy:
        Yadd = O.gpr_predict_f(X, Y, Xadd, prm)[0]
    return stacked(np.vstack([X, Xadd]), np.vstack([Y, Yadd]), Xs, prm)


def graph_rows(m, D, P, k, sources=None, seed=17):
    """k rows to append to the graph tests' data, their sources cycling through `sources` (None: 0..m), with
    seeded normal targets, and NSTAR test points of every source."""
    rng = np.random.default_rng(seed)
    src = np.arange(m + 1) if sources is None else np.asarray(sources)
    Xadd = np.hstack([rng.random((k, D)), src[np.arange(k) % len(src)][:, None].astype(np.float64)])
    Xs = np.hstack([rng.random((NSTAR, D)), (np.arange(NSTAR) % (m + 1))[:, None].astype(np.float64)])
    return Xadd, rng.standard_normal((k, P)), Xs
