"""fp64 CPU references for leave-group-out cross-validation -- TEST INFRASTRUCTURE ONLY.

  brute         for every group S: the oracle's own predict_f(full_cov=True) of a model built WITHOUT the rows
                of S, asked at those rows' inputs (oracle.mfgp_oracle.gpr_predict_f_full_cov; graph models:
                oracle.graph_oracle.predict_f_full_cov), and the joint Gaussian log density of y_S under that
                prediction with the likelihood variance added back.  One Gram, one factorization and one
                predict per group: what a user does today.  THE reference of the GPU tests.
  closed_numpy  the closed form the device evaluates, in numpy from one factorization of K_y = K + s2 I:
                C = L^{-1}[:, S], G = C^T C, H = C^T L^{-1} Y, E = G^{-1} H, mean = Y_S - E,
                Sigma_f = G^{-1} - s2 I, log p = -1/2 H^T G^{-1} H + 1/2 log det G - |S| / 2 log 2 pi.

tests/test_leave_out_host.py holds the two to 1e-12 max(1, |ref|) (the identity); the deviation between
them is also what bounds the GPU tests' log density (see tests/test_gpu_leave_out.py).  The cases are built
here once and shared by both files; nothing here runs the code under test.
"""
import functools
import math

import numpy as np
import scipy.linalg as sla
import torch

from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O

LOG2PI = math.log(2.0 * math.pi)


def _lists(groups):
    return [np.sort(np.asarray(g, dtype=np.int64).reshape(-1)) for g in groups]


def lists_from_labels(labels):
    """Index lists of a label array: equal labels >= 0, in order of first appearance (-1: left in)."""
    first, out = {}, []
    for i, lab in enumerate(np.asarray(labels).tolist()):
        if lab < 0:
            continue
        if lab not in first:
            first[lab] = len(out)
            out.append([])
        out[first[lab]].append(i)
    return [np.array(g, dtype=np.int64) for g in out]


def _assemble(groups, means, covs, dens, P):
    gmax = max(len(g) for g in groups)
    cov = np.zeros((len(groups), gmax, gmax))
    for k, c in enumerate(covs):
        cov[k, :c.shape[0], :c.shape[0]] = c
    var = np.concatenate([np.diag(c) for c in covs])
    return dict(rows=np.concatenate(groups), group=np.repeat(np.arange(len(groups)), [len(g) for g in groups]),
                mean=np.vstack(means), var=np.tile(var[:, None], (1, P)), log_density=np.vstack(dens), cov=cov)


def _mvn_logpdf(y, mean, cov):
    """Per output column c: log N(y[:, c] | mean[:, c], cov)."""
    L = np.linalg.cholesky(cov)
    w = sla.solve_triangular(L, y - mean, lower=True)
    return -0.5 * np.sum(w * w, axis=0) - np.sum(np.log(np.diag(L))) - 0.5 * y.shape[0] * LOG2PI


def graph_refit_valid(X, m):
    """Rows of a graph-kernel training set at which the oracle's predict_f of a refit is the held-out
    prediction of the joint model even when rho_LF is not symmetric: LF source 0 and the HF rows.
    The graph kernel takes the LF-LF entry K(a, b) from the ROW source's kernel and rho_LF[sa, sb]
    (graph.py:61-63), and the factorization reads the lower triangle.  The training rows come source
    after source, so for a held-out row of LF source j >= 1 the refit's K(X_kept, x) holds
    rho_LF[i, j] (i < j) where the joint's lower triangle holds rho_LF[j, i]: another model, whose
    variance at a training input can even be negative.  Source 0 (every other LF row is below it)
    and HF (rho_LF does not enter) columns are the lower triangle's."""
    f = np.asarray(X)[:, -1]
    return (f == 0.0) | (f == float(m))


def brute_joint(X, Y, prm, groups, noise):
    """Refit per group of the graph model AS ITS FACTORIZATION DEFINES IT: the joint covariance is the
    lower triangle of graph_K mirrored (what a Cholesky reads) + s2 I; for each group one factorization
    of the kept block and the Gaussian conditional of the left-out rows.  Equal to `brute` wherever
    graph_refit_valid holds (tests/test_gpu_leave_out.py checks that), and defined for every row."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    groups = _lists(groups)
    s2 = float(noise)
    Xt = torch.tensor(X)
    K = GO.graph_K(Xt, Xt, prm).numpy()
    K = np.tril(K) + np.tril(K, -1).T
    means, covs, dens = [], [], []
    for S in groups:
        keep = np.setdiff1d(np.arange(X.shape[0]), S)
        Lk = np.linalg.cholesky(K[np.ix_(keep, keep)] + s2 * np.eye(len(keep)))
        A = sla.solve_triangular(Lk, K[np.ix_(keep, S)], lower=True)
        m = A.T @ sla.solve_triangular(Lk, Y[keep], lower=True)
        c = K[np.ix_(S, S)] - A.T @ A
        means.append(m)
        covs.append(c)
        dens.append(_mvn_logpdf(Y[S], m, c + s2 * np.eye(len(S))))
    return _assemble(groups, means, covs, dens, Y.shape[1])


def brute(X, Y, prm, groups, noise=None):
    """Refit per group.  prm: O.MFParams (its own noise), or the graph oracle's dict with `noise`."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    groups = _lists(groups)
    graph = isinstance(prm, dict)
    s2 = float(noise) if graph else float(prm.noise)
    means, covs, dens = [], [], []
    for S in groups:
        keep = np.setdiff1d(np.arange(X.shape[0]), S)
        if graph:
            m, c = GO.predict_f_full_cov(torch.tensor(X[keep]), torch.tensor(Y[keep]), torch.tensor(X[S]), prm, s2)
            m, c = m.numpy(), c.numpy()
        else:
            m, c = O.gpr_predict_f_full_cov(X[keep], Y[keep], X[S], prm)
            c = c[0]
        means.append(m)
        covs.append(c)
        dens.append(_mvn_logpdf(Y[S], m, c + s2 * np.eye(len(S))))
    return _assemble(groups, means, covs, dens, Y.shape[1])


def closed_numpy(X, Y, prm, groups, noise=None):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    groups = _lists(groups)
    if isinstance(prm, dict):
        s2 = float(noise)
        Xt = torch.tensor(X)
        K = GO.graph_K(Xt, Xt, prm).numpy()   # the kernel's own 1e-6 jitter is part of K
    else:
        s2 = float(prm.noise)
        K = O.mf_K(X, None, prm)
    K[np.diag_indices_from(K)] += s2
    L = np.linalg.cholesky(K)
    Li = sla.solve_triangular(L, np.eye(X.shape[0]), lower=True)
    Z = Li @ Y
    means, covs, dens = [], [], []
    for S in groups:
        C = Li[:, S]
        G, H = C.T @ C, C.T @ Z
        Lg = np.linalg.cholesky(G)
        W = sla.solve_triangular(Lg, H, lower=True)
        E = sla.solve_triangular(Lg.T, W, lower=False)
        Gi = sla.solve_triangular(Lg.T, sla.solve_triangular(Lg, np.eye(len(S)), lower=True), lower=False)
        means.append(Y[S] - E)
        covs.append(Gi - s2 * np.eye(len(S)))
        dens.append(-0.5 * np.sum(W * W, axis=0) + np.sum(np.log(np.diag(Lg))) - 0.5 * len(S) * LOG2PI)
    return _assemble(groups, means, covs, dens, Y.shape[1])


def deviation(a, b):
    """Largest deviations (mean, var, cov, log density) of two results."""
    return {k: float(np.abs(a[k] - b[k]).max()) for k in ("mean", "var", "cov", "log_density")}


# ---------------------------------------------------------------- the shared cases
def _params(D, P, seed, noise=1e-2):
    """The posterior tests' seeded parameters (lengthscales 0.5-2) at noise 1e-2: cond(K + s2 I) < 1e6."""
    rng = np.random.default_rng(seed)
    return O.MFParams(1.0 + 0.5 * rng.random(), 0.5 + 1.5 * rng.random(D), 0.3 + rng.random(), 0.5 + rng.random(D),
                      np.full((P, 1), 0.7 + 0.6 * rng.random()), noise)


def _data(which):
    if which == "hbs":
        from conftest import HBS_DIR
        d = O.load_powerspecs(HBS_DIR)
        return d["X"], d["Y"], O.MFParams.initial(d["X"].shape[1] - 1, d["Y"].shape[1])
    if which == "n500":
        from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
        X, Y, _, _ = synthetic_multifidelity(400, 100, 3, 3, 8, seed=500)
        return X, Y, _params(3, 3, 500)
    import _input_grad_oracle as G
    shape = {"n25": (20, 5, 1, 1, 1), "n79": (70, 9, 3, 3, 33), "n180": (150, 30, 65, 32, 70)}[which]
    X, Y, _, prm = G.gpr_synthetic(*shape)[:4]
    return X, Y, prm


def _drawn(n, sizes, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, s, replace=False)) for s in sizes]


def _groups(which, n):
    """name -> index lists.  The pair groups of HBS are written out (groups_by_input is under test)."""
    singles = [np.array([i]) for i in range(n)]
    if which == "hbs":
        return {"singles": singles, "pairs": [np.array([0, 52]), np.array([9, 50]), np.array([46, 51])]}
    if which == "n25":
        return {"singles": singles}
    if which == "n79":
        # sizes 1, 2, 3, 7, 16, 32; the pair spans the first and the last row tile
        g = _drawn(n, (1, 3, 7, 16, 32), 79)
        labels = np.where(np.arange(n) < 60, np.arange(n) // 10, -1)
        labels[[3, 77]] = 6   # -1 rows between the members of a group; row 3 leaves group 0
        return {"sizes": [g[0], np.array([0, 78])] + g[1:], "labels": lists_from_labels(labels), "_labels": labels}
    if which == "n180":
        rng = np.random.default_rng(180)
        mixed = _drawn(n, (2, 5, 1, 9, 32, 3, 12, 4), 181)
        return {"singles": singles, "singles33": [np.array([i]) for i in rng.choice(n, 33, replace=False)],
                "mixed": mixed}
    if which == "n500":
        rng = np.random.default_rng(500)
        sizes = [1, 32] + list(rng.integers(1, 33, 10))
        return {"twelve": _drawn(n, sizes, 501)}
    raise KeyError(which)


@functools.lru_cache(maxsize=None)
def case(which):
    """(X, Y, prm, groups): groups maps a name to its index lists ('_labels': the label array form)."""
    X, Y, prm = _data(which)
    return X, Y, prm, _groups(which, X.shape[0])


@functools.lru_cache(maxsize=None)
def reference(which, name):
    """(brute, closed_numpy, their deviation) of one group set of one case, computed once."""
    X, Y, prm, groups = case(which)
    b, c = brute(X, Y, prm, groups[name]), closed_numpy(X, Y, prm, groups[name])
    return b, c, deviation(b, c)
