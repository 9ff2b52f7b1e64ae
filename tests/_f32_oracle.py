"""float32 NumPy restatement of oracle.mfgp_oracle.gpr_lml_and_grad (test infrastructure only).

It is not a bit-model of csrc/mfgp_f32.hip.  It measures what honest fp32 arithmetic costs at a
given input: the inputs rounded to float32, K in the direct-difference form in float32, a float32
Cholesky, Z, alpha, L^-1 and W = alpha alpha^T - P K^-1 in float32, the products with dK/dtheta in
float32 and only their sums in float64 (as the kernel reduces them).  The distance of its gradient
from the fp64 oracle's, per component and on the scale of the component's group, is the unit the
fp32 GPU tests bound the kernel by (tests/test_gpu_f32_edges.py), and tests/test_f32_oracle_host.py
keeps that unit small enough for the bound to mean something.

Also here, so the CPU and the GPU test see the same inputs: the cases of test_gpu_f32_edges.py."""
import functools

import numpy as np
import scipy.linalg as sla

from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from oracle import mfgp_oracle as O

F = np.float32
D = 10   # every case: the input-dimension template paths are covered elsewhere


def grad_groups(d):
    """Index groups of the gradient vector [vL, lL(d), vD, lD(d), rho0, noise] (include/mfgp.h)."""
    return {"vL": np.array([0]), "lL": np.arange(1, 1 + d), "vD": np.array([1 + d]),
            "lD": np.arange(2 + d, 2 + 2 * d), "rho0": np.array([2 + 2 * d]), "noise": np.array([3 + 2 * d])}


def gvec(g):
    return np.concatenate([[g["vL"]], g["lL"], [g["vD"]], g["lD"], [g["rho0"]], [g["noise"]]]).astype(np.float64)


def _sq_dist32(Xc, ls):
    """sum_d ((x_id - x_jd) / l_d)^2 in float32, direct-difference form."""
    a = Xc * (F(1.0) / ls.astype(F))
    r2 = np.zeros((len(a), len(a)), dtype=F)
    for d in range(a.shape[1]):
        u = a[:, d][:, None] - a[:, d][None, :]
        r2 += u * u
    return r2


def gpr_lml_and_grad_f32(X, Y, p: O.MFParams):
    """(lml, dict(vL, lL[D], vD, lD[D], rho0, noise)): the layout of O.gpr_lml_and_grad."""
    X32, Y32 = np.asarray(X).astype(F), np.asarray(Y).astype(F)
    N, P = Y32.shape
    fid, Xc = X32[:, -1], np.ascontiguousarray(X32[:, :-1])
    isL, isH = (fid == 0).astype(F), (fid == 1).astype(F)
    s, h = isL + F(p.rho0) * isH, isH
    SS, HH = np.outer(s, s), np.outer(h, h)
    SH = np.outer(h, s) + np.outer(s, h)
    eL = np.exp(F(-0.5) * _sq_dist32(Xc, np.asarray(p.lL)))
    eD = np.exp(F(-0.5) * _sq_dist32(Xc, np.asarray(p.lD)))
    kL, kD = F(p.vL) * eL, F(p.vD) * eD
    K = SS * kL + HH * kD          # rows of any other fidelity stay 0 (linear.py:67-70)
    K[np.diag_indices(N)] += F(p.noise)
    assert K.dtype == F
    L = np.linalg.cholesky(K)
    Z = sla.solve_triangular(L, Y32, lower=True)
    Linv = sla.solve_triangular(L, np.eye(N, dtype=F), lower=True)
    alpha = Linv.T @ Z
    W = alpha @ alpha.T - F(P) * (Linv.T @ Linv)
    assert L.dtype == F and Z.dtype == F and W.dtype == F
    lml = float(-0.5 * np.sum(Z * Z, dtype=np.float64) - P * np.sum(np.log(np.diag(L).astype(np.float64)))
                - 0.5 * N * P * O.LOG2PI)
    half = lambda A: 0.5 * float(np.sum(A, dtype=np.float64))
    g = {"vL": half(W * SS * eL), "vD": half(W * HH * eD), "rho0": half(W * SH * kL),
         "noise": 0.5 * float(np.sum(np.diag(W), dtype=np.float64))}
    cL, cD = W * SS * kL, W * HH * kD
    gl, gd = np.zeros(Xc.shape[1]), np.zeros(Xc.shape[1])
    for d in range(Xc.shape[1]):
        u = Xc[:, d][:, None] - Xc[:, d][None, :]
        u2 = u * u
        gl[d] = half(cL * u2) / p.lL[d] ** 3
        gd[d] = half(cD * u2) / p.lD[d] ** 3
    g["lL"], g["lD"] = gl, gd
    return lml, g


def group_scales(g64v, d):
    """s_q = max |g64| over q's group, per component."""
    s = np.empty_like(g64v)
    for idx in grad_groups(d).values():
        s[idx] = np.max(np.abs(g64v[idx]))
    return s


def restatement_cost(g32v, g64v, d):
    """c = max_q |g32_q - g64_q| / s_q."""
    return float(np.max(np.abs(g32v - g64v) / group_scales(g64v, d)))


# ---------------------------------------------------------------- the cases of test_gpu_f32_edges.py
# name -> (n_lf, n_hf, p, n*, seed)
EDGE_SHAPES = {
    "T1": (30, 10, 1, 1, 1),             # n = 40: one partial tile, p = 1, n* = 1
    "full128": (100, 28, 128, 128, 1),   # n = p = n* = 128: exactly one full tile everywhere
    "one_row": (100, 29, 129, 129, 1),   # n = p = n* = 129: a one-row second tile
    "nopad384": (300, 84, 3, 64, 1),     # n = 384 = 3 * 128: no identity-padding row
    "p257": (500, 100, 257, 130, 1),     # n = 600: T = 5, Tp = 3, a second 256-column block in k64_kmat
}
FRAC_SHAPES = {
    "frac129": (100, 29, 3, 16, 1),
    "frac600": (500, 100, 20, 16, 1),
}
PANEL_SHAPE = {"panel600": (500, 100, 20, 64, 1)}     # T = 5
SCHED_SHAPE = {"sched700": (600, 100, 8, 32, 1)}      # T = 6
ALL_CASES = {**EDGE_SHAPES, **FRAC_SHAPES, **PANEL_SHAPE, **SCHED_SHAPE}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, Y, Xt) of a case.  The fractional cases carry fidelity 0.5 on one LF and one HF training
    row (in different row tiles at n = 600) and on one test row."""
    n_lf, n_hf, p, ns, seed = ALL_CASES[name]
    X, Y, Xt, _ = synthetic_multifidelity(n_lf, n_hf, D, p, ns, seed=seed)
    if name in FRAC_SHAPES:
        X[5, -1] = 0.5
        X[n_lf + 7, -1] = 0.5
        Xt[3, -1] = 0.5
    for a in (X, Y, Xt):
        a.setflags(write=False)
    return X, Y, Xt


FRAC_TEST_ROW = 3


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The fp64 oracle's and the float32 restatement's LML and gradient of a case, computed once:
    dict(l64, g64, l32, g32, s, c) with the gradients as vectors, s the per-component group scale
    and c the restatement's cost."""
    X, Y, _ = case_data(name)
    p0 = O.MFParams.initial(D, Y.shape[1])
    l64, g64 = O.gpr_lml_and_grad(X, Y, p0)
    l32, g32 = gpr_lml_and_grad_f32(X, Y, p0)
    g64v, g32v = gvec(g64), gvec(g32)
    ref = dict(l64=l64, g64=g64v, l32=l32, g32=g32v, s=group_scales(g64v, D), c=restatement_cost(g32v, g64v, D))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
