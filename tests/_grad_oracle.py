"""Extended-precision restatement of the fp64 LML gradient, and the scale its error is measured on
(test infrastructure only).

gpr_grad_ref restates oracle.mfgp_oracle.gpr_lml_and_grad, and graph_grad_ref the gradient autograd
takes through oracle.graph_oracle.lml, in np.longdouble (x87 80-bit, eps 2^-64): r^2 in the
direct-difference form, a hand-written Cholesky and triangular inverse (NumPy's linalg has no long
double), W = alpha alpha^T - P K^-1, and 1/2 sum_ab W_ab dK_ab/dtheta_q per component.  Beside the
gradient g_ref it returns each component's absolute mass

    S_q = 1/2 sum_ab |W_ab dK_ab/dtheta_q|      (for the noise: 1/2 sum_a |W_aa|)

with the 1 / l^3 factor of the lengthscale entries applied.  Every component is a heavily
cancelling sum (S_q is 1 to 1e6 times |g_q|), and S_q is the scale on which a wrong or missing
term shows, whatever the other components' sizes are.

case_reference(name)["c"] is what honest fp64 costs at a case's input on that scale,

    c = max( max_q |g64_q - g_ref_q| / S_q,  n 2^-53 )

with g64 the fp64 NumPy / torch oracle and n 2^-53 the floor of a length-n fp64 sum.  The GPU tests
(tests/test_gpu_grad_components.py) bound every component of the HIP gradient by 8 c S_q;
tests/test_grad_oracle_host.py keeps c <= 1e-11 and the restatement equal to the oracle's algebra.

For the linear kernel c is the larger of two such units.  The second one takes for g64 a float64
restatement in the HIP step schedule's order (gpr_grad_blocked64: tile Cholesky with explicit
inverses of the diagonal tiles' factors, tile partial sums, then tasks), at tile 32 and 64.  The
oracle's LAPACK factorization is up to 20 times more accurate than that in dLML/dnoise = 1/2 tr W at
the cases where the first unit sits on its floor, and the HIP step schedule missed 8 times the
first unit alone there (hfblock at tile 32: 13.0) while the flow schedule, another algorithm, kept
0.7: the noise derivative carries the factorization's rounding undamped, and which fp64
factorization is luckier varies case by case.  The graph cases keep the torch oracle's unit alone.

Where long double is no wider than double (eps >= 2^-60) the same code runs on mpmath numbers at 40
digits; where mpmath is missing too, require_wide() skips the tests.  float64 is never a stand-in.

Also here, so the CPU test, the GPU tests and the chunk worker see the same arrays: the cases."""
import functools

import numpy as np
import pytest

from _f32_oracle import grad_groups, gvec
from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from oracle import mfgp_oracle as O

LD = np.longdouble
NOISE = 1e-3
GRAPH_JITTER = 1e-6   # oracle.graph_oracle.JITTER (graph.py:96), inside K
GRAPH_ASYM = 1e-3     # rho_LF[s][t] - rho_LF[t][s] = 2e-3 where the rows are interleaved (graph_data)


# ---------------------------------------------------------------- the number formats
class _LongDouble:
    name = "np.longdouble"
    wide = bool(np.finfo(LD).eps < 2.0 ** -60)
    exp, sqrt, log = staticmethod(np.exp), staticmethod(np.sqrt), staticmethod(np.log)

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=LD)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=LD)

    @staticmethod
    def f64(a):
        return np.asarray(a, dtype=np.float64)


class _MPMath:
    """np.ndarray(dtype=object) of mpmath.mpf at 40 digits: +, -, *, /, @, abs and sum work entry by
    entry.  Slow (seconds at n = 64): the fallback of hosts whose long double is a double."""
    name = "mpmath (40 digits)"

    def __init__(self):
        import mpmath
        self.mp = mpmath
        mpmath.mp.dps = 40
        self._mpf = np.frompyfunc(lambda v: mpmath.mpf(float(v)) if not isinstance(v, mpmath.mpf) else v, 1, 1)
        self.exp = np.frompyfunc(mpmath.exp, 1, 1)
        self.sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)
        self.log = np.frompyfunc(mpmath.log, 1, 1)
        self.wide = True

    def arr(self, a):
        return np.asarray(self._mpf(np.asarray(a)), dtype=object)

    def zeros(self, shape):
        return self.arr(np.zeros(shape))

    @staticmethod
    def f64(a):
        return np.asarray(np.frompyfunc(float, 1, 1)(np.asarray(a, dtype=object)), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def backend(force=None):
    """The format the references are computed in: long double where it is wider than double, else
    mpmath at 40 digits, else None (never float64)."""
    if force != "mpmath" and _LongDouble.wide:
        return _LongDouble
    try:
        return _MPMath()
    except ImportError:
        return None


def require_wide():
    if backend() is None:
        pytest.skip("np.longdouble is no wider than float64 here (eps >= 2^-60) and mpmath does not import: "
                    "no extended-precision reference for the fp64 gradient")


# ---------------------------------------------------------------- factorization
def _factor(K, B):
    """(L, L^-1) of the symmetric positive definite K, from its lower triangle.  Column-by-column
    Cholesky and row-by-row forward substitution, vector operations inside."""
    n = K.shape[0]
    L, Li = B.zeros((n, n)), B.zeros((n, n))
    for j in range(n):
        col = K[j:, j] - (L[j:, :j] @ L[j, :j] if j else 0)
        L[j, j] = B.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    for i in range(n):
        e = B.zeros(i + 1)
        e[i] = e[i] + 1
        Li[i, :i + 1] = (e - (L[i, :i] @ Li[:i, :i + 1] if i else 0)) / L[i, i]
    return L, Li


def _weights(K, Y, B):
    """lml and W = alpha alpha^T - P K^-1."""
    n, P = Y.shape
    L, Li = _factor(K, B)
    Z = Li @ Y
    alpha = Li.T @ Z
    lml = -(Z * Z).sum() / 2 - P * B.log(np.diagonal(L)).sum() - B.arr(O.LOG2PI) * n * P / 2
    return lml, alpha @ alpha.T - P * (Li.T @ Li)


def _diff2(Xc):
    """[D, n, n] squared coordinate differences."""
    return np.stack([(Xc[:, d][:, None] - Xc[:, d][None, :]) ** 2 for d in range(Xc.shape[1])])


def _contract(W, dK):
    """(g, S) = (1/2 sum W dK, 1/2 sum |W dK|)."""
    t = W * dK
    return t.sum() / 2, np.abs(t).sum() / 2


# ---------------------------------------------------------------- linear (AR1) kernel
def gpr_grad_ref(X, Y, p: O.MFParams, B=None):
    """(lml, g_ref, S) of oracle.mfgp_oracle.gpr_lml_and_grad's quantity in extended precision, as
    float64 vectors in the layout [vL, lL(D), vD, lD(D), rho0, noise].  Rows whose fidelity is
    neither 0 nor 1 have zero rows in K (linear.py:67-70) and still carry 1/2 W_aa in the noise
    entry: K + s2 I has s2 on their diagonal."""
    B = B or backend()
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    D = X.shape[1] - 1
    f = X[:, -1]
    Xc, Yw = B.arr(X[:, :-1]), B.arr(Y)
    vL, vD, rho, s2 = B.arr(p.vL), B.arr(p.vD), B.arr(p.rho0), B.arr(p.noise)
    lL, lD = B.arr(np.asarray(p.lL)), B.arr(np.asarray(p.lD))
    isL, isH = B.arr((f == 0).astype(float)), B.arr((f == 1).astype(float))
    s, h = isL + rho * isH, isH
    SS, HH = np.outer(s, s), np.outer(h, h)
    SH = np.outer(h, s) + np.outer(s, h)
    d2 = _diff2(Xc)
    eL = B.exp(-sum(d2[d] / (lL[d] * lL[d]) for d in range(D)) / 2)
    eD = B.exp(-sum(d2[d] / (lD[d] * lD[d]) for d in range(D)) / 2)
    kL, kD = vL * eL, vD * eD
    K = SS * kL + HH * kD
    n = K.shape[0]
    K[np.arange(n), np.arange(n)] += s2
    lml, W = _weights(K, Yw, B)
    out = [_contract(W, SS * eL)]
    out += [_contract(W, SS * kL * d2[d] / lL[d] ** 3) for d in range(D)]
    out += [_contract(W, HH * eD)]
    out += [_contract(W, HH * kD * d2[d] / lD[d] ** 3) for d in range(D)]
    out += [_contract(W, SH * kL)]
    dg = np.diagonal(W)
    out += [(dg.sum() / 2, np.abs(dg).sum() / 2)]
    g, S = B.f64([o[0] for o in out]), B.f64([o[1] for o in out])
    return float(B.f64(lml)), g, S


def oracle_terms64(X, Y, p: O.MFParams):
    """The fp64 oracle's own W, exp(-r2/2) and k blocks (oracle.mfgp_oracle.gpr_lml_and_grad's lines),
    for the tests that take single terms out of its sums."""
    import scipy.linalg as sla
    X = np.asarray(X, dtype=np.float64)
    N, P = Y.shape
    K = O.mf_K(X, None, p)
    K[np.diag_indices_from(K)] += p.noise
    L = np.linalg.cholesky(K)
    Z = sla.solve_triangular(L, Y, lower=True)
    alpha = sla.solve_triangular(L.T, Z, lower=False)
    Linv = sla.solve_triangular(L, np.eye(N), lower=True)
    W = alpha @ alpha.T - P * (Linv.T @ Linv)
    Xc = X[:, :-1]
    eL, eD = O.rbf_K(Xc, Xc, 1.0, p.lL), O.rbf_K(Xc, Xc, 1.0, p.lD)
    return dict(W=W, eL=eL, eD=eD, kL=p.vL * eL, kD=p.vD * eD)


def gpr_grad_blocked64(X, Y, p: O.MFParams, nb):
    """The same gradient in float64 NumPy in the order the HIP step schedule takes (a model of its
    algorithm, not of its bits): K in the direct-difference form, padded with identity rows to T nb;
    the right-looking tile Cholesky of k_chol_step with the EXPLICIT inverse D_k of every diagonal
    tile's factor (L_ik = A_ik D_k^T, X_k = D_k R_k on R = [I | Y], R_i -= L_ik X_k); alpha = sum_k
    X_k^T Z_k; W = -P (sum_m X_mi^T X_mj - alpha_i alpha_j^T / P) tile by tile; and the contraction
    as k_grad sums it: one partial per lower nb x nb tile (mirrored tiles doubled, 1 / l^3 applied to
    the partial), then the partials in task order.  LAPACK's potrf / trtri-free solves in
    oracle.mfgp_oracle are more accurate than this on some inputs (the noise derivative, 1/2 tr W,
    carries the factorization's rounding undamped), so the unit c takes both: see case_reference."""
    import scipy.linalg as sla
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, P = Y.shape
    D = X.shape[1] - 1
    f, Xc = X[:, -1], X[:, :-1]
    isL, isH = (f == 0).astype(float), (f == 1).astype(float)
    s, h = isL + p.rho0 * isH, isH
    SS, HH, SH = np.outer(s, s), np.outer(h, h), np.outer(h, s) + np.outer(s, h)
    d2 = _diff2(Xc)
    eL = np.exp(-0.5 * sum(d2[d] * (1.0 / (p.lL[d] * p.lL[d])) for d in range(D)))
    eD = np.exp(-0.5 * sum(d2[d] * (1.0 / (p.lD[d] * p.lD[d])) for d in range(D)))
    kL, kD = p.vL * eL, p.vD * eD
    T = -(-n // nb)
    N = T * nb
    A = np.eye(N)
    A[:n, :n] = SS * kL + HH * kD
    A[np.arange(n), np.arange(n)] += p.noise
    R = np.zeros((N, N + P))
    R[:, :N] = np.eye(N)
    R[:n, N:] = Y
    Xo = np.zeros_like(R)
    sl = lambda t: slice(t * nb, (t + 1) * nb)
    for k in range(T):
        Dk = sla.solve_triangular(np.linalg.cholesky(A[sl(k), sl(k)]), np.eye(nb), lower=True)
        Xo[sl(k)] = Dk @ R[sl(k)]
        Pk = {i: A[sl(i), sl(k)] @ Dk.T for i in range(k + 1, T)}
        for i in range(k + 1, T):
            for j in range(k + 1, i + 1):
                A[sl(i), sl(j)] -= Pk[i] @ Pk[j].T
            R[sl(i)] -= Pk[i] @ Xo[sl(k)]
    Li, Z = Xo[:, :N], Xo[:, N:]
    alpha = np.zeros((N, P))
    for k in range(T):
        alpha += Li[sl(k)].T @ Z[sl(k)]
    terms = [SS * eL] + [SS * kL * d2[d] for d in range(D)] + [HH * eD] + [HH * kD * d2[d] for d in range(D)] \
        + [SH * kL, np.eye(n)]
    TT = np.zeros((len(terms), N, N))
    TT[:, :n, :n] = np.stack(terms)
    scale = np.concatenate([[1.0], 1.0 / p.lL ** 3, [1.0], 1.0 / p.lD ** 3, [1.0, 1.0]])
    g = np.zeros(len(terms))
    for i in range(T):
        for j in range(i + 1):
            acc = -alpha[sl(i)] @ alpha[sl(j)].T / P
            for m in range(i, T):
                acc = acc + Li[sl(m), sl(i)].T @ Li[sl(m), sl(j)]
            w = acc * ((0.5 if i == j else 1.0) * -P)
            g += (TT[:, sl(i), sl(j)] * w).sum(axis=(1, 2)) * scale
    return g


# ---------------------------------------------------------------- graph kernel
def graph_grad_ref(X, Y, prm, noise, B=None):
    """(lml, g_ref, S) of the gradient autograd takes through oracle.graph_oracle.lml, in the theta
    layout of include/mfgp.h: per source s = 0..m [v_s, l_s(D)], rho(m), rho_LF(m x m), noise.
    prm: NumPy v [m+1], l [m+1, D], rho [m], rhoLF [m, m].  The factorization reads K's lower
    triangle; the gradient is 1/2 sum over ALL (a, b) of W_ab dK_ab/dtheta, entry by entry, so an
    asymmetric rho_LF gets graph.py's gradient (W is symmetric, K's LF-LF block need not be)."""
    B = B or backend()
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, D = X.shape[0], X.shape[1] - 1
    m = len(prm["rho"])
    f = X[:, -1]
    Xc, Yw = B.arr(X[:, :-1]), B.arr(Y)
    v, l, rho, rlf = B.arr(prm["v"]), B.arr(prm["l"]), B.arr(prm["rho"]), B.arr(prm["rhoLF"])
    ind = [B.arr((f == s).astype(float)) for s in range(m + 1)]
    d2 = _diff2(Xc)
    e = [B.exp(-sum(d2[d] / (l[s, d] * l[s, d]) for d in range(D)) / 2) for s in range(m + 1)]
    pair = lambda a, b: np.outer(ind[a], ind[b])
    HH = pair(m, m)
    coef = []   # dK/dk_s
    for s in range(m):
        c = pair(s, s) + (pair(s, m) + pair(m, s)) * rho[s] + HH * rho[s] * rho[s]
        for t in range(m):
            if t != s:
                c = c + pair(s, t) * rlf[s, t]
        coef.append(c)
    coef.append(HH)
    K = sum(coef[s] * (v[s] * e[s]) for s in range(m + 1))
    K[np.arange(n), np.arange(n)] += B.arr(GRAPH_JITTER) + B.arr(noise)
    Ksym = np.tril(K) + np.tril(K, -1).T
    lml, W = _weights(Ksym, Yw, B)
    out = []
    for s in range(m + 1):
        out += [_contract(W, coef[s] * e[s])]
        out += [_contract(W, coef[s] * (v[s] * e[s]) * d2[d] / l[s, d] ** 3) for d in range(D)]
    out += [_contract(W, (pair(s, m) + pair(m, s) + HH * 2 * rho[s]) * (v[s] * e[s])) for s in range(m)]
    for s in range(m):
        for t in range(m):
            out += [_contract(W, pair(s, t) * (v[s] * e[s])) if s != t else (B.arr(0.0), B.arr(0.0))]
    dg = np.diagonal(W)
    out += [(dg.sum() / 2, np.abs(dg).sum() / 2)]
    g, S = B.f64([o[0] for o in out]), B.f64([o[1] for o in out])
    return float(B.f64(lml)), g, S


def graph_groups(m, d):
    """Index groups of the graph gradient vector."""
    g = {}
    for s in range(m + 1):
        g[f"v{s}"] = np.array([s * (1 + d)])
        g[f"l{s}"] = np.arange(s * (1 + d) + 1, (s + 1) * (1 + d))
    ro = (m + 1) * (1 + d)
    g["rho"] = np.arange(ro, ro + m)
    g["rhoLF"] = np.arange(ro + m, ro + m + m * m)
    g["noise"] = np.array([ro + m + m * m])
    return g


def graph_oracle_lml_grad(X, Y, prm, noise):
    """oracle.graph_oracle.lml and its autograd gradient (fp64 torch on the CPU), same layout."""
    import torch
    from oracle import graph_oracle as GO
    m = len(prm["rho"])
    t = {k: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for k, a in prm.items()}
    nz = torch.tensor(noise, dtype=torch.float64, requires_grad=True)
    lo = GO.lml(torch.tensor(np.asarray(X)), torch.tensor(np.asarray(Y)), t, nz)
    lo.backward()
    grl = t["rhoLF"].grad.numpy().ravel() if t["rhoLF"].grad is not None else np.zeros(m * m)
    go = np.concatenate([np.concatenate([[t["v"].grad[s]], t["l"].grad[s].numpy()]) for s in range(m + 1)]
                        + [t["rho"].grad.numpy(), grl, [nz.grad]])
    return float(lo.detach()), go


# ---------------------------------------------------------------- the cases
def _params(D, P, seed=0, scale=1.0):
    """test_gpu_parity._params: theta randomised around the reference's initial values."""
    rng = np.random.default_rng(seed)
    return O.MFParams(1.0 + 0.5 * rng.random() * scale, 0.5 + 1.5 * rng.random(D) * scale, 0.3 + rng.random() * scale,
                      0.5 + rng.random(D) * scale, np.full((P, 1), 0.7 + 0.6 * rng.random() * scale), NOISE)


MIXED_N, MIXED_FRAC_ROW, MIXED_NEAR_ONE_ROW = 130, 7, 100   # tile 0, and tile 3 at NB = 32 (tile 1 at NB = 64)

# name -> (n_lf, n_hf, p, D, seed); the fidelity edits of "mixed" and "tinyfrac" are in case_data
LINEAR_SHAPES = {
    "t1": (15, 5, 1, 1, 1),           # n = 20: one partial tile, nq = 2
    "full64": (44, 20, 32, 15, 2),    # n = 64: no padded row; D = 15: the last fully prefetched at NB = 32
    "onerow": (45, 20, 33, 16, 3),    # n = 65: a one-row third tile, Tp = 2; D = 16: the first remainder entry
    "d32": (70, 27, 3, 32, 4),        # n = 97: MAXD, three passes of the remainder loop, 64 il2 entries
    "hfblock": (40, 70, 5, 5, 5),     # n = 110: tiles of HF rows only
    "mixed": (87, 43, 49, 5, 6),      # n = 130: every third row HF, two fractional rows
    "d7": (44, 20, 3, 7, 7),          # NB = 64: the last fully prefetched D
    "d8": (45, 20, 3, 8, 8),          # NB = 64: the first remainder entry, a one-row second tile
    "d32_64": (100, 29, 2, 32, 9),    # NB = 64: n = 129, a one-row third tile at MAXD
    "tiny64": (40, 24, 64, 16, 10),   # k_gpr_tiny: n = p = 64, TINY_MAXD
    "tinyfrac": (50, 3, 49, 5, 11),   # k_gpr_tiny: the HBS shape with one 0.5-fidelity row
    "chunk64": (120, 40, 33, 10, 12),  # n = 160: T = 3 at NB = 64 (the m-chunk cases)
    "t6": (125, 40, 3, 4, 13),        # n = 165: T = 6 at NB = 32, where chunk 3 leaves a 3-item task without alpha rows
}
NB32_CASES = ("t1", "full64", "onerow", "d32", "hfblock", "mixed")
NB64_CASES = ("d7", "d8", "d32_64", "mixed")
TINY_CASES = ("t1", "tiny64", "tinyfrac")
CHUNK_CASES = (("mixed", 32), ("t6", 32), ("chunk64", 64))   # (case, tile)
CHUNKS = (1, 2, 3, 24, 2048)
TINYFRAC_ROW = 9


def chunk_task_items(T, Tp, chunk):
    """{(m-chunk index, item count)} over k_grad's tasks (csrc/mfgp_kernels.hip grad_decode): row i
    splits its m-tiles i..T-1 into chunks of `chunk`; chunk 0 also carries the Tp alpha items."""
    items = set()
    for i in range(T):
        for ch in range(-(-(T - i) // chunk)):
            m0 = i + ch * chunk
            items.add((ch, min(T, m0 + chunk) - m0 + (Tp if ch == 0 else 0)))
    return items

# name -> (m, sizes per source, p, D, interleaved, seed)
GRAPH_SHAPES = {
    "g1": (1, (45, 20), 3, 16, False, 21),        # n = 65, one LF source (the linear model + 1e-6 I), sorted
    "g2": (2, (33, 32, 32), 4, 8, True, 22),      # n = 97, source = row mod 3, asymmetric rho_LF
}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, Y, p) of a linear-kernel case; the arrays are shared and read-only."""
    n_lf, n_hf, P, D, seed = LINEAR_SHAPES[name]
    X, Y, _, _ = synthetic_multifidelity(n_lf, n_hf, D, P, 1, seed=seed)
    if name == "mixed":
        n = n_lf + n_hf
        assert n == MIXED_N
        hf = np.arange(n) % 3 == 2
        assert hf.sum() == n_hf
        src = np.empty(n, dtype=int)
        src[~hf], src[hf] = np.arange(n_lf), n_lf + np.arange(n_hf)
        X, Y = X[src], Y[src]
        X[MIXED_FRAC_ROW, -1] = 0.5
        X[MIXED_NEAR_ONE_ROW, -1] = 0.9999999999999999
    if name == "tinyfrac":
        X[TINYFRAC_ROW, -1] = 0.5
    p = _params(D, P, seed=seed)
    X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
    _freeze(X, Y, p.lL, p.lD, p.rho)
    return X, Y, p


def theta_vector(p: O.MFParams):
    """[vL, lL(D), vD, lD(D), rho0, noise]: the theta layout of include/mfgp.h."""
    return np.concatenate([[p.vL], p.lL, [p.vD], p.lD, [p.rho0], [p.noise]])


def _unit(g64, g_ref, S, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(S > 0, np.abs(g64 - g_ref) / S, 0.0)
    return max(float(rel.max()), n * 2.0 ** -53), rel


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """dict(l_ref, g_ref, S, l64, g64, rel, c, c_oracle, c_blocked, theta) of a linear-kernel case,
    computed once.  c is the larger of two units: the fp64 oracle's (LAPACK factorization, whole-matrix
    sums) and that of the fp64 restatement in the HIP path's order (gpr_grad_blocked64, at either
    tile size), both floored at n 2^-53."""
    X, Y, p = case_data(name)
    l_ref, g_ref, S = gpr_grad_ref(X, Y, p)
    l64, g = O.gpr_lml_and_grad(X, Y, p)
    g64 = gvec(g)
    c_oracle, rel = _unit(g64, g_ref, S, X.shape[0])
    c_blocked = {nb: _unit(gpr_grad_blocked64(X, Y, p, nb), g_ref, S, X.shape[0])[0] for nb in (32, 64)}
    c = max(c_oracle, *c_blocked.values())
    ref = dict(l_ref=l_ref, g_ref=g_ref, S=S, l64=l64, g64=g64, rel=rel, c=c, c_oracle=c_oracle,
               c_blocked=c_blocked, theta=theta_vector(p))
    _freeze(*[a for a in ref.values() if isinstance(a, np.ndarray)])
    return ref


def case_unit(name):
    """c = max(max_q |g64_q - g_ref_q| / S_q, n 2^-53): what honest fp64 costs at this input."""
    return (graph_reference if name in GRAPH_SHAPES else case_reference)(name)["c"]


def case_groups(name):
    if name in GRAPH_SHAPES:
        return graph_groups(GRAPH_SHAPES[name][0], GRAPH_SHAPES[name][3])
    return grad_groups(LINEAR_SHAPES[name][3])


@functools.lru_cache(maxsize=None)
def fractional_noise_share(name):
    """1/2 sum W_aa over the rows of a case whose fidelity is neither 0 nor 1 (fp64 oracle)."""
    X, Y, p = case_data(name)
    rows = np.nonzero((X[:, -1] != 0) & (X[:, -1] != 1))[0]
    W = oracle_terms64(X, Y, p)["W"]
    return rows, 0.5 * float(W[rows, rows].sum())


@functools.lru_cache(maxsize=None)
def graph_data(name):
    """(X, Y, prm, theta) of a graph-kernel case: test_gpu_graph_paths' recipe (weights / sqrt(D),
    lengthscales scaled by sqrt(D / 3), the LF sources sharing one kernel, rho_LF in 0.2-0.5)."""
    m, sizes, P, D, interleaved, seed = GRAPH_SHAPES[name]
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((D, P)) / np.sqrt(D)
    Xs, Ys = [], []
    for s, n in enumerate(sizes):
        x = rng.uniform(0, 1, (n, D))
        Xs.append(np.hstack([x, np.full((n, 1), float(s))]))
        Ys.append(np.sin(3 * x @ w) * (1 + 0.3 * s) + 0.05 * rng.standard_normal((n, P)))
    X, Y = np.vstack(Xs), np.vstack(Ys)
    if interleaved:   # row r holds source r mod (m + 1)
        n = len(X)
        order = np.empty(n, dtype=int)
        start = np.concatenate([[0], np.cumsum(sizes)])
        for s in range(m + 1):
            rows = np.arange(s, n, m + 1)
            assert len(rows) == sizes[s]
            order[rows] = start[s] + np.arange(sizes[s])
        X, Y = X[order], Y[order]
        assert np.array_equal(X[:, -1], np.arange(n) % (m + 1))
    scale = np.sqrt(D / 3.0)
    lsh, vsh = (0.5 + rng.random(D)) * scale, 0.5 + rng.random()
    prm = dict(v=np.array([vsh] * m + [0.2 + 0.3 * rng.random()]),
               l=np.vstack([lsh] * m + [(0.5 + rng.random(D)) * scale]),
               rho=0.6 + rng.random(m), rhoLF=0.2 + 0.3 * rng.random((m, m)))
    if interleaved:
        # The lower triangle of an interleaved K reads both rho_LF[s][t] and rho_LF[t][s]; the
        # matrix it defines stays positive definite at noise 1e-3 only while the two differ by about
        # noise / n_LF (measured: smallest eigenvalue 1.6e-3 at a difference of 2e-3, -0.04 at 2e-2).
        # 2e-3 is 1e8 times what the bound resolves, so a swapped index still shows.
        r = 0.5 * (prm["rhoLF"] + prm["rhoLF"].T)
        prm["rhoLF"] = r + GRAPH_ASYM * (np.triu(np.ones((m, m)), 1) - np.tril(np.ones((m, m)), -1))
    theta = np.concatenate([np.concatenate([[prm["v"][s]], prm["l"][s]]) for s in range(m + 1)]
                           + [prm["rho"], prm["rhoLF"].ravel(), [NOISE]])
    X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
    _freeze(X, Y, theta, *prm.values())
    return X, Y, prm, theta


@functools.lru_cache(maxsize=None)
def graph_reference(name):
    """As case_reference, with oracle.graph_oracle's autograd gradient as g64."""
    X, Y, prm, theta = graph_data(name)
    l_ref, g_ref, S = graph_grad_ref(X, Y, prm, NOISE)
    l64, g64 = graph_oracle_lml_grad(X, Y, prm, NOISE)
    c, rel = _unit(g64, g_ref, S, X.shape[0])
    ref = dict(l_ref=l_ref, g_ref=g_ref, S=S, l64=l64, g64=g64, rel=rel, c=c, theta=theta)
    _freeze(*[a for a in ref.values() if isinstance(a, np.ndarray)])
    return ref


# ---------------------------------------------------------------- the GPU tests' one check
FACTOR = 8.0   # test_gpu_f32_edges.FACTOR: the project's allowance for another summation order


def component_report(name, lml, g, tag=""):
    """Prints the achieved |g_q - g_ref_q| / (c S_q) per group and returns (ratio, lml_rel, old)."""
    ref = (graph_reference if name in GRAPH_SHAPES else case_reference)(name)
    err = np.abs(np.asarray(g) - ref["g_ref"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref["S"] > 0, err / (ref["c"] * ref["S"]), np.where(err > 0, np.inf, 0.0))
    lrel = abs(lml - ref["l_ref"]) / abs(ref["l_ref"])
    old = float(err.max() / np.abs(ref["g64"]).max())
    print(f"{name}{tag}: c {ref['c']:.2e}; |g - g_ref| / (c S) per group "
          + ", ".join(f"{k} {ratio[idx].max():.2f}" for k, idx in case_groups(name).items())
          + f"; of max |g| {old:.2e}; LML rel {lrel:.2e}")
    return ratio, lrel, old


def check_components(name, lml, g, tag=""):
    """Every component within 8 c S_q of the extended-precision gradient, LML rel <= 1e-11, and the
    project's older bound (1e-8 of the largest component) alongside."""
    g = np.asarray(g)
    ratio, lrel, old = component_report(name, lml, g, tag)
    assert g.shape == ratio.shape and np.all(np.isfinite(g))
    assert lrel <= 1e-11, (name, tag, lrel)
    assert old <= 1e-8, (name, tag, old)
    bad = {k: float(ratio[idx].max()) for k, idx in case_groups(name).items() if ratio[idx].max() > FACTOR}
    assert not bad, f"{name}{tag}: components beyond {FACTOR:g} c S_q: {bad}"
    return float(ratio.max())
