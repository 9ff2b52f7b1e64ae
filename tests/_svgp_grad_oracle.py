"""Extended-precision restatement of the SVGP ELBO gradient, and the scale its error is measured on
(test infrastructure only).

svgp_grad_ref restates oracle.svgp_oracle.elbo_t (and tests/_het_oracle.het_elbo_t, tests/
_masked_oracle.masked_elbo_t) and the gradient of VE scale - kl_mult KL with respect to the
constrained parameters, in the wide format of tests/_grad_oracle.py (np.longdouble where it is wider
than double, else mpmath at 40 digits, never float64), with its hand-written Cholesky and triangular
inverse.  Whitened q(u), jitter 1e-6 on K_uu, r^2 in the direct-difference form, dK/dv = exp(-r^2/2).
Per latent, with L = chol(K_uu), A = L^-1 K_uf, S = tril(q_sqrt):

    bm_i = dE/dmu_i,  bv_i = dE/dvar_i        (the likelihood block, mixed through W)
    GA   = q_mu bm^T + 2 (-A + S S^T A) diag(bv)
    Kbar = dE/dK_uf = L^-T GA,   dE/dL = -Kbar A^T
    Sig  = dE/dK_uu = sym(L^-T Phi(L^T dE/dL) L^-1)   (Phi: lower triangle, diagonal halved)
    beta = dE/dk_diag = bv

Beside the gradient g_ref it returns each scalar component's absolute mass S_q, the same sum with
every term replaced by its modulus:

    theta_q, Z[a, d]   sum |Sig_ab dK_uu,ab| + sum |Kbar_ai dK_uf,ai| + sum |beta_i dk_diag,i|
                       (1 / l^3 applied; both arguments of K_uu counted for Z; Z summed over latents)
    q_mu[a, l]         sum_i |A_ai bm_i| + |kl_mult q_mu|
    q_sqrt[l, a, b]    sum_i |2 bv_i A_ai (S^T A)_bi| + |kl_mult S_ab| + [a = b] |kl_mult / S_aa|
    W[p, l], noise     one term per entry (i, p) of Y, in modulus

A component whose mass is 0 (the fidelity column of dZ, the unused last column of theta, a row of Z
that is neither LF nor HF, an output without observations) must be exactly 0.

case_reference(name)["c"] = max(max_q |g64_q - g_ref_q| / S_q, N 2^-53): what honest fp64 costs at
the case's input on that scale, g64 being fp64 torch autograd through the oracle.  No device code
enters it.  For the case `shift` (every coordinate + 1000) the oracle is given the inputs translated
back by exactly 1000 (the subtraction is exact in fp64 and the kernel depends on differences only, so
it is the same input): oracle.svgp_oracle.rbf_t forms r^2 = |a|^2 + |b|^2 - 2 a.b, which at
coordinates of 1000 costs 1e-9 of the mass and is the very defect the case is there to find in
k_kgrad; c_raw keeps that figure.

tests/test_svgp_grad_oracle_host.py keeps c <= 1e-11 and the restatement equal to the oracle's
algebra; tests/test_gpu_svgp_grad_components.py bounds every component of the HIP gradient by
8 c S_q."""
import functools

import numpy as np
import torch

import _grad_oracle as GR
import multi_fidelity_gpflow_amd as M
from _het_oracle import het_elbo_t, synthetic_uncertainties
from _masked_oracle import masked_elbo_t
from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from multi_fidelity_gpflow_amd.svgp import DEFAULT_JITTER
from oracle import svgp_oracle as S

FACTOR = GR.FACTOR
CAP = 1e-11
KEYS = ("Z", "theta", "q_mu", "q_sqrt", "W", "noise")
SHIFT = 1000.0
ANISO_L = 20.0


class _Float64:
    """The restatement on float64 arrays: for the algebra check and the negative controls of
    tests/test_svgp_grad_oracle_host.py only, never a reference."""
    name = "float64"
    wide = False
    exp, sqrt, log = staticmethod(np.exp), staticmethod(np.sqrt), staticmethod(np.log)

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=np.float64)

    f64 = arr


# ---------------------------------------------------------------- the cases
# name -> kind, (n_lf, n_hf), d, P, L, M, data seed, parameter seed
SHAPES = {
    "d3": ("latent", (150, 40), 3, 6, 3, 40, 43, 53),      # DC = 4; N = 190, M = 40: a ragged second 32-row tile
    "sb33": ("singlebin", (150, 40), 5, 4, 4, 33, 61, 71),  # one row past a tile; W = NULL
    "d10": ("latent", (240, 60), 10, 6, 2, 70, 62, 72),    # DC = 12; N = 300: two K_uf column blocks, 160 + 140
    "d14": ("latent", (150, 40), 14, 6, 3, 40, 54, 64),    # DC = 16, two waves per SIMD
    "d20": ("latent", (150, 40), 20, 6, 3, 40, 60, 70),    # DC = 32, one wave per SIMD
    "wide": ("latent", (150, 40), 5, 6, 2, 270, 63, 73),   # M = 270: two K_uu column blocks, M > one tile
    "shift": ("latent", (150, 40), 5, 6, 3, 40, 64, 74),   # every coordinate + 1000: the centring
    "aniso": ("latent", (150, 40), 5, 6, 3, 40, 65, 75),   # lL[0] = lD[0] = 20
    "mixed": ("latent", (150, 40), 5, 6, 3, 40, 66, 76),   # HF rows interleaved, two fractional Z rows
    "lfz": ("latent", (150, 40), 5, 6, 3, 40, 67, 77),     # every Z row LF
    "klm": ("latent", (150, 40), 3, 6, 3, 40, 43, 53),     # d3 with kl_multiplier 0.3, num_data = 3 N
    "het": ("het", (150, 40), 5, 6, 3, 40, 68, 78),        # k_ve_bwd_het, k_ve_het_reduce
    "msk": ("msk", (150, 40), 5, 6, 3, 40, 69, 79),        # k_ve_bwd_masked, k_ve_masked_nreduce
}
TILE64_CASES = ("d3", "d10", "wide")
# Lengthscales of _randomize times this factor, where c would otherwise pass the cap: cond(K_uu) is what
# sets c (through q_mu and q_sqrt, which carry L^-1 K_uf), and 40 inducing points in 3 dimensions, or 270
# in 5, at lengthscales 0.5 .. 1.5 put it at the jitter's limit (measured c: d3 1.6e-11, klm 6.8e-11,
# wide 3.2e-10 at factor 1).
LSCALE = {"d3": 0.5, "klm": 0.5, "wide": 0.4}
SNAP_Z = ("d10", "mixed")   # KMeans centres that mix fidelities (21 of 70 at d10) go to the nearer one
MIXED_FRAC_ROWS = ((5, 0.5), (20, 0.9999999999999999))
MSK_NAN, MSK_EMPTY_COL = 0.15, 2


def _spread(n, k, first):
    """k distinct positions spread over range(n)."""
    pos = first + (np.arange(k) * n) // k
    assert len(set(pos.tolist())) == k and pos.max() < n
    return pos


def _interleave(is_hf):
    """A permutation that spreads the rows for which is_hf holds evenly among the others."""
    n, k = len(is_hf), int(is_hf.sum())
    order = np.empty(n, dtype=int)
    slot = np.zeros(n, bool)
    slot[_spread(n, k, 2)] = True
    order[slot], order[~slot] = np.flatnonzero(is_hf), np.flatnonzero(~is_hf)
    return order


def _kern(d):
    return M.SquaredExponential(lengthscales=np.ones(d))


def _randomize(model, seed, W):
    """tests/test_gpu_svgp._randomize (the same draws in the same order), then a dense W and, for a
    (P,) variance, one draw per output."""
    rng = np.random.default_rng(seed)
    M_, L = model.q_mu.shape
    model.q_mu.assign(rng.standard_normal((M_, L)) * 0.3)
    model.q_sqrt.assign(np.tril(rng.standard_normal((L, M_, M_)) * 0.05) + np.eye(M_)[None] * 0.4)
    for k in model.kernel.kernels:
        D = k.kernel_L.lengthscales.shape[0]
        k.kernel_L.variance.assign(0.5 + rng.random())
        k.kernel_L.lengthscales.assign(0.5 + rng.random(D))
        k.kernel_delta.variance.assign(0.2 + rng.random())
        k.kernel_delta.lengthscales.assign(0.5 + rng.random(D))
        k.rho.assign(np.full((1, 1), 0.5 + rng.random()))
    v = model.likelihood.variance
    v.assign(0.05 + rng.random(v.shape) * 0.1)
    if W:
        P = model.kernel.W.shape[0]
        model.kernel.W.assign(rng.standard_normal((P, L)) * 0.4)   # dense, both signs


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, kind, model, X, Y (targets as elbo_and_grad takes them), Yobs, U, Z, theta [L, 2d+4],
    q_mu, q_sqrt (lower), W or None, noise (1 or P entries), kl_mult, scale) of a case.  The model is
    built on the host; the arrays are read back from it, so the oracle sees the values the device gets.
    Shared and read-only."""
    kind, (n_lf, n_hf), d, P, L, Mi, dseed, pseed = SHAPES[name]
    X, Y, _, _ = synthetic_multifidelity(n_lf, n_hf, d, P, 8, seed=dseed)
    N = X.shape[0]
    if name == "mixed":
        order = _interleave(X[:, -1] == 1)
        X, Y = np.ascontiguousarray(X[order]), np.ascontiguousarray(Y[order])
    Yobs, U, Yt = Y, None, Y
    if kind == "het":
        U = synthetic_uncertainties(Y.shape, dseed)
        Yt = np.hstack([Y, U])
    if kind == "msk":
        rng = np.random.default_rng(dseed)
        miss = rng.random(Y.shape) < MSK_NAN
        miss[:, MSK_EMPTY_COL] = True
        Yobs = Yt = np.where(miss, np.nan, Y)
    if kind == "singlebin":
        m = M.SingleBinSVGP(X, Y, _kern(d), _kern(d), P, Z=np.zeros((Mi, d + 1)))
    else:
        # the constructor's KMeans needs M <= N rows: `wide` gets its own Z below
        m = M.LatentMFCoregionalizationSVGP(X, Yt, _kern(d), _kern(d), num_latents=L, num_inducing=Mi if Mi <= N else 8,
                                            num_outputs=P, w_type='diagonal', heterosed=kind == "het",
                                            missing_outputs=kind == "msk")
    Z = m.inducing_variable.numpy().copy()   # the KMeans centres of X, fidelity column included
    if name == "wide":
        rng = np.random.default_rng(dseed + 1000)
        Z = np.hstack([rng.random((Mi, d)), (rng.random((Mi, 1)) < 0.25).astype(float)])
        m._setup(Z, np.zeros((Mi, L)), np.tile(np.eye(Mi)[None], (L, 1, 1)), m.likelihood, N)
    if name == "lfz" or name in SNAP_Z:
        Z[:, -1] = 0.0 if name == "lfz" else (Z[:, -1] >= 0.5)
    if name == "mixed":
        hf = Z[:, -1] == 1
        if hf.sum() < 8:   # at least a fifth of the inducing points on the HF side
            hf[np.argsort(Z[:, 0])[:8]] = True
            Z[:, -1] = hf
        Z = np.ascontiguousarray(Z[_interleave(Z[:, -1] == 1)])
        for row, f in MIXED_FRAC_ROWS:
            Z[row, -1] = f
    if name == "shift":
        X = X.copy()
        X[:, :-1] += SHIFT
        Z[:, :-1] += SHIFT
    m.inducing_variable.assign(Z)
    _randomize(m, pseed, W=kind != "singlebin")
    if name in LSCALE:
        for k in m.kernel.kernels:
            for kk in (k.kernel_L, k.kernel_delta):
                kk.lengthscales.assign(kk.lengthscales.numpy() * LSCALE[name])
    if name == "aniso":
        for k in m.kernel.kernels:
            for kk in (k.kernel_L, k.kernel_delta):
                l = kk.lengthscales.numpy().copy()
                l[0] = ANISO_L
                kk.lengthscales.assign(l)
    kl_mult = 0.3 if name == "klm" else 1.0
    if name == "klm":
        m.num_data = 3 * N
    theta = np.stack([k.theta_vector(d) for k in m.kernel.kernels])
    c = dict(name=name, kind=kind, model=m, X=X, Y=Yt, Yobs=Yobs, U=U, Z=m.inducing_variable.numpy().copy(),
             theta=theta, q_mu=m.q_mu.numpy().copy(), q_sqrt=np.tril(m.q_sqrt.numpy()),
             W=None if kind == "singlebin" else m.kernel.W.numpy().copy(),
             noise=np.reshape(m.likelihood.variance.numpy(), -1).astype(np.float64).copy(),
             kl_mult=kl_mult, scale=(m.num_data / N) if m.num_data else 1.0)
    assert c["Z"].shape == (Mi, d + 1) and theta.shape == (L, 2 * d + 4) and c["q_mu"].shape == (Mi, L)
    assert np.array_equal(c["Z"][:, -1], Z[:, -1])
    GR._freeze(*[a for a in c.values() if isinstance(a, np.ndarray)])
    return c


# ---------------------------------------------------------------- the restatement
def _pairs(Ac, fa, Bc, fb, th, B):
    """Kernel blocks between rows (Ac, fa) and (Bc, fb): the fidelity weights, exp(-r^2/2) of both
    kernels and the coordinate differences [D, na, nb].  Rows whose fidelity is neither 0 nor 1 are
    zero rows, as in oracle.svgp_oracle.mf_K_t."""
    D = Ac.shape[1]
    La, Ha = B.arr((fa == 0).astype(float)), B.arr((fa == 1).astype(float))
    Lb, Hb = B.arr((fb == 0).astype(float)), B.arr((fb == 1).astype(float))
    sa, sb = La + th["rho"] * Ha, Lb + th["rho"] * Hb
    diff = np.stack([Ac[:, d][:, None] - Bc[:, d][None, :] for d in range(D)])
    d2 = diff * diff
    eL = B.exp(-sum(d2[d] / (th["lL"][d] * th["lL"][d]) for d in range(D)) / 2)
    eD = B.exp(-sum(d2[d] / (th["lD"][d] * th["lD"][d]) for d in range(D)) / 2)
    return dict(ss=np.outer(sa, sb), hh=np.outer(Ha, Hb), dss=np.outer(Ha, sb) + np.outer(sa, Hb), eL=eL, eD=eD,
                kL=th["vL"] * eL, kD=th["vD"] * eD, diff=diff, d2=d2)


def _sum3(*terms):
    """(sum, sum of moduli) over every entry of every term."""
    return sum(t.sum() for t in terms), sum(np.abs(t).sum() for t in terms)


def _tril(a):
    n = a.shape[0]
    return a * np.tril(np.ones((n, n)))


def svgp_grad_ref(c, B=None, detail=False):
    """(ELBO = VE scale - KL, g = d(VE scale - kl_mult KL), S) of a case in the format B (default: the
    wide one), as elbo_and_grad returns them: the ELBO as a float and two dicts
    of float64 arrays by key, in elbo_and_grad's layout (q_sqrt [L, M, M], lower; noise [1] or [P]).
    detail: also the per-latent intermediates, in B's numbers (for the host tests' controls)."""
    B = B or GR.backend()
    X, Z = np.asarray(c["X"]), np.asarray(c["Z"])
    N, D = X.shape[0], X.shape[1] - 1
    Mi, L = c["q_mu"].shape
    fx, fz = X[:, -1], Z[:, -1]
    Xc, Zc = B.arr(X[:, :-1]), B.arr(Z[:, :-1])
    obs64 = ~np.isnan(c["Yobs"])
    P = obs64.shape[1]
    obs = B.arr(obs64.astype(float))
    Y = B.arr(np.where(obs64, c["Yobs"], 0.0))
    Wm = B.arr(np.eye(P) if c["W"] is None else c["W"])
    noise = B.arr(c["noise"])
    sig2 = B.zeros((N, P)) + (noise[None, :] if noise.shape[0] == P else noise[0])
    if c["U"] is not None:
        sig2 = sig2 + B.arr(c["U"]) * B.arr(c["U"])
    scale, klm, half = B.arr(c["scale"]), B.arr(c["kl_mult"]), B.arr(0.5)
    q_mu, q_sqrt = B.arr(c["q_mu"]), B.arr(c["q_sqrt"])
    isLx, isHx = B.arr((fx == 0).astype(float)), B.arr((fx == 1).astype(float))
    lat = []
    for l in range(L):
        t = B.arr(c["theta"][l])
        th = dict(vL=t[0], lL=t[1:1 + D], vD=t[1 + D], lD=t[2 + D:2 + 2 * D], rho=t[2 + 2 * D])
        uu, uf = _pairs(Zc, fz, Zc, fz, th, B), _pairs(Zc, fz, Xc, fx, th, B)
        Kuu = uu["ss"] * uu["kL"] + uu["hh"] * uu["kD"]
        Kuu[np.arange(Mi), np.arange(Mi)] += B.arr(DEFAULT_JITTER)
        Kuf = uf["ss"] * uf["kL"] + uf["hh"] * uf["kD"]
        Lm, Li = GR._factor(Kuu, B)
        A = Li @ Kuf
        Sq = _tril(q_sqrt[l])
        STA = Sq.T @ A
        kdiag = th["vL"] * (isLx + th["rho"] * th["rho"] * isHx) + th["vD"] * isHx
        lat.append(dict(th=th, uu=uu, uf=uf, Lm=Lm, Li=Li, A=A, Sq=Sq, STA=STA, mu=A.T @ q_mu[:, l],
                        var=kdiag - (A * A).sum(0) + (STA * STA).sum(0)))
    MU, VAR = np.stack([s["mu"] for s in lat], 1), np.stack([s["var"] for s in lat], 1)
    fm, fv = MU @ Wm.T, VAR @ (Wm * Wm).T
    res = (Y - fm) * obs
    ve = (obs * (-B.arr(S.LOG2PI) * half - B.log(sig2) * half - (res * res + fv) / sig2 * half)).sum()
    Sall = np.stack([s["Sq"] for s in lat])
    dg = np.stack([np.diagonal(s["Sq"]) for s in lat])
    kl = ((q_mu * q_mu).sum() - Mi * L + (Sall * Sall).sum() - B.log(dg * dg).sum()) * half
    elbo = ve * scale - kl      # the ELBO itself: kl_mult weighs the KL in the gradient's objective only
    bm = ((res / sig2) @ Wm) * scale              # dE/dmu   [N, L]
    bv = -((obs / sig2) @ (Wm * Wm)) * scale * half   # dE/dvar  [N, L]
    gth, Sth = B.zeros((L, 2 * D + 4)), B.zeros((L, 2 * D + 4))
    gZ, SZ = B.zeros((Mi, D + 1)), B.zeros((Mi, D + 1))
    gqm, Sqm = B.zeros((Mi, L)), B.zeros((Mi, L))
    gqs, Sqs = B.zeros((L, Mi, Mi)), B.zeros((L, Mi, Mi))
    for l, s in enumerate(lat):
        th, uu, uf, A, Li, Lm, Sq, STA = s["th"], s["uu"], s["uf"], s["A"], s["Li"], s["Lm"], s["Sq"], s["STA"]
        gmu, gvv = bm[:, l], bv[:, l]
        GA = np.outer(q_mu[:, l], gmu) + (Sq @ STA - A) * (gvv * 2)[None, :]
        Kbar = Li.T @ GA
        Ph = _tril(Lm.T @ (-(Kbar @ A.T)))
        Ph[np.arange(Mi), np.arange(Mi)] *= half
        Sg = Li.T @ Ph @ Li
        Sig = (Sg + Sg.T) * half
        s.update(Kbar=Kbar, Sig=Sig, beta=gvv)
        rho, vL = th["rho"], th["vL"]
        comp = [_sum3(Sig * uu["ss"] * uu["eL"], Kbar * uf["ss"] * uf["eL"], gvv * (isLx + rho * rho * isHx))]
        comp += [_sum3(Sig * uu["ss"] * uu["kL"] * uu["d2"][d] / th["lL"][d] ** 3,
                       Kbar * uf["ss"] * uf["kL"] * uf["d2"][d] / th["lL"][d] ** 3) for d in range(D)]
        comp += [_sum3(Sig * uu["hh"] * uu["eD"], Kbar * uf["hh"] * uf["eD"], gvv * isHx)]
        comp += [_sum3(Sig * uu["hh"] * uu["kD"] * uu["d2"][d] / th["lD"][d] ** 3,
                       Kbar * uf["hh"] * uf["kD"] * uf["d2"][d] / th["lD"][d] ** 3) for d in range(D)]
        comp += [_sum3(Sig * uu["dss"] * uu["kL"], Kbar * uf["dss"] * uf["kL"], gvv * (rho * vL * 2) * isHx)]
        for q, (gq, Sq_) in enumerate(comp):
            gth[l, q], Sth[l, q] = gq, Sq_
        for d in range(D):
            il2, id2 = 1 / (th["lL"][d] * th["lL"][d]), 1 / (th["lD"][d] * th["lD"][d])
            tuu = -(Sig + Sig.T) * uu["diff"][d] * (uu["ss"] * uu["kL"] * il2 + uu["hh"] * uu["kD"] * id2)
            tuf = -Kbar * uf["diff"][d] * (uf["ss"] * uf["kL"] * il2 + uf["hh"] * uf["kD"] * id2)
            gZ[:, d] = gZ[:, d] + tuu.sum(1) + tuf.sum(1)
            SZ[:, d] = SZ[:, d] + np.abs(tuu).sum(1) + np.abs(tuf).sum(1)
        tq = A * gmu[None, :]
        gqm[:, l] = tq.sum(1) - klm * q_mu[:, l]
        Sqm[:, l] = np.abs(tq).sum(1) + np.abs(klm * q_mu[:, l])
        Ag = A * (gvv * 2)[None, :]
        eye = np.eye(Mi)
        dinv = klm / np.diagonal(Sq)
        gqs[l] = _tril(Ag @ STA.T - klm * Sq) + eye * dinv[None, :]
        Sqs[l] = _tril(np.abs(Ag) @ np.abs(STA).T + np.abs(klm * Sq)) + eye * np.abs(dinv)[None, :]
    out = dict(Z=(gZ, SZ), theta=(gth, Sth), q_mu=(gqm, Sqm), q_sqrt=(gqs, Sqs))
    if c["W"] is not None:
        gW, SW = B.zeros((P, L)), B.zeros((P, L))
        for l in range(L):
            tw = (res * MU[:, l][:, None] - obs * Wm[:, l][None, :] * VAR[:, l][:, None]) / sig2 * scale
            gW[:, l], SW[:, l] = tw.sum(0), np.abs(tw).sum(0)
        out["W"] = (gW, SW)
    tn = obs * ((res * res + fv) / (sig2 * sig2) - 1 / sig2) * half * scale
    if noise.shape[0] == P and P > 1:
        out["noise"] = (tn.sum(0), np.abs(tn).sum(0))
    else:
        out["noise"] = (B.arr([tn.sum()]), B.arr([np.abs(tn).sum()]))
    g = {k: B.f64(v[0]) for k, v in out.items()}
    Sm = {k: B.f64(v[1]) for k, v in out.items()}
    e = float(B.f64(elbo))
    return (e, g, Sm, lat) if detail else (e, g, Sm)


# ---------------------------------------------------------------- fp64 autograd through the oracle
def _torch_state(c, X, Z):
    D = X.shape[1] - 1
    kps = [dict(vL=torch.tensor(t[0]), lL=torch.tensor(t[1:1 + D].copy()), vD=torch.tensor(t[1 + D]),
                lD=torch.tensor(t[2 + D:2 + 2 * D].copy()), rho=torch.tensor(t[2 + 2 * D])) for t in c["theta"]]
    return (torch.tensor(Z), kps, torch.tensor(c["q_mu"].copy()), torch.tensor(c["q_sqrt"].copy()),
            None if c["W"] is None else torch.tensor(c["W"].copy()),
            torch.tensor(c["noise"].copy() if c["kind"] in ("het", "msk") else float(c["noise"][0]),
                         dtype=torch.float64))


def oracle_grad64(c, translate=0.0):
    """(ELBO, g = d(VE scale - kl_mult KL)) by fp64 torch autograd through oracle.svgp_oracle.elbo_t (het_elbo_t, masked_elbo_t):
    tests/test_gpu_svgp._autograd_grads on a case's arrays.  translate: subtracted from every
    coordinate of X and Z first."""
    X, Zn = np.array(c["X"]), np.array(c["Z"])
    X[:, :-1] -= translate
    Zn[:, :-1] -= translate
    D = X.shape[1] - 1
    Z, kps, q_mu, q_sqrt, Wt, noise = _torch_state(c, X, Zn)
    leaves = [Z, q_mu, q_sqrt, noise] + ([Wt] if Wt is not None else [])
    for kp in kps:
        leaves += list(kp.values())
    for t in leaves:
        t.requires_grad_(True)
    num_data = c["scale"] * X.shape[0]
    Xt, Yt = torch.tensor(X), torch.tensor(np.array(c["Yobs"]))
    if c["kind"] == "het":
        e, kl, _ = het_elbo_t(Xt, Yt, torch.tensor(np.array(c["U"])), Z, kps, q_mu, q_sqrt, Wt, noise, num_data=num_data)
    elif c["kind"] == "msk":
        e, kl, _ = masked_elbo_t(Xt, Yt, Z, kps, q_mu, q_sqrt, Wt, noise, num_data=num_data)
    else:
        e, kl, _ = S.elbo_t(Xt, Yt, Z, kps, q_mu, q_sqrt, Wt, noise, num_data=num_data)
    obj = e - (c["kl_mult"] - 1.0) * kl
    obj.backward()
    th = np.zeros((len(kps), 2 * D + 4))
    for l, kp in enumerate(kps):
        th[l, 0] = kp["vL"].grad
        th[l, 1:1 + D] = kp["lL"].grad.numpy()
        th[l, 1 + D] = kp["vD"].grad
        th[l, 2 + D:2 + 2 * D] = kp["lD"].grad.numpy()
        th[l, 2 + 2 * D] = kp["rho"].grad
    g = dict(Z=Z.grad.numpy(), theta=th, q_mu=q_mu.grad.numpy(), q_sqrt=np.tril(q_sqrt.grad.numpy()),
             noise=noise.grad.numpy().reshape(-1))
    if Wt is not None:
        g["W"] = Wt.grad.numpy()
    return float(e.detach()), g


# ---------------------------------------------------------------- the unit and the check
def ratios(g, g_ref, Sm, unit):
    """{key: |g - g_ref| / (unit S)}; where the mass is 0 the entry is 0 if g is exactly 0, else inf."""
    out = {}
    for k, ref in g_ref.items():
        err = np.abs(np.asarray(g[k], dtype=np.float64).reshape(ref.shape) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = np.where(Sm[k] > 0, err / (unit * Sm[k]), np.where(err > 0, np.inf, 0.0))
    return out


def unit_of(g64, g_ref, Sm, n):
    """max(max_q |g64_q - g_ref_q| / S_q, n 2^-53)."""
    return max(max(float(r.max()) for r in ratios(g64, g_ref, Sm, 1.0).values()), n * 2.0 ** -53)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """dict(e_ref, g_ref, S, e64, g64, c, c_raw) of a case, computed once.  c_raw differs from c at
    `shift` alone (module docstring): the oracle at the untranslated coordinates."""
    c = case(name)
    e_ref, g_ref, Sm = svgp_grad_ref(c)
    n = c["X"].shape[0]
    e64, g64 = oracle_grad64(c, translate=SHIFT if name == "shift" else 0.0)
    unit = unit_of(g64, g_ref, Sm, n)
    raw = unit_of(oracle_grad64(c)[1], g_ref, Sm, n) if name == "shift" else unit
    for d in (g_ref, Sm, g64):
        GR._freeze(*d.values())
    return dict(e_ref=e_ref, g_ref=g_ref, S=Sm, e64=e64, g64=g64, c=unit, c_raw=raw)


def old_gate(g, ref):
    """The SVGP tests' older gate per key: max |g - ref| / max |ref| (test_gpu_svgp._check_grads)."""
    return {k: float(np.abs(np.asarray(g[k]).reshape(r.shape) - r).max() / max(np.abs(r).max(), 1e-30))
            for k, r in ref.items()}


def component_report(name, elbo, g, tag=""):
    """Prints the largest |g_q - g_ref_q| / (c S_q) per key and returns ({key: largest}, ELBO rel)."""
    ref = case_reference(name)
    r = {k: float(v.max()) for k, v in ratios(g, ref["g_ref"], ref["S"], ref["c"]).items()}
    erel = abs(elbo - ref["e_ref"]) / abs(ref["e_ref"])
    print(f"{name}{tag}: c {ref['c']:.2e}; largest |g - g_ref| / (c S) per key "
          + ", ".join(f"{k} {v:.2f}" for k, v in r.items())
          + "; of max |g| " + ", ".join(f"{k} {v:.1e}" for k, v in old_gate(g, ref["g_ref"]).items())
          + f"; ELBO rel {erel:.1e}")
    return r, erel


def check_components(name, elbo, g, tag="", keys=None):
    """Every component of every key within 8 c S_q of the wide gradient, the fidelity column of dZ
    exactly 0, the ELBO within 1e-13 relative of the wide value."""
    ref = case_reference(name)
    assert set(g) >= set(ref["g_ref"]), (sorted(g), sorted(ref["g_ref"]))
    for k, r in ref["g_ref"].items():
        assert np.asarray(g[k]).size == r.size and np.all(np.isfinite(np.asarray(g[k]))), k
    r, erel = component_report(name, elbo, g, tag)
    assert np.all(np.asarray(g["Z"]).reshape(ref["g_ref"]["Z"].shape)[:, -1] == 0.0)
    assert erel <= 1e-13, (name, tag, erel)
    bad = {k: v for k, v in r.items() if v > FACTOR and (keys is None or k in keys)}
    assert not bad, f"{name}{tag}: components beyond {FACTOR:g} c S_q: {bad}"
    return r
