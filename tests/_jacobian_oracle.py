"""fp64 CPU references for the emulator Jacobian and Fisher matrix -- TEST INFRASTRUCTURE ONLY.

The Jacobian ``J[s, c, k] = d mean[s, c] / d Xnew[s, k]`` (the D input columns; the fidelity column is detached
by the oracle's kernel and has no slot) three independent ways:

  autograd_*(form="chol" / "solve")  torch.autograd.functional.jacobian through tests/_input_grad_oracle's
          gpr_loss_fn / svgp_loss_fn (the Cholesky and the solve form), the per-row diagonal taken;
  closed_*                           the numpy closed form the kernels implement: alpha = K^{-1} Y (SVGP:
          Lm^{-T} q_mu per latent) against dK / dx.

and the Fisher matrix ``F[s] = J_s^T (diag(var_s + obs_var_s) + obs_cov)^{-1} J_s`` by numpy's solve.
tests/test_jacobian_host.py holds the three to a tenth of the GPU tests' bounds on every case built here; the
cases and the bounds are tests/_input_grad_oracle's (BOUND max(1, |ref|max), Goku GOKU_BOUND |ref|max), the
Fisher bound BOUND max(1, |F|max) with obs_cov from _sample_oracle.spd at cond 1e3, as the log-density tests
take theirs.  Every reference is computed once (lru_cache) and shared."""
import functools

import numpy as np
import torch

import _input_grad_oracle as G
from _input_grad_oracle import BOUND, GOKU_BOUND, GPR_CASES, SVGP_CASE  # noqa: F401  (the shared cases / bounds)
from oracle import mfgp_oracle as O

ROW_BLOCK = 8   # rows of Xnew per autograd.functional.jacobian call (its output is [b, P, b, D + 1])


def autograd_jacobian(fn, Xs):
    """[N*, P, D] from fn: Xs tensor -> (mean [N*, P], var): the full Jacobian of a block of rows, then its
    per-row diagonal (a row's mean depends on that row alone), the fidelity column dropped."""
    Xs = np.asarray(Xs, dtype=np.float64)
    out = []
    for s0 in range(0, Xs.shape[0], ROW_BLOCK):
        Xt = torch.tensor(Xs[s0:s0 + ROW_BLOCK])
        full = torch.autograd.functional.jacobian(lambda x: fn(x)[0], Xt, vectorize=True)   # [b, P, b, D + 1]
        b = Xt.shape[0]
        out.append(full[torch.arange(b), :, torch.arange(b), :-1].numpy())
    return np.concatenate(out) if out else np.zeros((0, 0, Xs.shape[1] - 1))


def _dk_terms(X, Xs, vL, lL, vD, lD, rho):
    """wL [N, N*] = cL vL kL and wD [N, N*] = cD vD kD, the two terms of the kernel entry (cL = 1 | rho | rho^2,
    cD = 1 for HF x HF; zero for a fidelity that is neither 0 nor 1), and diff [N, N*, D] = x_i - xs_s."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    diff = X[:, None, :-1] - Xs[None, :, :-1]
    kL = vL * np.exp(-0.5 * ((diff / lL) ** 2).sum(-1))
    kD = vD * np.exp(-0.5 * ((diff / lD) ** 2).sum(-1))
    s1 = (X[:, -1] == 0) + rho * (X[:, -1] == 1)
    s2 = (Xs[:, -1] == 0) + rho * (Xs[:, -1] == 1)
    hh = np.outer(X[:, -1] == 1, Xs[:, -1] == 1)
    return np.outer(s1, s2) * kL, hh * kD, diff


def _contract(alpha, wL, wD, diff, lL, lD):
    """J[s, c, k] = sum_i alpha[i, c] (wL[i, s] / lL_k^2 + wD[i, s] / lD_k^2) diff[i, s, k]"""
    G_ = (wL[:, :, None] / lL ** 2 + wD[:, :, None] / lD ** 2) * diff      # [N, N*, D]
    return np.einsum("ic,isk->sck", alpha, G_)


def closed_gpr(X, Y, Xs, p: O.MFParams):
    """The numpy closed form of the GPR Jacobian, [N*, P, D]."""
    Ky = O.mf_K(X, None, p) + p.noise * np.eye(X.shape[0])
    alpha = np.linalg.solve(Ky, np.asarray(Y, dtype=np.float64))
    lL, lD = np.asarray(p.lL, dtype=np.float64), np.asarray(p.lD, dtype=np.float64)
    wL, wD, diff = _dk_terms(X, Xs, p.vL, lL, p.vD, lD, p.rho0)
    return _contract(alpha, wL, wD, diff, lL, lD)


def closed_svgp(state, Xs):
    """The numpy closed form of the SVGP Jacobian: per latent alpha_l = Lm_l^{-T} q_mu[:, l] against dK_l / dx,
    then mixed with W in latent order (no W: a latent per output)."""
    Z, kps, q_mu, q_sqrt, W = state
    Zn, qn = Z.numpy(), q_mu.numpy()
    M = Zn.shape[0]
    dg = []
    for l, kp in enumerate(kps):
        vL, lL, vD, lD, rho = (np.asarray(kp[k].numpy(), dtype=np.float64) for k in ("vL", "lL", "vD", "lD", "rho"))
        rho = float(rho.reshape(-1)[0])
        prm = O.MFParams(float(vL), lL, float(vD), lD, np.full((1, 1), rho), 0.0)
        Lm = np.linalg.cholesky(O.mf_K(Zn, None, prm) + G.S.JITTER * np.eye(M))
        alpha = np.linalg.solve(Lm.T, qn[:, l])
        wL, wD, diff = _dk_terms(Zn, Xs, float(vL), lL, float(vD), lD, rho)
        dg.append(_contract(alpha[:, None], wL, wD, diff, lL, lD)[:, 0, :])   # [N*, D]
    dg = np.stack(dg, 1)                                                      # [N*, L, D]
    return dg if W is None else np.einsum("cl,slk->sck", W.numpy(), dg)


def fisher(J, var, obs_var=None, obs_cov=None):
    """F [N*, D, D] = J_s^T solve(Sigma_s, J_s); J [N*, P, D], var [N*, P], obs_var None / scalar / [P] /
    [N*, P], obs_cov None / [P, P]."""
    J, var = np.asarray(J, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ns, p, d = J.shape
    tot = var + (0.0 if obs_var is None else np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (ns, p)))
    out = np.empty((ns, d, d))
    for s in range(ns):
        S = np.diag(tot[s]) + (0.0 if obs_cov is None else np.asarray(obs_cov, dtype=np.float64))
        out[s] = J[s].T @ np.linalg.solve(S, J[s])
    return out


def obs_cov(p, seed):
    """[P, P] SPD with eigenvalues log-spaced over cond 1e3 (the log-density tests' obs_cov)."""
    from _sample_oracle import spd
    return spd(p, 1, seed, lam_hi=1.0, lam_lo=1e-3)[0]


def bound(ref, goku=False):
    amax = np.abs(ref).max() if np.size(ref) else 0.0
    return GOKU_BOUND * amax if goku else BOUND * max(1.0, amax)


# ---------------------------------------------------------------- the shared cases and their references
def _gpr_refs(X, Y, Xs, prm):
    fn = G.gpr_loss_fn(X, Y, prm, "chol")
    with torch.no_grad():
        mean, var = (t.numpy() for t in fn(torch.tensor(Xs)))
    return dict(X=X, Y=Y, Xs=Xs, prm=prm, mean=mean, var=var, chol=autograd_jacobian(fn, Xs))


@functools.lru_cache(maxsize=None)
def gpr_synthetic(n_lf, n_hf, P, D, nstar):
    X, Y, Xs, prm = G.gpr_synthetic(n_lf, n_hf, P, D, nstar)[:4]
    return _gpr_refs(X, Y, Xs, prm)


@functools.lru_cache(maxsize=None)
def gpr_dataset(which):
    X, Y, Xs, prm = G.gpr_dataset(which)[:4]
    return _gpr_refs(X, Y, Xs, prm)


def gpr_solve_form(case):
    return autograd_jacobian(G.gpr_loss_fn(case["X"], case["Y"], case["prm"], "solve"), case["Xs"])


@functools.lru_cache(maxsize=None)
def gpr_edge_rows():
    """test_gpr_vjp_edge_rows' construction on GPR_CASES[1]: a training row and an Xnew row of fidelity
    0.9999999999999999, two Xnew rows equal to training rows."""
    n_lf = GPR_CASES[1][0]
    X, Y, Xs, prm = G.gpr_synthetic(*GPR_CASES[1])[:4]
    X, Xs = X.copy(), Xs.copy()
    X[40, -1] = 0.9999999999999999
    Xs[5, -1] = 0.9999999999999999
    Xs[7] = X[3]
    Xs[8] = X[n_lf + 2]
    return _gpr_refs(X, Y, Xs, prm)


def svgp_refs(state, Xs):
    fn = G.svgp_loss_fn(*state, "chol")
    with torch.no_grad():
        mean, var = (t.numpy() for t in fn(torch.tensor(Xs)))
    return dict(state=state, Xs=Xs, mean=mean, var=var, chol=autograd_jacobian(fn, Xs))


def svgp_solve_form(case):
    return autograd_jacobian(G.svgp_loss_fn(*case["state"], "solve"), case["Xs"])


@functools.lru_cache(maxsize=None)
def svgp_synthetic():
    state, Xs = G.svgp_synthetic()[:2]
    return svgp_refs(state, Xs)


@functools.lru_cache(maxsize=None)
def svgp_hbs(which):
    m, Wm, Xs = G.svgp_hbs_model(which)
    return svgp_refs(G.svgp_state(m, Wm), Xs)
