"""numpy restatement of the batched Gaussian log-density of include/mfgp.h ``mfgp_mvn_logpdf`` and of
``posterior.log_density`` / ``predict_log_density`` (tests/test_logdens_host.py, tests/test_gpu_logdens.py).

Per row s, with Sigma_s = obs_cov + diag(var_s + obs_var_s) and r = y_s - mean_s:

    logp_s     = -1/2 r^T Sigma_s^{-1} r - 1/2 log det Sigma_s - (P / 2) log 2 pi
    gmean_s    = a = Sigma_s^{-1} r                       (d logp / d mean)
    gvar_s[c]  = 1/2 (a_c^2 - (Sigma_s^{-1})_cc)          (d logp / d var_s[c])

Diagonal form (no obs_cov): a NaN target is a missing output, no term and zero gradients.
"""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))
BOUND = 1e-9   # the GPU tests' bound: BOUND * max(1, |ref|max), logp / gmean / gvar each


def lower_sym(C):
    C = np.asarray(C, dtype=np.float64)
    return np.tril(C) + np.tril(C, -1).T


def dense_row(mean, y, var, obs_var, obs_cov):
    """One row of the dense form: mean, y, var (a scalar broadcasts), obs_var (or None) [P]; obs_cov [P, P]
    (its lower triangle is read) -> (logp, gmean [P], gvar [P])."""
    p = mean.shape[0]
    d = np.broadcast_to(np.asarray(var, dtype=np.float64), (p,)).copy()
    if obs_var is not None:
        d = d + obs_var
    S = lower_sym(obs_cov) + np.diag(d)
    L = np.linalg.cholesky(S)
    r = y - mean
    z = np.linalg.solve(L, r)
    Li = np.linalg.solve(L, np.eye(p))
    a = Li.T @ z
    logp = -0.5 * (z @ z) - np.log(np.diag(L)).sum() - 0.5 * p * LOG2PI
    return logp, a, 0.5 * (a * a - (Li * Li).sum(axis=0))


def diag_row(mean, y, var, obs_var):
    """One row of the diagonal form; NaN targets are left out."""
    p = mean.shape[0]
    v = np.broadcast_to(np.asarray(var, dtype=np.float64), (p,)).copy()
    if obs_var is not None:
        v = v + obs_var
    ok = ~np.isnan(y)
    r = np.where(ok, y - mean, 0.0)
    a = np.where(ok, r / v, 0.0)
    logp = -0.5 * np.sum(np.where(ok, r * r / v + np.log(v) + LOG2PI, 0.0))
    return logp, a, np.where(ok, 0.5 * (a * a - 1.0 / v), 0.0)


def logpdf(mean, Y, var, obs_var=None, obs_cov=None):
    """mean [ns, p]; Y [p] or [ns, p]; var [ns] (one per row) or [ns, p]; obs_var None / scalar / [p] /
    [ns, p]; obs_cov None / [p, p] -> (logp [ns], gmean [ns, p], gvar [ns, p])."""
    mean = np.asarray(mean, dtype=np.float64)
    ns, p = mean.shape
    Y = np.broadcast_to(np.asarray(Y, dtype=np.float64), (ns, p))
    var = np.asarray(var, dtype=np.float64)
    var = np.broadcast_to(var[:, None] if var.ndim == 1 else var, (ns, p))
    ov = None if obs_var is None else np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (ns, p))
    logp, gm, gv = np.empty(ns), np.empty((ns, p)), np.empty((ns, p))
    for s in range(ns):
        o = None if ov is None else ov[s]
        if obs_cov is None:
            logp[s], gm[s], gv[s] = diag_row(mean[s], Y[s], var[s], o)
        else:
            logp[s], gm[s], gv[s] = dense_row(mean[s], Y[s], var[s], o, obs_cov)
    return logp, gm, gv


def emulate_abi(ns, p, mean, ldm, Y, y_rs, var, var_rs, var_cs, obs_var, ov_rs, obs_cov, ldc, ldgm, ldgv):
    """mfgp_mvn_logpdf on flat host arrays, element by element through the header's strides (y_rs = 0: one
    shared vector; var_cs = 0: one variance per row; ov_rs = 0: shared; only obs_cov's lower triangle is
    looked at).  Returns (logp [ns], gmean flat [ns * ldgm], gvar flat [ns * ldgv]), padding NaN."""
    logp = np.empty(ns)
    gm, gv = np.full((ns * ldgm,), np.nan), np.full((ns * ldgv,), np.nan)
    C = None
    if obs_cov is not None:
        C = np.array([[obs_cov[i * ldc + j] if j <= i else np.nan for j in range(p)] for i in range(p)])
    for s in range(ns):
        m = np.array([mean[s * ldm + c] for c in range(p)])
        y = np.array([Y[s * y_rs + c] for c in range(p)])
        v = np.array([var[s * var_rs + c * var_cs] for c in range(p)])
        o = None if obs_var is None else np.array([obs_var[s * ov_rs + c] for c in range(p)])
        logp[s], a, g = diag_row(m, y, v, o) if C is None else dense_row(m, y, v, o, C)
        gm[s * ldgm:s * ldgm + p] = a
        gv[s * ldgv:s * ldgv + p] = g
    return logp, gm, gv


def torch_reference(mean, Y, var, obs_var=None, obs_cov=None):
    """The same quantities from torch autograd on the textbook expression (dense form only)."""
    import torch
    m = torch.tensor(np.asarray(mean, dtype=np.float64), requires_grad=True)
    ns, p = m.shape
    v = np.asarray(var, dtype=np.float64)
    v = torch.tensor(np.broadcast_to(v[:, None] if v.ndim == 1 else v, (ns, p)).copy(), requires_grad=True)
    y = torch.tensor(np.broadcast_to(np.asarray(Y, dtype=np.float64), (ns, p)).copy())
    d = v if obs_var is None else v + torch.tensor(np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (ns, p)).copy())
    S = torch.tensor(lower_sym(obs_cov))[None] + torch.diag_embed(d)
    L = torch.linalg.cholesky(S)
    r = (y - m)[..., None]
    quad = (r * torch.cholesky_solve(r, L)).sum(dim=(1, 2))
    logp = -0.5 * quad - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(dim=1) - 0.5 * p * LOG2PI
    logp.sum().backward()
    return logp.detach().numpy(), m.grad.numpy(), v.grad.numpy()


def case(ns, p, seed, cond=1e3, per_row_y=True, var_cols=True, obs_var="row"):
    """A seeded dense case: obs_cov from _sample_oracle.spd (eigenvalues log-spaced over `cond`), mean / Y
    standard normal, var and obs_var uniform in [0.05, 0.5]."""
    from _sample_oracle import spd
    rng = np.random.default_rng(seed)
    C = spd(p, 1, seed + 1, lam_hi=1.0, lam_lo=1.0 / cond)[0]
    mean = rng.standard_normal((ns, p))
    Y = rng.standard_normal((ns, p) if per_row_y else (p,))
    var = rng.uniform(0.05, 0.5, (ns, p) if var_cols else (ns,))
    ov = {None: None, "shared": rng.uniform(0.05, 0.5, (p,)), "row": rng.uniform(0.05, 0.5, (ns, p))}[obs_var]
    return mean, Y, var, ov, C
