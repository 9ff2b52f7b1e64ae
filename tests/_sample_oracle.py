"""numpy restatement of GPflow 2.9 ``GPModel.predict_f_samples`` / ``conditionals.util.sample_mvn`` and the
case builders of the sampling tests (tests/test_sample_host.py, tests/test_gpu_sample.py).

    full_cov=True:   mean [N, P], cov [P, N, N]
                     L_p = cholesky(cov_p + jitter I)      (lower factor of the LOWER triangle, as TF)
                     sample[s, :, p] = mean[:, p] + L_p @ eps[s, :, p]
    full_cov=False:  sample = mean + sqrt(var) * eps       (no jitter, no clamp of var)
    result [S, N, P]; with num_samples=None one draw [N, P]
"""
import numpy as np

JITTER = 1e-6   # gpflow.default_jitter()


def lower_sym(C):
    """The symmetric matrix whose lower triangle is C's (what a lower Cholesky reads); batched."""
    C = np.asarray(C, dtype=np.float64)
    lo = np.tril(C)
    return lo + np.swapaxes(np.tril(C, -1), -1, -2)


def chol_lower(C, jitter=JITTER):
    """cholesky(C + jitter I) from the lower triangle of C ([..., N, N])."""
    A = lower_sym(C)
    n = A.shape[-1]
    return np.linalg.cholesky(A + jitter * np.eye(n))


def sample_mvn(mean, cov, eps, full_cov=True, jitter=JITTER):
    """mean [N, P]; cov [P, N, N] (full_cov) or var [N, P]; eps [S, N, P] -> [S, N, P]."""
    mean, eps = np.asarray(mean, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    if not full_cov:
        return mean[None] + np.sqrt(np.asarray(cov, dtype=np.float64))[None] * eps
    L = chol_lower(cov, jitter)                        # [P, N, N]
    return mean[None] + np.einsum("pij,sjp->sip", L, eps)


def predict_f_samples(mean, cov, eps, num_samples=None, full_cov=True, full_output_cov=False, jitter=JITTER):
    """GPModel.predict_f_samples on given moments: eps [S, N, P], or [N, P] with num_samples=None."""
    if full_cov and full_output_cov:
        raise NotImplementedError("The combination of both `full_cov` and `full_output_cov` is not permitted.")
    if full_output_cov:
        raise NotImplementedError("full_output_cov")
    eps = np.asarray(eps, dtype=np.float64)
    if num_samples is None:
        return sample_mvn(mean, cov, eps[None], full_cov, jitter)[0]
    assert eps.shape[0] == num_samples
    return sample_mvn(mean, cov, eps, full_cov, jitter)


# ---------------------------------------------------------------- cases
def spd(n, batch, seed, lam_hi=1e1, lam_lo=1e-2, zeros=0):
    """[batch, n, n] of Q diag(lambda) Q^T, lambda log-spaced in [lam_lo, lam_hi] (the last `zeros` of them
    exactly 0: a posterior-like singular matrix), Q a seeded random orthogonal matrix."""
    rng = np.random.default_rng(seed)
    out = np.empty((batch, n, n))
    for b in range(batch):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = np.logspace(np.log10(lam_hi), np.log10(lam_lo), n) if n > 1 else np.array([lam_hi])
        if zeros:
            lam[n - min(zeros, n - 1):] = 0.0
        S = (Q * lam) @ Q.T
        out[b] = 0.5 * (S + S.T)
    return out


def identity_eps(n, width):
    """eps [n, n, width] with eps[s, j, c] = delta_sj: draw s is column s of every factor."""
    return np.ascontiguousarray(np.broadcast_to(np.eye(n)[:, :, None], (n, n, width)))


def factors_from_identity_draws(out, mean):
    """out [n, n, W] of identity draws -> L [W, n, n] (L_c[i][s] = out[s, i, c] - mean[i, c])."""
    return np.transpose(out - mean[None], (2, 1, 0))


# ---------------------------------------------------------------- addressing of the C ABI (pure numpy)
def emulate_abi(n, batch, nsamp, ncol, cov, ldc, sC, jitter, mean, mean_rs, mean_bs, eps, rs, ss, bs, out_size):
    """mfgp_mvn_sample on flat host arrays, element by element through the header's strides."""
    out = np.full((out_size,), np.nan)
    for b in range(batch):
        C = np.array([[cov[b * sC + i * ldc + j] if j <= i else np.nan for j in range(n)] for i in range(n)])
        L = chol_lower(C, jitter)
        for s in range(nsamp):
            for i in range(n):
                for c in range(ncol):
                    acc = 0.0
                    for j in range(i + 1):
                        acc += L[i, j] * eps[b * bs + s * ss + j * rs + c]
                    out[b * bs + s * ss + i * rs + c] = mean[b * mean_bs + i * mean_rs + c] + acc
    return out
