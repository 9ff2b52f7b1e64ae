"""fp64 torch-CPU restatement of the MaskedGaussian likelihood -- TEST HELPER.

notebooks/demo: missing output.ipynb, cell 2 (MaskedGaussian._variational_expectations) on top of
oracle.svgp_oracle (which is pinned by the notebook KAT and may not change): the same latent moments,
mixing and KL as ``elbo_t``; only the variational expectations differ.  With obs = ~isnan(Y) and one
noise variance s2[c] per output (a scalar is broadcast),

    VE = sum_{obs} -1/2 log 2 pi - 1/2 log s2[c] - 1/2 ((Y - f_mu)**2 + f_var) / s2[c]

Like the notebook, Y, f_mu and f_var are filled with zeros where Y is NaN BEFORE the arithmetic and the
result is selected again afterwards, so no NaN reaches the tape: a missing entry has an exact zero
gradient.  ELBO = VE * num_data / N - KL with N the row count.  With no NaN and a scalar noise this is
``elbo_t`` (tests/test_masked_host.py ties the two).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import svgp_oracle as S
from oracle.mfgp_oracle import softplus_inverse


def masked_elbo_t(X, Y, Z, kps, q_mu, q_sqrt, W, noise, num_data=None):
    """(ELBO, KL, VE) of GPflow SVGP.elbo (whiten=True) under MaskedGaussian.
    Y: [N, P] with NaN where missing; noise: fp64 tensor, shape (), (1,) or (P,)."""
    if not (torch.is_tensor(noise) and noise.dtype == torch.float64):
        raise TypeError("masked_elbo_t: noise must be a float64 tensor")
    gm, gv = S.latent_moments(X, Z, kps, q_mu, q_sqrt)
    if W is not None:
        fm, fv = gm @ W.T, gv @ (W * W).T
    else:
        fm, fv = gm, gv
    obs = ~torch.isnan(Y)
    zero = torch.zeros_like(Y)
    Yf, fmf, fvf = torch.where(obs, Y, zero), torch.where(obs, fm, zero), torch.where(obs, fv, zero)
    s2 = noise.reshape(-1)[None, :]       # [1, 1] or [1, P]
    ve_e = -0.5 * S.LOG2PI - 0.5 * torch.log(s2) - 0.5 * ((Yf - fmf) ** 2 + fvf) / s2
    ve = torch.where(obs, ve_e, zero).sum()
    Lq = torch.tril(q_sqrt)
    M, L = q_mu.shape
    kl = 0.5 * ((q_mu ** 2).sum() - M * L + (Lq ** 2).sum()
                - torch.log(torch.diagonal(Lq, dim1=-2, dim2=-1) ** 2).sum())
    scale = (num_data / X.shape[0]) if num_data else 1.0
    return ve * scale - kl, kl, ve


class MaskedLatentTrainer(S.LatentTrainer):
    """LatentMFCoregionalizationSVGP(missing_outputs=True).optimize restated with torch autograd: Y has
    NaN where an output is missing; the noise variable has shape (P,) at softplus_inverse(1 - 1e-6)
    under Shift(1e-6) o Softplus (Gaussian's own transform: variance 1.0), trainable from step 0."""

    def __init__(self, X, Y, kw, lr=0.005, max_iters=10000, kl_multiplier=1.0):
        P = kw["num_outputs"]
        super().__init__(X, np.asarray(Y, dtype=np.float64), kw, lr=lr, max_iters=max_iters,
                         kl_multiplier=kl_multiplier)
        self.vars["noise"] = torch.full((P,), float(softplus_inverse(1.0 - 1e-6)), dtype=torch.float64,
                                        requires_grad=True)
        self.m = {k: torch.zeros_like(v) for k, v in self.vars.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.vars.items()}

    def noise(self):
        return S.tf_softplus_t(self.vars["noise"]) + 1e-6

    def neg_elbo(self):
        Z, kps, q_mu, q_sqrt, _ = self.constrained()
        e, kl, _ = masked_elbo_t(self.X, self.Y, Z, kps, q_mu, q_sqrt, self.vars["W"], self.noise(),
                                 num_data=self.X.shape[0])
        return -e + (self.klm - 1.0) * kl


def synthetic_mask(X, P, seed, scatter=0.3):
    """(missing [N, P] bool, full_row, full_col) for inputs X whose last column is the fidelity (0: LF).
    The union of
      * `scatter` of the entries, drawn independently,
      * one LF row entirely missing and one column entirely missing (both drawn),
      * the multi-fidelity block: every LF row misses the last third of the columns;
    every column but full_col keeps at least 2 observed entries: where the draws left fewer, scattered
    draws of that column (outside the full row and the block) are taken back in row order."""
    X = np.asarray(X)
    N = X.shape[0]
    rng = np.random.default_rng(seed)
    lf = X[:, -1] == 0
    scat = rng.random((N, P)) < scatter
    full_row = int(rng.choice(np.flatnonzero(lf)))
    full_col = int(rng.integers(P))
    fixed = np.zeros((N, P), bool)
    fixed[full_row, :] = True
    fixed[:, full_col] = True
    fixed[np.ix_(lf, np.arange(P) >= P - P // 3)] = True
    for c in range(P):
        if c == full_col:
            continue
        for n in np.flatnonzero(scat[:, c] & ~fixed[:, c]):
            if ((~scat[:, c]) & (~fixed[:, c])).sum() >= 2:
                break
            scat[n, c] = False
    return scat | fixed, full_row, full_col


def apply_mask(Y, missing):
    Ym = np.array(Y, dtype=np.float64, copy=True)
    Ym[missing] = np.nan
    return Ym
