"""fp64 torch-CPU restatement of the HeteroscedasticGaussian likelihood -- TEST HELPER.

mfgpflow/linear_svgp.py:243-267 on top of oracle.svgp_oracle (which is pinned by the notebook
KAT and may not change): the same latent moments, mixing and KL as ``elbo_t``; only the
variational expectations differ.  Per observation (n, c) the noise variance is

    v[n, c] = noise + U[n, c]**2          (the code squares Y_unc; its docstring does not)
    VE = sum -1/2 log 2 pi - 1/2 log v - 1/2 ((Y - f_mu)**2 + f_var) / v

With U = 0 this is ``elbo_t`` (tests/test_het_host.py ties the two to 1e-14).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import svgp_oracle as S
from oracle.mfgp_oracle import softplus_inverse


def het_elbo_t(X, Y, U, Z, kps, q_mu, q_sqrt, W, noise, num_data=None):
    """(ELBO, KL, VE) of GPflow SVGP.elbo (whiten=True) under HeteroscedasticGaussian.
    Y, U: [N, P] observations and uncertainties; noise: fp64 tensor, shape () or (1,)."""
    if not (torch.is_tensor(noise) and noise.dtype == torch.float64):
        raise TypeError("het_elbo_t: noise must be a float64 tensor")
    gm, gv = S.latent_moments(X, Z, kps, q_mu, q_sqrt)
    if W is not None:
        fm, fv = gm @ W.T, gv @ (W * W).T
    else:
        fm, fv = gm, gv
    v = noise + U ** 2
    ve = (-0.5 * S.LOG2PI - 0.5 * torch.log(v) - 0.5 * ((Y - fm) ** 2 + fv) / v).sum()
    Lq = torch.tril(q_sqrt)
    M, L = q_mu.shape
    kl = 0.5 * ((q_mu ** 2).sum() - M * L + (Lq ** 2).sum()
                - torch.log(torch.diagonal(Lq, dim1=-2, dim2=-1) ** 2).sum())
    scale = (num_data / X.shape[0]) if num_data else 1.0
    return ve * scale - kl, kl, ve


class HetLatentTrainer(S.LatentTrainer):
    """LatentMFCoregionalizationSVGP(heterosed=True).optimize restated with torch autograd: targets
    [Y_obs | Y_unc] of shape [N, 2P]; the noise variable is softplus_inverse(1.0) under a PLAIN
    Softplus (gpflow.utilities.positive(), no Shift(1e-6)), shape (1,), trainable from step 0."""

    def __init__(self, X, Y2, kw, lr=0.005, max_iters=10000, kl_multiplier=1.0):
        P = kw["num_outputs"]
        Y2 = np.asarray(Y2, dtype=np.float64)
        assert Y2.shape[1] == 2 * P
        super().__init__(X, Y2[:, :P], kw, lr=lr, max_iters=max_iters, kl_multiplier=kl_multiplier)
        self.U = torch.tensor(Y2[:, P:], dtype=torch.float64)
        self.vars["noise"] = torch.full((1,), float(softplus_inverse(1.0)), dtype=torch.float64, requires_grad=True)
        self.m = {k: torch.zeros_like(v) for k, v in self.vars.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.vars.items()}

    def noise(self):
        return S.tf_softplus_t(self.vars["noise"])

    def neg_elbo(self):
        Z, kps, q_mu, q_sqrt, _ = self.constrained()
        e, kl, _ = het_elbo_t(self.X, self.Y, self.U, Z, kps, q_mu, q_sqrt, self.vars["W"], self.noise(),
                              num_data=self.X.shape[0])
        return -e + (self.klm - 1.0) * kl


def synthetic_uncertainties(shape, seed):
    """Y_unc ~ U[0.05, 0.5], about a fifth of the entries exactly 0 (there v is the baseline);
    the draws differ between rows and between columns."""
    rng = np.random.default_rng(seed)
    U = rng.uniform(0.05, 0.5, size=shape)
    U[rng.random(shape) < 0.2] = 0.0
    return U
