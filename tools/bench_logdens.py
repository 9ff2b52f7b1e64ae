"""Per-call time of the emulator log-likelihood with its input gradient: ``post.log_density(Xnew, y, obs_cov=C,
grad=True)`` (mfgp_*_posterior_logdens) against the formulation a user writes without it through unchanged API
on the same device: ``post.predict_f`` of an Xnew that requires grad, ``torch.linalg.cholesky`` of the
[N*, P, P] covariances, ``torch.cholesky_solve`` and ``.backward()``.

  GPR   MultiFidelityGPModel posterior at Goku (N = 1164, P = 64): 64 and 1024 walkers, dense obs_cov
  SVGP  LatentMFCoregionalizationSVGP posterior at Goku (L = 15, M = 300, P = 64): the same

Variants (every input already on the device):
  log_density  value and gradient from the fused call (its one host read, of info, included)
  torch        the autograd formulation (torch.linalg.cholesky's own info check included)
  density      the density launch alone, Engine.mvn_logpdf with gradients on a given mean / var
  predict_f    one cached predict_f call, for scale

Method (tools/bench_posterior.py's, windows and medians as tools/bench_posterior_grad.py): every case and
variant is warmed first; a window is a host clock around `--calls` calls that ends in a device synchronise;
the variants alternate window by window in this one process; `--windows` windows per variant, reported as
median with min / max.  The torch route is unchanged code, so its figure is also the previous commit's.
Prints one JSON line and writes it to profiles/logdens/bench.json.  GPU box: python tools/bench_logdens.py
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import multi_fidelity_gpflow_amd as M   # noqa: E402
from multi_fidelity_gpflow_amd.engine import Engine   # noqa: E402
from oracle.mfgp_oracle import load_powerspecs   # noqa: E402
from bench_posterior import GOKU_DIR, gpr_model, measure   # noqa: E402
from bench_sample import inputs   # noqa: E402

LOG2PI = math.log(2.0 * math.pi)


def latent_model(d):
    X, Y = d["X"], d["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    k = lambda: M.SquaredExponential(lengthscales=np.ones(D))
    m = M.LatentMFCoregionalizationSVGP(X, Y, k(), k(), num_latents=15, num_inducing=300, num_outputs=P)
    rng = np.random.default_rng(8)
    m.q_mu.assign(rng.standard_normal(m.q_mu.shape) * 0.3)
    return m


def torch_route(post, Xd, y, C):
    """(logp [N*], d sum(logp) / d Xnew) through autograd predict_f and batched torch.linalg."""
    Xt = Xd.detach().clone().requires_grad_(True)
    mean, var = post.predict_f(Xt)
    mean, var = mean.as_subclass(torch.Tensor), var.as_subclass(torch.Tensor)
    L = torch.linalg.cholesky(C[None] + torch.diag_embed(var))
    r = (y - mean)[..., None]
    quad = (r * torch.cholesky_solve(r, L)).sum(dim=(1, 2))
    logp = -0.5 * quad - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(dim=1) - 0.5 * y.shape[-1] * LOG2PI
    logp.sum().backward()
    return logp.detach(), Xt.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logdens", "bench.json"))
    a = ap.parse_args()
    eng = Engine.get()
    d = load_powerspecs(GOKU_DIR)
    P = d["Y"].shape[1]
    out = dict(bench="logdens", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), unit="us per call on N* walkers (host clock, window ends in a device synchronise)")
    rng = np.random.default_rng(12)
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    Cm = (Q * np.logspace(-1, -4, P)) @ Q.T     # an observational covariance, cond 1e3
    C = torch.tensor(0.5 * (Cm + Cm.T), device=eng.device)
    y = torch.tensor(d["Ytest"][0], device=eng.device)   # one data vector for every walker
    for name, make in (("gpr_goku", gpr_model), ("svgp_latent_goku_l15_m300", latent_model)):
        post = make(d).posterior()
        svgp = isinstance(post, M.SVGPPosterior)
        for ns in (64, 1024):
            Xd = torch.tensor(inputs(d, ns, 1024), device=eng.device)
            got = post.log_density(Xd, y, obs_cov=C, grad=True)
            ref = torch_route(post, Xd, y, C)
            mean = got.mean.as_subclass(torch.Tensor)
            var = got.var.as_subclass(torch.Tensor)
            var = var if svgp else var[:, 0].contiguous()
            r = measure({"torch": lambda: torch_route(post, Xd, y, C),
                         "log_density": lambda: post.log_density(Xd, y, obs_cov=C, grad=True),
                         "density": lambda: eng.mvn_logpdf(mean, y, var, None, C, grad=True, sum_gvar=not svgp),
                         "predict_f": lambda: post.predict_f(Xd)}, a.calls, a.windows, a.warmup)
            r["ratio_torch_over_log_density"] = round(r["torch"]["median_us"] / r["log_density"]["median_us"], 3)
            r["ratio_density_over_predict_f"] = round(r["density"]["median_us"] / r["predict_f"]["median_us"], 3)
            r["max_abs_diff_logp"] = float((got.logp.as_subclass(torch.Tensor) - ref[0]).abs().max())
            r["max_rel_diff_grad"] = float((got.grad_X.as_subclass(torch.Tensor) - ref[1]).abs().max()
                                           / ref[1].abs().max())
            out[f"{name}_walkers{ns}"] = r
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
