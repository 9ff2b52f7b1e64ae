"""Per-call time of joint posterior draws: ``post.predict_f_samples(Xnew, S, eps=eps)`` (mfgp_mvn_sample)
against what a user can do without it through unchanged API: ``post.predict_f(Xnew, full_cov=True)``, then
``torch.linalg.cholesky(cov + 1e-6 I) @ eps + mean`` on the device.

  GPR   MultiFidelityGPModel posterior at Goku (N = 1164, P = 64): N* = 36, S = 100 and N* = 512, S = 16
  SVGP  SingleBinSVGP posterior at Goku (M = 300, L = P = 64): N* = 36, S = 100

Method (tools/bench_posterior.py's): every case and variant is warmed first; a window is a host clock
around `--calls` calls that ends in a device synchronise; the two variants alternate window by window in
this one process; `--windows` windows per variant, reported as median with min / max.  Xnew and eps are
device tensors for both.  The torch route is unchanged code, so its figure is also the previous commit's.
Prints one JSON line and writes it to profiles/sample/bench.json.  GPU box: python tools/bench_sample.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from multi_fidelity_gpflow_amd.engine import Engine   # noqa: E402
from oracle.mfgp_oracle import load_powerspecs   # noqa: E402
from bench_posterior import GOKU_DIR, gpr_model, measure, svgp_model   # noqa: E402

JITTER = 1e-6


def torch_route(post, Xd, eps):
    """[S, N*, P] draws through predict_f(full_cov=True) and torch.linalg.cholesky."""
    mean, cov = post.predict_f(Xd, full_cov=True)
    mean, cov = mean.as_subclass(torch.Tensor), cov.as_subclass(torch.Tensor)
    eye = torch.eye(cov.shape[-1], dtype=cov.dtype, device=cov.device)
    L = torch.linalg.cholesky(cov + JITTER * eye)
    return mean[None] + torch.matmul(L, eps.permute(2, 1, 0)).permute(2, 1, 0)


def inputs(d, ns, seed):
    """ns HF rows: the dataset's test inputs, or seeded points near training inputs when it has fewer."""
    Xt = d["Xtest"]
    if ns <= Xt.shape[0]:
        return np.ascontiguousarray(Xt[:ns])
    rng = np.random.default_rng(seed)
    X = d["X"]
    Xs = X[rng.choice(X.shape[0], ns, replace=True)].copy()
    Xs[:, :-1] += 0.05 * rng.standard_normal((ns, X.shape[1] - 1))
    Xs[:, -1] = 1.0
    return Xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample", "bench.json"))
    a = ap.parse_args()
    eng = Engine.get()
    d = load_powerspecs(GOKU_DIR)
    out = dict(bench="sample", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), unit="us per call of S joint draws (host clock, window ends in a device synchronise)")
    cases = (("gpr_goku", gpr_model, 36, 100), ("gpr_goku", gpr_model, 512, 16),
             ("svgp_singlebin_goku_m300", svgp_model, 36, 100))
    posts = {}
    for name, make, ns, S in cases:
        if name not in posts:
            posts[name] = make(d).posterior()
        post = posts[name]
        Xd = torch.tensor(inputs(d, ns, 512), device=eng.device)
        p = d["Y"].shape[1]
        eps = torch.randn((S, ns, p), dtype=torch.float64, device=eng.device,
                          generator=torch.Generator(device=eng.device).manual_seed(ns + S))
        got, ref = post.predict_f_samples(Xd, S, eps=eps), torch_route(post, Xd, eps)
        r = measure({"torch": lambda: torch_route(post, Xd, eps),
                     "samples": lambda: post.predict_f_samples(Xd, S, eps=eps)}, a.calls, a.windows, a.warmup)
        r["ratio_torch_over_samples"] = round(r["torch"]["median_us"] / r["samples"]["median_us"], 3)
        r["max_abs_diff"] = float((got.as_subclass(torch.Tensor) - ref).abs().max())
        out[f"{name}_nstar{ns}_s{S}"] = r
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
