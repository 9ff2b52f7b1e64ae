"""Per-call time of predict_f: the model's own (Gram + factorization every call) against the cached
posterior's (model.posterior().predict_f), at the emulator's use: one or a few X* rows per call.

  GPR   MultiFidelityGPModel at Goku (N = 1164, P = 64), nstar in {1, 36}
  SVGP  SingleBinSVGP at Goku (M = 300, L = P = 64), nstar in {1, 36}

Method: every shape and variant is warmed first; a window is a host clock around `--calls` calls
that ends in a device synchronise; the variants alternate window by window in this one process;
`--windows` windows per variant, reported as median with min / max (the spread).  X* is a host
array (what a sampler hands over), so both variants include its upload; "post_dev" is the cached
call with X* already on the device.  The model's predict_f is unchanged code, so its figure is also
the previous commit's.  Prints one JSON line.  GPU box: python tools/bench_posterior.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multi_fidelity_gpflow_amd as M   # noqa: E402
from multi_fidelity_gpflow_amd.engine import Engine   # noqa: E402
from oracle.mfgp_oracle import load_powerspecs   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GOKU_DIR = os.path.join(GOLDEN, "data", "matter_power_1128_Box1000_Part750_36_Box1000_Part3000_z0")


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6   # us per call


def measure(variants, calls, windows, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():   # alternate the variants window by window
            times[k].append(window(fn, calls))
    return {k: dict(median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2),
                    max_us=round(float(np.max(v)), 2)) for k, v in times.items()}


def gpr_model(d):
    X, Y = d["X"], d["Y"]
    D = X.shape[1] - 1
    rng = np.random.default_rng(7)
    m = M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=0.5 + 1.5 * rng.random(D)),
                               M.SquaredExponential(lengthscales=0.5 + rng.random(D)))
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 0.9))
    return m


def svgp_model(d):
    X, Y = d["X"], d["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                        M.SquaredExponential(lengthscales=np.ones(D)), P, Z=np.zeros((300, D + 1)))
    m.inducing_variable.assign(np.load(os.path.join(GOLDEN, "goku_kmeans_z300.npy")))
    rng = np.random.default_rng(8)
    m.q_mu.assign(rng.standard_normal(m.q_mu.shape) * 0.3)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    eng = Engine.get()
    d = load_powerspecs(GOKU_DIR)
    out = dict(bench="posterior", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), unit="us per predict_f call (host clock, window ends in a device synchronise)")
    for name, model in (("gpr_goku", gpr_model(d)), ("svgp_singlebin_goku_m300", svgp_model(d))):
        post = model.posterior()
        for ns in (1, 36):
            Xs = np.ascontiguousarray(d["Xtest"][:ns])
            Xd = torch.tensor(Xs, device=eng.device)
            ref, got = model.predict_f(Xs), post.predict_f(Xs)
            err = max(float((ref[0] - got[0]).abs().max()), float((ref[1] - got[1]).abs().max()))
            r = measure({"model": lambda: model.predict_f(Xs), "post": lambda: post.predict_f(Xs),
                         "post_dev": lambda: post.predict_f(Xd)}, a.calls, a.windows, a.warmup)
            r["max_abs_diff_model_vs_post"] = err
            out[f"{name}_nstar{ns}"] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
