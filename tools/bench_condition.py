"""Per-call time of conditioning the cached GPR posterior on k new rows (GPRPosterior.condition_on) against
the route it replaces.

  MultiFidelityGPModel at Goku (N = 1164, P = 64, D = 10), tile 32, the initial parameters; k = 1, 8, 32
  seeded rows (fidelities alternating) with seeded normal targets, on the device.

Variants, per k:
  condition_k   post.condition_on(Xadd, Yadd): allocates the new block, the C call, stacks the data and reads info
  c_call_k      mfgp_gpr_posterior_append alone, into a preallocated block (no host read)
  rebuild_k     the route it replaces: building the posterior of the stacked data (Gram, factorization, inverse
                factor), timed as update_cache() of a conditioned posterior, which runs only the build

Method as tools/bench_posterior.py: every variant warmed; a window is a host clock around `--calls` calls
that ends in a device synchronise; the variants alternate window by window in one process; median with
min / max over `--windows` windows.  Also records the largest relative difference between the two routes'
predict_f at 256 seeded points.  Prints one JSON line (and writes it to --out).
GPU box: python tools/bench_condition.py --out profiles/condition/bench.json
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
from bench_leave_out import initial_model   # noqa: E402
from bench_posterior import GOKU_DIR, measure   # noqa: E402

KS = (1, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    eng = Engine.get()
    eng.set_tile(32)
    d = load_powerspecs(GOKU_DIR)
    X, Y = d["X"], d["Y"]
    n, p, D = X.shape[0], Y.shape[1], X.shape[1] - 1
    post = initial_model(X, Y).posterior()
    rng = np.random.default_rng(4096)
    dev = lambda v: torch.tensor(np.ascontiguousarray(v), device=eng.device)
    Xs = dev(np.hstack([rng.random((256, D)), (np.arange(256) % 2)[:, None].astype(np.float64)]))
    variants, diff = {}, {}
    for k in KS:
        Xadd = dev(np.hstack([rng.random((k, D)), (np.arange(k) % 2)[:, None].astype(np.float64)]))
        Yadd = dev(rng.standard_normal((k, p)))
        cond = post.condition_on(Xadd, Yadd)
        rebuilt = post.condition_on(Xadd, Yadd)
        rebuilt.update_cache()
        (m0, v0), (m1, v1) = cond.predict_f(Xs), rebuilt.predict_f(Xs)
        diff[f"k{k}"] = dict(mean=float(((m0 - m1).abs().max() / m1.abs().max()).item()),
                             var=float(((v0 - v1).abs().max() / v1.abs().max()).item()))
        out = torch.empty_like(cond.cache)

        def c_call(Xadd=Xadd, Yadd=Yadd, out=out):
            return eng.gpr_posterior_append(0, (n, p, D), post.cache, Xadd, Yadd, out)

        variants[f"condition_{k}"] = lambda Xadd=Xadd, Yadd=Yadd: post.condition_on(Xadd, Yadd)
        variants[f"c_call_{k}"] = c_call
        variants[f"rebuild_{k}"] = rebuilt.update_cache
    res = dict(bench="condition", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), n=int(n), p=int(p), d=int(D), ks=list(KS),
               unit="us per call (host clock, window ends in a device synchronise)",
               condition_vs_rebuild_predict_rel_diff=diff)
    r = measure(variants, a.calls, a.windows, a.warmup)
    res.update(r)
    for k in KS:
        res[f"condition_over_rebuild_{k}"] = round(r[f"condition_{k}"]["median_us"] / r[f"rebuild_{k}"]["median_us"], 4)
        res[f"c_call_over_rebuild_{k}"] = round(r[f"c_call_{k}"]["median_us"] / r[f"rebuild_{k}"]["median_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
