"""Per-call time of leave-group-out cross-validation from the cached GPR posterior
(GPRPosterior.leave_out) against one of the refits it replaces.

  MultiFidelityGPModel at Goku (N = 1164, P = 64, D = 10), tile 32, the initial parameters.

Variants:
  pairs    post.leave_out(groups_by_input(X, only_hf=True)): the 36 HF rows, each with its LF twin
  singles  post.leave_out(): all 1164 rows, one at a time
  refit    what a user does today for ONE of the 36 groups: update_cache() of a posterior of a model
           built without the pair, and its predict_f at the pair's two inputs
  pairs_device, singles_device   the C call of the first two alone (two launches), table and outputs
           already on the device: leave_out without its host work (table, upload, output ops, info read)

Method as tools/bench_posterior.py: every variant warmed; a window is a host clock around `--calls`
calls that ends in a device synchronise; the variants alternate window by window in one process;
median with min / max over `--windows` windows.  Prints one JSON line (and writes it to --out).
GPU box: python tools/bench_leave_out.py --out profiles/leave_out/bench.json
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
import multi_fidelity_gpflow_amd as M   # noqa: E402
from multi_fidelity_gpflow_amd.engine import Engine   # noqa: E402
from multi_fidelity_gpflow_amd.posteriors import normalize_groups   # noqa: E402
from oracle.mfgp_oracle import load_powerspecs   # noqa: E402
from bench_posterior import GOKU_DIR, measure   # noqa: E402


def initial_model(X, Y):
    D = X.shape[1] - 1
    return M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                  M.SquaredExponential(lengthscales=np.ones(D)))


def device_call(eng, post, groups):
    """The engine call alone (the C call's two launches), the group table and the outputs already on the device:
    what leave_out spends on the device, without the host's table, upload, output ops and info read."""
    p = post._shape[1]
    offsets, rows, gmax = normalize_groups(groups, post._shape[0])
    ng, nr = offsets.shape[0] - 1, rows.shape[0]
    dev = eng.device
    d_off, d_rows = torch.from_numpy(offsets).to(dev), torch.from_numpy(rows).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = (torch.empty((nr, p), **f64), torch.empty((nr, gmax), **f64), torch.empty((ng, p), **f64),
           torch.empty((ng,), dtype=torch.int32, device=dev))
    return lambda: eng.gpr_posterior_leave_out(0, post._shape, post.cache, d_off, d_rows, gmax, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    eng = Engine.get()
    eng.set_tile(32)
    d = load_powerspecs(GOKU_DIR)
    X, Y = d["X"], d["Y"]
    labels = M.groups_by_input(X, only_hf=True)
    post = initial_model(X, Y).posterior()
    pairs = post.leave_out(labels, full_cov=True)
    ng = int(labels.max()) + 1
    sizes = np.bincount(pairs.group, minlength=ng)
    # the refit of the first group, and how far the closed form is from it
    S = pairs.rows[pairs.group == 0]
    keep = np.setdiff1d(np.arange(X.shape[0]), S)
    refit_post = initial_model(X[keep], Y[keep]).posterior()
    Xs = torch.tensor(np.ascontiguousarray(X[S]), device=eng.device)
    rm, rc = refit_post.predict_f(Xs, full_cov=True)
    k = len(S)
    dev_mean = float((rm - pairs.mean[:k]).abs().max())
    dev_cov = float((rc[0] - pairs.cov[0, :k, :k]).abs().max())

    def refit():
        refit_post.update_cache()
        return refit_post.predict_f(Xs)

    out = dict(bench="leave_out", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), n=int(X.shape[0]), p=int(Y.shape[1]), groups=ng, group_sizes=sorted(set(sizes.tolist())),
               rows_in_groups=int(pairs.rows.size),
               unit="us per call (host clock, window ends in a device synchronise)",
               first_group_vs_refit=dict(rows=S.tolist(), mean=dev_mean, cov=dev_cov))
    r = measure({"pairs": lambda: post.leave_out(labels), "singles": lambda: post.leave_out(), "refit": refit,
                 "pairs_device": device_call(eng, post, labels), "singles_device": device_call(eng, post, None)},
                a.calls, a.windows, a.warmup)
    out.update(r)
    out["pairs_over_refit"] = round(r["pairs"]["median_us"] / r["refit"]["median_us"], 4)
    out["singles_over_refit"] = round(r["singles"]["median_us"] / r["refit"]["median_us"], 4)
    out["refits_replaced_by_pairs"] = ng
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
