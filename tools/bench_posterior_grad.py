"""Per-call time of the cached posterior's input gradient (predict_f_vjp) against the forward alone
and against what the previous commit offered for a gradient: central differences, one cached
predict_f call on 2 D N* rows.

  GPR   MultiFidelityGPModel at Goku (N = 1164, P = 64, D = 10), nstar in {1, 36}
  SVGP  SingleBinSVGP at Goku (M = 300, L = P = 64), nstar in {1, 36}

Variants (every input already on the device, so the figures are the calls' own):
  forward  post.predict_f(X*)
  vjp      post.predict_f_vjp(X*, gm, gv): value and gradient
  fd       post.predict_f on the 2 D N* displaced rows (the differencing itself is not counted)

Method as tools/bench_posterior.py: every variant warmed; a window is a host clock around `--calls`
calls that ends in a device synchronise; the variants alternate window by window in one process;
median with min / max over `--windows` windows.  Prints one JSON line (and writes it to --out).
GPU box: python tools/bench_posterior_grad.py --out profiles/posterior_grad/bench.json
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


def fd_rows(Xs, h=1e-5):
    """The 2 D N* rows of central differences over the D inputs of every row."""
    ns, D = Xs.shape[0], Xs.shape[1] - 1
    rows = np.repeat(Xs[None], 2 * D, axis=0)           # [2 D, N*, D + 1]
    for k in range(D):
        rows[2 * k, :, k] += h
        rows[2 * k + 1, :, k] -= h
    return rows.reshape(2 * D * ns, D + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    eng = Engine.get()
    d = load_powerspecs(GOKU_DIR)
    out = dict(bench="posterior_grad", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), unit="us per call (host clock, window ends in a device synchronise)")
    rng = np.random.default_rng(11)
    for name, model in (("gpr_goku", gpr_model(d)), ("svgp_singlebin_goku_m300", svgp_model(d))):
        post = model.posterior()
        P = d["Y"].shape[1]
        for ns in (1, 36):
            Xs = np.ascontiguousarray(d["Xtest"][:ns])
            Xd = torch.tensor(Xs, device=eng.device)
            Xfd = torch.tensor(fd_rows(Xs), device=eng.device)
            gm = torch.tensor(rng.standard_normal((ns, P)), device=eng.device)
            gv = torch.tensor(rng.standard_normal((ns, P)), device=eng.device)
            # the two gradients agree (at the level central differences reach)
            gX = post.predict_f_vjp(Xd, gm, gv)[2]
            fm, fv = post.predict_f(Xfd)
            D = Xs.shape[1] - 1
            loss = ((fm.reshape(2 * D, ns, P) * gm).sum(-1) + (fv.reshape(2 * D, ns, P) * gv).sum(-1))
            fd = ((loss[0::2] - loss[1::2]) / 2e-5).T
            err = float((fd - gX[:, :D]).abs().max() / gX.abs().max())
            r = measure({"forward": lambda: post.predict_f(Xd), "vjp": lambda: post.predict_f_vjp(Xd, gm, gv),
                         "fd": lambda: post.predict_f(Xfd)}, a.calls, a.windows, a.warmup)
            r["fd_rows"] = int(Xfd.shape[0])
            r["vjp_over_forward"] = round(r["vjp"]["median_us"] / r["forward"]["median_us"], 3)
            r["fd_over_vjp"] = round(r["fd"]["median_us"] / r["vjp"]["median_us"], 3)
            r["rel_diff_fd_vs_vjp"] = err
            out[f"{name}_nstar{ns}"] = r
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
