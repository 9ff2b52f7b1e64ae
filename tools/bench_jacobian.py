"""Per-call time of the emulator Jacobian and Fisher matrix: ``post.mean_jacobian(Xnew)`` (mfgp_*_jacobian) and
``post.fisher(Xnew, obs_cov=C)`` (+ mfgp_mvn_fisher) against the route a user writes without them through
unchanged API on the same device: P ``predict_f_vjp`` calls with one-hot ``grad_mean`` (P forwards and P VJP
launches), and for the Fisher matrix that route plus batched ``torch.linalg.cholesky`` / ``torch.cholesky_solve``
on the [N*, P, P] covariances.

  GPR   MultiFidelityGPModel posterior at Goku (N = 1164, P = 64, D = 10): N* = 64 and 1024
  SVGP  LatentMFCoregionalizationSVGP posterior at Goku (L = 15, M = 300, P = 64): the same

Variants (every input already on the device):
  mean_jacobian  mean, var and J [N*, P, D] from the fused call
  one_hot        J from P one-hot predict_f_vjp calls
  fisher         F [N*, D, D] from the fused call with a dense obs_cov (its one host read, of info, included)
  fisher_torch   one_hot, then torch.linalg.cholesky / cholesky_solve and J^T (Sigma^-1 J)
  predict_f      one cached predict_f call, for scale

Method (tools/bench_logdens.py's): every case and variant is warmed first; a window is a host clock around
`--calls` calls that ends in a device synchronise; the variants alternate window by window in this one
process; `--windows` windows per variant, reported as median with min / max.  The one-hot route is unchanged
code, so its figure is also the previous commit's.  Prints one JSON line and writes it to
profiles/jacobian/bench.json.  GPU box: python tools/bench_jacobian.py
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
from bench_logdens import latent_model   # noqa: E402
from bench_posterior import GOKU_DIR, gpr_model, measure   # noqa: E402
from bench_sample import inputs   # noqa: E402


def one_hot_route(post, Xd, eye):
    """(mean, var, J [N*, P, D]) from P predict_f_vjp calls with one-hot grad_mean (eye: [P, N*, P])."""
    cols = []
    for c in range(eye.shape[0]):
        mean, var, gX = post.predict_f_vjp(Xd, eye[c], None)
        cols.append(gX.as_subclass(torch.Tensor)[:, :-1])
    return mean.as_subclass(torch.Tensor), var.as_subclass(torch.Tensor), torch.stack(cols, dim=1)


def fisher_torch_route(post, Xd, eye, C):
    _, var, J = one_hot_route(post, Xd, eye)
    L = torch.linalg.cholesky(C[None] + torch.diag_embed(var))
    return J.transpose(1, 2) @ torch.cholesky_solve(J, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jacobian", "bench.json"))
    a = ap.parse_args()
    eng = Engine.get()
    d = load_powerspecs(GOKU_DIR)
    P = d["Y"].shape[1]
    out = dict(bench="jacobian", device=torch.cuda.get_device_name(eng.index), calls=a.calls, windows=a.windows,
               tile=eng.tile(), unit="us per call on N* rows (host clock, window ends in a device synchronise)")
    rng = np.random.default_rng(12)
    Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
    Cm = (Q * np.logspace(-1, -4, P)) @ Q.T     # an observational covariance, cond 1e3
    C = torch.tensor(0.5 * (Cm + Cm.T), device=eng.device)
    for name, make in (("gpr_goku", gpr_model), ("svgp_latent_goku_l15_m300", latent_model)):
        post = make(d).posterior()
        for ns in (64, 1024):
            Xd = torch.tensor(inputs(d, ns, 1024), device=eng.device)
            eye = torch.eye(P, dtype=torch.float64, device=eng.device)[:, None, :].expand(P, ns, P).contiguous()
            J = post.mean_jacobian(Xd)[2].as_subclass(torch.Tensor)
            F = post.fisher(Xd, obs_cov=C).fisher.as_subclass(torch.Tensor)
            Jr = one_hot_route(post, Xd, eye)[2]
            Fr = fisher_torch_route(post, Xd, eye, C)
            r = measure({"one_hot": lambda: one_hot_route(post, Xd, eye),
                         "mean_jacobian": lambda: post.mean_jacobian(Xd),
                         "fisher_torch": lambda: fisher_torch_route(post, Xd, eye, C),
                         "fisher": lambda: post.fisher(Xd, obs_cov=C),
                         "predict_f": lambda: post.predict_f(Xd)}, a.calls, a.windows, a.warmup)
            r["ratio_one_hot_over_mean_jacobian"] = round(r["one_hot"]["median_us"] / r["mean_jacobian"]["median_us"], 3)
            r["ratio_fisher_torch_over_fisher"] = round(r["fisher_torch"]["median_us"] / r["fisher"]["median_us"], 3)
            r["ratio_mean_jacobian_over_predict_f"] = round(r["mean_jacobian"]["median_us"] / r["predict_f"]["median_us"], 3)
            r["max_rel_diff_jacobian"] = float((J - Jr).abs().max() / Jr.abs().max())
            r["max_rel_diff_fisher"] = float((F - Fr).abs().max() / Fr.abs().max())
            out[f"{name}_rows{ns}"] = r
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
