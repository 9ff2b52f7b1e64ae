#!/usr/bin/env python
"""SVGP training step timing on Goku (README.md:86-87 configurations):
single-bin SVGP (M=300, one latent per bin, P=64) and latent SVGP (L=15, M=300).
Prints one JSON line per model: seconds per optimize() iteration (hipGraph replay).
--heterosed: the latent model with the HeteroscedasticGaussian likelihood (targets [Y | U], synthetic
U ~ U[0.05, 0.5] with a fifth of the entries 0, seed 0): the fused VE reverse kernel k_ve_bwd_het
against the homoscedastic k_ve_bwd -> k_ab -> k_gw of a run without the flag.
--masked: the latent model with the MaskedGaussian likelihood (missing_outputs=True: one variance per
output, 30% of the targets NaN, seed 0): k_ve_bwd_masked against k_ve_bwd_het of a --heterosed run."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multi_fidelity_gpflow_amd as M
from bench import load_goku

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--which", default="both")
ap.add_argument("--heterosed", action="store_true")
ap.add_argument("--masked", action="store_true")
a = ap.parse_args()
X, Y, Xt, Yt = load_goku()
D, P = X.shape[1] - 1, Y.shape[1]
k = lambda: M.SquaredExponential(lengthscales=np.ones(D))
res = []
if a.which in ("both", "single"):
    m = M.SingleBinSVGP(X, Y, k(), k(), P, Z=np.zeros((300, D + 1)))
    tr = M.svgp._SVGPTrainer(m, (X, Y), max_iters=a.iters + 10, initial_lr=0.1, graph=True, graph_chunk=10)
    tr.run(10); tr.sync()
    t0 = time.perf_counter(); tr.run(a.iters); tr.sync(); dt = (time.perf_counter() - t0) / a.iters
    res.append({"model": "SingleBinSVGP goku M=300 L=P=64", "s_per_iter": dt,
                "ref_m1_s_per_iter": 2237.47 / 1000, "loss_last": tr.loss_at(a.iters + 9)})
if a.which in ("both", "latent"):
    Yl = Y
    if a.heterosed:
        rng = np.random.default_rng(0)
        U = rng.uniform(0.05, 0.5, Y.shape)
        U[rng.random(Y.shape) < 0.2] = 0.0
        Yl = np.hstack([Y, U])
    if a.masked:
        Yl = np.array(Y, dtype=np.float64, copy=True)
        Yl[np.random.default_rng(0).random(Y.shape) < 0.3] = np.nan
    m = M.LatentMFCoregionalizationSVGP(X, Yl, k(), k(), num_latents=15, num_inducing=300, num_outputs=P,
                                        heterosed=a.heterosed, missing_outputs=a.masked)
    tr = M.svgp._SVGPTrainer(m, (X, Yl), max_iters=a.iters + 10, initial_lr=0.1, graph=True, graph_chunk=10)
    tr.run(10); tr.sync()
    t0 = time.perf_counter(); tr.run(a.iters); tr.sync(); dt = (time.perf_counter() - t0) / a.iters
    res.append({"model": "LatentMFCoregionalizationSVGP goku L=15 M=300" + (" heterosed" if a.heterosed else "") +
                (" masked" if a.masked else ""),
                "s_per_iter": dt,
                "ref_m1_s_per_iter": 1020.22 / 2000, "loss_last": tr.loss_at(a.iters + 9)})
for r in res:
    print(json.dumps(r))
