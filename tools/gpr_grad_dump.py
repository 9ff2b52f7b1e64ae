"""Dump GPR LML value + gradient outputs (Goku and HBS at a few theta, every schedule the handle
offers: flow / steps / tiny) to an .npz, for bitwise A/B of library builds:
  MFGP_LIB_PATH=<lib> python tools/gpr_grad_dump.py OUT.npz ;  python tools/gpr_grad_dump.py --compare A B
--sweep OUT.npz dumps small synthetic problems instead, one for every path of the GPR host layer (tiny /
steps / flow at both tile sizes, the graph kernel, resident mode, the Adam entries, predict with and
without cov, the fp32 path under its knobs, potrf_inv, the posterior build): a few seconds per library."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(out):
    import torch
    from multi_fidelity_gpflow_amd.engine import Engine
    from conftest import GOKU_DIR, HBS_DIR
    from oracle.mfgp_oracle import load_powerspecs
    eng = Engine.get()
    res = {}
    rng = np.random.default_rng(3)
    for name, dd in (("goku", GOKU_DIR), ("hbs", HBS_DIR)):
        g = load_powerspecs(dd)
        X = torch.tensor(g["X"], device=eng.device)
        Y = torch.tensor(g["Y"], device=eng.device)
        d = X.shape[1] - 1
        for s in range(3):
            th = np.concatenate([[0.5 + rng.random()], 0.5 + rng.random(d), [0.1 + rng.random()], 0.5 + rng.random(d),
                                 [0.5 + rng.random()], [1e-3]])
            t = torch.tensor(th, dtype=torch.float64, device=eng.device)
            for flow in (True, False):
                eng.set_flow(flow)
                o, info = eng.gpr_lml(X, Y, t, want_grad=True)
                torch.cuda.synchronize()
                res[f"{name}_{s}_{'flow' if flow else 'steps'}"] = o.cpu().numpy().copy()
        eng.set_flow(True)
    np.savez(out, **res)


def _theta(rng, d, nlf=0):
    if nlf:
        g = (nlf + 1) * (1 + d) + nlf + nlf * nlf + 1
        return np.concatenate([0.5 + rng.random(g - 1), [1e-3]])
    return np.concatenate([[0.5 + rng.random()], 0.5 + rng.random(d), [0.1 + rng.random()], 0.5 + rng.random(d),
                           [0.5 + rng.random()], [1e-3]])


def sweep(out):
    import ctypes as C
    import torch
    from multi_fidelity_gpflow_amd.engine import AdamState, Engine
    from multi_fidelity_gpflow_amd._lib import check, ptr
    eng = Engine.get()
    dev = eng.device
    rng = np.random.default_rng(11)
    res, infos = {}, {}
    d = 3

    def data(n, p, nlf=0, dtype=torch.float64):
        X = np.concatenate([rng.random((n, d)), (np.arange(n) % (max(nlf, 1) + 1))[:, None].astype(float)], axis=1)
        Y = np.sin(3.0 * X[:, :d].sum(1))[:, None] * (1.0 + 0.1 * np.arange(p))[None, :] + 0.05 * rng.standard_normal((n, p))
        return torch.tensor(X, dtype=dtype, device=dev), torch.tensor(Y, dtype=dtype, device=dev)

    def put(key, *ts, info=None):
        torch.cuda.synchronize()
        for i, t in enumerate(ts):
            res[f"{key}.{i}"] = t.cpu().numpy().copy()
        if info is not None:
            infos[key] = info.cpu().numpy().reshape(-1).tolist()

    def mode(tile, flow):
        eng.set_tile(tile)
        eng.set_flow(flow != 0, any_size=flow == 3)

    dt = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    # AR1 kernel: tiny, steps (T < 8, and tile 64), flow at any size, the smallest default flow
    for p in (3, 33):
        for n, tile, flow in ((20, 32, 1), (70, 32, 1), (70, 32, 3), (230, 32, 1), (70, 64, 1)):
            mode(tile, flow)
            X, Y = data(n, p)
            th = dt(_theta(rng, d))
            for wg in (0, 1):
                o, info = eng.gpr_lml(X, Y, th, want_grad=bool(wg))
                put(f"ar1_n{n}_p{p}_t{tile}_f{flow}_g{wg}", o if wg else o[:1], info=info)
    # graph kernel: k_gram + flow / steps at both tiles; n = 740: more lower tiles than CUs
    for n, tile, flow in ((70, 32, 1), (70, 32, 3), (230, 32, 1), (230, 32, 0), (70, 64, 1), (230, 64, 1), (740, 32, 1)):
        mode(tile, flow)
        X, Y = data(n, 3, nlf=1)
        th = dt(_theta(rng, d, 1))
        for wg in (0, 1):
            o, info = eng.gmf_lml(1, X, Y, th, want_grad=bool(wg))
            put(f"gmf_n{n}_t{tile}_f{flow}_g{wg}", o if wg else o[:1], info=info)
    # resident mode: the second call skips the set-up, the n = 70 call invalidates the residency
    mode(32, 1)
    Xa, Ya = data(230, 3)
    Xb, Yb = data(70, 3)
    tha, thb = dt(_theta(rng, d)), dt(_theta(rng, d))
    ws = eng.private_workspace(eng.gpr_workspace_bytes(230, 3, d))
    with eng.resident():
        for i, (X, Y, th) in enumerate(((Xa, Ya, tha), (Xa, Ya, thb), (Xb, Yb, tha), (Xa, Ya, tha), (Xa, Ya, thb))):
            o, info = eng.gpr_lml(X, Y, th, want_grad=True, ws=ws)
            put(f"resident_{i}", o, info=info)
    # Adam: one step, three steps fusable / tiny / with the fusion off
    G = 2 * d + 4
    for name, n, nsteps, fusion in (("step", 230, 1, True), ("steps_fused", 230, 3, True), ("steps_tiny", 20, 3, True),
                                    ("steps_plain", 230, 3, False), ("steps_short", 70, 3, True)):
        eng.set_step_fusion(fusion)
        X, Y = data(n, 3)
        st = AdamState(dev, rng.standard_normal(G) * 0.3, np.ones(G, bool), np.arange(G), 0.05)
        eng.theta_from_u(st.u, st.theta, G - 1)
        hist = torch.zeros(8, dtype=torch.float64, device=dev)
        o = torch.zeros(1 + G, dtype=torch.float64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        if name == "step":
            eng.gpr_adam_step(X, Y, st, hist, o, info)
        else:
            eng.gpr_adam_steps(X, Y, st, hist, o, info, nsteps=nsteps)
        put(f"adam_{name}", st.theta, st.u, st.m, st.v, hist, o, st.step, info=info)
    eng.set_step_fusion(True)
    # predict: tiny and general, both kernels, with and without cov
    for n in (20, 70):
        for ns in (5, 33):
            for nlf in (0, 1):
                X, Y = data(n, 3, nlf)
                Xs, _ = data(ns, 3, nlf)
                th = dt(_theta(rng, d, nlf))
                m, v, info = eng.gmf_predict(nlf, X, Y, Xs, th) if nlf else eng.gpr_predict(X, Y, Xs, th)
                put(f"pred_n{n}_s{ns}_lf{nlf}", m, v, info=info)
                m, v, c, info = eng.gpr_predict_cov(nlf, X, Y, Xs, th)
                put(f"predcov_n{n}_s{ns}_lf{nlf}", m, v, c, info=info)
    # fp32: T = 2 at the 128-tile, under panel / look-ahead / refine
    X, Y = data(130, 3, dtype=torch.float32)
    Xs, _ = data(33, 3, dtype=torch.float32)
    th = dt(_theta(rng, d))
    for panel in (1, 6):
        for la in (0, 1):
            for refine in (0, 2):
                eng.set_f32_panel(panel); eng.set_f32_lookahead(bool(la)); eng.set_f32_refine(refine)
                k = f"f32_w{panel}_la{la}_r{refine}"
                for wg in (0, 1):
                    o, info = eng.gpr_lml(X, Y, th, want_grad=bool(wg))
                    put(f"{k}_g{wg}", o if wg else o[:1], info=info)
                st = AdamState(dev, np.linspace(-0.5, 0.5, G), np.ones(G, bool), np.arange(G), 0.05)
                eng.theta_from_u(st.u, st.theta, G - 1)
                hist = torch.zeros(8, dtype=torch.float64, device=dev)
                o = torch.zeros(1 + G, dtype=torch.float64, device=dev)
                info = torch.zeros(1, dtype=torch.int32, device=dev)
                eng.gpr_adam_step(X, Y, st, hist, o, info)
                put(f"{k}_adam", st.theta, st.u, st.m, st.v, hist, o, info=info)
                m, v, info = eng.gpr_predict(X, Y, Xs, th)
                put(f"{k}_pred", m, v, info=info)
                m, v, c, info = eng.gpr_predict_cov(0, X, Y, Xs, th)
                put(f"{k}_predcov", m, v, c, info=info)
    eng.set_f32_panel(6); eng.set_f32_lookahead(True); eng.set_f32_refine(2)
    # potrf_inv, with and without ldiag
    for tile in (32, 64):
        mode(tile, 1)
        B = rng.standard_normal((2, 33, 33))
        A = dt(B @ B.transpose(0, 2, 1) + 33 * np.eye(33))
        Li, ld, info = eng.potrf_inv(A)
        put(f"potrf_t{tile}", Li, ld, info=info)
        Li2 = torch.zeros_like(A)
        nb = C.c_size_t(0)
        check(eng.lib.mfgp_potrf_inv_workspace_size(eng.h, 33, 2, C.byref(nb)), "size")
        w = eng.private_workspace(nb.value)
        check(eng.lib.mfgp_potrf_inv(eng.h, 33, 2, ptr(A), 33, 33 * 33, ptr(w), w.numel(), ptr(Li2), 33, 33 * 33, None,
                                     ptr(info)), "mfgp_potrf_inv")
        put(f"potrf_t{tile}_noldiag", Li2, info=info)
        # posterior build: the cache bytes
        for nlf in (0, 1):
            X, Y = data(70, 3, nlf)
            th = dt(_theta(rng, d, nlf))
            cache = torch.zeros(eng.gpr_posterior_bytes(nlf, 70, 3, d), dtype=torch.uint8, device=dev)
            info = eng.gpr_posterior_build(nlf, X, Y, th, cache)
            put(f"postbuild_t{tile}_lf{nlf}", cache, info=info)
    mode(32, 1)
    bad = {k: v for k, v in infos.items() if any(v)}
    print(f"{len(res)} arrays dumped; nonzero info: {bad if bad else 'none'}")
    np.savez(out, **res)


if __name__ == "__main__":
    if sys.argv[1] == "--sweep":
        sweep(sys.argv[2])
    elif sys.argv[1] == "--compare":
        A, B = np.load(sys.argv[2]), np.load(sys.argv[3])
        bad = 0
        assert sorted(A.files) == sorted(B.files), "the two dumps hold different arrays"
        for k in A.files:
            same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()   # NaN-safe
            if not same or len(A.files) < 40:
                a, b = A[k].astype(np.float64), B[k].astype(np.float64)
                d = float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300)) if a.shape == b.shape else float("inf")
                print(f"{k:18s} {'bitwise' if same else 'DIFF'} rel {d:.1e}")
            bad += not same
        print(f"{len(A.files)} arrays compared: " + ("all bitwise equal" if not bad else f"{bad} arrays differ"))
        sys.exit(1 if bad else 0)
    else:
        dump(sys.argv[1])
