"""Dump every output array of every cached-posterior call (build, predict with and without cov, VJP,
log-density with and without gradient, leave-out, design score and append row, append) at small shapes
and both tile sizes to an .npz, for a bitwise A/B of library builds (a few seconds per library):
  MFGP_LIB_PATH=<lib> python tools/posterior_dump.py OUT.npz ;  python tools/posterior_dump.py --compare A B
GPR: n = 70, p = 3, d = 3, nlf 0 and 2, nstar 1 and 33; SVGP: m = 40, l = 2, p = 3 mixed and l = p = 3
unmixed; leave-out groups of 1 and 3 rows; design nref = 5, ncand = 7, q = 2; append k 1 and 3.
--compare A B C holds an array that differs between A and B (two runs of one library) to that spread
in C instead of to equality."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _theta(rng, d, nlf=0):
    if nlf:   # per-source kernels, rho, no LF-to-LF coupling (so that the Gram is positive definite), noise
        return np.concatenate([0.5 + rng.random((nlf + 1) * (1 + d) + nlf), np.zeros(nlf * nlf), [1e-2]])
    return np.concatenate([0.5 + rng.random(2 * d + 3), [1e-3]])


def dump(out):
    import torch
    from multi_fidelity_gpflow_amd.engine import Engine
    eng = Engine.get()
    dev = eng.device
    rng = np.random.default_rng(17)
    res, infos = {}, {}
    d = 3
    dt = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)

    def inputs(n, nlf=0):
        return np.concatenate([rng.random((n, d)), (np.arange(n) % (nlf + 1 if nlf else 2))[:, None].astype(float)], axis=1)

    def put(key, *ts, info=None):
        torch.cuda.synchronize()
        for i, t in enumerate(ts):
            if t is not None:
                res[f"{key}.{i}"] = t.cpu().numpy().copy()
        if info is not None:
            infos[key] = info.cpu().numpy().reshape(-1).tolist()

    for tile in (32, 64):
        eng.set_tile(tile)
        n, p = 70, 3
        for nlf in (0, 2):
            X = inputs(n, nlf)
            Y = np.sin(3.0 * X[:, :d].sum(1))[:, None] * (1.0 + 0.1 * np.arange(p))[None, :] + 0.05 * rng.standard_normal((n, p))
            X, Y, th = dt(X), dt(Y), dt(_theta(rng, d, nlf))
            shape, tag = (n, p, d), f"gpr_t{tile}_lf{nlf}"
            cache = torch.zeros(eng.gpr_posterior_bytes(nlf, n, p, d), dtype=torch.uint8, device=dev)
            put(f"{tag}_build", cache, info=eng.gpr_posterior_build(nlf, X, Y, th, cache))
            for ns in (1, 33):
                Xs, Ys = dt(inputs(ns, nlf)), dt(rng.standard_normal((ns, p)))
                ov, oc = dt(0.1 + rng.random((ns, p))), rng.standard_normal((p, p))
                oc = dt(oc @ oc.T + p * np.eye(p))
                put(f"{tag}_s{ns}_pred", *eng.gpr_posterior_predict(nlf, shape, cache, Xs))
                put(f"{tag}_s{ns}_predcov", *eng.gpr_posterior_predict(nlf, shape, cache, Xs, full_cov=True))
                put(f"{tag}_s{ns}_dens", *eng.gpr_posterior_logdens(nlf, shape, cache, Xs, Ys, obs_var=ov))
                put(f"{tag}_s{ns}_denscov", *eng.gpr_posterior_logdens(nlf, shape, cache, Xs, Ys[0], obs_cov=oc))
                if nlf == 0:
                    g = (dt(rng.standard_normal((ns, p))), dt(rng.standard_normal(ns)))
                    put(f"{tag}_s{ns}_vjp", *eng.gpr_posterior_predict(nlf, shape, cache, Xs, grad=g))
                    put(f"{tag}_s{ns}_vjp_nogvar", *eng.gpr_posterior_predict(nlf, shape, cache, Xs, grad=(g[0], None)))
                    put(f"{tag}_s{ns}_densgrad", *eng.gpr_posterior_logdens(nlf, shape, cache, Xs, Ys, obs_var=ov, grad=True))
                    put(f"{tag}_s{ns}_denscovgrad", *eng.gpr_posterior_logdens(nlf, shape, cache, Xs, Ys, obs_cov=oc, grad=True))
            for gs in (1, 3):
                rows = rng.permutation(n)[:12].astype(np.int32)
                offs = np.arange(0, 12 + 1, gs, dtype=np.int32)
                r = eng.gpr_posterior_leave_out(nlf, shape, cache, i32(offs), i32(rows), gs)
                put(f"{tag}_lo{gs}", *r[:3], info=r[3])
            nref, ncand, q = 5, 7, 2
            Xall = dt(inputs(nref + ncand, nlf))
            ws = eng.gpr_posterior_design_workspace(nlf, shape, nref, ncand, q)
            E = torch.zeros((q - 1, nref + ncand), dtype=torch.float64, device=dev)
            for w, wt in ((None, "w0"), (dt(0.5 + rng.random(nref)), "w1")):
                s0 = eng.gpr_posterior_design_score(nlf, shape, cache, Xall, nref, w, E, 0, ws)
                eng.gpr_posterior_design_append(nlf, shape, cache, Xall, nref, torch.argmax(s0).to(torch.int32), E, 0, ws)
                s1 = eng.gpr_posterior_design_score(nlf, shape, cache, Xall, nref, w, E, 1, ws)
                put(f"{tag}_design_{wt}", s0, E, s1)
            for k in (1, 3):
                Xa, Ya = dt(inputs(k, nlf)), dt(rng.standard_normal((k, p)))
                for Yk, yt in ((Ya, "y"), (None, "fant")):
                    oc = torch.zeros(eng.gpr_posterior_bytes(nlf, n + k, p, d), dtype=torch.uint8, device=dev)
                    mean, info = eng.gpr_posterior_append(nlf, shape, cache, Xa, Yk, oc)
                    put(f"{tag}_append{k}_{yt}", oc, mean, info=info)
        m = 40
        for mixed, L, p in ((True, 2, 3), (False, 3, 3)):
            Z = dt(inputs(m))
            thetas = dt(np.stack([_theta(rng, d) for _ in range(L)]))
            q_mu = dt(rng.standard_normal((m, L)) * 0.3)
            q_sqrt = dt(np.tril(rng.standard_normal((L, m, m)) * 0.05) + np.eye(m)[None] * 0.4)
            W = dt(rng.standard_normal((p, L)) * 0.4) if mixed else None
            shape, tag = (m, L, p, d, mixed), f"svgp_t{tile}_{'mixed' if mixed else 'plain'}"
            cache = torch.zeros(eng.svgp_posterior_bytes(m, L, p, d), dtype=torch.uint8, device=dev)
            put(f"{tag}_build", cache, info=eng.svgp_posterior_build(Z, thetas, q_mu, q_sqrt, W, p, 1e-6, cache))
            for ns in (1, 33):
                Xs, Ys = dt(inputs(ns)), dt(rng.standard_normal((ns, p)))
                ov, oc = dt(0.1 + rng.random(p)), rng.standard_normal((p, p))
                oc = dt(oc @ oc.T + p * np.eye(p))
                g = (dt(rng.standard_normal((ns, p))), dt(rng.standard_normal((ns, p))))
                put(f"{tag}_s{ns}_pred", *eng.svgp_posterior_predict(shape, cache, Xs))
                put(f"{tag}_s{ns}_vjp", *eng.svgp_posterior_predict(shape, cache, Xs, grad=g))
                put(f"{tag}_s{ns}_vjp_nogmean", *eng.svgp_posterior_predict(shape, cache, Xs, grad=(None, g[1])))
                for gr in (False, True):
                    put(f"{tag}_s{ns}_dens_g{int(gr)}", *eng.svgp_posterior_logdens(shape, cache, Xs, Ys, obs_var=ov, grad=gr))
                    put(f"{tag}_s{ns}_denscov_g{int(gr)}", *eng.svgp_posterior_logdens(shape, cache, Xs, Ys, obs_cov=oc, grad=gr))
    eng.set_tile(32)
    bad = {k: v for k, v in infos.items() if any(v)}
    print(f"{len(res)} arrays dumped; nonzero info: {bad if bad else 'none'}")
    np.savez(out, **res)


def _spread(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.abs(a - b).max()) if a.shape == b.shape else float("inf")


def compare(paths):
    A, B = np.load(paths[0]), np.load(paths[1])
    C = np.load(paths[2]) if len(paths) > 2 else None
    assert sorted(A.files) == sorted(B.files) and (C is None or sorted(C.files) == sorted(A.files)), \
        "the dumps hold different arrays"
    bad = loose = 0
    for k in A.files:
        same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()   # NaN-safe
        if C is None:
            if not same:
                print(f"{k:40s} DIFF max abs {_spread(A[k], B[k]):.1e}")
            bad += not same
        elif same:
            ok = A[k].shape == C[k].shape and A[k].tobytes() == C[k].tobytes()
            if not ok:
                print(f"{k:40s} DIFF max abs {_spread(A[k], C[k]):.1e}")
            bad += not ok
        else:   # not reproducible by the first library itself: within its own spread of either run
            loose += 1
            s, t = _spread(A[k], B[k]), min(_spread(A[k], C[k]), _spread(B[k], C[k]))
            print(f"{k:40s} run-to-run {s:.1e}, third {t:.1e} {'ok' if t <= s else 'DIFF'}")
            bad += not t <= s
    print(f"{len(A.files)} arrays compared: " + ("all bitwise equal" if not bad and not loose else
                                                 f"{bad} arrays differ, {loose} held to the run-to-run spread"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
