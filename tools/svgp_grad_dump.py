"""Dump SVGP outputs to an .npz, for bitwise A/B of library builds:
  MFGP_LIB_PATH=<lib> python tools/svgp_grad_dump.py OUT.npz
then  python tools/svgp_grad_dump.py --compare A.npz B.npz
Value + gradient (all outputs) of one Goku single-bin and one HBS latent model; of a heteroscedastic and a
masked (some NaN targets) HBS latent model; predict_f with every covariance form of the HBS latent model on
40 rows; and the HBS latent model again at tile 64.  Every parameter is seeded."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(out):
    import multi_fidelity_gpflow_amd as M
    from multi_fidelity_gpflow_amd.engine import Engine
    from conftest import GOKU_DIR, HBS_DIR
    from oracle.mfgp_oracle import load_powerspecs
    res = {}
    g = load_powerspecs(GOKU_DIR)
    X, Y = g["X"], g["Y"]
    Zfix = np.load(os.path.join(ROOT, "tests", "golden", "goku_kmeans_z300.npy"))
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(10)),
                        M.SquaredExponential(lengthscales=np.ones(10)), 64, Z=np.zeros((300, 11)))
    m.inducing_variable.assign(Zfix)
    rng = np.random.default_rng(7)
    m.q_mu.assign(rng.standard_normal((300, 64)) * 0.5)
    m.q_sqrt.assign(np.tril(rng.standard_normal((64, 300, 300)) * 0.01) + 0.1 * np.eye(300)[None])
    e, gd = m.elbo_and_grad((X, Y))
    res["goku_elbo"] = np.array(e)
    for k, v in gd.items():
        res["goku_" + k] = np.asarray(v)
    h = load_powerspecs(HBS_DIR)
    X, Y = h["X"], h["Y"]
    D, P = X.shape[1] - 1, Y.shape[1]
    m = M.LatentMFCoregionalizationSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                        M.SquaredExponential(lengthscales=np.ones(D)), num_latents=5,
                                        num_inducing=30, num_outputs=P, w_type='diagonal')
    e, gd = m.elbo_and_grad((X, Y))
    res["hbs_elbo"] = np.array(e)
    for k, v in gd.items():
        res["hbs_" + k] = np.asarray(v)

    def latent(Yc, seed, **kw):
        m = M.LatentMFCoregionalizationSVGP(X, Yc, M.SquaredExponential(lengthscales=np.ones(D)),
                                            M.SquaredExponential(lengthscales=np.ones(D)), num_latents=5,
                                            num_inducing=30, num_outputs=P, w_type='diagonal', **kw)
        _seed(m, seed)
        return m

    def grads(tag, m, data):
        e, gd = m.elbo_and_grad(data)
        res[tag + "_elbo"] = np.array(e)
        for k, v in gd.items():
            res[tag + "_" + k] = np.asarray(v)

    rng = np.random.default_rng(11)
    grads("het", latent(Y, 21, heterosed=True), (X, np.hstack([Y, 0.05 + 0.1 * rng.random(Y.shape)])))
    Yn = Y.copy()
    Yn[rng.random(Y.shape) < 0.15] = np.nan
    Yn[:, 3] = np.nan                                   # one output with no observation at all
    grads("msk", latent(Yn, 22, missing_outputs=True), (X, Yn))
    m = latent(Y, 23)
    Xs = X[:40].copy()
    Xs[:, :-1] += 0.01 * rng.standard_normal((40, D))
    Xs[:, -1] = np.arange(40) % 2
    for fc, foc in ((False, False), (True, False), (False, True), (True, True)):
        mean, cov = m.predict_f(Xs, full_cov=fc, full_output_cov=foc)
        res[f"pred{int(fc)}{int(foc)}_mean"] = np.asarray(mean.numpy())
        res[f"pred{int(fc)}{int(foc)}_cov"] = np.asarray(cov.numpy())
    eng = Engine.get()
    nb = eng.tile()
    eng.set_tile(64)
    try:
        grads("t64", m, (X, Y))
    finally:
        eng.set_tile(nb)
    np.savez(out, **res)


def _seed(model, seed):
    rng = np.random.default_rng(seed)
    Mi, L = model.q_mu.shape
    model.q_mu.assign(rng.standard_normal((Mi, L)) * 0.3)
    model.q_sqrt.assign(np.tril(rng.standard_normal((L, Mi, Mi)) * 0.05) + np.eye(Mi)[None] * 0.4)
    for k in model.kernel.kernels:
        D = k.kernel_L.lengthscales.shape[0]
        k.kernel_L.variance.assign(0.5 + rng.random())
        k.kernel_L.lengthscales.assign(0.5 + rng.random(D))
        k.kernel_delta.variance.assign(0.2 + rng.random())
        k.kernel_delta.lengthscales.assign(0.5 + rng.random(D))
        k.rho.assign(np.full((1, 1), 0.5 + rng.random()))
    v = model.likelihood.variance
    v.assign(0.05 + rng.random(v.shape) * 0.1)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        same = np.array_equal(A[k], B[k])
        d = float(np.abs(A[k] - B[k]).max() / max(np.abs(A[k]).max(), 1e-300))
        print(f"{k:16s} {'bitwise' if same else 'DIFF'} rel {d:.1e}")
        bad += not same
    print("all bitwise equal" if not bad else f"{bad} arrays differ")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[1])
