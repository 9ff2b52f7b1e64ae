"""HeteroscedasticGaussian SVGP path (mfgp_svgp_elbo_het / mfgp_svgp_elbo_grad_het: k_svgp_ve_het, the
fused row-tiled reverse kernel k_ve_bwd_het and k_ve_het_reduce) against torch autograd through the
fp64 restatement tests/_het_oracle.py, which test_het_host.py ties to the KAT-pinned oracle.

Bounds are the homoscedastic pipeline's own (tests/test_gpu_svgp.py): ELBO 1e-13 relative, every
gradient block 1e-10 of its largest entry, the 20-step training trajectory 1e-12 relative.  The
uncertainties are U[0.05, 0.5] with a fifth of the entries exactly 0 and differ by row and column,
the baseline noise is 0.05-0.15 (_randomize).  Every test prints its measured errors (-s)."""
import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from multi_fidelity_gpflow_amd.engine import Engine, theta_size, to_dev
from multi_fidelity_gpflow_amd.svgp import DEFAULT_JITTER

from _het_oracle import HetLatentTrainer, het_elbo_t, synthetic_uncertainties

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- helpers (after tests/test_gpu_svgp.py)
def _oracle_state(model, W=None):
    D = model.inducing_variable.shape[1] - 1
    kps = []
    for k in model.kernel.kernels:
        t = k.theta_vector(D)
        kps.append(dict(vL=torch.tensor(t[0]), lL=torch.tensor(t[1:1 + D]), vD=torch.tensor(t[1 + D]),
                        lD=torch.tensor(t[2 + D:2 + 2 * D]), rho=torch.tensor(t[2 + 2 * D])))
    noise = torch.tensor(np.reshape(model.likelihood.variance.numpy(), (1,)), dtype=torch.float64)
    return (torch.tensor(model.inducing_variable.numpy()), kps, torch.tensor(model.q_mu.numpy()),
            torch.tensor(model.q_sqrt.numpy()), None if W is None else torch.tensor(W), noise)


def _randomize(model, seed):
    rng = np.random.default_rng(seed)
    M_, L = model.q_mu.shape
    model.q_mu.assign(rng.standard_normal((M_, L)) * 0.3)
    qs = np.tril(rng.standard_normal((L, M_, M_)) * 0.05) + np.eye(M_)[None] * 0.4
    model.q_sqrt.assign(qs)
    for k in model.kernel.kernels:
        D = k.kernel_L.lengthscales.shape[0]
        k.kernel_L.variance.assign(0.5 + rng.random())
        k.kernel_L.lengthscales.assign(0.5 + rng.random(D))
        k.kernel_delta.variance.assign(0.2 + rng.random())
        k.kernel_delta.lengthscales.assign(0.5 + rng.random(D))
        k.rho.assign(np.full((1, 1), 0.5 + rng.random()))
    model.likelihood.variance.assign(0.05 + rng.random() * 0.1)


def _autograd_grads(model, X, Y, U, W=None, num_data=None, kl_mult=1.0):
    """d(VE*scale - kl_mult*KL)/d(constrained params) by torch autograd through het_elbo_t."""
    D = model.inducing_variable.shape[1] - 1
    Z, kps, q_mu, q_sqrt, Wt, noise = _oracle_state(model, W)
    leaves = [Z, q_mu, q_sqrt, noise] + ([Wt] if Wt is not None else [])
    for kp in kps:
        leaves += list(kp.values())
    for t in leaves:
        t.requires_grad_(True)
    e, kl, ve = het_elbo_t(torch.tensor(X), torch.tensor(Y), torch.tensor(U), Z, kps, q_mu, q_sqrt, Wt, noise,
                           num_data=num_data)
    obj = e - (kl_mult - 1.0) * kl
    obj.backward()
    th = np.zeros((len(kps), 2 * D + 4))
    for l, kp in enumerate(kps):
        th[l, 0] = kp["vL"].grad
        th[l, 1:1 + D] = kp["lL"].grad.numpy()
        th[l, 1 + D] = kp["vD"].grad
        th[l, 2 + D:2 + 2 * D] = kp["lD"].grad.numpy()
        th[l, 2 + 2 * D] = kp["rho"].grad
    g = dict(Z=Z.grad.numpy(), q_mu=q_mu.grad.numpy(), q_sqrt=np.tril(q_sqrt.grad.numpy()), noise=noise.grad.numpy(),
             theta=th)
    if Wt is not None:
        g["W"] = Wt.grad.numpy()
    return float(e.detach()), g


def _close(name, got, ref, tol, rel=False):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max() / (np.abs(ref).max() if rel else 1.0)
    print(f"{name} {'rel' if rel else 'abs'} err {err:.1e} (bound {tol:.0e})")
    assert err < tol, (name, err)
    return err


def _value_ok(e, eo, tol):
    rel = abs(e - eo) / abs(eo)
    print(f"ELBO rel err {rel:.1e} (bound {tol:.0e})")
    assert rel < tol, rel


def _check_grads(gd, ga, tol):
    errs = {}
    for k, ref in ga.items():
        got = np.asarray(gd[k]).reshape(np.shape(ref))
        scale = max(np.abs(ref).max(), 1e-30)
        errs[k] = np.abs(got - ref).max() / scale
    print("gradient rel err", {k: f"{v:.1e}" for k, v in errs.items()}, f"(bound {tol:.0e})")
    for k, err in errs.items():
        assert err < tol, (k, err)


def _latent(X, Y, L, Mi, **kw):
    D, P = X.shape[1] - 1, Y.shape[1]
    return M.LatentMFCoregionalizationSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                           M.SquaredExponential(lengthscales=np.ones(D)), num_latents=L,
                                           num_inducing=Mi, num_outputs=P, w_type='diagonal', **kw)


def _engine_grad(model, X, Y, Yunc, qs_packed=False, kl_mult=1.0, scale=1.0, ws=None):
    """One Engine.svgp_elbo_grad call at the model's state.  Y / Yunc: device tensors (views allowed);
    Yunc None: the existing homoscedastic entry point.  Returns (out[3], gradients by name, q_sqrt's
    unpacked to [L, M, M])."""
    eng, Z, thetas, q_mu, q_sqrt, W = model._dev_state()
    Xd = to_dev(X, eng.device)
    n, m, L, p, d = Xd.shape[0], Z.shape[0], thetas.shape[0], Y.shape[1], Xd.shape[1] - 1
    f64 = dict(dtype=torch.float64, device=eng.device)
    ti, tj = np.tril_indices(m)
    tid, tjd = torch.as_tensor(ti, device=eng.device), torch.as_tensor(tj, device=eng.device)
    qs = q_sqrt[:, tid, tjd].contiguous() if qs_packed else q_sqrt
    noise = torch.tensor(np.reshape(model.likelihood.variance.numpy(), (1,)), **f64)
    out, g_mu, g_var = torch.zeros(3, **f64), torch.empty((L, n), **f64), torch.empty((L, n), **f64)
    g = dict(Z=torch.zeros((m, d + 1), **f64), theta=torch.zeros((L, theta_size(d)), **f64),
             q_mu=torch.zeros((m, L), **f64), q_sqrt=torch.zeros_like(qs), noise=torch.zeros(1, **f64))
    if W is not None:
        g["W"] = torch.zeros((p, L), **f64)
    info = torch.zeros((L,), dtype=torch.int32, device=eng.device)
    eng.svgp_elbo_grad(Xd, Y, Z, thetas, q_mu, qs, W, noise, scale, kl_mult, DEFAULT_JITTER, out, g_mu, g_var, g["Z"],
                       g["theta"], g["q_mu"], g["q_sqrt"], g.get("W"), g["noise"], info, ws=ws, qs_packed=qs_packed,
                       Yunc=Yunc)
    torch.cuda.synchronize()
    assert int(info.abs().max().item()) == 0
    if qs_packed:
        dense = torch.zeros((L, m, m), **f64)
        dense[:, tid, tjd] = g["q_sqrt"]
        g["q_sqrt"] = dense
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


# ---------------------------------------------------------------- 3. model level, value + gradient
def _shape_case(which, hbs):
    """(X, Y, L, M): the row-tile (16 rows a workgroup) sees N = 53 / 190 / 70 / 52, none a multiple;
    P = 65 crosses a 64-lane boundary; P = 130 halves the row tile (8 rows: LDS budget), and with
    L = 31 W no longer fits the kernel's LDS share and is read from global memory."""
    if which == "hbs":
        return hbs["X"], hbs["Y"], 4, 24
    n_lf, n_hf, d, P, L, Mi = {"syn190": (150, 40, 3, 6, 3, 40), "syn_p65": (50, 20, 3, 65, 2, 16),
                               "syn_p130": (40, 12, 3, 130, 2, 16), "syn_p130_l31": (40, 12, 3, 130, 31, 8)}[which]
    X, Y, _, _ = synthetic_multifidelity(n_lf, n_hf, d, P, 8, seed=40 + P)
    return X, Y, L, Mi


@pytest.mark.parametrize("which,kl_mult", [("hbs", 1.0), ("hbs", 0.3), ("syn190", 1.0), ("syn_p65", 1.0),
                                           ("syn_p130", 1.0), ("syn_p130_l31", 1.0)])
def test_het_latent_elbo_grad_vs_autograd(hbs, which, kl_mult):
    X, Y, L, Mi = _shape_case(which, hbs)
    U = synthetic_uncertainties(Y.shape, 11)
    Y2 = np.hstack([Y, U])
    m = _latent(X, Y2[:, :Y.shape[1]], L, Mi, heterosed=True)
    _randomize(m, 22)
    e, gd = m.elbo_and_grad((X, Y2), kl_multiplier=kl_mult)
    eo, ga = _autograd_grads(m, X, Y, U, m.kernel.W.numpy(), num_data=X.shape[0], kl_mult=kl_mult)
    _value_ok(e, eo, 1e-13)
    _check_grads(gd, ga, 1e-10)
    _value_ok(float(m.elbo((X, Y2)).numpy()), eo, 1e-13)      # the value-only entry point
    assert float(m.training_loss((X, Y2)).numpy()) == -float(m.elbo((X, Y2)).numpy())


# ---------------------------------------------------------------- 4. engine level, W = None
def _singlebin7(hbs, seed=21):
    X, Y = hbs["X"], np.ascontiguousarray(hbs["Y"][:, :7])
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(5)),
                        M.SquaredExponential(lengthscales=np.ones(5)), 7, Z=np.zeros((20, 6)))
    _randomize(m, seed)
    return m, X, Y


@pytest.mark.parametrize("qs_packed", [False, True])
def test_het_engine_identity_mixing(hbs, qs_packed):
    """W == NULL (L = P = 7, M = 20), Yunc a separate tensor whose row stride (11) differs from Y's (7);
    the q_sqrt layout travels in the call's qs_packed argument."""
    m, X, Y = _singlebin7(hbs)
    dev = Engine.get().device
    U = synthetic_uncertainties(Y.shape, 12)
    Yd = to_dev(Y, dev)
    Ubuf = torch.full((Y.shape[0], 11), float("nan"), dtype=torch.float64, device=dev)
    Ubuf[:, :7] = to_dev(U, dev)
    Ud = Ubuf[:, :7]
    assert Ud.stride(0) == 11 and Yd.stride(0) == 7
    out, gd = _engine_grad(m, X, Yd, Ud, qs_packed=qs_packed)
    eo, ga = _autograd_grads(m, X, Y, U)
    _value_ok(out[0], eo, 1e-13)
    _check_grads(gd, ga, 1e-10)
    eng, Z, thetas, q_mu, q_sqrt, W = m._dev_state()
    v, _, _, info = eng.svgp_elbo(to_dev(X, dev), Yd, Z, thetas, q_mu, q_sqrt, None, m._noise(), 1.0, DEFAULT_JITTER,
                                  Yunc=Ud)
    assert int(info.max().item()) == 0
    _value_ok(float(v[0].item()), eo, 1e-13)


# ---------------------------------------------------------------- 5. zeros are the homoscedastic call
@pytest.mark.parametrize("which", ["identity", "mixed"])
def test_het_zero_uncertainty_equals_homoscedastic(hbs, which):
    if which == "identity":
        m, X, Y = _singlebin7(hbs)
        scale = 1.0
    else:
        X, Y = hbs["X"], hbs["Y"]
        m = _latent(X, Y, 4, 24)
        _randomize(m, 23)
        scale = 1.7
    dev = Engine.get().device
    Yd = to_dev(Y, dev)
    out0, g0 = _engine_grad(m, X, Yd, None, qs_packed=True, kl_mult=0.6, scale=scale)
    out1, g1 = _engine_grad(m, X, Yd, torch.zeros_like(Yd), qs_packed=True, kl_mult=0.6, scale=scale)
    _close("out [elbo, KL, VE]", out1, out0, 1e-13 * np.abs(out0).max())
    _check_grads(g1, g0, 1e-12)
    eng, Z, thetas, q_mu, q_sqrt, W = m._dev_state()
    args = (to_dev(X, dev), Yd, Z, thetas, q_mu, q_sqrt, W, m._noise(), scale, DEFAULT_JITTER)
    v0 = eng.svgp_elbo(*args)[0].cpu().numpy()
    v1 = eng.svgp_elbo(*args, Yunc=torch.zeros_like(Yd))[0].cpu().numpy()
    _close("value-only out", v1, v0, 1e-13 * np.abs(v0).max())


# ---------------------------------------------------------------- 6. reproducibility
def test_het_gradients_bitwise_reproducible_and_workspace_independent(hbs):
    """Two calls at one state are bitwise equal, and stay so with the workspace filled with NaN bytes
    (0xFF) in between: no atomics, every partial the reductions read is written first in the same call."""
    X, Y = hbs["X"], hbs["Y"]
    m = _latent(X, Y, 4, 40)
    _randomize(m, 41)
    eng = Engine.get()
    U = synthetic_uncertainties(Y.shape, 13)
    Y2 = to_dev(np.hstack([Y, U]), eng.device)
    P = Y.shape[1]
    Yd, Ud = Y2[:, :P], Y2[:, P:]
    ws = eng.private_workspace(eng.svgp_grad_workspace_bytes(X.shape[0], 40, 4, P, X.shape[1] - 1))
    ws.fill_(255)
    runs = []
    for fill in (None, None, 255):
        if fill is not None:
            ws.fill_(fill)
        runs.append(_engine_grad(m, X, Yd, Ud, qs_packed=True, kl_mult=0.3, scale=1.0, ws=ws))
    for out, g in runs[1:]:
        np.testing.assert_array_equal(out, runs[0][0])
        for k, v in g.items():
            np.testing.assert_array_equal(v, runs[0][1][k], err_msg=k)
    eo, ga = _autograd_grads(m, X, Y, U, m.kernel.W.numpy(), kl_mult=0.3)
    _value_ok(runs[0][0][0], eo, 1e-13)
    _check_grads(runs[0][1], ga, 1e-10)


# ---------------------------------------------------------------- 7. / 8. training, prediction, save / load
TRAIN_KW = dict(num_latents=3, num_inducing=16, w_type='diagonal')


def _het_model(X, Y2, P):
    D = X.shape[1] - 1
    return M.LatentMFCoregionalizationSVGP(X, Y2, M.SquaredExponential(lengthscales=np.ones(D)),
                                           M.SquaredExponential(lengthscales=np.ones(D)), num_outputs=P,
                                           heterosed=True, **TRAIN_KW)


@pytest.fixture(scope="module")
def trained(hbs):
    """20 optimize() steps (graph replay, the default) of the heteroscedastic latent model on HBS."""
    X, Y = hbs["X"], hbs["Y"]
    Y2 = np.hstack([Y, synthetic_uncertainties(Y.shape, 14)])
    m = _het_model(X, Y2, Y.shape[1])
    m.optimize((X, Y2), max_iters=20, initial_lr=0.05)
    return m, X, Y, Y2


def test_het_latent_training_matches_oracle(hbs, trained):
    """The 1e-12 relative bound that test_latent_training_matches_oracle holds for the homoscedastic
    model at these shapes (HBS, L = 3, M = 16, 20 steps, lr 0.05)."""
    m, X, Y, Y2 = trained
    hist = np.array(m.loss_history)
    assert hist.shape == (20,) and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    v = m.likelihood.variance.numpy()
    assert v.shape == (1,) and v[0] != 1.0 and abs(v[0] - 1.0) > 1e-3      # trained from step 0
    ref = HetLatentTrainer(X, Y2, dict(TRAIN_KW, num_outputs=Y.shape[1]), lr=0.05, max_iters=20)
    oh = [ref.step() for _ in range(20)]
    _close("heteroscedastic -ELBO trajectory", hist, oh, 1e-12, rel=True)
    _close("trained baseline variance", v, ref.noise().detach().numpy(), 1e-10, rel=True)
    # without graph replay: the same trajectory, bit for bit
    m2 = _het_model(X, Y2, Y.shape[1])
    m2.optimize((X, Y2), max_iters=20, initial_lr=0.05, graph=False)
    np.testing.assert_array_equal(np.array(m2.loss_history), hist)
    np.testing.assert_array_equal(m2.likelihood.variance.numpy(), v)
    np.testing.assert_array_equal(m2.kernel.W.numpy(), m.kernel.W.numpy())


def test_het_predict_and_save_load(hbs, trained, tmp_path):
    m, X, Y, Y2 = trained
    Xs = hbs["Xtest"]
    mf, vf = m.predict_f(Xs)
    my, vy = m.predict_y(Xs)
    np.testing.assert_array_equal(my.numpy(), mf.numpy())
    s2 = m.likelihood.variance.numpy()[0]
    _close("predict_y - predict_f variance vs the baseline", vy.numpy() - vf.numpy(), np.full(vf.shape, s2), 1e-15)
    path = str(tmp_path / "het_latent.pkl")
    m.save_model(path)
    D = X.shape[1] - 1
    m2 = M.LatentMFCoregionalizationSVGP.load_model(
        path, X, Y2, M.SquaredExponential(lengthscales=np.ones(D)), M.SquaredExponential(lengthscales=np.ones(D)),
        TRAIN_KW["num_latents"], TRAIN_KW["num_inducing"], Y.shape[1], True, True)
    assert m2.likelihood.variance.shape == (1,)
    mf2, vf2 = m2.predict_f(Xs)
    np.testing.assert_array_equal(mf2.numpy(), mf.numpy())
    np.testing.assert_array_equal(vf2.numpy(), vf.numpy())
