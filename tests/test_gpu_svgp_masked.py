"""MaskedGaussian SVGP path (mfgp_svgp_elbo_masked / mfgp_svgp_elbo_grad_masked: k_svgp_ve_masked, the
row-tiled reverse kernel k_ve_bwd_masked, k_ve_masked_nreduce and k_ve_het_reduce) against torch
autograd through the fp64 restatement tests/_masked_oracle.py, which test_masked_host.py ties to the
KAT-pinned oracle.

Bounds are the homoscedastic pipeline's own (tests/test_gpu_svgp.py): ELBO 1e-13 relative, every
gradient block 1e-10 of its largest entry, the 20-step training trajectory 1e-12 relative.  The masks
are seeded (_masked_oracle.synthetic_mask): about 30% scattered NaN, one row and one column entirely
NaN, and every LF row missing the last third of the columns; the per-output noise is 0.05-0.15.
The training tests use the block mask alone plus one fully missing column (_block_targets), with W
windows that reach observed columns (TRAIN_KW says why).  Every test prints its measured errors (-s)."""
import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from multi_fidelity_gpflow_amd.engine import Engine, theta_size, to_dev
from multi_fidelity_gpflow_amd.svgp import DEFAULT_JITTER

from _masked_oracle import MaskedLatentTrainer, apply_mask, masked_elbo_t, synthetic_mask

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- helpers (after tests/test_gpu_svgp_het.py)
def _oracle_state(model, W=None, noise=None):
    D = model.inducing_variable.shape[1] - 1
    kps = []
    for k in model.kernel.kernels:
        t = k.theta_vector(D)
        kps.append(dict(vL=torch.tensor(t[0]), lL=torch.tensor(t[1:1 + D]), vD=torch.tensor(t[1 + D]),
                        lD=torch.tensor(t[2 + D:2 + 2 * D]), rho=torch.tensor(t[2 + 2 * D])))
    nv = model.likelihood.variance.numpy() if noise is None else noise
    noise = torch.tensor(np.reshape(nv, -1), dtype=torch.float64)
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
    v = model.likelihood.variance
    v.assign(0.05 + rng.random(v.shape) * 0.1)


def _autograd_grads(model, X, Y, W=None, noise=None, num_data=None, kl_mult=1.0):
    """d(VE*scale - kl_mult*KL)/d(constrained params) by torch autograd through masked_elbo_t."""
    D = model.inducing_variable.shape[1] - 1
    Z, kps, q_mu, q_sqrt, Wt, noise = _oracle_state(model, W, noise)
    leaves = [Z, q_mu, q_sqrt, noise] + ([Wt] if Wt is not None else [])
    for kp in kps:
        leaves += list(kp.values())
    for t in leaves:
        t.requires_grad_(True)
    e, kl, ve = masked_elbo_t(torch.tensor(X), torch.tensor(Y), Z, kps, q_mu, q_sqrt, Wt, noise, num_data=num_data)
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
        assert np.all(np.isfinite(got)), k
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


def _masked_targets(X, Y, seed):
    """(Y with NaN, full_col); asserts on the mask itself what the module docstring promises."""
    P = Y.shape[1]
    miss, row, col = synthetic_mask(X, P, seed)
    obs = ~miss
    lf = np.asarray(X)[:, -1] == 0
    assert miss[row].all() and miss[:, col].all()
    assert miss[np.ix_(lf, np.arange(P) >= P - P // 3)].all() and P // 3 >= 1
    assert 0.3 < miss.mean() < 0.9
    assert all(obs[:, c].sum() >= 2 for c in range(P) if c != col)
    Yn = apply_mask(Y, miss)
    assert np.array_equal(np.isnan(Yn), miss)
    return Yn, col


def _engine_grad(model, X, Y, noise, masked, qs_packed=False, kl_mult=1.0, scale=1.0, ws=None):
    """One Engine.svgp_elbo_grad call at the model's state.  Y: a device tensor (a view is allowed);
    noise: a host array of 1 or P variances; masked False: the existing homoscedastic entry point.
    Returns (out[3], gradients by name, q_sqrt's unpacked to [L, M, M])."""
    eng, Z, thetas, q_mu, q_sqrt, W = model._dev_state()
    Xd = to_dev(X, eng.device)
    n, m, L, p, d = Xd.shape[0], Z.shape[0], thetas.shape[0], Y.shape[1], Xd.shape[1] - 1
    f64 = dict(dtype=torch.float64, device=eng.device)
    ti, tj = np.tril_indices(m)
    tid, tjd = torch.as_tensor(ti, device=eng.device), torch.as_tensor(tj, device=eng.device)
    qs = q_sqrt[:, tid, tjd].contiguous() if qs_packed else q_sqrt
    noise = torch.tensor(np.reshape(noise, -1), **f64)
    out, g_mu, g_var = torch.zeros(3, **f64), torch.empty((L, n), **f64), torch.empty((L, n), **f64)
    g = dict(Z=torch.zeros((m, d + 1), **f64), theta=torch.zeros((L, theta_size(d)), **f64),
             q_mu=torch.zeros((m, L), **f64), q_sqrt=torch.zeros_like(qs),
             noise=torch.full((noise.numel(),), float("nan"), **f64))
    if W is not None:
        g["W"] = torch.zeros((p, L), **f64)
    info = torch.zeros((L,), dtype=torch.int32, device=eng.device)
    eng.svgp_elbo_grad(Xd, Y, Z, thetas, q_mu, qs, W, noise, scale, kl_mult, DEFAULT_JITTER, out, g_mu, g_var, g["Z"],
                       g["theta"], g["q_mu"], g["q_sqrt"], g.get("W"), g["noise"], info, ws=ws, qs_packed=qs_packed,
                       masked=masked)
    torch.cuda.synchronize()
    assert int(info.abs().max().item()) == 0
    if qs_packed:
        dense = torch.zeros((L, m, m), **f64)
        dense[:, tid, tjd] = g["q_sqrt"]
        g["q_sqrt"] = dense
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


# ---------------------------------------------------------------- 1. model level, value + gradient
def _shape_case(which, hbs):
    """(X, Y, L, M): the row tile (16 rows a workgroup) sees N = 53 / 190 / 70 / 52, none a multiple;
    P = 65 crosses a 64-lane boundary; P = 130 halves the row tile (8 rows: the LDS budget), and with
    L = 31 W no longer fits the kernel's LDS share and is read from global memory."""
    if which == "hbs":
        return hbs["X"], hbs["Y"], 4, 24
    n_lf, n_hf, d, P, L, Mi = {"syn190": (150, 40, 3, 6, 3, 40), "syn_p65": (50, 20, 3, 65, 2, 16),
                               "syn_p130": (40, 12, 3, 130, 2, 16), "syn_p130_l31": (40, 12, 3, 130, 31, 8)}[which]
    X, Y, _, _ = synthetic_multifidelity(n_lf, n_hf, d, P, 8, seed=40 + P)
    return X, Y, L, Mi


@pytest.mark.parametrize("which,kl_mult", [("hbs", 1.0), ("hbs", 0.3), ("syn190", 1.0), ("syn_p65", 1.0),
                                           ("syn_p130", 1.0), ("syn_p130_l31", 1.0)])
def test_masked_latent_elbo_grad_vs_autograd(hbs, which, kl_mult):
    X, Y, L, Mi = _shape_case(which, hbs)
    Yn, col = _masked_targets(X, Y, 11)
    m = _latent(X, Yn, L, Mi, missing_outputs=True)
    _randomize(m, 22)
    assert m.likelihood.variance.shape == (Y.shape[1],)
    e, gd = m.elbo_and_grad((X, Yn), kl_multiplier=kl_mult)
    eo, ga = _autograd_grads(m, X, Yn, m.kernel.W.numpy(), num_data=X.shape[0], kl_mult=kl_mult)
    _value_ok(e, eo, 1e-13)
    _check_grads(gd, ga, 1e-10)
    gn = np.asarray(gd["noise"])
    assert gn.shape == (Y.shape[1],) and gn[col] == 0.0 and ga["noise"][col] == 0.0
    assert np.all(np.asarray(gd["W"])[col] == 0.0)
    _value_ok(float(m.elbo((X, Yn)).numpy()), eo, 1e-13)      # the value-only entry point
    assert float(m.training_loss((X, Yn)).numpy()) == -float(m.elbo((X, Yn)).numpy())


# ---------------------------------------------------------------- 2. engine level, W = None
def _singlebin7(hbs, seed=21, **kw):
    X, Y = hbs["X"], np.ascontiguousarray(hbs["Y"][:, :7])
    m = M.SingleBinSVGP(X, Y, M.SquaredExponential(lengthscales=np.ones(5)),
                        M.SquaredExponential(lengthscales=np.ones(5)), 7, Z=np.zeros((20, 6)), **kw)
    _randomize(m, seed)
    return m, X, Y


@pytest.mark.parametrize("qs_packed", [False, True])
@pytest.mark.parametrize("pn", [1, 7])
def test_masked_engine_identity_mixing(hbs, qs_packed, pn):
    """W == NULL (L = P = 7, M = 20), Y a view whose row stride (11) differs from P; the q_sqrt layout
    travels in the call's qs_packed argument; one shared variance (pn = 1) or one per output."""
    m, X, Y = _singlebin7(hbs)
    dev = Engine.get().device
    Yn, col = _masked_targets(X, Y, 12)
    Ybuf = torch.full((Y.shape[0], 11), 7.0, dtype=torch.float64, device=dev)
    Ybuf[:, :7] = to_dev(Yn, dev)
    Yd = Ybuf[:, :7]
    assert Yd.stride(0) == 11
    noise = 0.05 + np.random.default_rng(5).random(pn) * 0.1
    out, gd = _engine_grad(m, X, Yd, noise, True, qs_packed=qs_packed)
    eo, ga = _autograd_grads(m, X, Yn, noise=noise)
    _value_ok(out[0], eo, 1e-13)
    _check_grads(gd, ga, 1e-10)
    assert gd["noise"].shape == (pn,)
    if pn == 7:
        assert gd["noise"][col] == 0.0
    eng, Z, thetas, q_mu, q_sqrt, W = m._dev_state()
    v, _, _, info = eng.svgp_elbo(to_dev(X, dev), Yd, Z, thetas, q_mu, q_sqrt, None, to_dev(noise, dev), 1.0,
                                  DEFAULT_JITTER, masked=True)
    assert int(info.max().item()) == 0
    _value_ok(float(v[0].item()), eo, 1e-13)


# ---------------------------------------------------------------- 3. no NaN, pn = 1: the homoscedastic call
@pytest.mark.parametrize("which", ["identity", "mixed"])
def test_masked_without_nan_equals_homoscedastic(hbs, which):
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
    noise = np.array([m._noise()])
    out0, g0 = _engine_grad(m, X, Yd, noise, False, qs_packed=True, kl_mult=0.6, scale=scale)
    out1, g1 = _engine_grad(m, X, Yd, noise, True, qs_packed=True, kl_mult=0.6, scale=scale)
    _close("out [elbo, KL, VE]", out1, out0, 1e-13 * np.abs(out0).max())
    _check_grads(g1, g0, 1e-12)
    eng, Z, thetas, q_mu, q_sqrt, W = m._dev_state()
    args = (to_dev(X, dev), Yd, Z, thetas, q_mu, q_sqrt, W)
    v0 = eng.svgp_elbo(*args, m._noise(), scale, DEFAULT_JITTER)[0].cpu().numpy()
    v1 = eng.svgp_elbo(*args, to_dev(noise, dev), scale, DEFAULT_JITTER, masked=True)[0].cpu().numpy()
    _close("value-only out", v1, v0, 1e-13 * np.abs(v0).max())


# ---------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("pn", [1, 49])
def test_masked_gradients_bitwise_reproducible_and_workspace_independent(hbs, pn):
    """Two calls at one state are bitwise equal, and stay so with the workspace filled with NaN bytes
    (0xFF) in between: no atomics, every partial the reductions read is written first in the same call."""
    X, Y = hbs["X"], hbs["Y"]
    m = _latent(X, Y, 4, 40)
    _randomize(m, 41)
    eng = Engine.get()
    Yn, col = _masked_targets(X, Y, 13)
    Yd = to_dev(Yn, eng.device)
    P = Y.shape[1]
    noise = 0.05 + np.random.default_rng(6).random(pn) * 0.1
    ws = eng.private_workspace(eng.svgp_grad_workspace_bytes(X.shape[0], 40, 4, P, X.shape[1] - 1))
    ws.fill_(255)
    runs = []
    for fill in (None, None, 255):
        if fill is not None:
            ws.fill_(fill)
        runs.append(_engine_grad(m, X, Yd, noise, True, qs_packed=True, kl_mult=0.3, scale=1.0, ws=ws))
    for out, g in runs[1:]:
        np.testing.assert_array_equal(out, runs[0][0])
        for k, v in g.items():
            np.testing.assert_array_equal(v, runs[0][1][k], err_msg=k)
    eo, ga = _autograd_grads(m, X, Yn, m.kernel.W.numpy(), noise=noise, kl_mult=0.3)
    _value_ok(runs[0][0][0], eo, 1e-13)
    _check_grads(runs[0][1], ga, 1e-10)


# ---------------------------------------------------------------- 5. / 6. training, prediction, save / load
# window_fraction = 1.0: every latent's window of W reaches columns that the LF rows observe.  With the
# constructor's default (0.4) latent 2 (columns 39..48) lies wholly inside the block mask and sees the 3
# HF rows alone; entries of its q_mu / q_sqrt gradient are then 1e-7 .. 1e-17, at or below Adam's epsilon
# (1e-7), where a step is lr g / eps and a rounding-level difference in g grows ~1e4 a step.  A 20-step
# trajectory is then not determined to 1e-12 by ANY implementation: the torch oracle's own moves by
# 5e-13 .. 1.4e-11 when X changes by one ulp (six draws; 1.6e-16 .. 3.1e-16 with no mask), the device's own
# by 9e-12 .. 6e-11, and the two differ by 1.7e-10 (2.2e-10 at step 19; variances 1.5e-11).  At 1.0 the
# oracle's own change under the same draws is 1.1e-16 .. 4.3e-16, so the comparison measures the code.
TRAIN_KW = dict(num_latents=3, num_inducing=16, w_type='diagonal', window_fraction=1.0)


def _masked_model(X, Yn, **kw):
    D = X.shape[1] - 1
    return M.LatentMFCoregionalizationSVGP(X, Yn, M.SquaredExponential(lengthscales=np.ones(D)),
                                           M.SquaredExponential(lengthscales=np.ones(D)), num_outputs=Yn.shape[1],
                                           **TRAIN_KW, **kw)


def _block_targets(X, Y, seed):
    """The multi-fidelity block mask alone (every LF row misses the last third of the columns) plus one
    drawn column entirely missing: (Y with NaN, that column)."""
    P = Y.shape[1]
    miss = np.zeros(Y.shape, bool)
    miss[np.ix_(np.asarray(X)[:, -1] == 0, np.arange(P) >= P - P // 3)] = True
    col = int(np.random.default_rng(seed).integers(P))
    miss[:, col] = True
    assert all((~miss)[:, c].sum() >= 2 for c in range(P) if c != col)
    return apply_mask(Y, miss), col


@pytest.fixture(scope="module")
def trained(hbs):
    """20 optimize() steps (graph replay, the default) of the masked latent model on HBS, block mask."""
    X, Y = hbs["X"], hbs["Y"]
    Yn, col = _block_targets(X, Y, 14)
    m = _masked_model(X, Yn, missing_outputs=True)
    v0 = m.likelihood.variance.numpy().copy()
    m.optimize((X, Yn), max_iters=20, initial_lr=0.05)
    return m, X, Yn, col, v0


def test_masked_latent_training_matches_oracle(hbs, trained):
    """The 1e-12 relative bound that test_latent_training_matches_oracle holds for the homoscedastic
    model at these shapes (HBS, L = 3, M = 16, 20 steps, lr 0.05), trained variances to 1e-10.
    The block mask plus one fully missing column; W windows as TRAIN_KW explains (the case has to be
    one whose reference trajectory is itself determined beyond the bound)."""
    m, X, Yn, col, v0 = trained
    P = Yn.shape[1]
    hist = np.array(m.loss_history)
    v = m.likelihood.variance.numpy()
    ref = MaskedLatentTrainer(X, Yn, dict(TRAIN_KW, num_outputs=P), lr=0.05, max_iters=20)
    oh = np.array([ref.step() for _ in range(20)])
    print("per-step rel err", " ".join(f"{e:.1e}" for e in np.abs(hist - oh) / np.abs(oh)))
    _close("masked -ELBO trajectory", hist, oh, 1e-12, rel=True)
    _close("trained variances", v, ref.noise().detach().numpy(), 1e-10, rel=True)
    assert v[col] == v0[col]                                             # no observation: Adam left it alone


def test_masked_latent_training_invariants(hbs, trained):
    """Every observed output's variance is trained
    from step 0, the unobserved output's is untouched bit for bit, and graph replay, eager stepping and
    an assigned likelihood give one trajectory."""
    m, X, Yn, col, v0 = trained
    P = Yn.shape[1]
    hist = np.array(m.loss_history)
    assert hist.shape == (20,) and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    v = m.likelihood.variance.numpy()
    keep = np.arange(P) != col
    assert v.shape == (P,) and np.all(np.abs(v[keep] - 1.0) > 1e-3)      # trained from step 0
    assert v[col] == v0[col]                                             # no observation: Adam left it alone
    assert np.unique(v[keep]).size > 1                                   # one variance per output
    # without graph replay, and with the likelihood assigned after construction: the same trajectory, bit for bit
    m2 = _masked_model(X, Yn)
    assert type(m2.likelihood) is M.Gaussian
    m2.likelihood = M.MaskedGaussian(variance=np.ones(P))
    m2.optimize((X, Yn), max_iters=20, initial_lr=0.05, graph=False)
    np.testing.assert_array_equal(np.array(m2.loss_history), hist)
    np.testing.assert_array_equal(m2.likelihood.variance.numpy(), v)
    np.testing.assert_array_equal(m2.kernel.W.numpy(), m.kernel.W.numpy())


def test_masked_singlebin_with_assigned_likelihood(hbs):
    """The single-bin model, flag or assigned likelihood: value against the oracle, a short optimize, and
    a shared () variance through the model (pn = 1)."""
    m, X, Y = _singlebin7(hbs, missing_outputs=True)
    Yn, col = _masked_targets(X, Y, 15)
    eo, _ = _autograd_grads(m, X, Yn)
    _value_ok(float(m.elbo((X, Yn)).numpy()), eo, 1e-13)
    s, _, _ = _singlebin7(hbs)
    s.likelihood = M.MaskedGaussian(0.3)
    assert s.likelihood.variance.shape == ()
    eo, ga = _autograd_grads(s, X, Yn)
    e, gd = s.elbo_and_grad((X, Yn))
    _value_ok(e, eo, 1e-13)
    _check_grads(gd, ga, 1e-10)
    v0 = m.likelihood.variance.numpy().copy()
    m.optimize((X, Yn), max_iters=3, initial_lr=0.01)
    v = m.likelihood.variance.numpy()
    assert len(m.loss_history) == 3 and np.all(np.isfinite(m.loss_history))
    assert v.shape == (7,) and v[col] == v0[col] and np.all(v[np.arange(7) != col] != v0[np.arange(7) != col])


def test_masked_predict_and_save_load(hbs, trained, tmp_path):
    m, X, Yn, col, v0 = trained
    Xs = hbs["Xtest"]
    P = Yn.shape[1]
    mf, vf = m.predict_f(Xs)
    my, vy = m.predict_y(Xs)
    assert tuple(mf.shape) == tuple(vf.shape) == tuple(my.shape) == tuple(vy.shape) == (Xs.shape[0], P)
    np.testing.assert_array_equal(my.numpy(), mf.numpy())
    s2 = m.likelihood.variance.numpy()
    np.testing.assert_array_equal(vy.numpy(), vf.numpy() + s2[None, :])
    _close("predict_y - predict_f variance vs variance[None, :]", vy.numpy() - vf.numpy(),
           np.broadcast_to(s2[None, :], vf.shape), 1e-15)
    path = str(tmp_path / "masked_latent.pkl")
    m.save_model(path)
    D = X.shape[1] - 1
    m2 = M.LatentMFCoregionalizationSVGP.load_model(
        path, X, Yn, M.SquaredExponential(lengthscales=np.ones(D)), M.SquaredExponential(lengthscales=np.ones(D)),
        TRAIN_KW["num_latents"], TRAIN_KW["num_inducing"], P, missing_outputs=True)
    assert type(m2.likelihood) is M.MaskedGaussian
    np.testing.assert_array_equal(m2.likelihood.variance.numpy(), s2)
    mf2, vf2 = m2.predict_f(Xs)
    my2, vy2 = m2.predict_y(Xs)
    np.testing.assert_array_equal(mf2.numpy(), mf.numpy())
    np.testing.assert_array_equal(vf2.numpy(), vf.numpy())
    np.testing.assert_array_equal(vy2.numpy(), vy.numpy())
    np.testing.assert_array_equal(float(m2.elbo((X, Yn)).numpy()), float(m.elbo((X, Yn)).numpy()))
    # NaN targets under the plain Gaussian are not masked silently: the old behaviour
    g = _masked_model(X, Yn)
    assert type(g.likelihood) is M.Gaussian
    assert np.isnan(float(g.elbo((X, Yn)).numpy()))
