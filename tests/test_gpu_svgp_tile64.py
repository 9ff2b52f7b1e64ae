"""Every SVGP entry point at tile size 64 (Engine.set_tile(64)): svgp_run<64> (k_svgp_cond<64> with an
explicit R = I, never the two-GEMM form), svgp_grad_run<64> (k_bgemm<64>, the sq<NB> / k_psi side of
Sigma_bar), svgp_predict_cov_run<64> and the batched k_chol_panel<64> / k_chol_update<64> steps.

Data: synthetic_multifidelity(150, 40, d = 5, P = 6): n = 190 is three 64-tiles with a partial last
one; 70 inducing points are two tiles with 6 rows in the second, 64 exactly one.  Every case is held
to the bound of its 32-tile twin (tests/test_gpu_svgp.py, test_gpu_svgp_het.py,
test_gpu_svgp_masked.py: ELBO 1e-13 relative, KL 1e-9, moments 1e-12, covariances 1e-10 max(1, |ref|),
gradients 1e-10 of each block's largest entry, the -ELBO trajectory 1e-12 relative) against the same
CPU oracles, and to the 32-tile result of the same model.  Every test prints its measured errors (-s).

Measured on an MI355X at tile 64: ELBO <= 3.4e-15 relative; moments <= 7.3e-14; gradients <= 4.1e-13 of a
block's largest entry (het 1.2e-13, masked 1.5e-13, NaN workspace 1.8e-13); 32 against 64: ELBO 3.4e-15,
gradients 4.0e-13, moments 7.2e-14; the five-step trajectory 5.0e-16 (8.3e-16 at tile 32).  Covariance
forms: latent 1.3e-13 (8 rows) / 3.3e-13 (70 rows); single bin 6.2e-12 / 1.4e-11, 7x under the 1e-10 bound.
That figure is the association's, not the tile's: the device forms G = Knn + Kuf^T (C^T C - Li^T Li) Kuf,
whose difference cancels at cond(K_uu) = 5.8e7, and the same expression in fp64 on the CPU differs from the
oracle's Knn - A^T A + B^T B by 6.3e-12 / 1.45e-11 on these inputs; the kernels are bitwise repeatable, so
the margin does not move from run to run."""
import functools

import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
import test_gpu_svgp_het as H
import test_gpu_svgp_masked as K
from _het_oracle import synthetic_uncertainties
from multi_fidelity_gpflow_amd.data import synthetic_multifidelity
from multi_fidelity_gpflow_amd.engine import Engine
from oracle import svgp_oracle as S
from test_gpu_svgp import _autograd_grads, _check_grads, _close, _oracle_state, _randomize, _value_ok

pytestmark = pytest.mark.gpu

D, P = 5, 6


@pytest.fixture(scope="module", autouse=True)
def tile64():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    e.set_tile(64)
    yield e
    e.set_tile(32)


@functools.lru_cache(maxsize=None)
def _data():
    X, Y, Xt, _ = synthetic_multifidelity(150, 40, D, P, 8, seed=64)
    assert X.shape == (190, D + 1) and Xt.shape == (8, D + 1)
    return X, Y, Xt


@functools.lru_cache(maxsize=None)
def _rows70():
    """70 prediction rows (more than one 64-column tile): the 8 HF test rows, then 62 rows near
    training inputs with the two fidelities alternating."""
    X, _, Xt = _data()
    rng = np.random.default_rng(70)
    Xs = X[rng.choice(X.shape[0], 62, replace=False)].copy()
    Xs[:, :-1] += 0.01 * rng.standard_normal((62, D))
    Xs[:, -1] = np.arange(62) % 2
    return np.vstack([Xt, Xs])


def _kern():
    return M.SquaredExponential(lengthscales=np.ones(D))


def _singlebin(seed=61, Mi=70):
    X, Y, _ = _data()
    m = M.SingleBinSVGP(X, Y, _kern(), _kern(), P, Z=np.zeros((Mi, D + 1)))
    _randomize(m, seed)
    return m


def _latent(Mi, seed=62, randomize=_randomize, Y=None, **kw):
    X, Y0, _ = _data()
    m = M.LatentMFCoregionalizationSVGP(X, Y0 if Y is None else Y, _kern(), _kern(), num_latents=3, num_inducing=Mi,
                                        num_outputs=P, w_type='diagonal', **kw)
    randomize(m, seed)
    return m


def _check_moments(m, Wm, Xs):
    Z, kps, q_mu, q_sqrt, W, _ = _oracle_state(m, Wm)
    mean, var = m.predict_f(Xs)
    gm, gv = S.latent_moments(torch.tensor(Xs), Z, kps, q_mu, q_sqrt)
    if W is not None:
        gm, gv = gm @ W.T, gv @ (W * W).T
    _close("predict mean", mean.numpy(), gm.numpy(), 1e-12)
    _close("predict var", var.numpy(), gv.numpy(), 1e-12)


# ---------------------------------------------------------------- 1. single bin
def test_singlebin_tile64(tile64):
    assert tile64.tile() == 64
    X, Y, Xt = _data()
    m = _singlebin()
    Z, kps, q_mu, q_sqrt, _, noise = _oracle_state(m)
    eo, klo, _ = S.elbo_t(torch.tensor(X), torch.tensor(Y), Z, kps, q_mu, q_sqrt, None, noise)
    _value_ok(float(m.elbo((X, Y))), float(eo), 1e-13)
    assert abs(m.prior_kl() - float(klo)) < 1e-9 * max(1, abs(float(klo)))
    _check_moments(m, None, Xt)
    _check_moments(m, None, _rows70())
    e, gd = m.elbo_and_grad((X, Y))
    ea, ga = _autograd_grads(m, X, Y)
    _value_ok(e, ea, 1e-13)
    _check_grads(gd, ga, 1e-10)


# ---------------------------------------------------------------- 2. latent model
@pytest.mark.parametrize("kl_mult", [1.0, 0.3])
@pytest.mark.parametrize("Mi", [70, 64])
def test_latent_tile64(Mi, kl_mult, tile64):
    X, Y, Xt = _data()
    m = _latent(Mi)
    assert m.inducing_variable.shape[0] == Mi
    Wm = m.kernel.W.numpy()
    Z, kps, q_mu, q_sqrt, W, noise = _oracle_state(m, Wm)
    eo, _, _ = S.elbo_t(torch.tensor(X), torch.tensor(Y), Z, kps, q_mu, q_sqrt, W, noise, num_data=X.shape[0])
    _value_ok(float(m.elbo((X, Y))), float(eo), 1e-13)
    _check_moments(m, Wm, Xt)
    _check_moments(m, Wm, _rows70())
    e, gd = m.elbo_and_grad((X, Y), kl_multiplier=kl_mult)
    ea, ga = _autograd_grads(m, X, Y, Wm, num_data=X.shape[0], kl_mult=kl_mult)
    _value_ok(e, ea, 1e-13)
    _check_grads(gd, ga, 1e-10)


# ---------------------------------------------------------------- 3. covariance forms
@pytest.mark.parametrize("rows", [8, 70])
@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_predict_f_covariance_forms_tile64(which, rows, tile64):
    """test_gpu_svgp.test_predict_f_covariance_forms at tile 64: 8 rows (one column tile) and 70 rows
    (two: the Knn Gram and G = Knn + Kuf^T F Kuf cross a 64-tile edge)."""
    m = _singlebin() if which == "singlebin" else _latent(70)
    Wm = None if which == "singlebin" else m.kernel.W.numpy()
    Xs = _data()[2] if rows == 8 else _rows70()
    ns = Xs.shape[0]
    assert ns == rows
    Z, kps, q_mu, q_sqrt, W, _ = _oracle_state(m, Wm)
    _, gc = S.latent_cov(torch.tensor(Xs), Z, kps, q_mu, q_sqrt)
    gv = torch.diagonal(gc, dim1=-2, dim2=-1).T.contiguous()   # [N*, L]
    mean0, var0 = m.predict_f(Xs)
    for fc, foc, shape in ((True, False, (P, ns, ns)), (False, True, (ns, P, P)), (True, True, (ns, P, ns, P))):
        mean, cov = m.predict_f(Xs, full_cov=fc, full_output_cov=foc)
        assert tuple(cov.shape) == shape
        ref = S.mix_cov(gc, gv, W, fc, foc).numpy()
        _close(f"cov {fc}/{foc}", cov.numpy(), ref, 1e-10 * max(1.0, np.abs(ref).max()))
        np.testing.assert_array_equal(mean.numpy(), mean0.numpy())
        c = cov.numpy()
        if fc and not foc:
            diag = np.diagonal(c, axis1=1, axis2=2).T
        elif foc and not fc:
            diag = np.diagonal(c, axis1=1, axis2=2)
        else:
            diag = np.stack([c[a, :, a, :].diagonal() for a in range(ns)])
        _close("cov diagonal vs var", diag, var0.numpy(), 1e-10)


# ---------------------------------------------------------------- 4. the other likelihoods
def test_het_latent_tile64(tile64):
    X, Y, _ = _data()
    U = synthetic_uncertainties(Y.shape, 11)
    Y2 = np.hstack([Y, U])
    m = _latent(70, seed=22, randomize=H._randomize, heterosed=True)
    e, gd = m.elbo_and_grad((X, Y2))
    eo, ga = H._autograd_grads(m, X, Y, U, m.kernel.W.numpy(), num_data=X.shape[0])
    H._value_ok(e, eo, 1e-13)
    H._check_grads(gd, ga, 1e-10)
    H._value_ok(float(m.elbo((X, Y2)).numpy()), eo, 1e-13)      # the value-only entry point


def test_masked_latent_tile64(tile64):
    X, Y, _ = _data()
    Yn, col = K._masked_targets(X, Y, 11)                       # one output (col) has no observation at all
    m = _latent(70, seed=22, randomize=K._randomize, Y=Yn, missing_outputs=True)
    assert m.likelihood.variance.shape == (P,)
    e, gd = m.elbo_and_grad((X, Yn))
    eo, ga = K._autograd_grads(m, X, Yn, m.kernel.W.numpy(), num_data=X.shape[0])
    K._value_ok(e, eo, 1e-13)
    K._check_grads(gd, ga, 1e-10)
    gn = np.asarray(gd["noise"])
    assert gn.shape == (P,) and gn[col] == 0.0 and ga["noise"][col] == 0.0
    assert np.all(np.asarray(gd["W"])[col] == 0.0)
    K._value_ok(float(m.elbo((X, Yn)).numpy()), eo, 1e-13)      # the value-only entry point


# ---------------------------------------------------------------- 5. workspace contents
def test_gradients_independent_of_workspace_contents_tile64(tile64):
    """test_gpu_svgp.test_gradients_independent_of_workspace_contents at tile 64, where the explicit
    R = I and the zero tiles above L^{-1} are written by other kernels than at 32 (the dense Gram and
    k_zero_upper_tiles with 64-wide tiles): NaN bytes in the workspace must not reach a gradient."""
    X, Y, _ = _data()
    m = _latent(70, seed=41)
    eng = tile64
    orig = eng.private_workspace
    eng.private_workspace = lambda nbytes: torch.full((int(nbytes),), 255, dtype=torch.uint8, device=eng.device)
    try:
        e, gd = m.elbo_and_grad((X, Y))
    finally:
        eng.private_workspace = orig
    eo, ga = _autograd_grads(m, X, Y, m.kernel.W.numpy(), num_data=X.shape[0])
    _value_ok(e, eo, 1e-13)
    _check_grads(gd, ga, 1e-10)


# ---------------------------------------------------------------- 6. tile 32 against tile 64
@pytest.mark.parametrize("which", ["singlebin", "latent70", "latent64"])
def test_tile32_and_tile64_agree(which, tile64):
    """The same model at both tile sizes: catches a 64-tile error that the oracle happens to share."""
    X, Y, Xt = _data()
    m = _singlebin() if which == "singlebin" else _latent(int(which[-2:]))
    res = {}
    try:
        for nb in (32, 64):
            tile64.set_tile(nb)
            e, gd = m.elbo_and_grad((X, Y))
            mean, var = m.predict_f(_rows70())
            res[nb] = (float(m.elbo((X, Y))), e, gd, mean.numpy(), var.numpy())
    finally:
        tile64.set_tile(64)
    _value_ok(res[64][0], res[32][0], 1e-13)
    _value_ok(res[64][1], res[32][1], 1e-13)
    _check_grads(res[64][2], res[32][2], 1e-10)
    _close("predict mean 64 vs 32", res[64][3], res[32][3], 1e-12)
    _close("predict var 64 vs 32", res[64][4], res[32][4], 1e-12)


# ---------------------------------------------------------------- 7. training
def test_latent_training_matches_oracle_tile64(tile64):
    """Five optimize() steps (one captured graph of five steps) at tile 32 and then, in the same
    process, at tile 64, each against the Adam / CosineDecay loop on the oracle's autograd gradients:
    the step graph of the second run is captured for the new tile."""
    X, Y, _ = _data()
    kw = dict(num_latents=3, num_inducing=70, num_outputs=P, w_type='diagonal')
    ref = S.LatentTrainer(X, Y, kw, lr=0.05, max_iters=5)
    oh = [ref.step() for _ in range(5)]
    try:
        for nb in (32, 64):
            tile64.set_tile(nb)
            m = M.LatentMFCoregionalizationSVGP(X, Y, _kern(), _kern(), **kw)
            m.optimize((X, Y), max_iters=5, initial_lr=0.05)
            hist = np.array(m.loss_history)
            assert hist.shape == (5,) and np.all(np.isfinite(hist))
            _close(f"latent -ELBO trajectory, tile {nb}", hist, oh, 1e-12, rel=True)
    finally:
        tile64.set_tile(64)
