"""Input gradients of the cached posterior on the HIP path: ``predict_f_vjp`` and the autograd attachment.

``mfgp_*_posterior_predict_vjp`` (the predict call's two launches and k_post_grad) against the CPU
references of tests/_input_grad_oracle.py, which tests/test_input_grad_oracle.py holds to a tenth of
the bounds used here.  Bounds (the project's own): |gX - ref|max <= 1e-9 max(1, |ref|max), predict_f's;
Goku 1e-8 |ref|max, the LML gradient's (Goku's factor enters twice at cond 7e5).  mean / var of the
call carry predict_f's bits.  Upstream gradients are seeded standard normals."""
import numpy as np
import pytest
import torch

import _input_grad_oracle as G
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType
from multi_fidelity_gpflow_amd.engine import Engine
from test_gpu_graph import _data as _graph_data, _model as _graph_model
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _err(name, gX, ref, bound=None):
    gX, ref = np.asarray(gX), np.asarray(ref)
    assert gX.shape == ref.shape, name
    amax = np.abs(ref).max()
    bound = G.BOUND * max(1.0, amax) if bound is None else bound
    err = np.abs(gX - ref).max()
    print(f"{name}: gX err {err:.1e} (|ref|max {amax:.1e}, bound {bound:.1e})")
    assert np.all(gX[:, -1] == 0.0), name
    assert err <= bound, (name, err)
    return err


def _np3(r):
    return r[0].numpy(), r[1].numpy(), r[2].numpy()


def _vjp_checked(name, post, Xs, gm, gv, ref, bound=None):
    """One VJP call: gX within the bound, mean / var equal to predict_f's bits, a second call bitwise equal."""
    mean, var, gX = _np3(post.predict_f_vjp(Xs, gm, gv))
    _err(name, gX, ref[2], bound)
    pm, pv = post.predict_f(Xs)
    np.testing.assert_array_equal(mean, pm.numpy())
    np.testing.assert_array_equal(var, pv.numpy())
    again = _np3(post.predict_f_vjp(Xs, gm, gv))
    for a, b in zip(again, (mean, var, gX)):
        np.testing.assert_array_equal(a, b)
    return mean, var, gX


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("case", G.GPR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpr_vjp_synthetic(case, nb, eng):
    """(n_lf, n_hf, P, D, N*) = (20, 5, 1, 1, 1): one tile, D = P = N* = 1; (70, 9, 3, 3, 33): three row
    tiles at NB = 32, a one-row tail in a second column tile; (150, 30, 65, 32, 70): more than 128 rows
    (two row groups), P across a 64-tile (two Z tiles per R tile at NB = 64, three at 32), D at the limit.
    Xnew mixes the fidelities.  References two ways on the CPU: 1.8e-15, 5.9e-13, 2.8e-14.
    Measured on an MI355X (NB = 32 / 64): 1.1e-15 / 1.8e-15, 5.6e-13 / 4.6e-13, 4.9e-14 / 5.2e-14
    (bounds 1.8e-9, 9.7e-9, 1.5e-8)."""
    X, Y, Xs, prm, gm, gv, ref = G.gpr_synthetic(*case)
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        _vjp_checked(f"gpr {case} nb{nb}", post, Xs, gm, gv, ref)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("which,nb", [("hbs", 32), ("hbs", 64), ("goku", 32)])
def test_gpr_vjp_datasets(which, nb, eng):
    """HBS (n = 53, P = 49, the 33-row mixed-fidelity Xnew) at both tiles and Goku (n = 1164, P = 64, its
    36 test rows; T = 37 row tiles in 8-tile chunks) at NB = 32, initial parameters.  Goku's bound is
    1e-8 |ref|max.  References two ways on the CPU: HBS 8.0e-14, Goku 1.3e-11.
    Measured on an MI355X: HBS 3.6e-13 (NB = 32) / 9.3e-14 (64), bound 1.5e-8; Goku 1.0e-11, bound 2.7e-7."""
    X, Y, Xs, prm, gm, gv, ref = G.gpr_dataset(which)
    assert Xs.shape[0] == (33 if which == "hbs" else 36)
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        bound = G.GOKU_BOUND * np.abs(ref[2]).max() if which == "goku" else None
        _vjp_checked(f"{which} nb{nb}", post, Xs, gm, gv, ref, bound)
    finally:
        eng.set_tile(32)


def test_gpr_vjp_edge_rows(eng):
    """A training row and an Xnew row with fidelity 0.9999999999999999 (neither 0 nor 1): that Xnew row's
    gradient is exactly 0 and the training row contributes nothing (the reference has the same zero
    row / column); an Xnew row equal to a training row (all differences 0 against it) stays in the bound.
    Measured on an MI355X: 4.6e-13 (bound 9.5e-9); the masked rows exactly 0."""
    n_lf, n_hf, P, D, ns = G.GPR_CASES[1]
    X, Y, Xs, prm, gm, gv, _ = G.gpr_synthetic(n_lf, n_hf, P, D, ns)
    X, Xs = X.copy(), Xs.copy()
    X[40, -1] = 0.9999999999999999
    Xs[5, -1] = 0.9999999999999999
    Xs[7] = X[3]
    Xs[8] = X[n_lf + 2]
    ref = G.gpr_vjp(X, Y, Xs, prm, gm, gv)
    post = _model(X, Y, prm).posterior()
    mean, var, gX = _vjp_checked("edge rows", post, Xs, gm, gv, ref)
    assert np.all(gX[5] == 0.0) and np.all(ref[2][5] == 0.0)
    assert np.all(mean[5] == 0.0) and np.all(var[5] == 0.0)
    # the masked training row contributes nothing: moving it leaves every bit in place
    X2 = X.copy()
    X2[40, :-1] += 0.25
    again = _np3(_model(X2, Y, prm).posterior().predict_f_vjp(Xs, gm, gv))
    np.testing.assert_array_equal(again[2], gX)


def test_gpr_vjp_argument_forms(eng):
    """grad_var=None equals a zero grad_var (and a [N*] grad_var equals the [N*, P] one it sums); grad_mean
    zeros / None with only grad_var set stays within the bound.
    Measured on an MI355X: grad_mean only 5.0e-13 (bound 9.6e-9); grad_var only 3.9e-14 (bound 1e-9)."""
    X, Y, Xs, prm, gm, gv, _ = G.gpr_synthetic(*G.GPR_CASES[1])
    post = _model(X, Y, prm).posterior()
    a = _np3(post.predict_f_vjp(Xs, gm))
    b = _np3(post.predict_f_vjp(Xs, gm, np.zeros_like(gv)))
    np.testing.assert_array_equal(a[2], b[2])
    _err("grad_mean only", a[2], G.gpr_vjp(X, Y, Xs, prm, gm, None)[2])
    ref_v = G.gpr_vjp(X, Y, Xs, prm, None, gv)[2]
    c = _np3(post.predict_f_vjp(Xs, np.zeros_like(gm), gv))
    _err("grad_var only (zero grad_mean)", c[2], ref_v)
    d = _np3(post.predict_f_vjp(Xs, None, gv))
    _err("grad_var only (grad_mean None)", d[2], ref_v)
    e = _np3(post.predict_f_vjp(Xs, gm, gv))
    f = _np3(post.predict_f_vjp(Xs, gm, torch.as_tensor(gv, device="cuda").sum(dim=1)))   # the sum the call forms
    np.testing.assert_array_equal(e[2], f[2])
    assert tuple(e[0].shape) == tuple(e[1].shape) == gm.shape and e[2].shape == Xs.shape
    with pytest.raises(ValueError):
        post.predict_f_vjp(Xs, gm[:, :1] if gm.shape[1] > 1 else gm[:1])
    empty = post.predict_f_vjp(Xs[:0], gm[:0], gv[:0])
    assert tuple(empty[2].shape) == (0, Xs.shape[1])


def test_gpr_vjp_snapshot(eng):
    """Like predict_f, the VJP is the snapshot's: new model parameters change nothing until update_cache().
    Measured on an MI355X after update_cache: 6.4e-13 (bound 1.2e-8)."""
    X, Y, Xs, prm, gm, gv, _ = G.gpr_synthetic(*G.GPR_CASES[1])
    m = _model(X, Y, prm)
    post = m.posterior()
    before = _np3(post.predict_f_vjp(Xs, gm, gv))
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.kernel.kernel_L.lengthscales.assign(0.8 * np.asarray(prm.lL))
    after = _np3(post.predict_f_vjp(Xs, gm, gv))
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b)
    new = prm.copy()
    new.rho, new.lL = np.full((Y.shape[1], 1), 1.234), 0.8 * np.asarray(prm.lL)
    post.update_cache()
    upd = _np3(post.predict_f_vjp(Xs, gm, gv))
    assert np.abs(upd[2] - before[2]).max() > 1e-3
    _err("after update_cache", upd[2], G.gpr_vjp(X, Y, Xs, new, gm, gv)[2])


def test_autograd_matches_vjp(eng):
    """torch.autograd.grad of sum(mean gm) + sum(var gv) through predict_f(Xnew.requires_grad_()) is the
    VJP call: the same bits.  Without requires_grad (or under no_grad) predict_f is detached as before; the
    covariance forms, NOCACHE posteriors and graph models raise NotImplementedError."""
    X, Y, Xs, prm, gm, gv, _ = G.gpr_synthetic(*G.GPR_CASES[1])
    m = _model(X, Y, prm)
    post = m.posterior()
    want = _np3(post.predict_f_vjp(Xs, gm, gv))
    for dev in ("cpu", "cuda"):
        Xt = torch.tensor(Xs, device=dev, requires_grad=True)
        mean, var = post.predict_f(Xt)
        assert mean.requires_grad and var.requires_grad
        np.testing.assert_array_equal(mean.numpy(), want[0])
        np.testing.assert_array_equal(var.numpy(), want[1])
        loss = (mean * torch.tensor(gm, device=mean.device)).sum() + (var * torch.tensor(gv, device=var.device)).sum()
        (g,) = torch.autograd.grad(loss, Xt)
        assert g.device == Xt.device and g.shape == Xt.shape
        np.testing.assert_array_equal(g.cpu().numpy(), want[2])
    Xt = torch.tensor(Xs, requires_grad=True)
    (g,) = torch.autograd.grad((post.predict_f(Xt)[0] * torch.tensor(gm, device="cuda")).sum(), Xt)   # var unused
    np.testing.assert_array_equal(g.numpy(), _np3(post.predict_f_vjp(Xs, gm))[2])
    with torch.no_grad():
        assert not post.predict_f(Xt)[0].requires_grad
    assert not post.predict_f(torch.tensor(Xs))[0].requires_grad
    with pytest.raises(NotImplementedError):
        post.predict_f(Xt, full_cov=True)
    with pytest.raises(NotImplementedError):
        post.predict_f(Xt, full_output_cov=True)
    nc = m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE)
    with pytest.raises(NotImplementedError):
        nc.predict_f_vjp(Xs, gm, gv)
    with pytest.raises(NotImplementedError):
        nc.predict_f(Xt)
    Xg, Yg = _graph_data(2, 3)
    gpost = _graph_model(Xg, Yg, 2, 3, asym=True).posterior()
    Xgs = Xg[:5].copy()
    with pytest.raises(NotImplementedError):
        gpost.predict_f_vjp(Xgs, np.zeros((5, Yg.shape[1])))
    with pytest.raises(NotImplementedError):
        gpost.predict_f(torch.tensor(Xgs, requires_grad=True))
    # SVGP: the same attachment
    sm, Wm, Xv = G.svgp_hbs_model("latent")
    spost = sm.posterior()
    sgm, sgv = G.upstream(Xv.shape[0], sm.num_outputs, 90)
    swant = _np3(spost.predict_f_vjp(Xv, sgm, sgv))
    Xt = torch.tensor(Xv, requires_grad=True)
    f_mu, f_var = spost.predict_f(Xt)
    loss = (f_mu * torch.tensor(sgm, device=f_mu.device)).sum() + (f_var * torch.tensor(sgv, device=f_var.device)).sum()
    (g,) = torch.autograd.grad(loss, Xt)
    np.testing.assert_array_equal(g.numpy(), swant[2])
    for kw in (dict(full_cov=True), dict(full_output_cov=True)):
        with pytest.raises(NotImplementedError):
            spost.predict_f(Xt, **kw)
    with pytest.raises(NotImplementedError):
        sm.posterior(precompute_cache=PrecomputeCacheType.NOCACHE).predict_f_vjp(Xv, sgm, sgv)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_vjp_hbs(which, eng):
    """The HBS single-bin model (M = 50, L = P = 49, no W: 2 x 2 x 49 = 196 < 256, chunked rows) and the
    HBS latent model (5 latents, M = 30, with W), Xnew of 8 + 33 rows (two column tiles); grad_var=None
    equals zeros, grad_var alone within the bound; snapshot semantics with q_mu changed.
    References two ways on the CPU: 1.9e-13 (single bin), 1.0e-14 (latent).
    Measured on an MI355X: single bin 1.4e-12 (bound 7.8e-9), grad_var only 2.4e-13, one row 5.5e-13, after
    update_cache 2.2e-12; latent 4.7e-14 (bound 1.7e-9), 2.4e-15, 1.0e-14, 7.7e-14."""
    m, Wm, Xs = G.svgp_hbs_model(which)
    state = G.svgp_state(m, Wm)
    gm, gv = G.upstream(Xs.shape[0], m.num_outputs, 90)
    post = m.posterior()
    assert isinstance(post, M.SVGPPosterior)
    got = _vjp_checked(f"svgp hbs {which}", post, Xs, gm, gv, G.svgp_vjp(state, Xs, gm, gv))
    a = _np3(post.predict_f_vjp(Xs, gm))
    b = _np3(post.predict_f_vjp(Xs, gm, np.zeros_like(gv)))
    np.testing.assert_array_equal(a[2], b[2])
    c = _np3(post.predict_f_vjp(Xs, None, gv))
    _err(f"svgp hbs {which} grad_var only", c[2], G.svgp_vjp(state, Xs, None, gv)[2])
    one = _np3(post.predict_f_vjp(Xs[:1], gm[:1], gv[:1]))
    _err(f"svgp hbs {which} one row", one[2], G.svgp_vjp(state, Xs[:1], gm[:1], gv[:1])[2])
    m.q_mu.assign(m.q_mu.numpy() + 0.25)
    after = _np3(post.predict_f_vjp(Xs, gm, gv))
    for x, y in zip(after, got):
        np.testing.assert_array_equal(x, y)
    post.update_cache()
    upd = _np3(post.predict_f_vjp(Xs, gm, gv))
    assert np.abs(upd[2] - got[2]).max() > 1e-3
    _err(f"svgp hbs {which} after update_cache", upd[2], G.svgp_vjp(G.svgp_state(m, Wm), Xs, gm, gv)[2])


@pytest.mark.parametrize("nb", [32, 64])
def test_svgp_vjp_eleven_latents(nb, eng):
    """A synthetic latent model with L = 11 latents (ggm = gm W and ggv = gv (W o W) per latent, the
    forward's 8 + 3 mixing loop), M = 70 (three row tiles at NB = 32, two at 64), P = 17, D = 5, N* = 33
    (a one-row tail in a second column tile at NB = 32).  Reference two ways on the CPU: 4.5e-14.
    Measured on an MI355X (NB = 32 / 64): 1.5e-13 / 2.1e-13 (bound 2.1e-9)."""
    ref_state, Xs, gm, gv, ref = G.svgp_synthetic()
    eng.set_tile(nb)
    try:
        m, Xs2 = G.svgp_synthetic_model()
        np.testing.assert_array_equal(Xs2, Xs)
        Wm = m.kernel.W.numpy()
        assert Wm.shape == (17, 11) and np.count_nonzero(Wm[:, 8:]) > 0
        _vjp_checked(f"svgp L=11 nb{nb}", m.posterior(), Xs, gm, gv, ref)
    finally:
        eng.set_tile(32)
