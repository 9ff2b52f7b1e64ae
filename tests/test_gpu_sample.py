"""Joint posterior draws on the HIP path: mfgp_mvn_sample (Engine.mvn_sample: the tile Cholesky that keeps
L and the triangular product L eps) against numpy, and ``predict_f_samples`` of the posteriors and the
four models against the CPU oracles (tests/_sample_oracle.py).

Bounds.  Forward: 1e-9 max(1, |ref|max) at cond <= 1e3 (asserted on the host): the forward error of a
backward-stable Cholesky is <~ c n cond u = 10 x 130 x 1e3 x 1.1e-16 = 1.4e-10.  Backward, independent of
the conditioning: max |L L^T - (Sigma + jitter I)| <= 1e-12 max|Sigma| on the lower triangle (c n u with a
wide margin at n <= 130).  Model level: the bounds the existing full_cov parity tests hold the covariance
to (tests/test_gpu_posterior.py: 1e-9 for GPR and the graph model; tests/test_gpu_svgp.py: 1e-10 max(1,
|ref|max) for SVGP)."""
import functools

import numpy as np
import pytest
import torch

import _input_grad_oracle as G
import _sample_oracle as SO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType
from multi_fidelity_gpflow_amd.engine import Engine
from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O
from oracle import svgp_oracle as S
from test_gpu_graph import _model as _graph_model, _oracle_params as _graph_oracle_params
from test_gpu_parity import _model, _oracle_params
from test_gpu_posterior import _graph_case, _syn_gpr

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 70, 130]
SHAPES = [(1, 1, 1), (1, 5, 3), (1, 64, 2), (3, 1, 7)]   # (batch, ncol, nsamp)
NSTAR = 35


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


@functools.lru_cache(maxsize=None)
def _sigma(n, batch, ill=False):
    """Q diag(lambda) Q^T: lambda log-spaced in [1e-2, 1e1] (cond 1e3), or posterior-like down to exactly 0."""
    if ill:
        return SO.spd(n, batch, 1000 + n, lam_hi=1e1, lam_lo=1e-9, zeros=max(1, n // 4) if n > 1 else 0)
    Sg = SO.spd(n, batch, 2000 + n)
    for b in range(batch):
        assert np.linalg.cond(Sg[b]) <= 1e3 * (1 + 1e-9)
    return Sg


def _dev_cov(eng, Sg, pad=3):
    """A device view [B, n, n] with ldc = n + pad whose upper triangle (and padding) is NaN."""
    b, n, _ = Sg.shape
    buf = np.full((b, n, n + pad), np.nan)
    buf[:, :, :n] = np.where(np.tri(n, dtype=bool)[None], Sg, np.nan)
    t = torch.tensor(buf, device=eng.device)
    view = t[:, :, :n]
    assert n == 1 or (view.stride(1) == n + pad and not view.is_contiguous())
    return view


def _call(eng, Sg, mean, eps, ncol, jitter=SO.JITTER):
    out, info = eng.mvn_sample(_dev_cov(eng, Sg), torch.tensor(mean, device=eng.device),
                               torch.tensor(eps, device=eng.device), ncol, jitter)
    return out.cpu().numpy(), info.cpu().numpy()


def _reference(Sg, mean, eps, ncol, jitter=SO.JITTER):
    cov = np.repeat(Sg, ncol, axis=0)   # output column b * ncol + c draws from Sigma_b
    return SO.sample_mvn(mean, cov, eps, True, jitter)


@pytest.mark.parametrize("n", SIZES)
def test_mvn_sample_against_numpy(n, eng):
    """n below, at and just above a tile, three tiles with a ragged last one, five tiles (a panel tile updated
    by several earlier columns) x a single column, a ragged 16-column block, several column blocks, a
    batched single-column case; ldc = n + 3 and a NaN upper triangle.  Bound 1e-9 max(1, |ref|max)."""
    for batch, ncol, nsamp in SHAPES:
        Sg = _sigma(n, batch)
        rng = np.random.default_rng(n * 100 + batch * 10 + ncol)
        w = batch * ncol
        mean, eps = rng.standard_normal((n, w)), rng.standard_normal((nsamp, n, w))
        got, info = _call(eng, Sg, mean, eps, ncol)
        ref = _reference(Sg, mean, eps, ncol)
        err, scale = np.abs(got - ref).max(), max(1.0, np.abs(ref).max())
        print(f"n={n} batch={batch} ncol={ncol} nsamp={nsamp}: err {err:.2e} (bound {1e-9 * scale:.2e})")
        assert not info.any(), info
        assert got.shape == (nsamp, n, w)
        assert err <= 1e-9 * scale


@pytest.mark.parametrize("ill", [False, True], ids=["cond1e3", "posterior-like"])
@pytest.mark.parametrize("n", SIZES)
def test_mvn_sample_backward_error(n, ill, eng):
    """Identity draws (nsamp = n, eps[s, j, c] = delta_sj, mean 0): out is L.  |L L^T - (Sigma + jitter I)| <=
    1e-12 max|Sigma| on the lower triangle whatever the conditioning (lambda down to exactly 0 with jitter
    1e-6 in the posterior-like case), and L's upper triangle is exactly zero."""
    for batch, ncol, _ in SHAPES:
        Sg = _sigma(n, batch, ill)
        w = batch * ncol
        mean = np.zeros((n, w))
        got, info = _call(eng, Sg, mean, SO.identity_eps(n, w), ncol)
        assert not info.any(), info
        L = SO.factors_from_identity_draws(got, mean)   # [w, n, n]
        assert not np.triu(L, 1).any()
        worst = 0.0
        for q in range(w):
            A = Sg[q // ncol] + SO.JITTER * np.eye(n)
            worst = max(worst, np.abs(np.tril(L[q] @ L[q].T - A)).max() / np.abs(Sg[q // ncol]).max())
            if q % ncol:
                np.testing.assert_array_equal(L[q], L[q - 1])   # one factor serves the ncol columns
        print(f"n={n} ill={ill} batch={batch} ncol={ncol}: backward error {worst:.2e} max|Sigma| (bound 1e-12)")
        assert worst <= 1e-12


def test_mvn_sample_determinism_and_info(eng):
    """Two calls on the same inputs give the same bits; in a batch of 3 with entry 1 = -I, info is [0, 1, 0]
    and entries 0 and 2 still match numpy; n = 0 and nsamp = 0 are no-ops."""
    n, ncol, nsamp = 70, 1, 7
    Sg = _sigma(n, 3).copy()
    rng = np.random.default_rng(11)
    mean, eps = rng.standard_normal((n, 3)), rng.standard_normal((nsamp, n, 3))
    a, ia = _call(eng, Sg, mean, eps, ncol)
    b, ib = _call(eng, Sg, mean, eps, ncol)
    np.testing.assert_array_equal(a, b)
    assert not ia.any() and not ib.any()
    ref = _reference(Sg, mean, eps, ncol)
    Sg[1] = -np.eye(n)
    got, info = _call(eng, Sg, mean, eps, ncol)
    np.testing.assert_array_equal(info, [0, 1, 0])
    for q in (0, 2):
        err = np.abs(got[:, :, q] - ref[:, :, q]).max()
        print(f"entry {q} beside a failed one: err {err:.2e}")
        assert err <= 1e-9 * max(1.0, np.abs(ref).max())
        np.testing.assert_array_equal(got[:, :, q], a[:, :, q])
    # a failure past the first tile column: rows 0..39 fine, pivot 41 negative
    bad = _sigma(n, 1).copy()
    bad[0, 40, :] = bad[0, :, 40] = 0.0
    bad[0, 40, 40] = -1.0
    _, info = _call(eng, bad, mean[:, :1], eps[:, :, :1], 1)
    np.testing.assert_array_equal(info, [41])
    out, info = eng.mvn_sample(torch.empty((2, 0, 0), dtype=torch.float64, device=eng.device),
                               torch.empty((0, 2), dtype=torch.float64, device=eng.device),
                               torch.empty((3, 0, 2), dtype=torch.float64, device=eng.device), 1)
    assert tuple(out.shape) == (3, 0, 2) and not info.cpu().numpy().any()
    out, info = _call(eng, _sigma(33, 1), mean[:33, :1], np.empty((0, 33, 1)), 1)
    assert out.shape == (0, 33, 1) and not info.any()


def test_mvn_sample_return_codes(eng):
    """include/mfgp.h: a negative count, batch < 1, ncol < 1, ldc < n, a null pointer or eps == out is
    MFGP_ERR_ARG (-1), a short workspace MFGP_ERR_WORKSPACE (-2), both before any device work (out and info
    keep their sentinels); n = 0 and nsamp = 0 are no-ops that return MFGP_OK."""
    import ctypes as C
    from multi_fidelity_gpflow_amd._lib import ptr
    lib, n, nsamp, ncol = eng.lib, 40, 2, 3
    sz = C.c_size_t(0)
    assert lib.mfgp_mvn_sample_workspace_size(eng.h, n, 2, C.byref(sz)) == 0 and sz.value >= 2 * 64 * 64 * 8
    assert lib.mfgp_mvn_sample_workspace_size(eng.h, -1, 1, C.byref(sz)) == -1
    assert lib.mfgp_mvn_sample_workspace_size(eng.h, n, 0, C.byref(sz)) == -1
    assert lib.mfgp_mvn_sample_workspace_size(eng.h, n, 1, None) == -1
    assert lib.mfgp_mvn_sample_workspace_size(eng.h, n, 1, C.byref(sz)) == 0
    f64 = dict(dtype=torch.float64, device=eng.device)
    cov, mean = torch.eye(n, **f64), torch.zeros((n, ncol), **f64)
    eps, out = torch.ones((nsamp, n, ncol), **f64), torch.full((nsamp, n, ncol), -7.0, **f64)
    info = torch.full((1,), 7, dtype=torch.int32, device=eng.device)
    ws = torch.empty(sz.value, dtype=torch.uint8, device=eng.device)
    base = dict(n=n, batch=1, nsamp=nsamp, ncol=ncol, cov=ptr(cov), ldc=n, mean=ptr(mean), eps=ptr(eps), out=ptr(out),
                ws=ptr(ws), ws_bytes=ws.numel(), info=ptr(info))

    def call(**over):
        a = dict(base, **over)
        return lib.mfgp_mvn_sample(eng.h, a["n"], a["batch"], a["nsamp"], a["ncol"], a["cov"], a["ldc"], 0, 1e-6,
                                   a["mean"], ncol, 0, a["eps"], a["out"], ncol, n * ncol, 0, a["ws"], a["ws_bytes"],
                                   a["info"])
    for over in (dict(n=-1), dict(nsamp=-1), dict(batch=0), dict(ncol=0), dict(ldc=n - 1), dict(cov=None),
                 dict(mean=None), dict(eps=None), dict(out=None), dict(ws=None), dict(info=None),
                 dict(eps=ptr(out))):
        assert call(**over) == -1, over
    assert call(ws_bytes=sz.value - 257) == -2
    assert call(n=0) == 0 and call(nsamp=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and int(info.item()) == 7   # nothing was enqueued by any of them
    assert call() == 0
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    np.testing.assert_allclose(out.cpu().numpy(), np.sqrt(1.0 + 1e-6), rtol=0, atol=1e-15)


# ---------------------------------------------------------------- posteriors and models
def _identity_cov(post_or_model, Xs, p):
    """(out - mean)(out - mean)^T of identity draws, per output [P, N*, N*], and the mean."""
    ns = Xs.shape[0]
    eps = SO.identity_eps(ns, p)
    out = post_or_model.predict_f_samples(Xs, ns, eps=eps).numpy()
    mean = post_or_model.predict_f(Xs, full_cov=True)[0].numpy()   # the covariance call's mean: the draws' bits
    L = SO.factors_from_identity_draws(out, mean)
    assert not np.triu(L, 1).any()   # (mean + 0) - mean
    return np.einsum("pij,pkj->pik", L, L), mean


def _plumbing(name, eng, post, Xs, p, S_=3, seed=0):
    """predict_f_samples == Engine.mvn_sample on the object's own full_cov moments, bit for bit."""
    ns = Xs.shape[0]
    eps = np.random.default_rng(500 + seed).standard_normal((S_, ns, p))
    got = post.predict_f_samples(Xs, S_, eps=eps)
    assert tuple(got.shape) == (S_, ns, p), name
    mean, cov = post.predict_f(Xs, full_cov=True)
    mean, cov = mean.as_subclass(torch.Tensor), cov.as_subclass(torch.Tensor)
    return got.numpy(), mean, cov, torch.tensor(eps, device=eng.device)


@functools.lru_cache(maxsize=None)
def _gpr_sample_case():
    X, Y, Xs, prm = _syn_gpr(150, 30, 3, 3, NSTAR, 35)
    Xadd = Xs[:5].copy() + 0.05
    Xadd[:, -1] = np.arange(5) % 2
    Yadd = np.random.default_rng(36).standard_normal((5, Y.shape[1]))
    ref = O.gpr_predict_f_full_cov(X, Y, Xs, prm)[1][0]
    ref_cond = O.gpr_predict_f_full_cov(np.vstack([X, Xadd]), np.vstack([Y, Yadd]), Xs, prm)[1][0]
    return X, Y, Xs, prm, Xadd, Yadd, ref, ref_cond


def _gpr_checks(name, eng, post, Xs, p, ref, bound):
    got, mean, cov, eps = _plumbing(name, eng, post, Xs, p)
    own, info = eng.mvn_sample(cov[:1], mean, eps, p)   # ONE block, batch 1, ncol P
    assert not info.cpu().numpy().any()
    np.testing.assert_array_equal(got, own.cpu().numpy())
    C, _ = _identity_cov(post, Xs, p)
    err = np.abs(C - (ref + SO.JITTER * np.eye(Xs.shape[0]))[None]).max()
    print(f"{name}: identity-draw covariance vs oracle + 1e-6 I: err {err:.2e} (bound {bound:.1e})")
    assert err <= bound


@pytest.mark.parametrize("nb", [32, 64])
def test_gpr_posterior_samples(nb, eng):
    """The linear multi-fidelity GPR (n = 180, P = 3, N* = 35) at both tile sizes, and the same checks on a
    condition_on result (5 more rows): layout bit for bit, covariance of identity draws at the full_cov
    parity bound 1e-9."""
    X, Y, Xs, prm, Xadd, Yadd, ref, ref_cond = _gpr_sample_case()
    p = Y.shape[1]
    try:
        post = _model(X, Y, prm).posterior()
        if nb != 32:
            eng.set_tile(nb)
            post.update_cache()
        _gpr_checks(f"gpr nb{nb}", eng, post, Xs, p, ref, 1e-9)
        _gpr_checks(f"gpr nb{nb} conditioned", eng, post.condition_on(Xadd, Yadd), Xs, p, ref_cond, 1e-9)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("nb", [32, 64])
def test_graph_posterior_samples(nb, eng):
    """The graph model (n = 290, two LF sources, N* = 35 over the three fidelities; a symmetric rho_LF, so
    that the covariance of mixed-fidelity rows is a symmetric matrix) at both tile sizes; bound 1e-9."""
    m, D, X, Y, Xs = _graph_case()
    assert Xs.shape[0] == NSTAR
    try:
        mod = _graph_model(X, Y, m, D, asym=False)
        post = mod.posterior()
        if nb != 32:
            eng.set_tile(nb)
            post.update_cache()
        co = GO.predict_f_full_cov(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), _graph_oracle_params(mod, D),
                                   1e-3)[1].numpy()
        _gpr_checks(f"graph nb{nb}", eng, post, Xs, Y.shape[1], co, 1e-9)
    finally:
        eng.set_tile(32)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_posterior_samples(which, eng):
    """The HBS single-bin (P = L = 49, no W) and latent (5 latents, W) models, N* = 8 + 33: layout bit for
    bit against mvn_sample with batch = P, ncol = 1 on the snapshot's [P, N*, N*], covariance of identity
    draws against latent_cov + mix_cov + 1e-6 I at 1e-10 max(1, |ref|max)."""
    m, Wm, Xs = G.svgp_hbs_model(which)
    p = m.num_outputs
    post = m.posterior()
    got, mean, cov, eps = _plumbing(which, eng, post, Xs, p)
    own, info = eng.mvn_sample(cov, mean, eps, 1)
    assert not info.cpu().numpy().any()
    np.testing.assert_array_equal(got, own.cpu().numpy())
    Z, kps, q_mu, q_sqrt, W = G.svgp_state(m, Wm)
    _, gc = S.latent_cov(torch.tensor(Xs), Z, kps, q_mu, q_sqrt)
    ref = S.mix_cov(gc, None, W, True, False).numpy()
    C, _ = _identity_cov(post, Xs, p)
    err, scale = np.abs(C - (ref + SO.JITTER * np.eye(Xs.shape[0])[None])).max(), max(1.0, np.abs(ref).max())
    print(f"svgp {which}: identity-draw covariance vs oracle + 1e-6 I: err {err:.2e} (bound {1e-10 * scale:.1e})")
    assert err <= 1e-10 * scale
    # the snapshot: the model moves, the draws do not
    m.q_mu.assign(m.q_mu.numpy() + 0.25)
    again = post.predict_f_samples(Xs, 3, eps=eps).numpy()
    np.testing.assert_array_equal(again, got)
    assert np.abs(m.predict_f_samples(Xs, 3, eps=eps).numpy() - got).max() > 1e-3


def _four_models(hbs_like=None):
    X, Y, Xs, prm = _gpr_sample_case()[:4]
    m, D, Xg, Yg, Xsg = _graph_case()
    yield "gpr", _model(X, Y, prm), Xs, 1e-9
    yield "graph", _graph_model(Xg, Yg, m, D, asym=False), Xsg, 1e-9
    for which in ("singlebin", "latent"):
        mod, _, Xv = G.svgp_hbs_model(which)
        yield which, mod, Xv, 1e-10


def test_marginal_form_and_surface(eng):
    """full_cov=False is mean + sqrt(var) eps to the last bit; num_samples=None is draw 0 of the [1, N*, P]
    call; eps=None draws with the generator; the models' predict_f_samples against their fresh posterior's;
    NOCACHE delegates; the refusals; a NaN row of Xnew is a CholeskyError through info."""
    for name, mod, Xs, tol in _four_models():
        post = mod.posterior()
        p, ns = int(post._num_outputs()), Xs.shape[0]
        eps = np.random.default_rng(77).standard_normal((4, ns, p))
        for obj in (post, mod):
            mean, var = obj.predict_f(Xs)
            e = torch.tensor(eps, device=mean.device)
            want = mean.as_subclass(torch.Tensor)[None] + torch.sqrt(var.as_subclass(torch.Tensor))[None] * e
            got = obj.predict_f_samples(Xs, 4, full_cov=False, eps=eps)
            np.testing.assert_array_equal(got.numpy(), want.cpu().numpy())
            np.testing.assert_allclose(got.numpy(), SO.sample_mvn(mean.numpy(), var.numpy(), eps, False), rtol=0,
                                       atol=1e-14 * max(1.0, np.abs(want.cpu().numpy()).max()))
            one = obj.predict_f_samples(Xs, eps=eps[0])
            assert tuple(one.shape) == (ns, p)
            np.testing.assert_array_equal(one.numpy(), obj.predict_f_samples(Xs, 1, eps=eps[:1]).numpy()[0])
        # The model at its current parameters against its fresh posterior.  Their moments come from different
        # kernels (dmean, dSigma apart: rounding), so the draws agree to the first-order perturbation of a
        # Cholesky factor, |dL|_F <= |dSigma|_F / (sqrt(2) sigma_min(L)) with sigma_min(L) >= sqrt(jitter),
        # plus the forward error of either factorization, 10 n cond u with cond <= n max|Sigma| / jitter.
        a, b = mod.predict_f_samples(Xs, 4, eps=eps).numpy(), post.predict_f_samples(Xs, 4, eps=eps).numpy()
        assert a.shape == b.shape == (4, ns, p)
        (mm, cm), (mp, cp) = [(x[0].numpy(), x[1].numpy()) for x in (mod.predict_f(Xs, full_cov=True),
                                                                      post.predict_f(Xs, full_cov=True))]
        dS = np.sqrt(((cm - cp) ** 2).sum(axis=(1, 2))).max()
        scale = max(1.0, np.abs(b).max())
        bound = (np.abs(mm - mp).max() + dS / np.sqrt(2.0 * SO.JITTER) * np.sqrt((eps ** 2).sum(axis=1)).max()
                 + 10 * ns * (ns * np.abs(cp).max() / SO.JITTER) * 1.1e-16 * scale)
        ref = SO.sample_mvn(mp, cp, eps)
        print(f"{name}: model vs posterior draws {np.abs(a - b).max():.2e} (bound {bound:.2e}), posterior vs numpy "
              f"on its own moments {np.abs(b - ref).max():.2e}")
        assert np.abs(a - b).max() <= bound
        assert np.abs(b - ref).max() <= bound
        # NOCACHE delegates to the model: the same bits as the model's own call
        lazy = mod.posterior(precompute_cache=PrecomputeCacheType.NOCACHE)
        np.testing.assert_array_equal(lazy.predict_f_samples(Xs, 4, eps=eps).numpy(), a)
        # generators
        g = lambda seed: torch.Generator(device=eng.device).manual_seed(seed)
        r1, r2 = post.predict_f_samples(Xs, 2, generator=g(5)), post.predict_f_samples(Xs, 2, generator=g(5))
        r3 = post.predict_f_samples(Xs, 2, generator=g(6))
        np.testing.assert_array_equal(r1.numpy(), r2.numpy())
        assert np.abs(r1.numpy() - r3.numpy()).max() > 1e-6
        assert tuple(post.predict_f_samples(Xs, generator=g(5)).shape) == (ns, p)
        # requires_grad: detached samples
        Xt = torch.tensor(Xs, device=eng.device, requires_grad=True)
        assert not post.predict_f_samples(Xt, 2, eps=eps[:2]).requires_grad
        for obj in (post, mod):
            with pytest.raises(NotImplementedError, match="both"):
                obj.predict_f_samples(Xs, 2, full_cov=True, full_output_cov=True)
            with pytest.raises(NotImplementedError, match="not built"):
                obj.predict_f_samples(Xs, 2, full_cov=False, full_output_cov=True)
            Xn = Xs.copy()
            Xn[3, :-1] = np.nan   # (the fidelity flag stays valid: the row's covariances are NaN, not zero)
            with pytest.raises(M.CholeskyError, match="predict_f_samples"):
                obj.predict_f_samples(Xn, 2, eps=eps[:2])


def test_float32_model_raises(hbs):
    D = hbs["X"].shape[1] - 1
    m = M.MultiFidelityGPModel(hbs["X"], hbs["Y"], M.SquaredExponential(lengthscales=np.ones(D)),
                               M.SquaredExponential(lengthscales=np.ones(D)), dtype="float32")
    with pytest.raises(NotImplementedError, match="float32"):
        m.predict_f_samples(hbs["Xtest"], 2)
