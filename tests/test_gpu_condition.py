"""Conditioning the cached GPR posterior on new rows (``GPRPosterior.condition_on`` / ``fantasize``,
mfgp_gpr_posterior_append) on the HIP path.

The reference is always the CPU oracle on the stacked data (tests/_condition_oracle.py ``stacked``; leave-out:
tests/_leave_out_oracle.py ``brute``; design: tests/_design_oracle.py ``closed`` / ``greedy``), never the code
under test.  Bounds, as in test_gpu_design.py: |err|max <= 1e-9 max(1, |ref|max) for means, <= 1e-9 |ref|max
for variances, covariances and scores; every case has cond(K + s2 I) < 1e6 (tests/test_condition_host.py).
Each comparison prints what it measured; the figures of an MI355X run are in DESIGN §5.11."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _condition_oracle as CO
import _design_oracle as DO
import _leave_out_oracle as LO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType
from multi_fidelity_gpflow_amd._lib import ptr
from multi_fidelity_gpflow_amd.engine import Engine
from multi_fidelity_gpflow_amd.session import CholeskyError
from test_gpu_graph import _data as _graph_data, _model as _graph_model, _oracle_params as _graph_oracle_params
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu

BOUND = 1e-9


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _np(a):
    return a.numpy() if hasattr(a, "numpy") else np.asarray(a)


def _check(name, got, ref, mean=False):
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{name}: err {err:.1e} |ref|max {scale:.3g} (bound {BOUND:.0e})")
    assert err <= BOUND * (max(1.0, scale) if mean else scale), (name, err, scale)


def _check_predict(name, post, Xs, ref):
    """predict_f, marginal and full_cov, against (mean, var [N*], cov [N*, N*])."""
    mean, var = post.predict_f(Xs)
    _check(name + " mean", mean, ref[0], mean=True)
    _check(name + " var", var, np.tile(ref[1][:, None], (1, ref[0].shape[1])))
    mean2, cov = post.predict_f(Xs, full_cov=True)
    _check(name + " full_cov mean", mean2, ref[0], mean=True)
    _check(name + " cov", cov[0], ref[2])


@functools.lru_cache(maxsize=None)
def _refs(which, k):
    """The oracle's answers for one case, computed once and shared by its tile sizes."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case(which, k)
    Xst, Yst = np.vstack([X, Xadd]), np.vstack([Y, Yadd])
    rows = np.arange(X.shape[0], X.shape[0] + k)
    Xref, Xcand, w = DO.case("n79" if which == "n64" else which)[3:]
    return (CO.reference(which, k), LO.brute(Xst, Yst, prm, [rows]), Xref, Xcand, w,
            DO.closed(Xst, Yst, prm, Xref, Xcand, w))


SHAPES = [("n25", 1, 32), ("n25", 7, 32), ("n25", 8, 32), ("n64", 1, 32), ("n64", 1, 64), ("n79", 32, 32),
          ("n79", 32, 64), ("n180", 17, 32), ("n180", 17, 64), ("hbs", 3, 32)]


@pytest.mark.parametrize("which,k,nb", SHAPES)
def test_condition_on(which, k, nb, eng):
    """n25 + 1: inside one tile.  n25 + 7 = 32: fills the tile, no padding left.  n25 + 8 = 33: a new tile
    row, the row stride changes.  n64 + 1: the source has no padding.  n79 + 32: the maximum k (T 3 -> 4 at
    NB 32, 2 -> 2 at NB 64), Xadd[0] a replicate of training row 12.  n180 + 17: P = 65 (two Z tiles), D = 32,
    two row groups of the forward.  hbs + 3 HF rows.  predict_f, full_cov at 40 points (the padded rows of A),
    leave_out of the appended rows and variance_reduction against the oracle on the stacked data, and
    predict_f against a device-built posterior of the stacked model."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case(which, k)
    ref, lo, Xref, Xcand, w, vr = _refs(which, k)
    n, name = X.shape[0], f"{which}+{k} nb{nb}"
    eng.set_tile(nb)
    try:
        src = _model(X, Y, prm).posterior()
        post = src.condition_on(Xadd, Yadd)
        assert isinstance(post, M.GPRPosterior) and post is not src and post.model is src.model
        assert post._shape == (n + k, Y.shape[1], X.shape[1] - 1) and src._shape[0] == n
        _check_predict(name, post, Xs, ref)
        res = post.leave_out([np.arange(n, n + k)], full_cov=True)
        _check(name + " leave_out mean", res.mean, lo["mean"], mean=True)
        _check(name + " leave_out var", res.var, lo["var"])
        _check(name + " leave_out cov", res.cov, lo["cov"])
        _check(name + " variance_reduction", post.variance_reduction(Xcand, Xref, weights=w), vr)
        built = _model(np.vstack([X, Xadd]), np.vstack([Y, Yadd]), prm).posterior()
        bm, bv = built.predict_f(Xs)
        _check(name + " vs device build, mean", post.predict_f(Xs)[0], bm, mean=True)
        _check(name + " vs device build, var", post.predict_f(Xs)[1], bv)
    finally:
        eng.set_tile(32)


def test_chain_and_rebuild(eng):
    """n79 + 5 then + 9 equals + 14 in one call and the oracle; update_cache() of the chained posterior (the
    exact rebuild from the stacked data at the frozen theta) agrees; a VARIABLE cache keeps its block."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case("n79", 14)
    ref = CO.reference("n79", 14)
    m = _model(X, Y, prm)
    src = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    once = src.condition_on(Xadd, Yadd)
    chain = src.condition_on(Xadd[:5], Yadd[:5]).condition_on(torch.tensor(Xadd[5:], device=eng.device),
                                                               torch.tensor(Yadd[5:], device=eng.device))
    assert chain._shape == once._shape == (93, 3, 3)
    _check_predict("n79+14 once", once, Xs, ref)
    _check_predict("n79+5+9", chain, Xs, ref)
    _check("chain vs once, mean", chain.predict_f(Xs)[0], once.predict_f(Xs)[0], mean=True)
    _check("chain vs once, var", chain.predict_f(Xs)[1], once.predict_f(Xs)[1])
    m.likelihood.variance.assign(0.5)   # the rebuild is at the FROZEN theta, not the model's
    ptr0 = chain.cache.data_ptr()
    chain.update_cache()
    assert chain.cache.data_ptr() == ptr0   # VARIABLE is inherited: the same block is rewritten
    _check_predict("n79+5+9 after update_cache", chain, Xs, ref)
    with pytest.raises(NotImplementedError, match="conditioned"):
        chain.fused_predict_f(Xs)


def test_fantasy(eng):
    """Rows without a value: the mean is the unstacked model's, the variance the stacked refit's."""
    X, Y, prm, Xadd, _, Xs = CO.case("n79", 32)
    src = _model(X, Y, prm).posterior()
    post = src.fantasize(Xadd)
    mean, var = post.predict_f(Xs)
    _check("fantasy mean vs unstacked oracle", mean, CO.stacked(X, Y, Xs, prm)[0], mean=True)
    _check("fantasy var vs stacked oracle", var[:, 0], CO.reference("n79", 32)[1])
    _check("fantasy cov vs stacked oracle", post.predict_f(Xs, full_cov=True)[1][0], CO.reference("n79", 32)[2])
    # the rows' Y for leave_out is the mean at Xadd the call computed: left out, they are predicted at it
    res = post.leave_out([np.arange(79, 111)])
    _check("fantasy leave_out mean", res.mean, CO.stacked(X, Y, Xadd, prm)[0], mean=True)


def test_agrees_with_select(eng):
    """select's second step is variance_reduction of the posterior fantasized on its first pick."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    picks, gain, margin = DO.greedy(X, Y, prm, Xref, Xcand, 2, w)
    assert np.all(margin >= 1e-6)
    post = _model(X, Y, prm).posterior()
    res = post.select(Xcand, Xref, 2, weights=w)
    assert res.picks.numpy().tolist() == picks.tolist()
    _check("select gain", res.gain, gain)
    vr = post.fantasize(Xcand[picks[:1]]).variance_reduction(Xcand, Xref, w).numpy()
    assert int(np.argmax(vr)) == picks[1]
    _check("fantasize -> variance_reduction, best score", vr.max(keepdims=True), gain[1:2])


@pytest.mark.parametrize("asym", [True, False])
def test_graph_model(asym, eng):
    """The graph kernel, m = 2, D = 3, against the graph oracle on the stacked data.  Symmetric rho_LF: the
    appended sources cycle 0, 1, 2.  Asymmetric rho_LF (the case that fails if the cross block is taken in
    predict_f's argument order): sources 1 and 2, because a source-0 row BELOW the source-1 rows reads
    rho_LF[0, 1] where the sorted training rows read rho_LF[1, 0] and the stacked matrix is indefinite
    (tests/test_condition_host.py asserts that on the oracle side); here such a row must raise CholeskyError."""
    m, D = 2, 3
    X, Y = _graph_data(m, D)
    mod = _graph_model(X, Y, m, D, asym=asym)
    prm, s2 = _graph_oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    Xadd, Yadd, Xs = CO.graph_rows(m, D, Y.shape[1], 9, sources=(1, 2) if asym else None)
    Xst, Yst = np.vstack([X, Xadd]), np.vstack([Y, Yadd])
    src = mod.posterior()
    post = src.condition_on(Xadd, Yadd)
    _check_predict(f"graph asym={asym} +9", post, Xs, CO.stacked(Xst, Yst, Xs, prm, s2))
    fant = src.fantasize(Xadd)
    _check("graph fantasy mean", fant.predict_f(Xs)[0], CO.stacked(X, Y, Xs, prm, s2)[0], mean=True)
    _check("graph fantasy var", fant.predict_f(Xs)[1][:, 0], CO.stacked(Xst, Yst, Xs, prm, s2)[1])
    if asym:
        before = src.predict_f(Xs)[0].numpy()
        with pytest.raises(CholeskyError):
            src.condition_on(CO.graph_rows(m, D, Y.shape[1], 3)[0])
        np.testing.assert_array_equal(src.predict_f(Xs)[0].numpy(), before)


def test_snapshot_and_repeatable(eng):
    """The source's block is not written; assigning to the model changes neither posterior; two identical
    calls give bit-equal blocks (every byte of the new block is written, in a fixed order)."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case("n79", 32)
    m = _model(X, Y, prm)
    src = m.posterior()
    block = src.cache.clone()
    a = src.condition_on(Xadd, Yadd)
    b = src.condition_on(Xadd, Yadd)
    assert torch.equal(block, src.cache)
    assert a.cache.data_ptr() != b.cache.data_ptr() and torch.equal(a.cache, b.cache)
    fa, fb = src.fantasize(Xadd[:8]), src.fantasize(Xadd[:8])
    assert torch.equal(fa.cache, fb.cache)
    mean_src, mean_a = src.predict_f(Xs)[0].numpy(), a.predict_f(Xs)[0].numpy()
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.likelihood.variance.assign(5e-3)
    np.testing.assert_array_equal(src.predict_f(Xs)[0].numpy(), mean_src)
    np.testing.assert_array_equal(a.predict_f(Xs)[0].numpy(), mean_a)
    c = src.condition_on(Xadd, Yadd)   # still the snapshot's hyper-parameters
    assert torch.equal(a.cache, c.cache)


def test_vjp(eng):
    """predict_f_vjp and autograd run on a conditioned posterior and agree with the device-built stacked one."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case("n79", 32)
    post = _model(X, Y, prm).posterior().condition_on(Xadd, Yadd)
    built = _model(np.vstack([X, Xadd]), np.vstack([Y, Yadd]), prm).posterior()
    rng = np.random.default_rng(7)
    gm, gv = rng.standard_normal((Xs.shape[0], Y.shape[1])), rng.standard_normal(Xs.shape[0])
    got, ref = post.predict_f_vjp(Xs, gm, gv)[2].numpy(), built.predict_f_vjp(Xs, gm, gv)[2].numpy()
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"vjp: err {err:.1e} largest gradient entry {scale:.3g}")
    assert err <= BOUND * scale and not got[:, -1].any()
    xs = torch.tensor(Xs, device=eng.device, requires_grad=True)
    mean, var = post.predict_f(xs)
    (mean * torch.tensor(gm, device=eng.device)).sum().backward()
    ref_m = built.predict_f_vjp(Xs, gm, None)[2].numpy()
    assert np.abs(xs.grad.cpu().numpy() - ref_m).max() <= BOUND * np.abs(ref_m).max()


def test_refusals(eng):
    X, Y, prm, Xadd, Yadd, Xs = CO.case("n79", 32)
    m = _model(X, Y, prm)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE).condition_on(Xadd, Yadd)
    post = m.posterior()
    before = [t.numpy() for t in post.predict_f(Xs)]
    block = post.cache.clone()
    for Xa, Ya in ((Xadd[:0], Yadd[:0]), (np.vstack([Xadd, Xadd[:1]]), None), (Xadd, Yadd[:31]), (Xadd, Yadd[:, :2]),
                   (Xadd[:, :3], None)):
        with pytest.raises(ValueError, match="condition_on"):
            post.condition_on(Xa, Ya)
    eng.set_tile(64)
    try:
        with pytest.raises(M.MFGPError, match="built for tile size 32"):
            post.condition_on(Xadd, Yadd)
    finally:
        eng.set_tile(32)
    half = Xadd.copy()
    half[5, -1] = 0.5
    with pytest.raises(ValueError, match="row 5"):
        post.condition_on(half, Yadd)
    nan = Xadd.copy()
    nan[3, 0] = np.nan
    with pytest.raises(CholeskyError):
        post.condition_on(nan, Yadd)
    assert torch.equal(block, post.cache)
    for b, t in zip(before, post.predict_f(Xs)):
        np.testing.assert_array_equal(t.numpy(), b)


def test_c_call_errors(eng):
    """MFGP_ERR_ARG / MFGP_ERR_WORKSPACE come before any device work (the outputs keep their fill); then one
    good call through the C ABI against the oracle."""
    X, Y, prm, Xadd, Yadd, Xs = CO.case("n79", 32)
    post = _model(X, Y, prm).posterior()
    n, p, d, k = 79, 3, 3, 32
    lib, dev = eng.lib, eng.device
    sz, osz = C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_append_workspace_size(eng.h, 0, n, p, d, k, C.byref(sz)) == 0
    for bad in (dict(k=0), dict(k=33), dict(nlf=5), dict(n=0)):
        a = dict(nlf=0, n=n, k=k)
        a.update(bad)
        assert lib.mfgp_gpr_posterior_append_workspace_size(eng.h, a["nlf"], a["n"], p, d, a["k"], C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_size(eng.h, 0, n + k, p, d, C.byref(osz)) == 0
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    xa, ya = torch.tensor(Xadd, device=dev), torch.tensor(Yadd, device=dev)
    out = torch.full((osz.value,), 7, dtype=torch.uint8, device=dev)
    mean = torch.full((k, p), 7.0, dtype=torch.float64, device=dev)
    info = torch.full((1,), 7, dtype=torch.int32, device=dev)

    def call(k=k, nlf=0, cb=None, wsb=None, ob=None, same=False):
        rc = lib.mfgp_gpr_posterior_append(eng.h, nlf, n, p, d, k, ptr(post.cache),
                                           post.cache.numel() if cb is None else cb, ptr(xa), d + 1, ptr(ya), p, ptr(ws),
                                           ws.numel() if wsb is None else wsb, ptr(post.cache) if same else ptr(out),
                                           out.numel() if ob is None else ob, ptr(mean), p, ptr(info))
        torch.cuda.synchronize()
        return rc

    block = post.cache.clone()
    untouched = lambda: bool((out == 7).all()) and bool((mean == 7).all()) and bool((info == 7).all())
    for kw, code in ((dict(k=0), -1), (dict(k=33), -1), (dict(nlf=5), -1), (dict(same=True), -1),
                     (dict(cb=post.cache.numel() - 1), -2), (dict(wsb=sz.value - 1), -2), (dict(ob=osz.value - 1), -2)):
        assert call(**kw) == code and untouched(), kw
    assert torch.equal(block, post.cache)
    assert post.cache.numel() == eng.gpr_posterior_bytes(0, n, p, d)   # "one byte short" above is of the exact size
    assert call() == 0 and int(info.item()) == 0 and not bool((out == 7).all())
    _check("C call, mean at Xadd", mean.cpu().numpy(), CO.stacked(X, Y, Xadd, prm)[0], mean=True)
    got = eng.gpr_posterior_predict(0, (n + k, p, d), out, torch.tensor(Xs, device=dev))
    ref = CO.reference("n79", 32)
    _check("C call, predict mean", got[0].cpu().numpy(), ref[0], mean=True)
    _check("C call, predict var", got[1].cpu().numpy(), ref[1])
