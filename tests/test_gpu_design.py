"""Simulation design from the cached GPR posterior (``GPRPosterior.variance_reduction`` / ``select``,
mfgp_gpr_posterior_design_score / _append) on the HIP path.

The reference of every score is ``closed`` of tests/_design_oracle.py (the oracle's own full_cov block and
marginal variance on the stacked points), that of every batch ``greedy`` (one oracle refit per candidate and
step); never the code under test.  Bound: |score - ref|max <= 1e-9 |ref|max per case.  The score is built
from the same A as predict_f(full_cov), which the project bounds at 1e-9 absolute on O(1) entries and
measures at ~1e-14, and every case has cond(K + s2 I) < 1e6.  Each comparison prints what it measured; the
figures of an MI355X run are in DESIGN §5.10."""
import ctypes as C

import numpy as np
import pytest
import torch

import _design_oracle as DO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType
from multi_fidelity_gpflow_amd._lib import ptr
from multi_fidelity_gpflow_amd.engine import Engine
from test_gpu_graph import _data as _graph_data, _model as _graph_model, _oracle_params as _graph_oracle_params
from test_gpu_parity import _model, _oracle_params

pytestmark = pytest.mark.gpu

BOUND = 1e-9


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _check(name, got, ref):
    got = got.numpy() if hasattr(got, "numpy") else np.asarray(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{name}: err {err:.1e} |ref|max {scale:.3g} relative {err / scale:.1e} (bound {BOUND:.0e})")
    assert err <= BOUND * scale, (name, err, scale)


@pytest.mark.parametrize("which,nb", [("n25", 32), ("n79", 32), ("n79", 64), ("n180", 32), ("n180", 64), ("hbs", 32)])
def test_variance_reduction(which, nb, eng):
    """n25: one tile, one column.  n79: three row tiles, two reference and two candidate tiles with a
    one-row tail on both sides, a candidate bit-equal to a training row, a candidate and a reference of
    fidelity 0.5.  n180: two row groups of the forward (P = 65, D = 32), three reference tiles.  HBS at
    the initial parameters.  Seeded U[0, 1) weights, and the default (ones)."""
    X, Y, prm, Xref, Xcand, w = DO.case(which)
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        got = post.variance_reduction(Xcand, Xref, weights=w)
        _check(f"{which} nb{nb} weighted", got, DO.reference(which))
        ones = post.variance_reduction(Xcand, Xref)
        _check(f"{which} nb{nb} ones", ones, DO.reference(which, weighted=False))
        np.testing.assert_array_equal(ones.numpy(), post.variance_reduction(Xcand, Xref, np.ones(len(w))).numpy())
        if which == "n79":
            assert got.numpy()[7] == 0.0 and ones.numpy()[7] == 0.0   # the fidelity-0.5 candidate: exactly 0
            w9 = w.copy()
            w9[9] = 123.0                                             # the fidelity-0.5 reference adds exactly 0
            np.testing.assert_array_equal(post.variance_reduction(Xcand, Xref, w9).numpy(), got.numpy())
    finally:
        eng.set_tile(32)


def test_zero_weight(eng):
    """One weight set to zero: to the bound against the oracle; and, the 33 references being one run of
    the kernel (a run sums its rows in row order, so the zero term drops out of the same sequence of
    additions), the bits of the call with that reference removed."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    post = _model(X, Y, prm).posterior()
    w0 = w.copy()
    w0[3] = 0.0
    got = post.variance_reduction(Xcand, Xref, w0)
    _check("n79 one zero weight", got, DO.closed(X, Y, prm, Xref, Xcand, w0))
    keep = np.arange(33) != 3
    np.testing.assert_array_equal(post.variance_reduction(Xcand, Xref[keep], w[keep]).numpy(), got.numpy())


@pytest.mark.parametrize("which,nb", [("n25", 32), ("n25s", 32), ("n79", 32), ("n79", 64), ("n180", 32), ("n180", 64)])
def test_select(which, nb, eng):
    """q = 4 with cost 1 for an LF and 4 for an HF run against q rounds of oracle refits: the same picks,
    the gains to the bound.  Only inputs whose oracle-side relative margin between the best and the
    second-best score / cost is >= 1e-6 at every step qualify (asserted).  n25 has one candidate (an
    infinite margin): the same column is conditioned on four times.  n25s picks a candidate twice."""
    X, Y, prm, Xref, Xcand, w = DO.case(which)
    picks, gain, margin = DO.greedy_reference(which)
    print(f"{which}: oracle picks {picks.tolist()} margins {margin}")
    assert np.all(margin >= 1e-6)
    if which in ("n25", "n25s"):
        assert len(set(picks.tolist())) < 4   # a replicate: no masking
    cost = DO.costs(Xcand)
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        res = post.select(Xcand, Xref, 4, weights=w, cost=cost)
        assert isinstance(res, M.DesignResult) and res.picks.dtype == torch.int64 and res.picks.is_cuda
        assert res.picks.numpy().tolist() == picks.tolist()
        _check(f"{which} nb{nb} gain", res.gain, gain)
        # step 0 is variance_reduction, bit for bit
        vr = post.variance_reduction(Xcand, Xref, weights=w).numpy()
        first = post.select(Xcand, Xref, 1, weights=w, cost=cost)
        assert int(first.picks.numpy()[0]) == int(np.argmax(vr / cost)) == picks[0]
        assert first.gain.numpy()[0] == vr[picks[0]] == res.gain.numpy()[0]
        again = post.select(Xcand, Xref, 4, weights=w, cost=cost)
        np.testing.assert_array_equal(again.picks.numpy(), res.picks.numpy())
        np.testing.assert_array_equal(again.gain.numpy(), res.gain.numpy())
    finally:
        eng.set_tile(32)


def test_select_device_inputs_and_no_cost(eng):
    """Device-resident inputs; without a cost the first pick is the argmax of the score."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    post = _model(X, Y, prm).posterior()
    dev = lambda a: torch.tensor(a, device=eng.device)
    res = post.select(dev(Xcand), dev(Xref), 3, weights=dev(w))
    ref = DO.greedy(X, Y, prm, Xref, Xcand, 3, w)
    assert np.all(ref[2] >= 1e-6) and res.picks.numpy().tolist() == ref[0].tolist()
    _check("n79 no cost gain", res.gain, ref[1])


def test_select_enqueues_without_host_read(eng):
    """With device-resident inputs (and no weights / cost, whose check of a device tensor is a host read)
    a whole batch is enqueued without one synchronising torch operation: torch's sync debug mode turns any
    (.item(), indexing by a device scalar, a blocking copy) into an error."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    post = _model(X, Y, prm).posterior()
    xc, xr = torch.tensor(Xcand, device=eng.device), torch.tensor(Xref, device=eng.device)
    ref = post.select(xc, xr, 4)          # also sizes the workspace
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=eng.device).item()   # the mode does see a host read
        res = post.select(xc, xr, 4)
        score = post.variance_reduction(xc, xr)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    np.testing.assert_array_equal(res.picks.numpy(), ref.picks.numpy())
    np.testing.assert_array_equal(res.gain.numpy(), ref.gain.numpy())
    assert score.numpy()[int(ref.picks.numpy()[0])] == ref.gain.numpy()[0]


@pytest.mark.parametrize("asym", [False, True])
def test_graph_model(asym, eng):
    """The graph kernel with two LF sources (three row tiles): with a symmetric rho_LF against one refit
    per candidate (rescaled to the likelihood variance alone: the refit observes the appended row with the
    kernel's 1e-6 jitter on top) and against the closed form; with the asymmetric rho_LF of the graph
    tests against the closed form, whose block is the one full_cov returns."""
    m, D = 2, 3
    X, Y = _graph_data(m, D)
    mod = _graph_model(X, Y, m, D, asym=asym)
    prm, s2 = _graph_oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    Xref, Xcand, w = DO.graph_points(m, D)
    post = mod.posterior()
    got = post.variance_reduction(Xcand, Xref, weights=w)
    _check(f"graph asym={asym} vs closed", got, DO.closed(X, Y, prm, Xref, Xcand, w, noise=s2))
    assert got.numpy()[4] == 0.0
    if not asym:
        _check("graph symmetric vs refit", got, DO.brute(X, Y, prm, Xref, Xcand, w, noise=s2))
    res = post.select(Xcand, Xref, 3, weights=w)   # the batch runs on the graph kernel too
    assert int(res.picks.numpy()[0]) == int(np.argmax(got.numpy())) and res.gain.numpy()[0] == got.numpy().max()
    assert np.all(np.diff(res.gain.numpy()) <= BOUND * got.numpy().max())   # conditioning only lowers the best gain


def test_repeatable_and_snapshot(eng):
    """Two calls return the same bits; neither call writes the cache block; assigning to the model changes
    nothing until update_cache(), after which the score follows the new snapshot; the same on a VARIABLE
    cache, whose block stays."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    m = _model(X, Y, prm)
    post = m.posterior()
    var_post = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    block = post.cache.clone()
    before = post.variance_reduction(Xcand, Xref, w).numpy()
    sel = post.select(Xcand, Xref, 4, weights=w)
    np.testing.assert_array_equal(before, post.variance_reduction(Xcand, Xref, w).numpy())
    assert torch.equal(block, post.cache)
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.kernel.kernel_L.lengthscales.assign(np.full(X.shape[1] - 1, 0.8))
    m.likelihood.variance.assign(5e-3)
    np.testing.assert_array_equal(before, post.variance_reduction(Xcand, Xref, w).numpy())
    np.testing.assert_array_equal(before, var_post.variance_reduction(Xcand, Xref, w).numpy())
    np.testing.assert_array_equal(sel.gain.numpy(), var_post.select(Xcand, Xref, 4, weights=w).gain.numpy())
    ref = DO.closed(X, Y, _oracle_params(m), Xref, Xcand, w)
    assert np.abs(before - ref).max() > 1e-6 * np.abs(ref).max()   # the change does move the score
    ptr0 = var_post.cache.data_ptr()
    post.update_cache()
    _check("after update_cache", post.variance_reduction(Xcand, Xref, w), ref)
    var_post.update_cache()
    assert var_post.cache.data_ptr() == ptr0
    _check("variable after update_cache", var_post.variance_reduction(Xcand, Xref, w), ref)


def test_empty_sets(eng):
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    post = _model(X, Y, prm).posterior()
    none = post.variance_reduction(Xcand[:0], Xref)
    assert tuple(none.shape) == (0,) and none.dtype == torch.float64
    zero = post.variance_reduction(Xcand, Xref[:0])
    assert tuple(zero.shape) == (33,) and not zero.numpy().any()
    res = post.select(Xcand, Xref[:0], 2)
    assert res.picks.numpy().tolist() == [0, 0] and not res.gain.numpy().any()


def test_refusals(eng):
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    m = _model(X, Y, prm)
    nocache = m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        nocache.variance_reduction(Xcand, Xref)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        nocache.select(Xcand, Xref, 2)
    post = m.posterior()
    with pytest.raises(ValueError):
        post.select(Xcand, Xref, 33)
    eng.set_tile(64)
    try:
        with pytest.raises(M.MFGPError, match="built for tile size 32"):
            post.variance_reduction(Xcand, Xref)
        with pytest.raises(M.MFGPError, match="built for tile size 32"):
            post.select(Xcand, Xref, 2)
    finally:
        eng.set_tile(32)


def test_c_call_errors(eng):
    """MFGP_ERR_ARG / MFGP_ERR_WORKSPACE come before any device work (the outputs keep their fill);
    ncand = 0 is a no-op; a pick outside the candidates appends a zero row."""
    X, Y, prm, Xref, Xcand, w = DO.case("n79")
    post = _model(X, Y, prm).posterior()
    n, p, d, nr, nc = 79, 3, 3, 33, 33
    lib, dev = eng.lib, eng.device
    f64 = dict(dtype=torch.float64, device=dev)
    Xall = torch.tensor(np.vstack([Xref, Xcand]), device=dev)
    sz = C.c_size_t()
    assert lib.mfgp_gpr_posterior_design_workspace_size(eng.h, 0, n, p, d, nr, nc, 32, C.byref(sz)) == 0
    assert lib.mfgp_gpr_posterior_design_workspace_size(eng.h, 0, n, p, d, nr, nc, 33, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_design_workspace_size(eng.h, 5, n, p, d, nr, nc, 4, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_design_workspace_size(eng.h, 0, n, p, d, -1, nc, 4, C.byref(sz)) == -1
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    E = torch.full((32, nr + nc), 7.0, **f64)

    def score(k=0, wsb=None, cb=None, ncand=nc, nlf=0, refresh=1):
        out = torch.full((nc,), 7.0, **f64)
        rc = lib.mfgp_gpr_posterior_design_score(eng.h, nlf, n, p, d, ptr(post.cache),
                                                 post.cache.numel() if cb is None else cb, ptr(Xall), d + 1, nr, ncand,
                                                 None, ptr(E), nr + nc, k, ptr(ws), ws.numel() if wsb is None else wsb,
                                                 ptr(out), refresh)
        torch.cuda.synchronize()
        return rc, out

    def append(pick, k, wsb=None):
        pk = torch.tensor([pick], dtype=torch.int32, device=dev)
        rc = lib.mfgp_gpr_posterior_design_append(eng.h, 0, n, p, d, ptr(post.cache), post.cache.numel(), ptr(Xall),
                                                  d + 1, nr, nc, ptr(ws), ws.numel() if wsb is None else wsb, ptr(pk),
                                                  ptr(E), nr + nc, k)
        torch.cuda.synchronize()
        return rc

    untouched = lambda out: bool((out == 7).all()) and bool((E == 7).all())
    for kw, code in ((dict(k=33), -1), (dict(k=-1), -1), (dict(nlf=5), -1), (dict(ncand=-2), -1),
                     (dict(wsb=sz.value - 1), -2), (dict(cb=1024), -2)):
        rc, out = score(**kw)
        assert rc == code and untouched(out), kw
    assert append(0, 32) == -1 and append(0, 0, wsb=sz.value - 1) == -2 and untouched(E)
    rc, out = score(ncand=0)
    assert rc == 0 and untouched(out)
    rc, out = score()
    assert rc == 0
    _check("C call, ones", out.cpu().numpy(), DO.reference("n79", weighted=False))
    assert append(nc, 0) == 0 and append(-1, 1) == 0                  # no such candidate: zero rows
    assert not E[:2].cpu().numpy().any() and bool((E[2:] == 7).all())
    rc, again = score(k=2, refresh=0)                                 # two zero rows condition on nothing
    assert rc == 0
    np.testing.assert_array_equal(again.cpu().numpy(), out.cpu().numpy())
