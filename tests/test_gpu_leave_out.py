"""Leave-group-out cross-validation from the cached GPR posterior (``GPRPosterior.leave_out``,
mfgp_gpr_posterior_leave_out) on the HIP path.

The reference of every comparison is ``brute`` of tests/_leave_out_oracle.py: a refit of the oracle
without the group, never the code under test.  Bounds: the project's predict bounds (mean 1e-9 max(1,
|mean|max), var / cov 1e-9; tests/test_gpu_posterior.py ``_check_gpr``); the log density, whose error is
amplified by 1 / var, max(1e-9, 10 x the deviation of the numpy closed form from ``brute`` on the same case)
x max(1, |ref|max): the factor 10 covers the device's other summation order.  Every case has cond(K + s2 I)
< 1e6.  Each comparison prints what it measured; the figures of an MI355X run are in DESIGN §5.9 (worst: mean
5.3e-12, var / cov 5.6e-15, log density 1.5e-9 at |ref| = 2439, all on the graph model or n = 500)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _leave_out_oracle as LO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType, groups_by_input
from multi_fidelity_gpflow_amd._lib import ptr
from multi_fidelity_gpflow_amd.engine import Engine
from test_gpu_graph import _data as _graph_data, _model as _graph_model, _oracle_params as _graph_oracle_params
from test_gpu_parity import _model, _oracle_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    yield e
    e.set_tile(32)


def _check(name, res, ref, dev):
    """A LeaveOutResult against brute's dict at the bounds of the module docstring."""
    np.testing.assert_array_equal(res.rows, ref["rows"])
    np.testing.assert_array_equal(res.group, ref["group"])
    mean, var, ld = res.mean.numpy(), res.var.numpy(), res.log_density.numpy()
    assert mean.shape == ref["mean"].shape and var.shape == ref["var"].shape and ld.shape == ref["log_density"].shape
    em, ev = np.abs(mean - ref["mean"]).max(), np.abs(var - ref["var"]).max()
    el, sl = np.abs(ld - ref["log_density"]).max(), max(1.0, np.abs(ref["log_density"]).max())
    bl = max(1e-9, 10.0 * dev["log_density"]) * sl
    ec = None
    if res.cov is not None:
        assert tuple(res.cov.shape) == ref["cov"].shape
        ec = np.abs(res.cov.numpy() - ref["cov"]).max()
    print(f"{name}: mean err {em:.1e} var err {ev:.1e} cov err {ec if ec is None else format(ec, '.1e')} "
          f"log density err {el:.1e} (bound {bl:.1e}; closed form vs refit {dev['log_density']:.1e}, |ref| {sl:.1f})")
    assert em <= 1e-9 * max(1.0, np.abs(ref["mean"]).max()), (name, em)
    assert ev <= 1e-9, (name, ev)
    assert ec is None or ec <= 1e-9, (name, ec)
    assert el <= bl, (name, el, bl)


def _run(name, post, which, key, groups, full_cov=False):
    ref, _, dev = LO.reference(which, key)
    res = post.leave_out(groups, full_cov=full_cov)
    assert (res.cov is not None) == full_cov
    _check(name, res, ref, dev)
    return res


@pytest.mark.parametrize("nb", [32, 64])
def test_hbs(nb, eng):
    """HBS at the initial parameters (n = 53, P = 49): two row tiles at 32 (the last of 21 rows), less
    than one at 64.  All 53 single rows, and the three HF rows together with their LF twins."""
    X, Y, prm, groups = LO.case("hbs")
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        _run(f"hbs nb{nb} singles", post, "hbs", "singles", None)
        labels = groups_by_input(X, only_hf=True)
        res = _run(f"hbs nb{nb} pairs", post, "hbs", "pairs", labels, full_cov=True)
        assert res.rows.tolist() == [0, 52, 9, 50, 46, 51] and tuple(res.cov.shape) == (3, 2, 2)
        np.testing.assert_array_equal(np.diagonal(res.cov.numpy(), axis1=1, axis2=2).reshape(-1), res.var.numpy()[:, 0])
    finally:
        eng.set_tile(32)


def test_one_tile_one_output(eng):
    """n = 25, P = D = 1: everything inside one tile, one output column."""
    X, Y, prm, _ = LO.case("n25")
    _run("n25 singles", _model(X, Y, prm).posterior(), "n25", "singles", None)


def test_group_sizes(eng):
    """n = 79, P = 3: groups of 1, 2, 3, 7, 16 and 32 rows (three tasks), the pair made of rows 0 and
    78 (columns in the first and the last row tile); and a label array with -1 entries."""
    X, Y, prm, groups = LO.case("n79")
    post = _model(X, Y, prm).posterior()
    assert sorted(len(g) for g in groups["sizes"]) == [1, 2, 3, 7, 16, 32]
    res = _run("n79 sizes", post, "n79", "sizes", groups["sizes"], full_cov=True)
    assert tuple(res.cov.shape) == (6, 32, 32)
    labels = groups["_labels"]
    assert np.count_nonzero(labels == -1) == 18
    _run("n79 labels", post, "n79", "labels", labels)


@pytest.mark.parametrize("nb", [32, 64])
def test_output_blocks_and_packing(nb, eng):
    """n = 180, P = 65 (one column past two 32-blocks of Z and past a 64-tile), D = 32: all 180 singles
    (6 tasks); 33 singles (the packing boundary, 32 + 1); small groups around one of 32 rows."""
    X, Y, prm, groups = LO.case("n180")
    eng.set_tile(nb)
    try:
        post = _model(X, Y, prm).posterior()
        _run(f"n180 nb{nb} singles", post, "n180", "singles", None)
        _run(f"n180 nb{nb} 33 singles", post, "n180", "singles33", groups["singles33"])
        _run(f"n180 nb{nb} mixed", post, "n180", "mixed", groups["mixed"], full_cov=True)
    finally:
        eng.set_tile(32)


def test_more_than_one_chunk(eng):
    """n = 500: 16 steps of 32 rows, four chunks a task; twelve seeded groups of 1 to 32 rows."""
    X, Y, prm, groups = LO.case("n500")
    assert X.shape[0] == 500 and len(groups["twelve"]) == 12
    _run("n500 twelve groups", _model(X, Y, prm).posterior(), "n500", "twelve", groups["twelve"], full_cov=True)


def test_graph_model(eng):
    """The graph kernel with two LF sources: its 1e-6 jitter is part of K and stays in the covariance;
    only the likelihood variance is subtracted.  groups_by_input groups (the inputs are all distinct: 82
    singles) and five singles of LF source 0 and HF rows.

    With the asymmetric rho_LF of the existing graph tests the oracle's predict_f of a refit is the
    held-out prediction only at rows of LF source 0 and at HF rows (_leave_out_oracle.graph_refit_valid:
    at a row of source 1 the refit's cross-covariance holds rho_LF[0, 1] where the factorized joint model
    holds rho_LF[1, 0], and the oracle's variance there is negative).  So `brute` is the reference on those
    52 rows; on all 82 the reference is `brute_joint`, the same refit with the joint covariance taken as
    the factorization reads it, which is first held to `brute` on the 52 rows on the CPU."""
    m, D = 2, 3
    X, Y = _graph_data(m, D)
    mod = _graph_model(X, Y, m, D, asym=True)
    prm, s2 = _graph_oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    post = mod.posterior()
    labels = groups_by_input(X)
    assert labels.tolist() == list(range(82))
    valid = np.flatnonzero(LO.graph_refit_valid(X, m))
    assert valid.size == 52
    lists = [[int(i)] for i in valid]
    ref, closed = LO.brute(X, Y, prm, lists, noise=s2), LO.closed_numpy(X, Y, prm, lists, noise=s2)
    dev = LO.deviation(ref, closed)
    _check("graph source 0 and HF rows vs refit", post.leave_out(lists, full_cov=True), ref, dev)
    five = [[0], [39], [70], [75], [81]]
    r5 = LO.brute(X, Y, prm, five, noise=s2)
    _check("graph five singles vs refit", post.leave_out(five, full_cov=True), r5,
           LO.deviation(r5, LO.closed_numpy(X, Y, prm, five, noise=s2)))
    alls = LO.lists_from_labels(labels)
    joint, closed = LO.brute_joint(X, Y, prm, alls, s2), LO.closed_numpy(X, Y, prm, alls, noise=s2)
    sub = LO.brute_joint(X, Y, prm, lists, s2)
    d = LO.deviation(ref, sub)
    print(f"graph: joint refit vs oracle refit on the 52 rows {d}")
    assert all(d[k] <= 1e-10 * max(1.0, np.abs(ref[k]).max()) for k in d)   # a tenth of the bounds below
    _check("graph by input (82 singles) vs joint refit", post.leave_out(labels, full_cov=True), joint,
           LO.deviation(joint, closed))


def _same(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            np.testing.assert_array_equal(np.asarray(x if isinstance(x, np.ndarray) else x.numpy()),
                                          np.asarray(y if isinstance(y, np.ndarray) else y.numpy()))


def test_repeatable_and_snapshot(eng):
    """Two calls return the same bits; assigning to the model changes nothing until update_cache(), after
    which the result is the refit's at the new parameters; the same on a VARIABLE cache, whose block stays."""
    X, Y, prm, groups = LO.case("hbs")
    pairs = groups["pairs"]
    m = _model(X, Y, prm)
    post = m.posterior()
    var_post = m.posterior(precompute_cache=PrecomputeCacheType.VARIABLE)
    before = post.leave_out(pairs, full_cov=True)
    _same(before, post.leave_out(pairs, full_cov=True))
    _same(post.leave_out(), post.leave_out())
    m.kernel.rho.assign(np.full((Y.shape[1], 1), 1.234))
    m.kernel.kernel_L.lengthscales.assign(np.full(X.shape[1] - 1, 0.8))
    m.likelihood.variance.assign(5e-3)
    _same(before, post.leave_out(pairs, full_cov=True))
    po = _oracle_params(m)
    ref, closed = LO.brute(X, Y, po, pairs), LO.closed_numpy(X, Y, po, pairs)
    dev = LO.deviation(ref, closed)
    assert np.abs(before.mean.numpy() - ref["mean"]).max() > 1e-6   # the change does move the prediction
    ptr0 = var_post.cache.data_ptr()
    _same(before, var_post.leave_out(pairs, full_cov=True))
    post.update_cache()
    _check("after update_cache", post.leave_out(pairs, full_cov=True), ref, dev)
    var_post.update_cache()
    assert var_post.cache.data_ptr() == ptr0
    _check("variable after update_cache", var_post.leave_out(pairs, full_cov=True), ref, dev)


def test_group_listed_twice(eng):
    """A group's rows do not depend on where the group sits in the call: listed twice (the second copy
    across a 4-pivot block of the factor), and on its own."""
    X, Y, prm, _ = LO.case("hbs")
    post = _model(X, Y, prm).posterior()
    res = post.leave_out([[0, 52], [9], [0, 52]], full_cov=True)
    assert res.rows.tolist() == [0, 52, 9, 0, 52] and res.group.tolist() == [0, 0, 1, 2, 2]
    for field in (res.mean, res.var):
        np.testing.assert_array_equal(field.numpy()[:2], field.numpy()[3:])
    np.testing.assert_array_equal(res.log_density.numpy()[0], res.log_density.numpy()[2])
    np.testing.assert_array_equal(res.cov.numpy()[0], res.cov.numpy()[2])
    alone = post.leave_out([[0, 52]], full_cov=True)
    np.testing.assert_array_equal(alone.mean.numpy(), res.mean.numpy()[:2])
    np.testing.assert_array_equal(alone.cov.numpy()[0], res.cov.numpy()[0])
    np.testing.assert_array_equal(alone.log_density.numpy()[0], res.log_density.numpy()[0])


def test_refusals(eng):
    X, Y, prm, _ = LO.case("n79")
    m = _model(X, Y, prm)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE).leave_out()
    post = m.posterior()
    for bad in ([np.arange(33)], [[4, 7, 4]], [[0, 79]], [[]]):
        with pytest.raises(ValueError):
            post.leave_out(bad)
    empty = post.leave_out(np.full(79, -1), full_cov=True)
    assert empty.rows.size == 0 and tuple(empty.mean.shape) == (0, 3) and tuple(empty.cov.shape) == (0, 0, 0)
    assert not hasattr(M.SVGPPosterior, "leave_out")
    eng.set_tile(64)
    try:
        with pytest.raises(M.MFGPError, match="built for tile size 32"):
            post.leave_out()
    finally:
        eng.set_tile(32)


def test_c_call_errors(eng):
    """MFGP_ERR_ARG / MFGP_ERR_WORKSPACE before any device work; ngroups = 0 is a no-op; a table the
    device rejects reports -1 on every group and writes nothing else."""
    X, Y, prm, _ = LO.case("n79")
    post = _model(X, Y, prm).posterior()
    n, p, d = 79, 3, 3
    lib, dev = eng.lib, eng.device
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    off, rows = i32([0, 2, 3]), i32([5, 40, 7])
    sz = C.c_size_t()
    assert lib.mfgp_gpr_posterior_leave_out_workspace_size(eng.h, 0, n, p, d, 2, 3, C.byref(sz)) == 0
    assert lib.mfgp_gpr_posterior_leave_out_workspace_size(eng.h, 0, n, p, d, 0, 3, C.byref(sz)) == -1
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)

    def call(off, rows, ng, nr, gmax, wsb=None, cb=None):
        out = (torch.full((nr, p), 7.0, **f64), torch.full((nr, max(gmax, 1)), 7.0, **f64),
               torch.full((max(ng, 1), p), 7.0, **f64), torch.full((max(ng, 1),), 7, dtype=torch.int32, device=dev))
        rc = lib.mfgp_gpr_posterior_leave_out(eng.h, 0, n, p, d, ptr(post.cache),
                                              post.cache.numel() if cb is None else cb, ng, ptr(off), ptr(rows), nr,
                                              gmax, ptr(ws), ws.numel() if wsb is None else wsb, ptr(out[0]), p,
                                              ptr(out[1]), max(gmax, 1), ptr(out[2]), ptr(out[3]))
        torch.cuda.synchronize()
        return rc, out

    assert call(off, rows, 2, 3, 33)[0] == -1              # MFGP_ERR_ARG
    assert call(off, rows, 2, 3, 0)[0] == -1
    assert call(off, rows, -1, 3, 2)[0] == -1
    assert call(off, rows, 2, 3, 2, wsb=16)[0] == -2        # MFGP_ERR_WORKSPACE
    assert call(off, rows, 2, 3, 2, cb=1024)[0] == -2
    rc, out = call(off, rows, 0, 3, 2)                      # no-op
    assert rc == 0 and all(bool((o == 7).all()) for o in out)
    rc, out = call(off, rows, 2, 3, 2)
    assert rc == 0 and out[3].tolist() == [0, 0]
    ref = LO.brute(X, Y, prm, [[5, 40], [7]])
    np.testing.assert_allclose(Y[[5, 40, 7]] - out[0].cpu().numpy(), ref["mean"], rtol=0,
                               atol=1e-9 * max(1.0, np.abs(ref["mean"]).max()))
    # a group larger than gmax, and a row index past the end: rejected on the device, nothing written
    for o, r, gmax in ((off, rows, 1), (off, i32([5, 79, 7]), 2), (i32([0, 3, 3]), rows, 3)):
        rc, out = call(o, r, 2, 3, gmax)
        assert rc == 0 and out[3].tolist() == [-1, -1]
        assert all(bool((x == 7).all()) for x in out[:3])
