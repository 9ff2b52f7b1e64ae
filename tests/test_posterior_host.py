"""Cached-posterior surface that needs no GPU: the PrecomputeCacheType enum and the argument /
size validation of the mfgp_*_posterior_* entry points (all of it happens before any device work)."""
import ctypes as C

import pytest

GOKU = dict(n=1164, p=64, d=10)


@pytest.fixture(scope="module")
def lib():
    from multi_fidelity_gpflow_amd import _lib
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    return _lib.load()


@pytest.fixture()
def h(lib):
    hp = C.c_void_p()
    assert lib.mfgp_create(0, C.byref(hp)) == 0
    yield hp
    lib.mfgp_destroy(hp)


def test_precompute_cache_type_names():
    import multi_fidelity_gpflow_amd as M
    from multi_fidelity_gpflow_amd.posteriors import PrecomputeCacheType, _cache_type
    assert M.PrecomputeCacheType is PrecomputeCacheType
    assert [t.name for t in PrecomputeCacheType] == ["TENSOR", "VARIABLE", "NOCACHE"]
    assert [t.value for t in PrecomputeCacheType] == ["tensor", "variable", "nocache"]   # the GPflow values
    assert _cache_type(None) is PrecomputeCacheType.NOCACHE
    assert _cache_type("Variable") is PrecomputeCacheType.VARIABLE
    assert _cache_type(PrecomputeCacheType.TENSOR) is PrecomputeCacheType.TENSOR
    with pytest.raises(ValueError):
        _cache_type("sometimes")
    for cls in (M.MultiFidelityGPModel, M.GraphMultiFidelityGPModel, M.SingleBinSVGP,
                M.LatentMFCoregionalizationSVGP):
        assert callable(getattr(cls, "posterior"))


def test_gpr_posterior_sizes(lib, h):
    n, p, d = GOKU["n"], GOKU["p"], GOKU["d"]
    sz = C.c_size_t()
    for nb in (32, 64):
        assert lib.mfgp_set_tile(h, nb) == 0
        npad, ppad = -(-n // nb) * nb, -(-p // nb) * nb
        for nlf in (0, 2):
            assert lib.mfgp_gpr_posterior_size(h, nlf, n, p, d, C.byref(sz)) == 0
            assert sz.value >= npad * (npad + ppad) * 8        # L^{-1} tiles | Z, the factor's Xo block
            assert sz.value < npad * (npad + ppad) * 8 + (1 << 20)
            for ns in (1, 36, 200):
                assert lib.mfgp_gpr_posterior_predict_workspace_size(h, nlf, n, p, d, ns, C.byref(sz)) == 0
                assert sz.value > 0
    assert lib.mfgp_set_tile(h, 32) == 0
    # the predict workspace grows with nstar only by whole column tiles
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 1, C.byref(a)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 32, C.byref(b)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 33, C.byref(c)) == 0
    assert a.value == b.value < c.value
    # d > 32: -4; null / zero arguments: -1
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, 33, C.byref(sz)) == -4
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, 33, 1, C.byref(sz)) == -4
    assert lib.mfgp_gpr_posterior_size(None, 0, n, p, d, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, d, None) == -1
    assert lib.mfgp_gpr_posterior_size(h, 0, 0, p, d, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_size(h, 0, n, 0, d, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_size(h, 5, n, p, d, C.byref(sz)) == -1      # more LF sources than supported
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 0, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 1, None) == -1


def test_svgp_posterior_sizes(lib, h):
    m, L, p, d = 300, 64, 64, 10
    sz = C.c_size_t()
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, C.byref(sz)) == 0
    mpad = -(-m // 32) * 32
    assert sz.value >= 2 * L * mpad * mpad * 8                 # Lm^{-1} and Lq^T Lm^{-1} per latent
    for ns in (1, 36):
        assert lib.mfgp_svgp_posterior_predict_workspace_size(h, ns, m, L, p, d, C.byref(sz)) == 0
        assert sz.value > 0
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, 33, C.byref(sz)) == -4
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, 1, m, L, p, 33, C.byref(sz)) == -4
    assert lib.mfgp_svgp_posterior_size(None, m, L, p, d, C.byref(sz)) == -1
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, None) == -1
    assert lib.mfgp_svgp_posterior_size(h, 0, L, p, d, C.byref(sz)) == -1
    assert lib.mfgp_svgp_posterior_size(h, m, 0, p, d, C.byref(sz)) == -1
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, 0, m, L, p, d, C.byref(sz)) == -1
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, 1, m, L, p, d, None) == -1


def _ntasks(T, chunk, full):
    """post_ntasks (mfgp_posterior.hip): row tile i has ceil((full ? T : i + 1) / chunk) tasks."""
    return sum(-(-(T if full else i + 1) // chunk) for i in range(T))


# (n or M, p, d, batch, svgp, nstar, whole rows?) of tests/test_gpu_posterior.py's schedule cases (NB = 32)
SCHEDULE_CASES = {
    "gpr-whole-rows-n500-ns512": (500, 3, 3, 1, False, 512, True),
    "gpr-chunked-n500-ns32": (500, 3, 3, 1, False, 32, False),
    "gpr-9-partials-n2081-ns33": (2081, 2, 1, 1, False, 33, False),
    "gpr-9-partials-n2081-ns1": (2081, 2, 1, 1, False, 1, False),
    "svgp-chunked-m270-l3-ns1": (270, 6, 5, 3, True, 1, False),
    "svgp-chunked-m270-l3-ns33": (270, 6, 5, 3, True, 33, False),
    "svgp-whole-rows-m270-l3-ns320": (270, 6, 5, 3, True, 320, True),
}


@pytest.mark.parametrize("case", list(SCHEDULE_CASES))
def test_posterior_shapes_reach_their_schedule(case, lib, h):
    """Which k_post_a schedule a shape takes (whole rows, or 8-tile chunks: post_chunk switches at
    batch T Ts >= 256) cannot be seen from a prediction, but it sets the workspace size: Apart (and
    Bpart for SVGP) is batch x ntask x Ts x nb^2 doubles.  The reported size must be the intended
    schedule's partials plus the other post_layout buffers (restated here, each aligned to 256 B), and the
    other schedule's partials plus the same buffers must not fit that size.  If this fails, the 256
    threshold or POST_CHUNK moved: revisit the shapes of tests/test_gpu_posterior.py's schedule tests,
    which then no longer run the paths they name."""
    nm, p, d, batch, svgp, nstar, whole = SCHEDULE_CASES[case]
    nb = 32
    T, Tp, Ts = -(-nm // nb), -(-p // nb), -(-nstar // nb)
    nspad, ngrp = Ts * nb, -(-T // 4)
    assert (batch * T * Ts >= 256) == whole, "the case is on the wrong side of the whole-row threshold"
    want, other = (T, 8) if whole else (8, T)
    nt_want, nt_other = _ntasks(T, want, svgp), _ntasks(T, other, svgp)
    assert nt_want != nt_other, "the two schedules cut this shape alike: the case tells nothing"
    if not whole and not svgp:
        assert T > 8
    if case.startswith("gpr-9-partials"):
        assert -(-T // 8) == 9            # the last row tile: more than post_sum's 8 loads at a time
    if svgp and not whole:
        assert T > 8                      # tasks wholly right of the diagonal, and nch > 1 partials
    sz = C.c_size_t()
    if svgp:
        assert lib.mfgp_svgp_posterior_predict_workspace_size(h, nstar, nm, batch, p, d, C.byref(sz)) == 0
        rest = [4 * Ts] + [8 * batch * ngrp * nspad] * 3 + [8 * batch * nspad] * 2
        nparts = 2
    else:
        assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, nm, p, d, nstar, C.byref(sz)) == 0
        rest = [4 * Ts, 8 * ngrp * nspad * Tp * nb, 8 * ngrp * nspad, 8 * T * nb * nspad, 8 * nspad * nspad,
                8 * nspad * nspad]
        nparts = 1
    part = lambda ntask: nparts * 8 * batch * ntask * Ts * nb * nb
    slack = 256 * (len(rest) + nparts + 1)            # the carve's alignment and its closing 256 B
    lo = part(nt_want) + sum(rest)
    print(f"{case}: {sz.value} B, partials {part(nt_want)} B ({nt_want} tasks; the other schedule: {nt_other})")
    assert part(nt_want) <= sz.value <= lo + slack
    assert lo <= sz.value
    lo_other = part(nt_other) + sum(rest)
    assert not (lo_other <= sz.value <= lo_other + slack)
    assert abs(part(nt_other) - part(nt_want)) > slack


def test_posterior_calls_validate_before_device_work(lib, h):
    """Null pointers: -1.  A cache or workspace below the reported size: MFGP_ERR_WORKSPACE (-2).  The
    pointers are never dereferenced on these paths (there is no device here to take them)."""
    n, p, d = GOKU["n"], GOKU["p"], GOKU["d"]
    fake = C.c_void_p(4096)
    csz, wsz = C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, d, C.byref(csz)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 36, C.byref(wsz)) == 0
    big = 1 << 40
    args = lambda cb, wb: (h, 0, n, p, d, 36, fake, cb, fake, d + 1, fake, wb, fake, p, fake, None, 0)
    assert lib.mfgp_gpr_posterior_predict(*args(csz.value - 1, big)) == -2
    assert lib.mfgp_gpr_posterior_predict(*args(big, wsz.value - 1)) == -2
    assert lib.mfgp_gpr_posterior_predict(h, 0, n, p, d, 36, None, big, fake, d + 1, fake, big, fake, p, fake,
                                          None, 0) == -1
    assert lib.mfgp_gpr_posterior_predict(h, 0, n, p, d, 0, fake, big, fake, d + 1, fake, big, fake, p, fake,
                                          None, 0) == -1
    assert lib.mfgp_gpr_posterior_predict(h, 0, n, p, 33, 36, fake, big, fake, 34, fake, big, fake, p, fake,
                                          None, 0) == -4
    # build: null data, then a too-small cache
    assert lib.mfgp_gpr_posterior_build(h, 0, n, p, d, None, d + 1, fake, p, fake, fake, big, fake, big, fake) == -1
    assert lib.mfgp_gpr_posterior_build(h, 0, n, p, d, fake, d + 1, fake, p, fake, fake, big, fake, csz.value - 1,
                                        fake) == -2
    assert lib.mfgp_gpr_posterior_build(h, 0, n, p, d, fake, d + 1, fake, p, fake, fake, 1024, fake, big, fake) == -2
    # SVGP
    m, L = 300, 64
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, C.byref(csz)) == 0
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, 36, m, L, p, d, C.byref(wsz)) == 0
    sargs = lambda cb, wb: (h, 36, m, L, p, d, 0, fake, cb, fake, d + 1, fake, wb, fake, fake)
    assert lib.mfgp_svgp_posterior_predict(*sargs(csz.value - 1, big)) == -2
    assert lib.mfgp_svgp_posterior_predict(*sargs(big, wsz.value - 1)) == -2
    assert lib.mfgp_svgp_posterior_predict(h, 36, m, L, p, d, 0, None, big, fake, d + 1, fake, big, fake, fake) == -1
    assert lib.mfgp_svgp_posterior_predict(h, 36, m, 15, p, d, 0, fake, big, fake, d + 1, fake, big, fake, fake) == -1
    assert lib.mfgp_svgp_posterior_build(h, m, L, p, d, None, d + 1, fake, fake, fake, None, 1e-6, fake, big, fake,
                                         big, fake) == -1
    assert lib.mfgp_svgp_posterior_build(h, m, L, p, d, fake, d + 1, fake, fake, fake, None, 1e-6, fake, big, fake,
                                         csz.value - 1, fake) == -2
    assert lib.mfgp_svgp_posterior_build(h, m, L, p, d, fake, d + 1, fake, fake, fake, None, 1e-6, fake, 1024, fake,
                                         big, fake) == -2
