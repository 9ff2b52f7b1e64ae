"""The mfgp_*_posterior_predict_vjp entry points without a GPU: workspace sizes and the argument / size
validation, all of which happens before any device work (the pointers are never dereferenced here)."""
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


def test_vjp_workspace_holds_the_predict_workspace_and_the_partials(lib, h):
    """The VJP workspace is the predict call's, then D x NB doubles per (task, column tile) and the
    counters; SVGP also keeps A and B of every latent (2 L Mpad Nspad doubles)."""
    n, p, d = GOKU["n"], GOKU["p"], GOKU["d"]
    pw, vw = C.c_size_t(), C.c_size_t()
    for nb in (32, 64):
        assert lib.mfgp_set_tile(h, nb) == 0
        for ns in (1, 36, 70):
            ts = -(-ns // nb)
            assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, ns, C.byref(pw)) == 0
            assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, d, ns, C.byref(vw)) == 0
            T = -(-n // nb)
            ntask = sum(-(-(i + 1) // 8) for i in range(T))          # 8-tile chunks: T Ts < 256
            extra = vw.value - pw.value
            assert 8 * ntask * ts * nb * d <= extra <= 8 * ntask * ts * nb * d + 4 * 2 * ts + 4 * 256
            m, L = 300, 64
            assert lib.mfgp_svgp_posterior_predict_workspace_size(h, ns, m, L, p, d, C.byref(pw)) == 0
            assert lib.mfgp_svgp_posterior_predict_vjp_workspace_size(h, ns, m, L, p, d, C.byref(vw)) == 0
            mpad = -(-m // nb) * nb
            assert vw.value - pw.value >= 8 * 2 * L * mpad * ts * nb
    sz = C.c_size_t()
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 1, n, p, d, 1, C.byref(sz)) == -1   # graph kernel
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, 33, 1, C.byref(sz)) == -4
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, d, 0, C.byref(sz)) == -1
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, d, 1, None) == -1
    assert lib.mfgp_svgp_posterior_predict_vjp_workspace_size(h, 1, 300, 64, p, 33, C.byref(sz)) == -4
    assert lib.mfgp_svgp_posterior_predict_vjp_workspace_size(h, 0, 300, 64, p, d, C.byref(sz)) == -1


def test_vjp_calls_validate_before_device_work(lib, h):
    """Null pointers and short leading dimensions: -1.  The graph kernel: -1.  A cache below its size, or a
    workspace that fits the predict call but not the VJP: MFGP_ERR_WORKSPACE (-2).  nstar = 0: a no-op."""
    n, p, d = GOKU["n"], GOKU["p"], GOKU["d"]
    fake, big = C.c_void_p(4096), 1 << 40
    csz, pw, vw = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, d, C.byref(csz)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, 36, C.byref(pw)) == 0
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, d, 36, C.byref(vw)) == 0

    def gpr(nlf=0, ns=36, cache=fake, cb=big, wb=big, gX=fake, ldgx=d + 1, gm=fake, ldgm=p, gv=fake, dd=d):
        return lib.mfgp_gpr_posterior_predict_vjp(h, nlf, n, p, dd, ns, cache, cb, fake, dd + 1, fake, wb, fake, p,
                                                  fake, gm, ldgm, gv, gX, ldgx)

    assert gpr(cb=csz.value - 1) == -2
    assert gpr(wb=vw.value - 1) == -2
    assert gpr(wb=pw.value) == -2            # the predict call's workspace is not enough
    assert gpr(nlf=1) == -1                  # graph kernel: not built
    assert gpr(cache=None) == -1
    assert gpr(gX=None) == -1
    assert gpr(ldgx=d) == -1
    assert gpr(ldgm=p - 1) == -1
    assert gpr(gm=None, ldgm=0, wb=vw.value - 1) == -2    # a NULL upstream gradient is zero, not an error
    assert gpr(dd=33) == -4
    assert gpr(ns=-1) == -1
    assert gpr(ns=0, cache=None, gX=None) == 0
    m, L = 300, 64
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, C.byref(csz)) == 0
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, 36, m, L, p, d, C.byref(pw)) == 0
    assert lib.mfgp_svgp_posterior_predict_vjp_workspace_size(h, 36, m, L, p, d, C.byref(vw)) == 0

    def svgp(ns=36, ll=L, cache=fake, cb=big, wb=big, gX=fake, ldgx=d + 1, ldgm=p):
        return lib.mfgp_svgp_posterior_predict_vjp(h, ns, m, ll, p, d, 0, cache, cb, fake, d + 1, fake, wb, fake, fake,
                                                   fake, ldgm, None, gX, ldgx)

    assert svgp(cb=csz.value - 1) == -2
    assert svgp(wb=vw.value - 1) == -2
    assert svgp(wb=pw.value) == -2
    assert svgp(cache=None) == -1
    assert svgp(gX=None) == -1
    assert svgp(ldgx=d) == -1
    assert svgp(ldgm=p - 1) == -1
    assert svgp(ll=15) == -1                 # no W: l must equal p
    assert svgp(ns=0, cache=None) == 0


def test_predict_f_vjp_surface():
    import multi_fidelity_gpflow_amd as M
    for cls in (M.GPRPosterior, M.SVGPPosterior):
        assert callable(getattr(cls, "predict_f_vjp"))
