"""The emulator Jacobian / Fisher feature without a GPU: the three CPU forms of the Jacobian (autograd through the
Cholesky form, autograd through the solve form, the numpy closed form the kernels implement) against each other
to a tenth of the GPU tests' bounds on every case tests/test_gpu_jacobian.py uses, the same for the Fisher
matrix; every ValueError / NotImplementedError of mean_jacobian / fisher, raised before any device work; and
the return codes of the new C entries (the pointers are never dereferenced here)."""
import ctypes as C

import numpy as np
import pytest

import _jacobian_oracle as JO
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType, engine as E, posteriors


def _tenth(name, got, ref, goku=False):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, name
    lim = 0.1 * JO.bound(ref, goku)
    err = np.abs(got - ref).max()
    print(f"{name}: err {err:.1e} (|ref|max {np.abs(ref).max():.1e}, a tenth of the bound {lim:.1e})")
    assert err <= lim, (name, err)


def _fisher_forms(name, case, forms, goku=False):
    """The Fisher matrix built from each form of the Jacobian, dense obs_cov (P <= 128 and the image fits) or
    a diagonal obs_var otherwise."""
    p, d = case["chol"].shape[1:]
    oc = JO.obs_cov(p, 7) if posteriors.fisher_dense_fits(p, d) else None
    ov = None if oc is not None else 0.3
    ref = JO.fisher(case["chol"], case["var"], ov, oc)
    for tag, J in forms:
        F = JO.fisher(J, case["var"], ov, oc)
        lim = 0.1 * JO.BOUND * max(1.0, np.abs(ref).max())
        err = np.abs(F - ref).max()
        print(f"{name} fisher {tag}: err {err:.1e} (|F|max {np.abs(ref).max():.1e}, a tenth of the bound {lim:.1e})")
        assert err <= lim, (name, tag, err)


@pytest.mark.parametrize("case", JO.GPR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpr_forms_agree_synthetic(case):
    """Measured (solve / closed vs chol): 1.3e-15 / 0, 3.0e-13 / 2.0e-13, 5.1e-15 / 1.0e-14."""
    c = JO.gpr_synthetic(*case)
    assert c["chol"].shape == (case[4], case[2], case[3])
    forms = [("solve", JO.gpr_solve_form(c)), ("closed", JO.closed_gpr(c["X"], c["Y"], c["Xs"], c["prm"]))]
    for tag, J in forms:
        _tenth(f"gpr {case} {tag}", J, c["chol"])
    _fisher_forms(f"gpr {case}", c, forms)


@pytest.mark.parametrize("which", ["hbs", "goku"])
def test_gpr_forms_agree_datasets(which):
    """Measured (solve / closed vs chol): HBS 9.9e-15 / 1.9e-14 (|ref|max 2.2); Goku 1.6e-12 / 3.1e-12
    (|ref|max 3.0, a tenth of its bound 3.0e-9).  Fisher, dense obs_cov: HBS 2.8e-11 (|F|max 8.9e2), Goku 3.0e-8
    (|F|max 3.1e4, a tenth of the bound 3.1e-6)."""
    c = JO.gpr_dataset(which)
    forms = [("solve", JO.gpr_solve_form(c)), ("closed", JO.closed_gpr(c["X"], c["Y"], c["Xs"], c["prm"]))]
    for tag, J in forms:
        _tenth(f"{which} {tag}", J, c["chol"], goku=which == "goku")
    _fisher_forms(which, c, forms)


def test_gpr_forms_agree_edge_rows():
    """The masked Xnew row has an exactly zero Jacobian in every form."""
    c = JO.gpr_edge_rows()
    closed = JO.closed_gpr(c["X"], c["Y"], c["Xs"], c["prm"])
    _tenth("edge rows solve", JO.gpr_solve_form(c), c["chol"])
    _tenth("edge rows closed", closed, c["chol"])
    assert np.all(c["chol"][5] == 0.0) and np.all(closed[5] == 0.0)


@pytest.mark.parametrize("which", ["synthetic", "singlebin", "latent"])
def test_svgp_forms_agree(which):
    """The L = 11 synthetic latent model and the two HBS models.  Measured (solve / closed vs chol):
    synthetic 1.6e-14 / 8.8e-14, single bin 6.3e-14 / 2.7e-13, latent 3.2e-15 / 6.3e-15."""
    c = JO.svgp_synthetic() if which == "synthetic" else JO.svgp_hbs(which)
    forms = [("solve", JO.svgp_solve_form(c)), ("closed", JO.closed_svgp(c["state"], c["Xs"]))]
    for tag, J in forms:
        _tenth(f"svgp {which} {tag}", J, c["chol"])
    _fisher_forms(f"svgp {which}", c, forms)


def test_fisher_oracle_is_symmetric_and_matches_cholesky_form():
    """J^T solve(Sigma, J) against (L^{-1} J)^T (L^{-1} J) at P = 64, D = 10, cond 1e3."""
    rng = np.random.default_rng(5)
    J, var = rng.standard_normal((3, 64, 10)), rng.uniform(0.05, 0.5, (3, 64))
    oc = JO.obs_cov(64, 9)
    assert np.linalg.cond(oc) <= 1e3 * (1 + 1e-9)
    F = JO.fisher(J, var, 0.1, oc)
    for s in range(3):
        A = np.linalg.solve(np.linalg.cholesky(oc + np.diag(var[s] + 0.1)), J[s])
        assert np.abs(F[s] - A.T @ A).max() <= 0.1 * JO.BOUND * np.abs(F).max()
        assert np.abs(F[s] - F[s].T).max() <= 1e-12 * np.abs(F).max()


# ---------------------------------------------------------------- the Python surface, before any device work
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def _bare_posterior(cls, shape, nlf=0, cache_type=PrecomputeCacheType.TENSOR):
    """A posterior object with a shape and a cache type but no device block: what the argument checks see."""
    post = object.__new__(cls)
    post._precompute_cache = cache_type
    post._shape, post._nlf = shape, nlf
    post.cache, post._valid = None, False
    return post


def test_refusals_come_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    Xs = np.zeros((4, 3))
    for cls, shape in ((M.GPRPosterior, (12, 3, 2)), (M.SVGPPosterior, (10, 3, 3, 2, False))):
        nc = _bare_posterior(cls, shape, cache_type=PrecomputeCacheType.NOCACHE)
        with pytest.raises(NotImplementedError, match="NOCACHE"):
            nc.mean_jacobian(Xs)
        with pytest.raises(NotImplementedError, match="NOCACHE"):
            nc.fisher(Xs)
        post = _bare_posterior(cls, shape)
        for bad in (np.zeros((4, 4)), np.zeros((4, 2)), np.zeros(3)):
            with pytest.raises(ValueError, match="Xnew"):
                post.mean_jacobian(bad)
            with pytest.raises(ValueError, match="Xnew"):
                post.fisher(bad)
        with pytest.raises(ValueError, match="obs_var has shape"):
            post.fisher(Xs, obs_var=np.ones(2))
        with pytest.raises(ValueError, match="obs_var has shape"):
            post.fisher(Xs, obs_var=np.ones((3, 3)))
        for neg in (-1.0, np.array([1.0, -1e-300, 1.0]), np.full((4, 3), np.nan)):
            with pytest.raises(ValueError, match="non-negative"):
                post.fisher(Xs, obs_var=neg)
        for bad in (np.eye(4), np.ones(3), np.ones((3, 3, 1))):
            with pytest.raises(ValueError, match="obs_cov has shape"):
                post.fisher(Xs, obs_cov=bad)
    graph = _bare_posterior(M.GPRPosterior, (12, 3, 2), nlf=2)
    with pytest.raises(NotImplementedError, match="graph kernel") as e0:
        graph.predict_f_vjp(Xs, np.zeros((4, 3)))
    for call in (lambda: graph.mean_jacobian(Xs), lambda: graph.fisher(Xs)):
        with pytest.raises(NotImplementedError, match="graph kernel") as e1:
            call()
        assert str(e1.value) == str(e0.value)   # _check_vjp's existing message
    assert M.FisherResult._fields == ("fisher", "mean", "var", "jacobian")


def test_dense_form_limit(monkeypatch):
    """P <= 128 and P8 + D <= 143: the (P8 + D) x ((P8 + D) | 1) image within 160 KiB."""
    _no_device(monkeypatch)
    fits = posteriors.fisher_dense_fits
    assert fits(64, 10) and fits(1, 1) and fits(65, 32) and fits(104, 32) and fits(128, 15) and fits(120, 23)
    assert not fits(128, 16) and not fits(105, 32) and not fits(129, 1) and not fits(121, 16)
    for p, d in ((128, 15), (128, 16), (105, 32), (64, 10)):
        r = ((p + 7) & ~7) + d
        assert fits(p, d) == (r * (r | 1) * 8 <= 160 * 1024)
    post = _bare_posterior(M.GPRPosterior, (12, 128, 16))
    with pytest.raises(ValueError, match=r"P8 \+ D <= 143.*obs_var"):
        post.fisher(np.zeros((2, 17)), obs_cov=np.eye(128))
    wide = _bare_posterior(M.SVGPPosterior, (10, 129, 129, 2, False))
    with pytest.raises(ValueError, match="P <= 128"):
        wide.fisher(np.zeros((2, 3)), obs_cov=np.eye(129))
    with pytest.raises(AssertionError, match="device was touched"):   # the diagonal form has no limit: next is the engine
        wide.fisher(np.zeros((2, 3)), obs_var=0.5)
    ok = _bare_posterior(M.GPRPosterior, (12, 128, 15))
    with pytest.raises(AssertionError, match="device was touched"):
        ok.fisher(np.zeros((2, 16)), obs_cov=np.eye(128))


def test_weights_attribute_is_read_with_a_default(monkeypatch):
    """Posterior objects are also made with object.__new__ (condition_on): no _jac_weights attribute there."""
    post = _bare_posterior(M.GPRPosterior, (12, 3, 2))
    assert not hasattr(post, "_jac_weights")
    made = []
    monkeypatch.setattr(M.GPRPosterior, "_make_weights", lambda self, eng: made.append(1) or "w")
    post.cache = object()
    assert post._weights(None) == "w" and post._weights(None) == "w" and made == [1]   # built once per block
    post.cache = object()
    assert post._weights(None) == "w" and made == [1, 1]                              # a replaced block: rebuilt


# ---------------------------------------------------------------- the C ABI, before any device work
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


OK, ARG, WS, DIM = 0, -1, -2, -4


def test_gpr_jacobian_return_codes(lib, h):
    n, p, d, ns = 1164, 64, 10, 36
    fake, big = C.c_void_p(4096), 1 << 40
    csz, wsz, jsz, psz = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, d, C.byref(csz)) == OK
    assert lib.mfgp_gpr_jacobian_weights_workspace_size(h, 0, n, p, d, C.byref(wsz)) == OK
    assert wsz.value >= 8 * n * p                                  # alpha [Npad x Ppad]
    assert lib.mfgp_gpr_jacobian_workspace_size(h, 0, n, p, d, ns, C.byref(jsz)) == OK
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, ns, C.byref(psz)) == OK
    assert jsz.value > psz.value                                   # the predict layout, then the partials
    for fn, args in ((lib.mfgp_gpr_jacobian_weights_workspace_size, ()), (lib.mfgp_gpr_jacobian_workspace_size, (ns,))):
        assert fn(None, 0, n, p, d, *args, C.byref(jsz)) == ARG
        assert fn(h, 0, n, p, 33, *args, C.byref(jsz)) == DIM and fn(h, 0, n, p, 0, *args, C.byref(jsz)) == DIM
        assert fn(h, 1, n, p, d, *args, C.byref(jsz)) == ARG       # the graph kernel
        assert fn(h, 0, 0, p, d, *args, C.byref(jsz)) == ARG and fn(h, 0, n, 0, d, *args, C.byref(jsz)) == ARG
        assert fn(h, 0, n, p, d, *args, None) == ARG
    assert lib.mfgp_gpr_jacobian_workspace_size(h, 0, n, p, d, 0, C.byref(jsz)) == ARG
    assert lib.mfgp_gpr_jacobian_workspace_size(h, 0, n, p, d, ns, C.byref(jsz)) == OK

    def weights(hh=h, nlf=0, dd=d, cache=fake, cb=big, w=fake, wb=big):
        return lib.mfgp_gpr_jacobian_weights(hh, nlf, n, p, dd, cache, cb, w, wb)

    assert weights(hh=None) == ARG and weights(dd=33) == DIM and weights(nlf=1) == ARG
    assert weights(cache=None) == ARG and weights(w=None) == ARG
    assert weights(cb=csz.value - 1) == WS and weights(wb=wsz.value - 1) == WS

    def jac(hh=h, nlf=0, dd=d, nstar=ns, cache=fake, cb=big, w=fake, wb=big, Xs=fake, ldxs=d + 1, ws=fake, wsb=big,
            mean=fake, ldm=p, var=fake, J=fake, ldj=p):
        return lib.mfgp_gpr_jacobian(hh, nlf, n, p, dd, nstar, cache, cb, w, wb, Xs, ldxs, ws, wsb, mean, ldm, var, J, ldj)

    assert jac(hh=None) == ARG and jac(dd=33) == DIM and jac(nlf=1) == ARG and jac(nlf=1, nstar=0) == ARG
    assert jac(nstar=0, cache=None, w=None, Xs=None, ws=None, mean=None, var=None, J=None) == OK   # a no-op
    assert jac(nstar=-1) == ARG
    for name in ("cache", "w", "Xs", "ws", "mean", "var", "J"):
        assert jac(**{name: None}) == ARG, name
    assert jac(ldxs=d) == ARG and jac(ldm=p - 1) == ARG and jac(ldj=p - 1) == ARG
    assert jac(cb=csz.value - 1) == WS and jac(wb=wsz.value - 1) == WS
    assert jac(wsb=jsz.value - 1) == WS and jac(wsb=psz.value) == WS
    assert jac(ldj=p - 1, wsb=0) == ARG                            # the argument error comes first


def test_svgp_jacobian_return_codes(lib, h):
    m, L, p, d, ns = 300, 15, 64, 10, 36
    fake, big = C.c_void_p(4096), 1 << 40
    csz, wsz, jsz, psz = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, C.byref(csz)) == OK
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(h, m, L, p, d, C.byref(wsz)) == OK
    assert 8 * L * m <= wsz.value <= 8 * L * (m + 64) + 256       # alpha [l x Mpad]
    assert lib.mfgp_svgp_jacobian_workspace_size(h, ns, m, L, p, d, C.byref(jsz)) == OK
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, ns, m, L, p, d, C.byref(psz)) == OK
    assert jsz.value > psz.value
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(None, m, L, p, d, C.byref(wsz)) == ARG
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(h, m, L, p, 33, C.byref(wsz)) == DIM
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(h, 0, L, p, d, C.byref(wsz)) == ARG
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(h, m, L, p, d, None) == ARG
    assert lib.mfgp_svgp_jacobian_weights_workspace_size(h, m, L, p, d, C.byref(wsz)) == OK
    assert lib.mfgp_svgp_jacobian_workspace_size(h, 0, m, L, p, d, C.byref(jsz)) == ARG
    assert lib.mfgp_svgp_jacobian_workspace_size(h, ns, m, L, p, 0, C.byref(jsz)) == DIM
    assert lib.mfgp_svgp_jacobian_workspace_size(h, ns, m, L, p, d, C.byref(jsz)) == OK

    def weights(hh=h, ll=L, mixed=1, cache=fake, cb=big, w=fake, wb=big):
        return lib.mfgp_svgp_jacobian_weights(hh, m, ll, p, d, mixed, cache, cb, w, wb)

    assert weights(hh=None) == ARG and weights(cache=None) == ARG and weights(w=None) == ARG
    assert weights(mixed=0) == ARG                                 # no W: l must equal p
    assert weights(cb=csz.value - 1) == WS and weights(wb=wsz.value - 1) == WS

    def jac(hh=h, nstar=ns, ll=L, mixed=1, cache=fake, cb=big, w=fake, wb=big, Xs=fake, ldxs=d + 1, ws=fake, wsb=big,
            mu=fake, fv=fake, J=fake, ldj=p):
        return lib.mfgp_svgp_jacobian(hh, nstar, m, ll, p, d, mixed, cache, cb, w, wb, Xs, ldxs, ws, wsb, mu, fv, J, ldj)

    assert jac(hh=None) == ARG and jac(nstar=-1) == ARG and jac(mixed=0) == ARG
    assert jac(nstar=0, cache=None, w=None, J=None) == OK
    for name in ("cache", "w", "Xs", "ws", "mu", "fv", "J"):
        assert jac(**{name: None}) == ARG, name
    assert jac(ldxs=d) == ARG and jac(ldj=p - 1) == ARG
    assert jac(cb=csz.value - 1) == WS and jac(wb=wsz.value - 1) == WS
    assert jac(wsb=jsz.value - 1) == WS and jac(wsb=psz.value) == WS


def test_mvn_fisher_return_codes(lib, h):
    fake, big = C.c_void_p(4096), 1 << 30
    sz = C.c_size_t()
    assert lib.mfgp_mvn_fisher_workspace_size(h, 1024, 64, 10, C.byref(sz)) == OK and sz.value >= 1
    assert lib.mfgp_mvn_fisher_workspace_size(None, 4, 64, 10, C.byref(sz)) == ARG
    assert lib.mfgp_mvn_fisher_workspace_size(h, -1, 64, 10, C.byref(sz)) == ARG
    assert lib.mfgp_mvn_fisher_workspace_size(h, 4, 0, 10, C.byref(sz)) == ARG
    assert lib.mfgp_mvn_fisher_workspace_size(h, 4, 4, 33, C.byref(sz)) == DIM
    assert lib.mfgp_mvn_fisher_workspace_size(h, 4, 4, 4, None) == ARG

    def call(hh=h, ns=4, p=8, d=3, J=fake, ldj=8, var=fake, var_rs=8, var_cs=1, ov=fake, ov_rs=0, oc=fake, ldc=8,
             ws=fake, wb=big, F=fake, info=fake):
        return lib.mfgp_mvn_fisher(hh, ns, p, d, J, ldj, var, var_rs, var_cs, ov, ov_rs, oc, ldc, ws, wb, F, info)

    assert call(hh=None) == ARG and call(d=0) == DIM and call(d=33) == DIM
    assert call(ns=0, J=None, var=None, ws=None, F=None, info=None) == OK   # a no-op, pointers unseen
    assert call(ns=-1) == ARG and call(p=0) == ARG
    assert call(ldj=7) == ARG and call(ldc=7) == ARG and call(ov_rs=7) == ARG and call(ov_rs=-8) == ARG
    assert call(var_cs=2) == ARG and call(var_rs=-1) == ARG
    for name in ("J", "var", "ws", "F", "info"):
        assert call(**{name: None}) == ARG, name
    assert call(wb=sz.value - 1) == WS and call(ov=None, wb=sz.value - 1) == WS   # (obs_var is optional)
    assert call(ns=-1, wb=0) == ARG                                # the argument error comes first
    # the dense form's limit: P <= 128 and P8 + D <= 143; the diagonal form takes any P
    wide = dict(ldj=200, var_rs=200, ldc=200)
    assert call(p=129, d=1, **wide) == ARG
    assert call(p=128, d=16, **wide) == ARG and call(p=105, d=32, **wide) == ARG
    assert call(p=128, d=15, wb=0, **wide) == WS and call(p=104, d=32, wb=0, **wide) == WS   # within: the next check
    assert call(p=200, d=32, oc=None, wb=0, **wide) == WS
    assert call(p=200, d=32, oc=None, ns=0, **wide) == OK
