"""The log-density feature without a GPU: the numpy oracle of tests/_logdens_oracle.py against scipy and torch
autograd (to a tenth of the GPU tests' bound), the C ABI's strides on flat arrays, the argument / size
validation of mfgp_mvn_logpdf and the fused posterior entries (all before any device work: the pointers are
never dereferenced here), and every ValueError / NotImplementedError of log_density / predict_log_density
that needs no device."""
import ctypes as C

import numpy as np
import pytest

import _logdens_oracle as LD
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import PrecomputeCacheType, posteriors

TENTH = 0.1 * LD.BOUND


def _close(name, got, ref, bound=TENTH):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, name
    err = np.abs(got - ref).max() if ref.size else 0.0
    lim = bound * max(1.0, np.abs(ref).max() if ref.size else 0.0)
    print(f"{name}: err {err:.1e} (bound {lim:.1e})")
    assert err <= lim, (name, err)


@pytest.mark.parametrize("p", [1, 2, 31, 64, 65, 128])
def test_oracle_against_scipy_and_autograd(p):
    """logp against scipy.stats.multivariate_normal.logpdf; logp, gmean and gvar against torch autograd of
    the textbook expression.  Measured: <= 4e-13 relative at every P."""
    from scipy.stats import multivariate_normal
    ns = 3
    mean, Y, var, ov, Cm = LD.case(ns, p, 100 + p)
    assert np.linalg.cond(Cm) <= 1e3 * (1 + 1e-9)
    logp, gm, gv = LD.logpdf(mean, Y, var, ov, Cm)
    for s in range(ns):
        S = LD.lower_sym(Cm) + np.diag(var[s] + ov[s])
        _close(f"scipy P={p} row {s}", logp[s], multivariate_normal.logpdf(Y[s], mean=mean[s], cov=S))
    tl, tm, tv = LD.torch_reference(mean, Y, var, ov, Cm)
    _close(f"autograd logp P={p}", logp, tl)
    _close(f"autograd gmean P={p}", gm, tm)
    _close(f"autograd gvar P={p}", gv, tv)
    # one variance per row: its derivative is the sum over the outputs
    mean, Y, var1, _, Cm = LD.case(ns, p, 200 + p, per_row_y=False, var_cols=False, obs_var=None)
    l1, m1, v1 = LD.logpdf(mean, Y, var1, None, Cm)
    tl, tm, tv = LD.torch_reference(mean, Y, var1, None, Cm)
    _close(f"autograd (shared Y, var [ns]) logp P={p}", l1, tl)
    _close(f"autograd (shared Y, var [ns]) gvar P={p}", v1, tv)


def test_oracle_diagonal_form_and_missing_targets():
    """Without obs_cov the dense oracle with a zero obs_cov gives the same numbers; NaN targets drop out
    (an all-NaN row: logp 0, gradients 0), and the result equals the sum over the present outputs."""
    ns, p = 4, 37
    rng = np.random.default_rng(5)
    mean, Y, var, ov, _ = LD.case(ns, p, 7)
    a = LD.logpdf(mean, Y, var, ov, None)
    b = LD.logpdf(mean, Y, var, ov, np.zeros((p, p)))
    for x, y, n in zip(a, b, ("logp", "gmean", "gvar")):
        _close(f"diag vs dense {n}", x, y)
    Yn = Y.copy()
    Yn[rng.random((ns, p)) < 0.15] = np.nan
    Yn[2] = np.nan
    logp, gm, gv = LD.logpdf(mean, Yn, var, ov, None)
    assert logp[2] == 0.0 and np.all(gm[2] == 0.0) and np.all(gv[2] == 0.0)
    for s in (0, 1, 3):
        ok = ~np.isnan(Yn[s])
        ref = LD.logpdf(mean[s:s + 1, ok], Yn[s:s + 1, ok], var[s:s + 1, ok], ov[s:s + 1, ok], None)
        _close(f"present outputs row {s}", logp[s], ref[0][0])
        assert np.all(gm[s][~ok] == 0.0) and np.all(gv[s][~ok] == 0.0)
        np.testing.assert_array_equal(gm[s][ok], ref[1][0])


@pytest.mark.parametrize("dense", [True, False])
def test_abi_strides_on_flat_arrays(dense):
    """y_rs = 0 (one shared vector), var_cs = 0 (one variance per row), ov_rs = 0 (shared), padded leading
    dimensions and a NaN upper triangle of obs_cov, element by element through the header's addressing."""
    ns, p, ldm, ldc, ldg = 3, 5, 7, 8, 6
    rng = np.random.default_rng(11)
    mean, Y, var, ov, Cm = LD.case(ns, p, 13, per_row_y=False, var_cols=False, obs_var="shared")
    fm = np.full((ns * ldm,), np.nan)
    for s in range(ns):
        fm[s * ldm:s * ldm + p] = mean[s]
    fc = None
    if dense:
        fc = np.full((p * ldc,), np.nan)
        for i in range(p):
            fc[i * ldc:i * ldc + i + 1] = Cm[i, :i + 1]
    logp, gm, gv = LD.emulate_abi(ns, p, fm, ldm, Y, 0, var, 1, 0, ov, 0, fc, ldc, ldg, ldg)
    ref = LD.logpdf(mean, Y, var, ov, Cm if dense else None)
    np.testing.assert_array_equal(logp, ref[0])
    np.testing.assert_array_equal(gm.reshape(ns, ldg)[:, :p], ref[1])
    np.testing.assert_array_equal(gv.reshape(ns, ldg)[:, :p], ref[2])
    assert np.all(np.isnan(gm.reshape(ns, ldg)[:, p:]))
    # per-row forms through the same addressing
    Yr, vr, orow = rng.standard_normal((ns, p)), rng.uniform(0.1, 0.4, (ns, p)), rng.uniform(0.1, 0.4, (ns, p))
    logp, gm, gv = LD.emulate_abi(ns, p, fm, ldm, Yr.ravel(), p, vr.ravel(), p, 1, orow.ravel(), p, fc, ldc, p, p)
    ref = LD.logpdf(mean, Yr, vr, orow, Cm if dense else None)
    np.testing.assert_array_equal(logp, ref[0])
    np.testing.assert_array_equal(gv.reshape(ns, p), ref[2])


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


def test_mvn_logpdf_validates_before_device_work(lib, h):
    fake, big = C.c_void_p(4096), 1 << 30
    sz = C.c_size_t()
    assert lib.mfgp_mvn_logpdf_workspace_size(h, 1024, 64, C.byref(sz)) == 0 and sz.value >= 1
    assert lib.mfgp_mvn_logpdf_workspace_size(h, -1, 64, C.byref(sz)) == -1
    assert lib.mfgp_mvn_logpdf_workspace_size(h, 4, 0, C.byref(sz)) == -1
    assert lib.mfgp_mvn_logpdf_workspace_size(h, 4, 4, None) == -1

    def call(ns=4, p=8, mean=fake, ldm=8, Y=fake, y_rs=8, var=fake, var_rs=8, var_cs=1, ov=fake, ov_rs=0, oc=fake,
             ldc=8, ws=fake, wb=big, logp=fake, gm=fake, ldgm=8, gv=fake, ldgv=8, info=fake):
        return lib.mfgp_mvn_logpdf(h, ns, p, mean, ldm, Y, y_rs, var, var_rs, var_cs, ov, ov_rs, oc, ldc, ws, wb, logp,
                                   gm, ldgm, gv, ldgv, info)

    assert call(ns=0, mean=None, Y=None, var=None, logp=None, info=None, ws=None) == 0   # a no-op, pointers unseen
    assert call(ns=-1) == -1 and call(p=0) == -1
    assert call(p=129, ldm=129, y_rs=129, var_rs=129, ldc=129, ldgm=129, ldgv=129) == -1   # dense: P <= 128
    assert call(p=129, ldm=129, y_rs=129, var_rs=129, ldgm=129, ldgv=129, oc=None, ns=0) == 0   # diagonal: any P
    assert call(ldm=7) == -1 and call(ldc=7) == -1 and call(ldgm=7) == -1 and call(ldgv=7) == -1
    assert call(y_rs=7) == -1 and call(ov_rs=7) == -1 and call(y_rs=-8) == -1 and call(var_cs=2) == -1
    assert call(ldgv=1) == -1                          # the summed gvar needs one variance per row
    assert call(ldgv=1, var_cs=0, var_rs=1, ns=0) == 0
    for name in ("mean", "Y", "var", "logp", "info", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(wb=sz.value - 1) == -2
    assert call(ns=-1, wb=0) == -1                     # the argument error comes first


def test_fused_entries_validate_before_device_work(lib, h):
    n, p, d, ns = 1164, 64, 10, 36
    fake, big = C.c_void_p(4096), 1 << 40
    csz, pw, vw, lw = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.mfgp_gpr_posterior_size(h, 0, n, p, d, C.byref(csz)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, ns, C.byref(pw)) == 0
    assert lib.mfgp_gpr_posterior_predict_vjp_workspace_size(h, 0, n, p, d, ns, C.byref(vw)) == 0
    assert lib.mfgp_gpr_posterior_logdens_workspace_size(h, 0, n, p, d, ns, C.byref(lw)) == 0
    # the VJP layout, then gmean [ns x p] and the summed gvar [ns]
    assert 8 * (ns * p + ns) <= lw.value - vw.value <= 8 * (ns * p + ns) + 4 * 256
    gw = C.c_size_t()
    assert lib.mfgp_gpr_posterior_logdens_workspace_size(h, 2, n, p, d, ns, C.byref(gw)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 2, n, p, d, ns, C.byref(pw)) == 0 and gw.value == pw.value
    assert lib.mfgp_gpr_posterior_logdens_workspace_size(h, 0, n, p, 33, ns, C.byref(lw)) == -4
    assert lib.mfgp_gpr_posterior_logdens_workspace_size(h, 0, n, p, d, 0, C.byref(lw)) == -1
    assert lib.mfgp_gpr_posterior_logdens_workspace_size(h, 0, n, p, d, ns, C.byref(lw)) == 0
    assert lib.mfgp_gpr_posterior_predict_workspace_size(h, 0, n, p, d, ns, C.byref(pw)) == 0

    def gpr(nlf=0, nstar=ns, pp=p, cache=fake, cb=big, wb=big, Y=fake, y_rs=0, oc=fake, ldc=p, logp=fake, gX=fake,
            ldgx=d + 1, info=fake):
        return lib.mfgp_gpr_posterior_logdens(h, nlf, n, pp, d, nstar, cache, cb, fake, d + 1, fake, wb, fake, pp, fake,
                                              Y, y_rs, None, 0, oc, ldc, logp, gX, ldgx, info)

    assert gpr(cb=csz.value - 1) == -2
    assert gpr(wb=lw.value - 1) == -2
    assert gpr(wb=vw.value) == -2                      # the VJP workspace lacks the density's gradients
    assert gpr(gX=None, wb=pw.value - 1) == -2         # the value alone needs the predict workspace only
    assert gpr(nlf=1) == -1                            # the graph kernel has no input gradient
    assert gpr(nlf=1, gX=None, wb=0) == -2             # ... but the value: the next check is the workspace
    assert gpr(pp=129, ldc=129) == -1                  # dense: P <= 128
    assert gpr(pp=129, oc=None, wb=0) == -2            # diagonal: any P
    assert gpr(ldc=p - 1) == -1 and gpr(ldgx=d) == -1 and gpr(y_rs=p - 1) == -1
    for name in ("cache", "Y", "logp", "info"):
        assert gpr(**{name: None}) == -1, name
    assert gpr(nstar=-1) == -1
    assert gpr(nstar=0, cache=None, Y=None, logp=None, info=None) == 0
    m, L = 300, 64
    assert lib.mfgp_svgp_posterior_size(h, m, L, p, d, C.byref(csz)) == 0
    assert lib.mfgp_svgp_posterior_predict_workspace_size(h, ns, m, L, p, d, C.byref(pw)) == 0
    assert lib.mfgp_svgp_posterior_predict_vjp_workspace_size(h, ns, m, L, p, d, C.byref(vw)) == 0
    assert lib.mfgp_svgp_posterior_logdens_workspace_size(h, ns, m, L, p, d, C.byref(lw)) == 0
    assert 8 * 2 * ns * p <= lw.value - vw.value <= 8 * 2 * ns * p + 4 * 256
    assert lib.mfgp_svgp_posterior_logdens_workspace_size(h, 0, m, L, p, d, C.byref(lw)) == -1
    assert lib.mfgp_svgp_posterior_logdens_workspace_size(h, ns, m, L, p, d, C.byref(lw)) == 0

    def svgp(nstar=ns, ll=L, cache=fake, cb=big, wb=big, oc=fake, ldc=p, gX=fake, ldgx=d + 1, info=fake):
        return lib.mfgp_svgp_posterior_logdens(h, nstar, m, ll, p, d, 0, cache, cb, fake, d + 1, fake, wb, fake, fake,
                                               fake, p, fake, p, oc, ldc, fake, gX, ldgx, info)

    assert svgp(cb=csz.value - 1) == -2
    assert svgp(wb=lw.value - 1) == -2 and svgp(wb=vw.value) == -2
    assert svgp(gX=None, wb=pw.value - 1) == -2
    assert svgp(cache=None) == -1 and svgp(info=None) == -1 and svgp(ldgx=d) == -1 and svgp(ldc=p - 1) == -1
    assert svgp(ll=15) == -1                           # no W: l must equal p
    assert svgp(nstar=0, cache=None) == 0


# ---------------------------------------------------------------- the Python surface, before any device work
def _gpr_model(P=3, D=2, dtype=None):
    rng = np.random.default_rng(3)
    X = np.hstack([rng.random((12, D)), (np.arange(12) % 2)[:, None].astype(float)])
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(D))
    return M.MultiFidelityGPModel(X, rng.standard_normal((12, P)), kern(), kern(), dtype=dtype)


def _bare_posterior(cls, shape, nlf=0):
    """A posterior object with a shape and a cache type but no device block: what the argument checks see."""
    post = object.__new__(cls)
    post._precompute_cache = PrecomputeCacheType.TENSOR
    post._shape, post._nlf = shape, nlf
    post.cache, post._valid = None, False
    return post


def test_density_plan_errors():
    ns, p = 4, 3
    Y, Yr = np.zeros(p), np.zeros((ns, p))
    posteriors.density_plan("t", ns, p, Y, None, None)
    posteriors.density_plan("t", ns, p, Yr, 0.5, np.eye(p))
    posteriors.density_plan("t", ns, p, Yr, np.ones(p), None)
    posteriors.density_plan("t", ns, p, Yr, np.ones((ns, p)), np.eye(p))
    for bad in (np.zeros(p + 1), np.zeros((ns + 1, p)), np.zeros((ns, p, 1)), 0.0):
        with pytest.raises(ValueError, match="Y has shape"):
            posteriors.density_plan("t", ns, p, bad, None, None)
    for bad in (np.ones(p + 1), np.ones((ns, p + 1)), np.ones((1, p))):
        with pytest.raises(ValueError, match="obs_var has shape"):
            posteriors.density_plan("t", ns, p, Y, bad, None)
    for bad in (-1e-3, np.array([1.0, -1.0, 1.0]), np.full((ns, p), np.nan)):
        with pytest.raises(ValueError, match="non-negative"):
            posteriors.density_plan("t", ns, p, Y, bad, None)
    for bad in (np.eye(p + 1), np.ones(p), np.ones((p, p, 1))):
        with pytest.raises(ValueError, match="obs_cov has shape"):
            posteriors.density_plan("t", ns, p, Y, None, bad)
    with pytest.raises(ValueError, match="P <= 128"):
        posteriors.density_plan("t", 2, 129, np.zeros(129), None, np.eye(129))
    posteriors.density_plan("t", 2, 129, np.zeros(129), 1.0, None)   # the diagonal form has no limit


def test_log_density_errors_before_device_work():
    """NOCACHE and the graph model's grad=True: NotImplementedError, as predict_f_vjp; then every ValueError
    of the arguments, raised before the engine is looked up (there is no device here)."""
    m = _gpr_model()
    Xs = np.zeros((4, 3))
    nc = m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE)
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        nc.log_density(Xs, np.zeros(3))
    with pytest.raises(NotImplementedError, match="NOCACHE"):
        nc.predict_f_vjp(Xs, np.zeros((4, 3)))
    graph = _bare_posterior(M.GPRPosterior, (12, 3, 2), nlf=2)
    with pytest.raises(NotImplementedError, match="graph kernel") as e1:
        graph.log_density(Xs, np.zeros(3), grad=True)
    with pytest.raises(NotImplementedError) as e2:
        graph.predict_f_vjp(Xs, np.zeros((4, 3)))
    assert str(e1.value) == str(e2.value)
    for post in (_bare_posterior(M.GPRPosterior, (12, 3, 2)), _bare_posterior(M.SVGPPosterior, (10, 3, 3, 2, False))):
        with pytest.raises(ValueError, match="Xnew"):
            post.log_density(np.zeros((4, 4)), np.zeros(3))
        with pytest.raises(ValueError, match="Y has shape"):
            post.log_density(Xs, np.zeros(4))
        with pytest.raises(ValueError, match="Y has shape"):
            post.log_density(Xs, np.zeros((3, 3)))
        with pytest.raises(ValueError, match="obs_var has shape"):
            post.log_density(Xs, np.zeros(3), obs_var=np.ones(2))
        with pytest.raises(ValueError, match="non-negative"):
            post.log_density(Xs, np.zeros(3), obs_var=-1.0)
        with pytest.raises(ValueError, match="obs_cov has shape"):
            post.log_density(Xs, np.zeros(3), obs_cov=np.eye(4), grad=True)
    wide = _bare_posterior(M.GPRPosterior, (12, 129, 2))
    with pytest.raises(ValueError, match="P <= 128"):
        wide.log_density(Xs, np.zeros(129), obs_cov=np.eye(129))
    assert M.LogDensityResult._fields == ("logp", "mean", "var", "grad_X")


def _svgp_model(kind, P=3, D=2):
    rng = np.random.default_rng(4)
    X = np.hstack([rng.random((14, D)), (np.arange(14) % 2)[:, None].astype(float)])
    kern = lambda: M.SquaredExponential(lengthscales=np.ones(D))
    if kind == "singlebin":
        return M.SingleBinSVGP(X, rng.standard_normal((14, P)), kern(), kern(), P, Z=X[:6].copy())
    if kind == "masked":
        return M.SingleBinSVGP(X, rng.standard_normal((14, P)), kern(), kern(), P, Z=X[:6].copy(),
                               missing_outputs=True)
    Y = rng.standard_normal((14, 2 * P if kind == "het" else P))
    return M.LatentMFCoregionalizationSVGP(X, Y, kern(), kern(), num_latents=2, num_inducing=6, num_outputs=P,
                                           heterosed=kind == "het")


@pytest.mark.parametrize("kind", ["gpr", "gpr32", "graph", "singlebin", "latent", "het", "masked"])
def test_predict_log_density_errors_before_device_work(kind):
    P, D = 3, 2
    if kind == "gpr":
        m = _gpr_model(P, D)
    elif kind == "gpr32":
        m = _gpr_model(P, D, dtype="float32")
    elif kind == "graph":
        rng = np.random.default_rng(6)
        X = np.hstack([rng.random((12, D)), (np.arange(12) % 3)[:, None].astype(float)])
        kern = lambda: M.SquaredExponential(lengthscales=np.ones(D))
        m = M.GraphMultiFidelityGPModel(X, rng.standard_normal((12, P)), [kern(), kern()], kern())
    else:
        m = _svgp_model(kind, P, D)
    Xs, Ys = np.zeros((5, D + 1)), np.zeros((5, P))
    objs = [m]
    if kind != "gpr32":   # (the float32 path has no posterior())
        objs.append(m.posterior(precompute_cache=PrecomputeCacheType.NOCACHE))
    for obj in objs:
        for kw in (dict(full_cov=True), dict(full_output_cov=True), dict(full_cov=True, full_output_cov=True)):
            with pytest.raises(NotImplementedError, match="full_cov=False and full_output_cov=False"):
                obj.predict_log_density((Xs, Ys), **kw)
        with pytest.raises(ValueError, match="pair"):
            obj.predict_log_density(Xs)
        with pytest.raises(ValueError, match="Xnew has shape"):
            obj.predict_log_density((np.zeros(5), Ys))
        with pytest.raises(ValueError, match="Ynew has shape"):
            obj.predict_log_density((Xs, np.zeros((4, P))))
        with pytest.raises(ValueError, match="Ynew has shape"):
            obj.predict_log_density((Xs, np.zeros((5, P + 1))))
        if kind != "het":   # only the heteroscedastic likelihood takes [Y_obs | Y_unc]
            with pytest.raises(ValueError, match="Ynew has shape"):
                obj.predict_log_density((Xs, np.zeros((5, 2 * P))))
