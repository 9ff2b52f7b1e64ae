"""fp32 GPR path (csrc/mfgp_f32.hip) at its tile edges, per gradient component, and under every
schedule knob, against the fp64 CPU oracle, through the model / Engine API.

Gradient bound.  tests/test_gpu_f32.py bounds max |g - g64| by 3e-4 of max |g64|, and max |g64| is
the noise derivative, 40 to 25,000 times every other component: the 2 D + 3 components of
k32_grad's per-dimension epilogue could all be wrong under it.  Here every component q is bounded on
the scale of its own group (vL, lL, vD, lD, rho0, noise):

    |g_q - g64_q| <= 8 c s_q,   s_q = max |g64| over q's group,
                                c = max_q |g32_q - g64_q| / s_q

with g32 the float32 NumPy restatement of the same algebra (tests/_f32_oracle.py) at the same
inputs; tests/test_f32_oracle_host.py keeps c <= 1e-3 (1.2e-5 to 1.8e-4 at these cases).  The
factor 8 is an allowance, not a measurement: the kernel sums in another order than NumPy (MFMA
tile accumulation over K = n, per-thread fp32 partials over 64 rows before the fp64 wave sum) and
uses __expf.  The project's older bounds (test_gpu_f32.py's header, n <= 2300) are asserted
alongside.

Shapes are (n_lf, n_hf, p, n*) from synthetic_multifidelity(..., D = 10, ...), see
_f32_oracle.EDGE_SHAPES: T = 1 with p = n* = 1; exactly one full tile in n, p and n*; a one-row
second tile in all three; n = 3 * 128 (no identity-padding row); p = 257 (Tp = 3, and a second
256-column block in the refinement's k64_kmat) with n* = 130."""
import functools

import numpy as np
import pytest
import torch

import _f32_oracle as F32
import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd.engine import Engine
from oracle import mfgp_oracle as O

pytestmark = pytest.mark.gpu

D = F32.D
FACTOR = 8.0
TILE = 128


def _defaults(e):
    e.set_f32_panel(6)   # the handle defaults (mfgp_capi.hip)
    e.set_f32_lookahead(True)
    e.set_f32_reserve(32)
    e.set_f32_refine(2)


@pytest.fixture(scope="module")
def eng_module():
    e = Engine.get()
    yield e
    _defaults(e)


@pytest.fixture
def eng(eng_module):
    _defaults(eng_module)   # no test inherits a knob from the one before it
    return eng_module


def _model(name):
    X, Y, _ = F32.case_data(name)
    return M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                  M.SquaredExponential(lengthscales=np.ones(D)), dtype="float32")


def _xt(name):
    return np.array(F32.case_data(name)[2])   # a writable copy: the shared case arrays are read-only


@functools.lru_cache(maxsize=None)
def _pred_ref(name):
    """fp64 oracle: (mean [n*, p], var [n*], cov [n*, n*]), computed once per case."""
    X, Y, Xt = F32.case_data(name)
    mo, co = O.gpr_predict_f_full_cov(X, Y, Xt, O.MFParams.initial(D, Y.shape[1]))
    out = (mo, np.diagonal(co[0]).copy(), co[0].copy())
    for a in out:
        a.setflags(write=False)
    return out


def _check_grad(name, lml, g, tag=""):
    """LML and every gradient component of one log_marginal_likelihood_and_grad() result."""
    ref = F32.case_reference(name)
    err = np.abs(g - ref["g64"])
    ratio = err / (ref["c"] * ref["s"])
    groups = F32.grad_groups(D)
    lerr = abs(lml - ref["l64"]) / abs(ref["l64"])
    old = np.max(err) / np.max(np.abs(ref["g64"]))
    print(f"{name}{tag}: c {ref['c']:.2e}; |g - g64| / (c s) per group "
          + ", ".join(f"{k} {ratio[idx].max():.2f}" for k, idx in groups.items())
          + f"; of max |g| {old:.2e}; LML rel {lerr:.2e}")
    assert g.shape == ref["g64"].shape and np.all(np.isfinite(g))
    assert lerr < 1e-4
    assert old < 3e-4
    bad = {k: float(ratio[idx].max()) for k, idx in groups.items() if ratio[idx].max() > FACTOR}
    assert not bad, f"{name}{tag}: components beyond {FACTOR:g} c s_q: {bad}"


def _check_predict(name, eng, m, tag="", skip_rows=()):
    """Value-only LML, mean and variance with 0, 1 and 2 refinement steps.  Returns the refine-2
    (lml, mean, var) for the callers that compare runs."""
    Xt = _xt(name)
    ref = F32.case_reference(name)
    mo, vo, _ = _pred_ref(name)
    keep = np.setdiff1d(np.arange(len(Xt)), np.asarray(skip_rows, dtype=int))
    scale = np.max(np.abs(mo))
    res = {}
    for refine in (0, 1, 2):
        eng.set_f32_refine(refine)
        lv = float(m.log_marginal_likelihood())
        mean, var = m.predict_f(Xt)
        assert mean.dtype == torch.float32 and tuple(mean.shape) == mo.shape and tuple(var.shape) == mo.shape
        mean, var = mean.numpy(), var.numpy()
        assert np.all(var == var[:, :1])   # one variance, tiled over the outputs
        res[refine] = (lv, mean, var, abs(lv - ref["l64"]) / abs(ref["l64"]),
                       np.max(np.abs(mean[keep] - mo[keep])) / scale, np.max(np.abs(var[keep, 0] - vo[keep])))
    print(f"{name}{tag}: LML rel {res[0][3]:.2e} -> {res[1][3]:.2e}; mean rel {res[0][4]:.2e} -> {res[1][4]:.2e} "
          f"-> {res[2][4]:.2e}; var abs {res[0][5]:.2e}")
    assert res[0][3] < 1e-4 and res[0][4] < 1e-2      # unrefined: not optional, refinement hides factor errors
    assert res[1][3] < 1e-5 and res[1][4] < 1e-4
    assert res[2][3] < 1e-5 and res[2][0] == res[1][0]   # the LML takes one step at either setting
    assert res[2][4] < 1e-5
    for refine in (0, 1, 2):
        assert res[refine][5] < 5e-5
        assert np.array_equal(res[refine][2], res[0][2])   # the variance is the fp32 one, never refined
    return res[2][:3]


def _check_full_cov(name, m):
    Y, Xt = F32.case_data(name)[1], _xt(name)
    mo, _, co = _pred_ref(name)
    mean, cov = m.predict_f(Xt, full_cov=True)
    ns, p = len(Xt), Y.shape[1]
    assert cov.dtype == torch.float32 and tuple(cov.shape) == (p, ns, ns)
    cov, mean = cov.numpy(), mean.numpy()
    _, var = m.predict_f(Xt)
    cerr = np.max(np.abs(cov[0] - co))
    derr = np.max(np.abs(np.diagonal(cov[0]) - var.numpy()[:, 0]))
    print(f"{name}: full_cov abs {cerr:.2e}, diagonal vs variance {derr:.2e}")
    assert np.max(np.abs(mean - mo)) / np.max(np.abs(mo)) < 1e-5   # two refinement steps (the default)
    assert cerr < 1e-4
    assert derr <= 2e-6
    assert np.array_equal(cov[0], cov[p - 1])
    return mean, cov


# ---------------------------------------------------------------- (a), (c): the tile edges
@pytest.mark.parametrize("name", list(F32.EDGE_SHAPES))
def test_f32_edge_gradient_per_component(eng, name):
    lml, g = _model(name).log_marginal_likelihood_and_grad()
    _check_grad(name, lml, g)


@pytest.mark.parametrize("name", list(F32.EDGE_SHAPES))
def test_f32_edge_value_mean_var_cov(eng, name):
    m = _model(name)
    _check_predict(name, eng, m)
    _check_full_cov(name, m)   # n* = 1, 128, 129, 64, 130


# ---------------------------------------------------------------- (b): fractional-fidelity rows
@pytest.mark.parametrize("name", list(F32.FRAC_SHAPES))
def test_f32_fractional_fidelity_rows(eng, name):
    """One LF and one HF training row and one test row carry fidelity 0.5 (linear.py:67-70: rows
    that are neither 0 nor 1 get a zero kernel row).  K + s2 I still has s2 on those training rows'
    diagonal, so their 1/2 W_jj belongs to dLML/dnoise, 60 to 100 % of it here
    (test_f32_oracle_host.py); k32_grad used to skip such rows before it took the noise term.
    (0.9999999999999999 is no such row in fp32: it rounds to 1.0f, an HF row.)  The test row's
    mean and variance are exactly 0, refined or not; the other rows keep the project's bounds."""
    X, Xt = F32.case_data(name)[0], _xt(name)
    n_lf = F32.ALL_CASES[name][0]
    assert X[5, -1] == 0.5 and X[n_lf + 7, -1] == 0.5 and Xt[F32.FRAC_TEST_ROW, -1] == 0.5
    m = _model(name)
    lml, g = m.log_marginal_likelihood_and_grad()
    _check_grad(name, lml, g)
    _check_predict(name, eng, m, skip_rows=(F32.FRAC_TEST_ROW,))
    for refine in (0, 1, 2):
        eng.set_f32_refine(refine)
        mean, var = m.predict_f(Xt)
        assert np.all(mean.numpy()[F32.FRAC_TEST_ROW] == 0.0), f"refine {refine}"
        assert np.all(var.numpy()[F32.FRAC_TEST_ROW] == 0.0), f"refine {refine}"


# ---------------------------------------------------------------- (d): panel widths
PANEL_CASE = "panel600"   # T = 5
PANELS = (1, 2, 3, 5, 9)


def _run_all(name, eng, m):
    """Everything a schedule must not change: value-only LML, LML + gradient, mean, variance, full_cov."""
    Xt = _xt(name)
    lv = float(m.log_marginal_likelihood())
    lg, g = m.log_marginal_likelihood_and_grad()
    mean, var = m.predict_f(Xt)
    mean_c, cov = m.predict_f(Xt, full_cov=True)
    return dict(lv=lv, lg=lg, g=g, mean=mean.numpy(), var=var.numpy(), mean_c=mean_c.numpy(), cov=cov.numpy())


def _assert_bitwise(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("panel", PANELS)
def test_f32_panel_widths(eng, panel):
    """Every panel width at T = 5: W = 1 (a trailing update per column), 2 and 3 (a short last
    panel, and the identity rows' fill starting at columns 0, 2, 4 / 0, 3), 5 and 9 (one panel, no
    trailing update)."""
    n_lf, n_hf = F32.ALL_CASES[PANEL_CASE][:2]
    assert -(-(n_lf + n_hf) // TILE) == 5
    eng.set_f32_panel(panel)
    m = _model(PANEL_CASE)
    lml, g = m.log_marginal_likelihood_and_grad()
    _check_grad(PANEL_CASE, lml, g, tag=f" W={panel}")
    _check_predict(PANEL_CASE, eng, m, tag=f" W={panel}")
    _check_full_cov(PANEL_CASE, m)


def test_f32_panel_5_and_9_bitwise(eng):
    """W = 5 and W = 9 at T = 5 are both one panel of five columns: the same launches on the same
    data, so the same bits.  (Other widths contract the trailing update in other pieces and agree
    only to rounding.)"""
    m = _model(PANEL_CASE)
    res = []
    for panel in (5, 9):
        eng.set_f32_panel(panel)
        res.append(_run_all(PANEL_CASE, eng, m))
    _assert_bitwise(res[0], res[1], "panel 5 vs 9")
    eng.set_f32_panel(2)
    other = _run_all(PANEL_CASE, eng, m)
    # each is within 1e-4 of the oracle (the project's bound), so within 2e-4 of the other
    assert abs(other["lg"] - res[0]["lg"]) <= 2e-4 * abs(res[0]["lg"])


# ---------------------------------------------------------------- (e): lookahead and reserve
SCHED_CASE = "sched700"   # T = 6


def test_f32_lookahead_and_reserve_bitwise(eng):
    """include/mfgp.h on mfgp_set_f32_reserve: "results do not depend on it".  T = 6 with panels of 2:
    after the first panel k2 = 4 < T, so the lookahead sweep forks (the side stream factors panel
    two beside the trailing update of columns 4..5).  reserve = ncu - 1 caps the trailing update at
    upd_slots = 2 workgroups, which walk all its tiles in k32_update's grid-stride loop; reserve 0
    and 32 leave it uncapped at this size.  With the one-stream schedule that is four orders of
    the same kernels on the same data: bitwise-equal results."""
    n_lf, n_hf, p, ns, _ = F32.ALL_CASES[SCHED_CASE]
    T = -(-(n_lf + n_hf) // TILE)
    ncu = torch.cuda.get_device_properties(eng.device).multi_processor_count
    assert T == 6 and 2 + 2 < T and ncu > 33
    # tiles of the forked trailing update (columns 4, 5; A rows below, then the Y^T rows): > 2 slots
    assert (T - 4) + (T - 5) + 2 * -(-p // TILE) > 2
    eng.set_f32_panel(2)
    m = _model(SCHED_CASE)
    runs = {}
    for la, reserve in ((True, 0), (True, 32), (True, ncu - 1), (False, 32)):
        eng.set_f32_lookahead(la)
        eng.set_f32_reserve(reserve)
        runs[(la, reserve)] = _run_all(SCHED_CASE, eng, m)
    base = runs[(False, 32)]
    for key, r in runs.items():
        _assert_bitwise(base, r, f"lookahead {key[0]}, reserve {key[1]} vs one stream")
    _check_grad(SCHED_CASE, base["lg"], base["g"], tag=" W=2")
    mo, vo, co = _pred_ref(SCHED_CASE)
    assert np.max(np.abs(base["mean"] - mo)) / np.max(np.abs(mo)) < 1e-5
    assert np.max(np.abs(base["var"][:, 0] - vo)) < 5e-5
    assert np.max(np.abs(base["cov"][0] - co)) < 1e-4
