"""Host-side logic of the shared session base (session.py) and of the theta write-back
(params.scatter_entries): no GPU, no stream."""
import numpy as np
import pytest

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd._lib import MFGP_FLOW_TIMEOUT, FlowTimeoutError, MFGPError
from multi_fidelity_gpflow_amd.params import scatter_entries
from multi_fidelity_gpflow_amd.session import (CholeskyError, _Session, _StepRunner, check_outcome,
                                               span_from_tie)


def _span_by_lead(tie):
    """The loop the shared-theta trainer had: a follower adds one to its group's first entry."""
    tie = np.asarray(tie)
    span = np.ones(tie.size, np.uint8)
    for q in range(tie.size):
        lead = int(np.argmax(tie == tie[q]))
        if lead != q:
            span[q] = 0
            span[lead] += 1
    return span


def _span_by_first_seen(tie):
    """The loop the graph-model session had, over keys seen so far."""
    span = np.ones(len(tie), np.uint8)
    first = {}
    for q, key in enumerate(tie):
        if key in first:
            span[q] = 0
            span[first[key]] += 1
        else:
            first[key] = q
    return span


@pytest.mark.parametrize("tie,expected", [
    (np.arange(10), [1] * 10),
    ([0, 1, 1, 1, 2, 3, 3, 3, 4, 5], [1, 3, 0, 0, 1, 3, 0, 0, 1, 1]),
    ([0, 0, 0, 0], [4, 0, 0, 0]),
])
def test_span_from_tie(tie, expected):
    span = span_from_tie(np.asarray(tie, np.int32))
    assert span.dtype == np.uint8
    np.testing.assert_array_equal(span, expected)
    np.testing.assert_array_equal(_span_by_lead(tie), expected)
    np.testing.assert_array_equal(_span_by_first_seen(list(tie)), expected)


# the per-session forms of check_outcome: (prefix, keywords, info word(s) of a clean run)
_FORMS = [("optimize", dict(cause=" (Cholesky or flow hand-off)"), 0),
          ("optimize", {}, 0),
          ("shared-theta optimize", dict(cause=" on some rank"), 0),
          ("SVGP optimize", dict(timeout=False, cause=" (Cholesky of K_uu)", chol="Cholesky of K_uu failed"),
           np.zeros(3, np.int32))]
_HIST = np.array([3.0, 2.0, 1.5, 1.25])


@pytest.mark.parametrize("prefix,kw,zero", _FORMS)
def test_check_outcome(prefix, kw, zero):
    check_outcome(prefix, zero, 4, 4, _HIST, **kw)                      # clean: nothing raised
    check_outcome(prefix, zero, 0, 0, _HIST[:0], **kw)
    with pytest.raises(MFGPError, match=f"^{prefix}: 2 of 4 steps failed.* and were retried") as e:
        check_outcome(prefix, zero, 2, 4, _HIST, **kw)                  # zero word, steps < done, finite
    assert type(e.value) is MFGPError
    with pytest.raises(CholeskyError, match=f"^{prefix}: Cholesky"):
        check_outcome(prefix, zero + 7, 4, 4, _HIST, **kw)              # non-zero word
    nan = _HIST.copy()
    nan[2] = np.nan
    with pytest.raises(CholeskyError, match=f"^{prefix}: Cholesky"):
        check_outcome(prefix, zero, 2, 4, nan, **kw)                    # NaN in the history, zero word
    if kw.get("timeout", True):
        with pytest.raises(FlowTimeoutError, match=f"^{prefix}"):
            check_outcome(prefix, MFGP_FLOW_TIMEOUT, 2, 4, nan, **kw)
    else:                                                               # SVGP: no timeout word
        with pytest.raises(CholeskyError):
            check_outcome(prefix, zero + MFGP_FLOW_TIMEOUT, 2, 4, nan, **kw)


def test_check_outcome_names_iteration_and_truncates_history():
    """The AdamSession form: the model's loss_history is cut after the first bad entry."""
    nan = _HIST.copy()
    nan[2] = np.nan
    hist = list(nan)
    with pytest.raises(CholeskyError, match="^optimize: Cholesky failed at iteration 2$"):
        check_outcome("optimize", 5, 2, 4, nan, history=hist)
    assert len(hist) == 3
    hist = list(_HIST)
    with pytest.raises(FlowTimeoutError, match=r"^optimize \(by iteration 3\)"):
        check_outcome("optimize", MFGP_FLOW_TIMEOUT, 3, 4, _HIST, history=hist)
    assert len(hist) == 4
    with pytest.raises(MFGPError, match="1 of 4 steps failed"):
        check_outcome("optimize", 0, 3, 4, _HIST, history=hist)
    assert len(hist) == 4


class _Counter:
    def __init__(self):
        self.calls = 0

    def step(self):
        self.calls += 1


@pytest.mark.parametrize("n", [0, 1, 3, 4, 7])
def test_step_runner_eager_calls_step_n_times(n):
    c = _Counter()
    r = _StepRunner(c.step, 0)
    r.run(n)
    r.prepare(n)   # chunk 0: nothing to capture
    assert c.calls == n and r.graphs == {}


def test_step_runner_holds_its_session_weakly():
    c = _Counter()
    r = _StepRunner(c.step, 0)
    del c
    with pytest.raises(MFGPError, match="released"):
        r.step()


class _HostSession(_Session):
    def __init__(self, max_iters, warm=True):
        self.calls = 0
        self.counted = []
        super().__init__(None, max_iters, 0, warm=warm)

    def _step(self):
        self.calls += 1

    def _count(self, n):
        super()._count(n)
        self.counted.append(self.done)


def test_session_without_stream():
    s = _HostSession(5)
    assert s.stream is None
    s.run(0)
    assert (s.calls, s.done, s.counted) == (0, 0, [])
    s.run(2)
    s.prepare(3)
    s.sync()
    assert (s.calls, s.done) == (2, 2)
    with pytest.raises(ValueError, match="^_HostSession: more iterations than max_iters$"):
        s.run(4)
    assert (s.calls, s.done) == (2, 2)
    with s as t:
        t.run(3)
    assert (s.calls, s.done) == (5, 5)
    assert _HostSession(0).max_iters == 1


def test_session_eager_first_step_is_counted_once():
    s = _HostSession(6, warm=False)
    s.prepare(3)                      # nothing before the eager first step
    s.run(3)
    assert (s.calls, s.done, s.counted) == (3, 3, [1, 3])
    s.run(3)
    assert (s.calls, s.done, s.counted) == (6, 6, [1, 3, 6])


def test_scatter_entries_scalar_shared_and_indexed():
    """One assignment per Parameter: a scalar owned by d entries is filled with its last entry's
    value; an indexed entry changes its element only."""
    iso = M.Parameter(1.0, transform=M.positive())                 # isotropic lengthscale, d = 3 entries
    ard = M.Parameter(np.ones(3), transform=M.positive())
    rho = M.Parameter(np.ones((2, 1)))                             # only rho[0, 0] is in theta
    rho_u1 = float(rho.unconstrained_variable[1, 0])
    entries = [(iso, None)] * 3 + [(ard, (i,)) for i in range(3)] + [(rho, (0, 0))]
    scatter_entries(entries, np.array([0.5, 0.5, 0.25, -1.0, -2.0, -3.0, 7.0]))
    assert iso.unconstrained_variable.shape == ()
    np.testing.assert_array_equal(iso.unconstrained_variable, 0.25)
    np.testing.assert_array_equal(ard.unconstrained_variable, [-1.0, -2.0, -3.0])
    np.testing.assert_array_equal(rho.unconstrained_variable, [[7.0], [rho_u1]])


def test_theta_map_set_u_round_trip():
    rng = np.random.default_rng(0)
    X = np.hstack([rng.random((8, 3)), np.r_[np.zeros(5), np.ones(3)][:, None]])
    m = M.MultiFidelityGPModel(X, rng.standard_normal((8, 2)), M.SquaredExponential(lengthscales=1.0),
                               M.SquaredExponential(lengthscales=np.ones(3)))
    tm = m._theta_map()
    rho_u1 = float(m.kernel.rho.unconstrained_variable[1, 0])        # not in theta: left as it is
    np.testing.assert_array_equal(tm.tie(), [0, 1, 1, 1, 2, 3, 4, 5, 6, 7])
    u = np.array([0.1, 0.2, 0.2, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
    tm.set_u(u)
    np.testing.assert_array_equal(tm.u(), u)
    np.testing.assert_array_equal(m.kernel.kernel_L.lengthscales.unconstrained_variable, 0.2)
    np.testing.assert_array_equal(m.kernel.kernel_delta.lengthscales.unconstrained_variable, [0.4, 0.5, 0.6])
    np.testing.assert_array_equal(m.kernel.rho.unconstrained_variable, [[0.7], [rho_u1]])
