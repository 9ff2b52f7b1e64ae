"""mfgp_gpr_adam_steps with step fusion (the head phase of k_chol_flow finishes the previous step)
against the same number of mfgp_gpr_adam_step calls: bitwise, on theta, u, m, v, step, the loss
history, out and info.  The single-step path is the launch sequence flow, grad, k_reduce_items; the
head phase sums the same items in the same order, so nothing but equality is accepted.

Shapes: the smallest at which each part can go wrong -- n = 65 (T = 3: the diag workgroup forms
every band tile, the last tile has one live row; p = 1, D = 1), n = 97 with p = 33 (two Y column
tiles) and D = 10 (G = 24 items, HF x HF pairs), n = 257 (T = 9: worker-owned A tiles and the row-3
band tiles; the default flow threshold, so no forcing)."""
import threading

import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd.engine import AdamState, Engine, theta_size

pytestmark = pytest.mark.gpu

SHAPES = [(65, 1, 1, 2), (97, 33, 10, 5), (257, 5, 3, 9)]   # n, p, D, HF rows


@pytest.fixture(scope="module")
def eng():
    e = Engine.get()
    e.set_tile(32)
    e.set_tiny(False)                    # n <= 64 would take the one-launch path (none here does)
    e.set_flow(True, any_size=True)      # the flow below its default size threshold too
    e.set_step_fusion(True)
    yield e
    e.set_step_fusion(True)
    e.set_flow(True)
    e.set_tiny(True)


def _data(n, p, D, nhf, seed=0):
    rng = np.random.default_rng(seed + 1000 * n)
    X = np.hstack([rng.random((n, D)), np.zeros((n, 1))])
    X[n - nhf:, -1] = 1.0
    f = np.sin(3.0 * X[:, :D].sum(axis=1, keepdims=True) + np.arange(p)[None, :])
    Y = f * (1.0 + 0.2 * X[:, -1:]) + 0.05 * rng.standard_normal((n, p))
    return X, Y


def _u0(D, seed=0):
    rng = np.random.default_rng(seed)
    u = 0.5413 + 0.3 * rng.standard_normal(theta_size(D))   # softplus(0.5413) = 1
    u[-1] = -4.6                                            # noise ~ 1e-2
    return u


def _run(eng, X, Y, u, nsteps, fused, trainable=None, tie=None, hist_len=None):
    """nsteps Adam steps from u on a workspace of their own: one mfgp_gpr_adam_steps call (fused)
    or nsteps mfgp_gpr_adam_step calls.  Returns every result as host arrays."""
    D = X.shape[1] - 1
    G = theta_size(D)
    dev = eng.device
    Xd = torch.tensor(X, dtype=torch.float64, device=dev)
    Yd = torch.tensor(Y, dtype=torch.float64, device=dev)
    st = AdamState(dev, np.asarray(u, np.float64), np.ones(G) if trainable is None else np.asarray(trainable),
                   np.arange(G) if tie is None else np.asarray(tie), 0.1)
    eng.theta_from_u(st.u, st.theta, G - 1)
    hist = torch.zeros((hist_len or nsteps,), dtype=torch.float64, device=dev)
    out = torch.zeros((1 + G,), dtype=torch.float64, device=dev)
    info = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = eng.private_workspace(eng.gpr_workspace_bytes(X.shape[0], Y.shape[1], D))
    if fused:
        eng.gpr_adam_steps(Xd, Yd, st, hist, out, info, ws=ws, nsteps=nsteps)
    else:
        for _ in range(nsteps):
            eng.gpr_adam_step(Xd, Yd, st, hist, out, info, ws=ws)
    torch.cuda.synchronize()
    return {"theta": st.theta.cpu().numpy(), "u": st.u.cpu().numpy(), "m": st.m.cpu().numpy(),
            "v": st.v.cpu().numpy(), "step": st.step.cpu().numpy(), "hist": hist.cpu().numpy(),
            "out": out.cpu().numpy(), "info": info.cpu().numpy()}


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


_single = {}


def _reference(eng, key, *args, **kw):
    """The single-step trajectory of a case: computed once, shared, never modified."""
    if key not in _single:
        _single[key] = _run(eng, *args, fused=False, **kw)
    return _single[key]


@pytest.mark.parametrize("nsteps", [1, 2, 7])
@pytest.mark.parametrize("n,p,D,nhf", SHAPES)
def test_fused_steps_equal_single_steps(eng, n, p, D, nhf, nsteps):
    X, Y = _data(n, p, D, nhf)
    u = _u0(D)
    ref = _reference(eng, (n, nsteps), X, Y, u, nsteps)
    assert ref["info"][0] == 0 and ref["step"][0] == nsteps and np.isfinite(ref["hist"]).all()
    assert not np.array_equal(ref["u"], u)            # the steps moved theta
    _same(_run(eng, X, Y, u, nsteps, fused=True), ref)


@pytest.mark.parametrize("n,p,D,nhf", SHAPES[1:])
def test_fused_steps_ties_and_fixed_entry(eng, n, p, D, nhf):
    """A tie map that sums two theta entries' gradients, and one entry that is not trainable."""
    X, Y = _data(n, p, D, nhf)
    G = theta_size(D)
    u = _u0(D, seed=1)
    u[2] = u[1]
    tie = np.arange(G)
    tie[2] = tie[1]
    trainable = np.ones(G)
    trainable[G - 1] = 0
    ref = _run(eng, X, Y, u, 3, fused=False, trainable=trainable, tie=tie)
    assert ref["u"][1] == ref["u"][2] and ref["u"][G - 1] == u[G - 1] and ref["step"][0] == 3
    _same(_run(eng, X, Y, u, 3, fused=True, trainable=trainable, tie=tie), ref)


def test_fusion_off_by_setter(eng):
    n, p, D, nhf = SHAPES[1]
    X, Y = _data(n, p, D, nhf)
    u = _u0(D)
    ref = _reference(eng, (n, 7), X, Y, u, 7)
    eng.set_step_fusion(False)
    try:
        assert eng.mode()[4] == 0
        _same(_run(eng, X, Y, u, 7, fused=True), ref)
    finally:
        eng.set_step_fusion(True)
    assert eng.mode()[4] == 1


def test_failed_evaluation_inside_a_call(eng):
    """Every evaluation of the call fails numerically (the inputs of test_gpu_parity's
    CholeskyError test: a variance of 1e300 overflows the trailing updates), so the head phase
    finalizes failed steps: no Adam step, NaN loss, and the same bits as single steps."""
    n, p, D, nhf = SHAPES[2]
    X, Y = _data(n, p, D, nhf)
    u = _u0(D)
    u[0] = 1e300           # softplus(u) = u at this size: vL = 1e300
    ref = _run(eng, X, Y, u, 3, fused=False, hist_len=4)
    got = _run(eng, X, Y, u, 3, fused=True, hist_len=4)
    for r in (ref, got):
        assert r["step"][0] == 0 and r["info"][0] != 0
        np.testing.assert_array_equal(r["u"], u)
        np.testing.assert_array_equal(r["m"], 0.0)
        np.testing.assert_array_equal(r["v"], 0.0)
        assert np.isnan(r["hist"][0]) and r["hist"][3] == 0.0
    _same(got, ref)
    np.testing.assert_array_equal(got["theta"], ref["theta"])


def _session_run(X, Y, D, chunk, steps, env_off, result):
    """One AdamSession of `steps` steps; env_off: on a fresh host thread, whose library handle is
    created with MFGP_STEP_FUSION=0 in the environment."""
    try:
        eng = Engine.get()
        if env_off:
            eng.set_tile(32)
            eng.set_tiny(False)
        result["fusion"] = eng.mode()[4]
        m = M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                                   M.SquaredExponential(lengthscales=np.ones(D)))
        sess = m.adam_session(0.1, steps, graph=True, graph_chunk=chunk)
        sess.run(steps)
        result["raised"] = None
        try:
            sess.finish()
        except M.MFGPError as e:
            result["raised"] = type(e)
        result["hist"] = np.array(m.loss_history)
        result["u"] = m._theta_map().u()
    except BaseException as e:   # handed to the test's thread
        result["error"] = e


def _in_thread_without_fusion(monkeypatch, *args):
    res = {}
    monkeypatch.setenv("MFGP_STEP_FUSION", "0")
    t = threading.Thread(target=_session_run, args=args + (True, res))
    t.start()
    t.join()
    monkeypatch.delenv("MFGP_STEP_FUSION")
    if "error" in res:
        raise res["error"]
    assert res["fusion"] == 0
    return res


def test_replayed_session_equals_unfused_session(eng, monkeypatch):
    """Chunks of 3 captured in a hipGraph through AdamSession: 7 steps are two replays and an
    eager remainder of one; against a session whose handle has MFGP_STEP_FUSION=0."""
    n, p, D, nhf = SHAPES[2]
    X, Y = _data(n, p, D, nhf)
    ref = _in_thread_without_fusion(monkeypatch, X, Y, D, 3, 7)
    got = {}
    _session_run(X, Y, D, 3, 7, False, got)
    if "error" in got:
        raise got["error"]
    assert got["fusion"] == 1 and got["raised"] is None and ref["raised"] is None
    assert len(got["hist"]) == 7 and np.isfinite(got["hist"]).all()
    np.testing.assert_array_equal(got["hist"], ref["hist"])
    np.testing.assert_array_equal(got["u"], ref["u"])


def test_failed_session_raises_as_before(eng):
    """finish() of a fused session whose evaluations fail raises CholeskyError, as single steps do."""
    n, p, D, nhf = SHAPES[2]
    X, Y = _data(n, p, D, nhf)
    m = M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D)),
                               M.SquaredExponential(lengthscales=np.ones(D)))
    m.kernel.kernel_L.variance.assign(1e300)
    sess = m.adam_session(0.1, 3, graph=False)
    sess.run(3)
    with pytest.raises(M.CholeskyError):
        sess.finish()


def test_goku_five_fused_steps(eng, goku):
    """The flagship problem from the benchmark's initial theta, at the library's default settings."""
    eng.set_flow(True)
    try:
        X, Y = goku["X"], goku["Y"]
        D = X.shape[1] - 1
        m = M.MultiFidelityGPModel(X, Y, M.SquaredExponential(lengthscales=np.ones(D), variance=1.0),
                                   M.SquaredExponential(lengthscales=np.ones(D), variance=1.0))
        tm = m._theta_map()
        kw = dict(trainable=np.asarray(tm.trainable()), tie=np.asarray(tm.tie()))
        ref = _run(eng, X, Y, tm.u(), 5, fused=False, **kw)
        assert ref["info"][0] == 0 and ref["step"][0] == 5
        _same(_run(eng, X, Y, tm.u(), 5, fused=True, **kw), ref)
    finally:
        eng.set_flow(True, any_size=True)
