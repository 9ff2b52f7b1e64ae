"""The graph model's kernel paths that test_gpu_graph.py's one shape family (n = 82, D = 3, m <= 3,
tile 32, sorted rows: the launch-per-step Cholesky, three tiles) never reaches:

  * k_chol_flow fed by an external Gram (FlowArgs::gram == 0: the graph model is its only user) at
    T = 3 (any_size), 8, 10, 26 and 37 tiles, against the step schedule and the oracle;
  * k_grad<64, true>, the chunked m-loop and the task-order table under the graph epilogue;
  * m = 4 (MFGP_MAX_LF), D = 1, 6, 10, 13 / 14 (either side of 64 KB of k_grad LDS) and 32
    (G = 186: the LDS maximum, finalize_body's staging, the posterior's theta staging, k_reduce_items'
    grid), rows not sorted by source (the per-element source branching of the epilogue and of
    graph_entry);
  * the parity pin: at m = 1 the graph kernel is the linear kernel + 1e-6 I, so HBS and Goku are
    compared with oracle/mfgp_oracle.py (pinned by the reference's recorded values) at noise
    1e-3 + 1e-6, not with graph_oracle;
  * dK/dv_s where a variance is 0 (finite, the autodiff of v * exp(-r2/2)).

Every other case is compared with oracle/graph_oracle.py (autograd), computed once per case.
Bounds, the project's own, unchanged: K entries 1e-13 abs; K_diag 1e-14; LML 1e-11 rel; gradient
1e-8 of the largest component; predict 1e-9; Adam losses 1e-9 rel; flow against step as
test_flow_matches_step_schedule (LML 1e-11 rel, gradient 1e-9 of the largest component).  The
oracle's own rounding spread under a row permutation of these cases is <= 9e-13 (LML) and <= 3e-12
(gradient), so the bounds hold for the reference alone with a 10x margin.

Inputs: test_gpu_graph's recipe with the weights scaled by 1 / sqrt(D) and the lengthscales by
sqrt(D / 3) (0.3 at D = 1), LF sources sharing one kernel, rho_LF in 0.2-0.5.  With shuffled rows
the factorization's lower triangle reads both rho_LF[i][j] and rho_LF[j][i], so rho_LF must be
symmetric there for K to be a covariance; the asymmetric block stays on sorted rows."""
import functools

import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd.engine import Engine
from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O
from test_gpu_graph import _data as _graph_data, _model, _oracle_params

pytestmark = pytest.mark.gpu

NOISE = 1e-3


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    try:
        yield e
    finally:
        e.set_tile(32)
        e.set_flow(True)
        e.set_tiny(True)


def _data(m, D, P, sizes, shuffle, seed=3):
    """test_gpu_graph._data with weights / sqrt(D) and, with `shuffle`, the rows permuted."""
    rng = np.random.default_rng(seed)
    Xs, Ys = [], []
    w = rng.standard_normal((D, P)) / np.sqrt(D)
    for s, n in enumerate(sizes[:m + 1]):
        x = rng.uniform(0, 1, (n, D))
        y = np.sin(3 * x @ w) * (1 + 0.3 * s) + 0.05 * rng.standard_normal((n, P))
        Xs.append(np.hstack([x, np.full((n, 1), float(s))]))
        Ys.append(y)
    X, Y = np.vstack(Xs), np.vstack(Ys)
    if shuffle:
        perm = np.random.default_rng(seed + 100).permutation(len(X))
        X, Y = X[perm], Y[perm]
    return X, Y


def _scaled_model(X, Y, m, D, symmetric, seed=5):
    """test_gpu_graph._model (shared LF kernels, rho_LF in 0.2-0.5) with every lengthscale scaled by
    sqrt(D / 3) (0.3 at D = 1); `symmetric` makes rho_LF symmetric (shuffled rows)."""
    mod = _model(X, Y, m, D, asym=True, seed=seed)
    scale = 0.3 if D == 1 else np.sqrt(D / 3.0)
    for k in mod.kernel.kernel_Ls + [mod.kernel.kernel_delta]:
        k.lengthscales.assign(k.lengthscales.numpy() * scale)
    if symmetric:
        r = mod.kernel.rho_LF.numpy()
        mod.kernel.rho_LF.assign(0.5 * (r + r.T))
    return mod


def _graph_oracle_lml_grad(X, Y, prm, noise=NOISE):
    """graph_oracle LML and its autograd gradient in the theta layout of include/mfgp.h."""
    m = prm["rho"].shape[0]
    prm = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    nz = torch.tensor(noise, dtype=torch.float64, requires_grad=True)
    lo = GO.lml(torch.tensor(X), torch.tensor(Y), prm, nz)
    lo.backward()
    grl = prm["rhoLF"].grad.numpy().ravel() if prm["rhoLF"].grad is not None else np.zeros(m * m)
    go = np.concatenate([np.concatenate([[prm["v"].grad[s]], prm["l"].grad[s].numpy()]) for s in range(m + 1)]
                        + [prm["rho"].grad.numpy(), grl, [nz.grad]])
    return float(lo.detach()), go


# case -> (m, D, P, sizes, shuffled); H is test_gpu_graph's own data and model
CASES = {
    "C": (2, 10, 5, (150, 100, 50), True),
    "D": (3, 6, 4, (400, 250, 120, 62), True),
    "E13": (4, 13, 2, (70, 60, 50, 40, 36), True),
    "E14": (4, 14, 2, (70, 60, 50, 40, 36), True),
    "F": (4, 32, 3, (90, 70, 60, 50, 30), True),
    "G": (3, 1, 2, (100, 90, 70, 40), False),
    "H": (2, 3, 4, (40, 30, 12), False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's model and its oracle LML / gradient (computed once, shared by every leg)."""
    m, D, P, sizes, shuffled = CASES[name]
    if name == "H":
        X, Y = _graph_data(m, D)
        mod = _model(X, Y, m, D, asym=True)
    else:
        X, Y = _data(m, D, P, sizes, shuffled)
        mod = _scaled_model(X, Y, m, D, symmetric=shuffled)
    assert X.shape == (sum(sizes), D + 1) and Y.shape[1] == P
    lo, go = _graph_oracle_lml_grad(X, Y, _oracle_params(mod, D))
    assert go.shape == ((m + 1) * (D + 1) + m + m * m + 1,)
    return mod, X, Y, lo, go


def _linear_params(D, P, seed):
    rng = np.random.default_rng(seed)
    return O.MFParams(0.8 + 0.7 * rng.random(), 0.6 + 1.4 * rng.random(D), 0.2 + 0.6 * rng.random(),
                      0.5 + 1.2 * rng.random(D), np.full((P, 1), 0.7 + 0.6 * rng.random()), NOISE + GO.JITTER)


@functools.lru_cache(maxsize=None)
def _pin_case(which):
    """HBS / Goku as a one-source graph model, and the linear oracle's LML, gradient (mapped into the
    graph theta layout, rho_LF[0][0] at 0) and predictions at noise 1e-3 + 1e-6."""
    from conftest import GOKU_DIR, HBS_DIR
    d = O.load_powerspecs(HBS_DIR if which == "A" else GOKU_DIR)
    X, Y, Xs = d["X"], d["Y"], d["Xtest"][:10]
    D, P = X.shape[1] - 1, Y.shape[1]
    p = _linear_params(D, P, seed=13)
    mod = M.GraphMultiFidelityGPModel(X, Y, [M.SquaredExponential(lengthscales=p.lL.copy(), variance=p.vL)],
                                      M.SquaredExponential(lengthscales=p.lD.copy(), variance=p.vD))
    mod.kernel.rho.assign(np.full((1, P), p.rho0))
    mod.kernel.rho_LF.assign(np.array([[0.37]]))
    lo, g = O.gpr_lml_and_grad(X, Y, p)
    go = np.concatenate([[g["vL"]], g["lL"], [g["vD"]], g["lD"], [g["rho0"]], [0.0], [g["noise"]]])
    mo, vo = O.gpr_predict_f(X, Y, Xs, p)
    return mod, X, Y, lo, go, Xs, mo, vo[:, 0]


def _set_schedule(eng, nb, sched, n):
    """Tile and Cholesky schedule of a leg; a flow leg must really take the flow."""
    eng.set_tile(nb)
    eng.set_tiny(True)
    eng.set_flow(sched != "step", any_size=(sched == "any"))
    if sched in ("flow", "any"):
        assert eng.flow_runs(n), "the leg would pass on the step path"
    elif sched == "step":
        assert not eng.flow_runs(n)


_results = {}


def _evaluate(eng, name, nb, sched):
    """(LML, gradient) of a leg on the device, kept for the flow-against-step comparison."""
    key = (name, nb, sched)
    if key not in _results:
        mod, X = (_pin_case(name) if name in ("A", "B") else _case(name))[:2]
        _set_schedule(eng, nb, sched, X.shape[0])
        try:
            _results[key] = mod.log_marginal_likelihood_and_grad()   # raises on info != 0
        finally:
            eng.set_tile(32)
            eng.set_flow(True)
    return _results[key]


def _check_lml_grad(tag, got, lo, go):
    lml, g = got
    e_l, e_g = abs(lml - lo) / abs(lo), np.abs(g - go).max() / np.abs(go).max()
    print(f"{tag}: lml {e_l:.1e} grad {e_g:.1e}")
    assert np.isfinite(g).all()
    assert e_l < 1e-11, (tag, e_l)
    assert g.shape == go.shape and e_g <= 1e-8, (tag, e_g)


def _check_predict(tag, got, mo, vo):
    mean, var = got[0].numpy(), got[1].numpy()
    assert mean.shape == mo.shape and var.shape == mean.shape
    e_m, e_v = np.abs(mean - mo).max(), np.abs(var - vo[:, None]).max()
    print(f"{tag}: mean {e_m:.1e} var {e_v:.1e}")
    assert e_m <= 1e-9 * max(1.0, np.abs(mo).max()), (tag, e_m)
    assert e_v <= 1e-9, (tag, e_v)


LEGS = [("H", 32, "any"),
        ("C", 32, "flow"), ("C", 32, "step"),
        ("D", 32, "default"), ("D", 64, "default"),
        ("E13", 32, "flow"), ("E14", 32, "flow"),
        ("F", 32, "default"), ("F", 64, "default"),
        ("G", 32, "flow"), ("G", 32, "step")]


@pytest.mark.parametrize("name,nb,sched", LEGS, ids=[f"{c}-nb{nb}-{s}" for c, nb, s in LEGS])
def test_graph_lml_and_grad_paths(name, nb, sched, eng):
    """LML and every gradient entry (rho_LF included) against graph_oracle.  `default` is the
    library's own choice: the flow at tile 32 (n >= 225 here), the step launches at tile 64."""
    mod, X, Y, lo, go = _case(name)
    if sched == "default" and nb == 32:
        sched = "flow"
    _check_lml_grad(f"{name} nb{nb} {sched}", _evaluate(eng, name, nb, sched), lo, go)


PIN_LEGS = [("A", 32, "step"), ("A", 64, "step"), ("B", 32, "flow"), ("B", 32, "step")]


@pytest.mark.parametrize("name,nb,sched", PIN_LEGS, ids=[f"{c}-nb{nb}-{s}" for c, nb, s in PIN_LEGS])
def test_graph_one_source_is_the_linear_model(name, nb, sched, eng):
    """The parity pin (A: HBS, B: Goku): LML, the 2D + 4 mapped gradient entries, an exactly zero
    rho_LF[0][0] entry and predict_f on 10 test points against oracle/mfgp_oracle.py at noise
    1e-3 + 1e-6; B also through the cached posterior()."""
    mod, X, Y, lo, go, Xs, mo, vo = _pin_case(name)
    D = X.shape[1] - 1
    got = _evaluate(eng, name, nb, sched)
    _check_lml_grad(f"{name} nb{nb} {sched}", got, lo, go)
    assert got[1][2 * D + 3] == 0.0   # rho_LF[0][0]: no entry of K reads it
    _set_schedule(eng, nb, sched, X.shape[0])
    try:
        _check_predict(f"{name} nb{nb} predict_f", mod.predict_f(Xs), mo, vo)
        if name == "B":
            _check_predict(f"{name} nb{nb} posterior", mod.posterior().predict_f(Xs), mo, vo)
    finally:
        eng.set_tile(32)
        eng.set_flow(True)


@pytest.mark.parametrize("name", ["B", "C", "G"])
def test_graph_flow_matches_step(name, eng):
    """The flow on an external Gram and the step launches: the same LML and gradient, to the bounds
    of test_flow_matches_step_schedule."""
    (lf, gf), (ls, gs) = _evaluate(eng, name, 32, "flow"), _evaluate(eng, name, 32, "step")
    e_l, e_g = abs(lf - ls) / abs(ls), np.abs(gf - gs).max() / np.abs(gs).max()
    print(f"{name} flow vs step: lml {e_l:.1e} grad {e_g:.1e}")
    assert e_l < 1e-11
    assert e_g <= 1e-9


@pytest.mark.parametrize("nb", [32, 64])
def test_graph_gram_rectangular_and_foreign_flags(nb, eng):
    """eng.gmf_gram on a rectangle (70 x 45: partial tiles on both sides at either tile size) with
    shuffled rows, m = 3, D = 6, and rows whose fidelity flag is no source (2.5, -1, 7): zero rows /
    columns of K and zero K_diag, as the reference's exact masks give."""
    m, D = 3, 6
    X1, Y1 = _data(m, D, 2, (25, 20, 15, 10), True, seed=7)
    X2, _ = _data(m, D, 2, (15, 12, 10, 8), True, seed=8)
    assert X1.shape[0] == 70 and X2.shape[0] == 45
    X1[[4, 33, 69], -1] = [2.5, -1.0, 7.0]
    X2[[0, 31, 44], -1] = [7.0, 2.5, -1.0]
    mod = _scaled_model(X1, Y1, m, D, symmetric=False)
    prm = _oracle_params(mod, D)
    th = torch.tensor(mod.kernel.theta_vector(D), dtype=torch.float64, device=eng.device)
    d1, d2 = torch.tensor(X1, device=eng.device), torch.tensor(X2, device=eng.device)
    eng.set_tile(nb)
    try:
        K = eng.gmf_gram(m, d1, d2, th, diag_add=0.0).cpu().numpy()
        kd = eng.gmf_kdiag(m, d1, th).cpu().numpy()
    finally:
        eng.set_tile(32)
    Ko = GO.graph_K(torch.tensor(X1), torch.tensor(X2), prm, jitter=False).numpy()
    kdo = GO.graph_Kdiag(torch.tensor(X1), prm).numpy()
    print(f"gmf_gram nb{nb}: K {np.abs(K - Ko).max():.1e} K_diag {np.abs(kd - kdo).max():.1e}")
    np.testing.assert_allclose(K, Ko, rtol=0, atol=1e-13)
    np.testing.assert_allclose(kd, kdo, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(K[[4, 33, 69]], 0.0)
    np.testing.assert_array_equal(K[:, [0, 31, 44]], 0.0)
    np.testing.assert_array_equal(kd[[4, 33, 69]], 0.0)
    assert np.abs(K).max() > 0.1


@pytest.mark.parametrize("nb", [32, 64])
def test_graph_predict_at_largest_theta(nb, eng):
    """Case F (G = 186 of the posterior's 192 staged theta entries): predict_f and the cached
    posterior on 9 points with mixed flags."""
    mod, X, Y, _, _ = _case("F")
    m, D = CASES["F"][:2]
    rng = np.random.default_rng(21)
    Xs = np.hstack([rng.uniform(0, 1, (9, D)), (np.arange(9)[:, None] % (m + 1)) * 1.0])
    mo, vo = GO.predict_f(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), _oracle_params(mod, D),
                          torch.tensor(NOISE, dtype=torch.float64))
    eng.set_tile(nb)
    try:
        _check_predict(f"F nb{nb} predict_f", mod.predict_f(Xs), mo.numpy(), vo.numpy())
        _check_predict(f"F nb{nb} posterior", mod.posterior().predict_f(Xs), mo.numpy(), vo.numpy())
    finally:
        eng.set_tile(32)


def test_graph_adam_at_largest_theta(eng):
    """Five Adam steps at G = 186 (_PackedAdam, k_reduce_items' 2 + G workgroups, the flow inside the
    captured step) against GraphTrainer; sorted rows, so the asymmetric rho_LF trains entry by entry."""
    m, D, P, sizes, _ = CASES["F"]
    X, Y = _data(m, D, P, sizes, False)
    mod = _scaled_model(X, Y, m, D, symmetric=False)
    k = mod.kernel
    ks = k.kernel_Ls + [k.kernel_delta]
    init = dict(v=[float(kk.variance.numpy()) for kk in ks], l=np.stack([kk.lengthscales.numpy() for kk in ks]),
                rho=k.rho.numpy(), rhoLF=k.rho_LF.numpy())
    tr = GO.GraphTrainer(X, Y, m, D, lr=0.01, init=init)
    ref = [tr.step() for _ in range(5)]
    eng.set_tile(32)
    eng.set_flow(True)
    assert eng.flow_runs(X.shape[0])
    mod.optimize(max_iters=5, learning_rate=0.01, use_adam=True, graph=True, graph_chunk=5)
    err = np.abs(np.array(mod.loss_history) / np.array(ref) - 1.0).max()
    print(f"F adam: losses {err:.1e}")
    np.testing.assert_allclose(mod.loss_history, ref, rtol=1e-9)
    off = ~np.eye(m, dtype=bool)
    np.testing.assert_allclose(k.rho_LF.numpy()[off], tr.params()["rhoLF"].detach().numpy()[off], rtol=1e-8)


@pytest.mark.parametrize("zero", ["delta", "lf0"])
def test_graph_grad_finite_at_zero_variance(zero, eng):
    """dK/dv_s = exp(-r2/2), the autodiff of v * exp(-r2/2): finite and equal to the oracle's where
    v_s = 0 (the form (sum w coef k_s) / v_s was 0/0 there, a point L-BFGS line searches reach).
    Case C's data, theta passed straight to gmf_lml.  With v_0 = 0 source 0 decouples from the
    others only if its rho_LF entries vanish too (K is no covariance otherwise, and the oracle's own
    Cholesky fails), so they are set to 0."""
    mod, X, Y, _, _ = _case("C")
    m, D = CASES["C"][:2]
    th = mod.kernel.theta_vector(D, noise=NOISE)
    prm = _oracle_params(mod, D)
    if zero == "delta":
        th[m * (1 + D)] = 0.0
        prm["v"][m] = 0.0
    else:
        th[0] = 0.0
        prm["v"][0] = 0.0
        ro = (m + 1) * (1 + D) + m
        th[ro:ro + m * m] = 0.0
        prm["rhoLF"][:] = 0.0
    lo, go = _graph_oracle_lml_grad(X, Y, prm)
    assert np.isfinite(go).all()
    eng.set_tile(32)
    eng.set_flow(True)
    out, info = eng.gmf_lml(m, torch.tensor(X, device=eng.device), torch.tensor(Y, device=eng.device),
                            torch.tensor(th, dtype=torch.float64, device=eng.device), want_grad=True)
    assert int(info.item()) == 0
    o = out.cpu().numpy()
    _check_lml_grad(f"C v_{zero} = 0", (float(o[0]), o[1:]), lo, go)
