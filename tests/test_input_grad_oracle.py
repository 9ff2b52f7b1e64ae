"""The references of tests/test_gpu_posterior_grad.py, checked on the CPU (no GPU needed).

tests/_input_grad_oracle.py computes the VJP of predict_f w.r.t. Xnew in two independent ways (autograd
through Cholesky + triangular solves; autograd through linalg.solve / the explicit inverse factor).
For every case the GPU tests use:

  * the two agree to a tenth of the GPU bound (1e-10 max(1, |ref|max); Goku 1e-9 |ref|max), so a GPU
    result within the bound of one is not an artefact of the reference's own solves;
  * the fidelity column's gradient is exactly 0 (the kernel reads it through == tests only);
  * a few components agree with central differences (h = 1e-5) to 1e-6 |ref|max: the truncation term
    h^2 |f'''| / 6 with lengthscales >= 0.5 stays below ~1e-8, the rounding term eps |loss| / h below
    ~1e-8 -- far from 1e-6, while a missing or mis-signed term of the VJP is of order |ref|max.

Measured (spread / |gX|max): GPR synthetic 1.8e-15 / 1.8, 5.9e-13 / 9.7, 2.8e-14 / 14.9; HBS 8.0e-14 / 14.7;
Goku 1.3e-11 / 27.1; SVGP L = 11 4.5e-14 / 2.1.  A case that fails the spread condition gets other
inputs, never another bound."""
import numpy as np
import pytest

import _input_grad_oracle as G


def _check(name, ref, other, fn, Xs, gm, gv, bound):
    gX = ref[2]
    scale = np.abs(gX).max()
    spread = np.abs(gX - other[2]).max()
    print(f"{name}: spread {spread:.1e}, |gX|max {scale:.1e}, bound / 10 = {0.1 * bound:.1e}")
    assert gX.shape == Xs.shape
    assert spread <= 0.1 * bound, (name, spread)
    assert np.all(gX[:, -1] == 0.0) and np.all(other[2][:, -1] == 0.0)
    # mean / var of the two forms: the forward the GPU tests compare with predict_f's own bound
    assert np.abs(ref[0] - other[0]).max() <= 1e-10 * max(1.0, np.abs(ref[0]).max())
    assert np.abs(ref[1] - other[1]).max() <= 1e-10
    rng = np.random.default_rng(5)
    ns, D = Xs.shape[0], Xs.shape[1] - 1
    comps = [(int(rng.integers(ns)), int(rng.integers(D))) for _ in range(3)]
    fd = G.central_difference(fn, Xs, gm, gv, comps)
    for (s, k), v in zip(comps, fd):
        assert abs(v - gX[s, k]) <= 1e-6 * scale, (name, s, k, v, gX[s, k])


@pytest.mark.parametrize("case", G.GPR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpr_synthetic_references_agree(case):
    X, Y, Xs, prm, gm, gv, ref = G.gpr_synthetic(*case)
    other = G.gpr_vjp(X, Y, Xs, prm, gm, gv, form="solve")
    bound = G.BOUND * max(1.0, np.abs(ref[2]).max())
    _check(f"gpr {case}", ref, other, G.gpr_loss_fn(X, Y, prm, "chol"), Xs, gm, gv, bound)


@pytest.mark.parametrize("which", ["hbs", "goku"])
def test_gpr_dataset_references_agree(which):
    X, Y, Xs, prm, gm, gv, ref = G.gpr_dataset(which)
    other = G.gpr_vjp(X, Y, Xs, prm, gm, gv, form="solve")
    amax = np.abs(ref[2]).max()
    bound = G.GOKU_BOUND * amax if which == "goku" else G.BOUND * max(1.0, amax)
    _check(which, ref, other, G.gpr_loss_fn(X, Y, prm, "chol"), Xs, gm, gv, bound)


def test_gpr_partial_upstreams_agree():
    """grad_var alone and grad_mean alone (the argument forms of the GPU tests) on the three-tile case."""
    X, Y, Xs, prm, gm, gv, _ = G.gpr_synthetic(*G.GPR_CASES[1])
    for a, b in ((None, gv), (gm, None)):
        ref = G.gpr_vjp(X, Y, Xs, prm, a, b)
        other = G.gpr_vjp(X, Y, Xs, prm, a, b, form="solve")
        assert np.abs(ref[2] - other[2]).max() <= 0.1 * G.BOUND * max(1.0, np.abs(ref[2]).max())
        assert np.abs(ref[2]).max() > 1e-3 and np.all(ref[2][:, -1] == 0.0)


def test_svgp_synthetic_references_agree():
    state, Xs, gm, gv, ref = G.svgp_synthetic()
    assert len(state[1]) == 11 and state[0].shape[0] == 70 and state[4].shape == (17, 11)
    other = G.svgp_vjp(state, Xs, gm, gv, form="solve")
    bound = G.BOUND * max(1.0, np.abs(ref[2]).max())
    _check("svgp L=11", ref, other, G.svgp_loss_fn(*state, "chol"), Xs, gm, gv, bound)


@pytest.mark.parametrize("which", ["singlebin", "latent"])
def test_svgp_hbs_references_agree(which):
    m, Wm, Xs = G.svgp_hbs_model(which)
    state = G.svgp_state(m, Wm)
    gm, gv = G.upstream(Xs.shape[0], m.num_outputs, 90)
    ref = G.svgp_vjp(state, Xs, gm, gv)
    other = G.svgp_vjp(state, Xs, gm, gv, form="solve")
    bound = G.BOUND * max(1.0, np.abs(ref[2]).max())
    _check(f"svgp hbs {which}", ref, other, G.svgp_loss_fn(*state, "chol"), Xs, gm, gv, bound)
