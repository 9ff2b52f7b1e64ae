"""The float32 restatement (tests/_f32_oracle.py) against the fp64 oracle, on the CPU, at every case
tests/test_gpu_f32_edges.py uses.

test_gpu_f32_edges.py bounds each gradient component of the fp32 HIP path by 8 c s_q, with
c = max_q |g32_q - g64_q| / s_q the restatement's own distance from the fp64 oracle and s_q the
largest |g64| of q's group (vL, lL, vD, lD, rho0, noise).  That bound only means something while c
is small, so c <= 1e-3 is asserted here, where it can be checked without a GPU.  A case that
violates it (a rho0 derivative that happens to be near zero, say) gets another seed, never a larger
cap."""
import numpy as np
import pytest

import _f32_oracle as F32
from oracle import mfgp_oracle as O


def test_grad_groups_partition_theta():
    g = F32.grad_groups(10)
    assert list(g) == ["vL", "lL", "vD", "lD", "rho0", "noise"]
    assert np.array_equal(np.sort(np.concatenate(list(g.values()))), np.arange(24))
    assert [len(v) for v in g.values()] == [1, 10, 1, 10, 1, 1]


def test_restatement_is_float32_and_not_the_oracle():
    """It must really compute in float32: exact agreement with fp64 would make c = 0 and the GPU
    bound vacuous in the other direction (every kernel would fail it)."""
    ref = F32.case_reference("T1")
    assert 0.0 < F32.restatement_cost(ref["g32"], ref["g64"], 10)
    assert ref["l32"] != ref["l64"]


@pytest.mark.parametrize("name", list(F32.ALL_CASES))
def test_restatement_cost_is_small(name):
    ref = F32.case_reference(name)
    rel = np.abs(ref["g32"] - ref["g64"]) / ref["s"]
    per_group = {k: float(rel[idx].max()) for k, idx in F32.grad_groups(10).items()}
    lerr = abs(ref["l32"] - ref["l64"]) / abs(ref["l64"])
    print(f"{name}: c = {ref['c']:.2e}, LML rel {lerr:.2e}, per group "
          + ", ".join(f"{k} {v:.1e}" for k, v in per_group.items()))
    assert ref["c"] <= 1e-3
    assert lerr <= 1e-4


@pytest.mark.parametrize("name", list(F32.FRAC_SHAPES))
def test_fractional_rows_carry_noise_gradient(name):
    """The fp64 oracle itself: a training row whose fidelity is neither 0 nor 1 has K_jj = s2, and
    its 1/2 W_jj belongs to dLML/dnoise (a large share of it: such a row's K^-1_jj is 1/s2).  Pins
    what the fractional-row GPU test relies on."""
    X, Y, _ = F32.case_data(name)
    n_lf = F32.ALL_CASES[name][0]
    assert X[5, -1] == 0.5 and X[n_lf + 7, -1] == 0.5
    p0 = O.MFParams.initial(10, Y.shape[1])
    K = O.mf_K(X, None, p0)
    assert not K[5].any() and not K[n_lf + 7].any()
    K[np.diag_indices_from(K)] += p0.noise
    Ki = np.linalg.inv(K)
    a = Ki @ Y
    W = a @ a.T - Y.shape[1] * Ki
    rows = [5, n_lf + 7]
    missing = 0.5 * W[rows, rows].sum()
    g_noise = F32.case_reference(name)["g64"][-1]
    print(f"{name}: g_noise {g_noise:.4e}, the two fractional rows' share {missing / g_noise:.3f}")
    # dropping the term must be visible even to the path's loosest criterion, 3e-4 of max |g|
    assert abs(missing) > 100 * 3e-4 * np.max(np.abs(F32.case_reference(name)["g64"]))
