"""The extended-precision gradient restatement (tests/_grad_oracle.py) against the fp64 oracles, on
the CPU, at every case tests/test_gpu_grad_components.py and tests/_grad_chunk_worker.py use.

The GPU tests bound each component q of the HIP gradient by 8 c S_q, with S_q = 1/2 sum_ab
|W_ab dK_ab/dtheta_q| the component's absolute mass and c what the fp64 oracle itself costs on that
scale (floored at n 2^-53).  Checked here, where no GPU is needed:

  * the restatement is the oracle's algebra: every component within 1e-9 S_q of it;
  * c <= 1e-11.  A condition on the cases, not a measurement: it keeps the GPU bound at least two
    orders below the older one.  A case beyond it gets fewer rows or a larger noise, never a larger
    cap.  (Measured here: 7.1e-15, the floor, to 1.2e-12; for the linear kernel c is the larger of
    the oracle's unit and the tile-order restatement's, _grad_oracle.gpr_grad_blocked64.)
  * the older bound, 1e-8 of the largest component, is at least 100 times 8 c S_q in some component
    of every case (measured: 3e4 to 4e9 times);
  * the bound can fail: one H-H pair's delta term and one L-H pair's rho term taken out of the fp64
    sums violate it."""
import numpy as np
import pytest

import _grad_oracle as GR
from oracle import mfgp_oracle as O


@pytest.fixture(autouse=True)
def _wide():
    GR.require_wide()


ALL = list(GR.LINEAR_SHAPES) + list(GR.GRAPH_SHAPES)


def _ref(name):
    return (GR.graph_reference if name in GR.GRAPH_SHAPES else GR.case_reference)(name)


def test_every_gpu_case_is_checked_here():
    used = set(GR.NB32_CASES) | set(GR.NB64_CASES) | set(GR.TINY_CASES) | {c for c, _ in GR.CHUNK_CASES}
    assert used == set(GR.LINEAR_SHAPES)
    assert GR.backend().wide and np.finfo(np.float64).eps > 2.0 ** -60   # the reference is not float64


@pytest.mark.parametrize("name", ALL)
def test_restatement_is_the_oracle_and_fp64_is_cheap(name):
    ref = _ref(name)
    groups = GR.case_groups(name)
    n = (GR.graph_data if name in GR.GRAPH_SHAPES else GR.case_data)(name)[0].shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mass = np.where(ref["g_ref"] != 0, ref["S"] / np.abs(ref["g_ref"]), 1.0)
    old = 1e-8 * np.abs(ref["g64"]).max()
    new = GR.FACTOR * ref["c"] * ref["S"]
    gain = np.where(new > 0, old / np.where(new > 0, new, 1.0), 0.0)
    units = "" if name in GR.GRAPH_SHAPES else (f"; oracle {ref['c_oracle']:.1e}, tile order "
                                                + ", ".join(f"nb{nb} {v:.1e}" for nb, v in ref["c_blocked"].items()))
    print(f"{name}: n {n}, c = {ref['c']:.2e} (floor {n * 2.0 ** -53:.1e}{units}), LML rel "
          f"{abs(ref['l64'] - ref['l_ref']) / abs(ref['l_ref']):.1e}; S_q / |g_q| per group "
          + ", ".join(f"{k} {mass[idx].max():.1e}" for k, idx in groups.items())
          + f"; old bound / new bound up to {gain.max():.1e}")
    assert ref["g_ref"].shape == ref["g64"].shape == ref["S"].shape == (sum(len(i) for i in groups.values()),)
    assert np.all(ref["S"] >= np.abs(ref["g_ref"]) * (1 - 1e-12))   # |sum| <= sum | |
    assert np.all(np.abs(ref["g64"] - ref["g_ref"]) <= 1e-9 * ref["S"])
    assert abs(ref["l64"] - ref["l_ref"]) <= 1e-11 * abs(ref["l_ref"])
    assert ref["c"] <= 1e-11
    assert ref["c"] == GR.case_unit(name) >= n * 2.0 ** -53
    assert gain.max() >= 100.0


def test_case_table_hits_what_it_claims():
    """The shapes' tile counts and the fidelity layout of `mixed`."""
    n = lambda name: sum(GR.LINEAR_SHAPES[name][:2])
    assert (n("t1"), n("full64"), n("onerow"), n("d32"), n("d32_64"), n("chunk64")) == (20, 64, 65, 97, 129, 160)
    assert -(-n("mixed") // 32) == 5 and -(-GR.LINEAR_SHAPES["mixed"][2] // 32) == 2   # T = 5, Tp = 2
    assert -(-n("chunk64") // 64) == 3 and -(-n("t6") // 32) == 6
    # k_grad's m-chunks: tasks past chunk 0 (no alpha rows) with 1, 2 and 3 items need T = 6; T = 5
    # has them with 1 and 2, and chunks 24 and 2048 are one chunk per row at these T
    later = lambda T, Tp: {nq for c in (1, 2, 3) for ch, nq in GR.chunk_task_items(T, Tp, c) if ch >= 1}
    assert later(5, 2) == {1, 2} and later(6, 1) == {1, 2, 3} and later(3, 1) == {1}
    for T, Tp in ((5, 2), (6, 1), (3, 1)):
        assert GR.chunk_task_items(T, Tp, 24) == GR.chunk_task_items(T, Tp, 2048)
        assert all(ch == 0 for ch, _ in GR.chunk_task_items(T, Tp, 24))
        assert 24 + T + Tp < 2048 <= 2048 + T + Tp   # the task-order table is built / left out
    X = GR.case_data("mixed")[0]
    f = X[:, -1]
    assert f[GR.MIXED_FRAC_ROW] == 0.5 and GR.MIXED_FRAC_ROW < 32
    assert f[GR.MIXED_NEAR_ONE_ROW] == 0.9999999999999999 != 1.0 and 96 <= GR.MIXED_NEAR_ONE_ROW < 128
    for nb in (32, 64):   # every tile pair holds L-L, L-H and H-H pairs
        for t in range(-(-len(f) // nb)):
            assert {0.0, 1.0} <= set(f[t * nb:(t + 1) * nb].tolist())
    assert not X.flags.writeable
    hf = GR.case_data("hfblock")[0][:, -1]
    assert np.all(hf[64:96] == 1.0)   # a tile of HF rows only
    Xg = GR.graph_data("g2")[0]
    assert np.array_equal(Xg[:, -1], np.arange(97) % 3)
    r = GR.graph_data("g2")[2]["rhoLF"]
    assert r[0, 1] != r[1, 0]


def test_fractional_rows_carry_noise_gradient():
    """`mixed`: the two rows that are neither LF nor HF have K_aa = s2, and their 1/2 W_aa is a share
    of dLML/dnoise that even the older bound would see."""
    rows, share = GR.fractional_noise_share("mixed")
    ref = GR.case_reference("mixed")
    assert rows.tolist() == [GR.MIXED_FRAC_ROW, GR.MIXED_NEAR_ONE_ROW]
    print(f"mixed: g_noise {ref['g64'][-1]:.4e}, the fractional rows' share {share / ref['g64'][-1]:.3f}")
    assert abs(share) > 100 * 1e-8 * np.abs(ref["g64"]).max()
    assert abs(share) > 100 * GR.FACTOR * ref["c"] * ref["S"][-1]


@pytest.mark.parametrize("name", ["mixed", "onerow"])
def test_one_dropped_pair_violates_the_bound(name):
    """Take the delta term of a single H-H entry (a, b), and the rho term of a single L-H entry, out
    of the fp64 oracle's sums: vD, every lD(d) and rho0 then miss 8 c S_q.  The entries are the ones
    of median size among their kind, not the largest."""
    X, Y, p = GR.case_data(name)
    ref = GR.case_reference(name)
    D = X.shape[1] - 1
    t = GR.oracle_terms64(X, Y, p)
    f = X[:, -1]
    H, L = np.nonzero(f == 1)[0], np.nonzero(f == 0)[0]

    def median_entry(rows, cols, M):
        cand = [(abs(M[a, b]), a, b) for a in rows for b in cols if a != b]
        cand.sort()
        return cand[len(cand) // 2][1:]

    a, b = median_entry(H, H, t["W"] * t["eD"])
    u, w = median_entry(L, H, t["W"] * t["kL"])
    g = ref["g64"].copy()
    g[1 + D] -= 0.5 * t["W"][a, b] * t["eD"][a, b]
    for d in range(D):
        g[2 + D + d] -= 0.5 * t["W"][a, b] * t["kD"][a, b] * (X[a, d] - X[b, d]) ** 2 / p.lD[d] ** 3
    g[2 + 2 * D] -= 0.5 * t["W"][u, w] * t["kL"][u, w]   # K_uw = rho kL: h_u s_w + s_u h_w = 1
    ratio = np.abs(g - ref["g_ref"]) / (ref["c"] * ref["S"])
    clean = np.abs(ref["g64"] - ref["g_ref"]) / (ref["c"] * ref["S"])
    groups = GR.case_groups(name)
    print(f"{name}: H-H entry ({a}, {b}) and L-H entry ({u}, {w}) dropped: |g - g_ref| / (c S) "
          + ", ".join(f"{k} {ratio[idx].max():.3g}" for k, idx in groups.items())
          + f"; of S: vD {ratio[1 + D] * ref['c']:.1e}, rho0 {ratio[2 + 2 * D] * ref['c']:.1e}")
    assert clean.max() <= 1.0   # the untouched oracle is within c by construction
    assert ratio[1 + D] > GR.FACTOR and ratio[2 + 2 * D] > GR.FACTOR
    assert ratio[groups["lD"]].max() > GR.FACTOR
    assert ratio[groups["vL"]].max() <= 1.0 and ratio[groups["noise"]].max() <= 1.0   # untouched groups


def test_mpmath_fallback_agrees():
    """Hosts whose long double is a double compute the references with mpmath at 40 digits: the same
    code on object arrays.  At the smallest case it gives the long-double result to fp64 rounding of
    the outputs."""
    pytest.importorskip("mpmath")
    B = GR.backend(force="mpmath")
    assert B.name.startswith("mpmath")
    X, Y, p = GR.case_data("t1")
    lml, g, S = GR.gpr_grad_ref(X, Y, p, B)
    ref = GR.case_reference("t1")
    assert abs(lml - ref["l_ref"]) <= 1e-13 * abs(ref["l_ref"])
    assert np.all(np.abs(g - ref["g_ref"]) <= 1e-2 * ref["c"] * ref["S"])   # the reference's own error: under c / 100
    np.testing.assert_allclose(S, ref["S"], rtol=1e-12)
