"""The extended-precision restatement of the SVGP ELBO gradient (tests/_svgp_grad_oracle.py) against
fp64 torch autograd through the oracle, on the CPU, at every case
tests/test_gpu_svgp_grad_components.py uses.

The GPU tests bound each component q of the HIP gradient by 8 c S_q, S_q the component's absolute
mass and c what the fp64 oracle itself costs on that scale (floored at N 2^-53).  Checked here, where
no GPU is needed:

  * algebra: the same code on float64 arrays gives autograd's gradient, every component within
    1e-9 S_q (one pair's term is 1e-5 to 1e-3 of S_q; measured 2e-15 to 4e-12);
  * formats: mpmath at 40 digits and long double agree to under c / 100 at d3;
  * c <= 1e-11 on every case.  A condition on the cases, not a measurement: a case beyond it gets
    shorter lengthscales or fewer inducing points (_svgp_grad_oracle.LSCALE), never a larger cap.
    Measured: 2.1e-14 (the floor, d14 and d20) to 2.0e-12 (klm); q_sqrt and q_mu, which carry L^-1 K_uf, set
    it at every case, theta and Z alone would be 3e-16 to 6e-14.  `shift` with the oracle at the
    untranslated coordinates: 7.9e-7 (the oracle's own r^2 is the uncentred expansion);
  * the gate has teeth: at `shift` the uncentred moment form of k_kgrad's K_uf sums, at `mixed` one
    HF x HF pair's delta term dropped from the K_uu sums, at `aniso` a relative error of 1e-6 in
    d/dlL[0] alone -- which passes the older gate, max |g - ref| / max |ref| < 1e-10 per key."""
import numpy as np
import pytest

import _grad_oracle as GR
import _svgp_grad_oracle as SG


@pytest.fixture(autouse=True)
def _wide():
    GR.require_wide()


def _skip_slow(name):
    if name == "wide" and not GR.backend().name.startswith("np.longdouble"):
        pytest.skip("the mpmath fallback is too slow at M = 270")


@pytest.fixture(scope="module")
def f64():
    """{name: (elbo, g, S, per-latent intermediates)} of the restatement on float64 arrays, on demand."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SG.svgp_grad_ref(SG.case(name), B=SG._Float64, detail=True)
        return cache[name]
    return get


def _worst(r):
    return max(float(v.max()) for v in r.values())


@pytest.mark.parametrize("name", list(SG.SHAPES))
def test_restatement_is_the_oracle_and_fp64_is_cheap(name, f64):
    _skip_slow(name)
    c, ref = SG.case(name), SG.case_reference(name)
    n = c["X"].shape[0]
    unit = SG.ratios(ref["g64"], ref["g_ref"], ref["S"], 1.0)
    e, g, Sm, _ = f64(name)
    alg = SG.ratios(g, ref["g64"], ref["S"], 1.0)
    new = {k: SG.FACTOR * ref["c"] * ref["S"][k] for k in ref["S"]}
    gain = max(float(np.max(np.where(new[k] > 0, 1e-10 * np.abs(ref["g64"][k]).max() / np.where(new[k] > 0, new[k], 1.0),
                                     0.0))) for k in new)
    with np.errstate(divide="ignore", invalid="ignore"):
        mass = {k: float(np.max(np.where(ref["g_ref"][k] != 0, ref["S"][k] / np.abs(ref["g_ref"][k]), 1.0)))
                for k in ref["S"]}
    print(f"{name}: N {n}, c = {ref['c']:.2e} (floor {n * 2.0 ** -53:.1e}"
          + (f", oracle at the untranslated coordinates {ref['c_raw']:.1e}" if name == "shift" else "")
          + f"), ELBO rel {abs(ref['e64'] - ref['e_ref']) / abs(ref['e_ref']):.1e}; |g64 - g_ref| / S per key "
          + ", ".join(f"{k} {v.max():.1e}" for k, v in unit.items())
          + "; float64 restatement vs autograd / S " + ", ".join(f"{k} {v.max():.1e}" for k, v in alg.items())
          + "; largest S_q / |g_q| " + ", ".join(f"{k} {v:.1e}" for k, v in mass.items())
          + f"; old bound / new bound up to {gain:.1e}")
    assert set(ref["g_ref"]) == set(ref["g64"]) == {k for k in SG.KEYS if k != "W" or c["W"] is not None}
    for k in ref["g_ref"]:
        assert ref["g_ref"][k].shape == ref["g64"][k].shape == ref["S"][k].shape
        assert np.all(ref["S"][k] >= np.abs(ref["g_ref"][k]) * (1 - 1e-12))   # |sum| <= sum | |
        np.testing.assert_allclose(Sm[k], ref["S"][k], rtol=1e-9)
    assert np.all(ref["g_ref"]["Z"][:, -1] == 0.0) and np.all(ref["S"]["Z"][:, -1] == 0.0)
    assert np.all(ref["g64"]["Z"][:, -1] == 0.0)
    assert _worst(alg) <= 1e-9                                               # the algebra
    assert abs(e - ref["e64"]) <= 1e-13 * abs(ref["e64"])
    assert abs(ref["e64"] - ref["e_ref"]) <= 1e-13 * abs(ref["e_ref"])
    assert n * 2.0 ** -53 <= ref["c"] <= SG.CAP                              # the cap
    assert ref["c"] == max(_worst(unit), n * 2.0 ** -53)
    assert gain >= 100.0


def test_shift_needs_the_oracle_translated():
    """At coordinates of 1000 the oracle's r^2 = |a|^2 + |b|^2 - 2 a.b is itself 1e5 times the cap off:
    the unit of `shift` is taken with the oracle's inputs translated back, which is exact."""
    c, ref = SG.case("shift"), SG.case_reference("shift")
    for A in (c["X"], c["Z"]):
        back = A[:, :-1] - SG.SHIFT
        assert np.array_equal(back + SG.SHIFT, A[:, :-1]) and back.min() >= -0.01 and back.max() <= 1.01
    print(f"shift: c {ref['c']:.2e}, with the oracle at the untranslated coordinates {ref['c_raw']:.2e}")
    assert ref["c"] <= SG.CAP < 1e3 * SG.CAP < ref["c_raw"]


def test_case_table_hits_what_it_claims():
    assert GR.backend().wide and np.finfo(np.float64).eps > 2.0 ** -60   # the reference is not float64
    assert set(SG.TILE64_CASES) <= set(SG.SHAPES)
    for name, (kind, (n_lf, n_hf), d, P, L, Mi, _, _) in SG.SHAPES.items():
        c = SG.case(name)
        assert c["X"].shape == (n_lf + n_hf, d + 1) and c["Z"].shape == (Mi, d + 1) and c["theta"].shape == (L, 2 * d + 4)
        assert (c["W"] is None) == (kind == "singlebin") and (c["W"] is None or np.all(c["W"] != 0.0))
        assert not c["X"].flags.writeable and np.all(np.triu(c["q_sqrt"], 1) == 0.0)
        assert np.all(c["theta"][:, -1] == 0.0)
    dc = lambda d: next(b for b in (4, 8, 12, 16, 32) if d <= b)
    assert [dc(SG.SHAPES[n][2]) for n in ("d3", "sb33", "d10", "d14", "d20")] == [4, 8, 12, 16, 32]
    assert SG.case("d3")["Z"].shape[0] % 32 == 8 and SG.case("sb33")["Z"].shape[0] == 33
    assert SG.case("d10")["X"].shape[0] == 300 and SG.case("d10")["Z"].shape[0] == 70
    assert SG.case("wide")["Z"].shape[0] > 256 > SG.case("wide")["X"].shape[0]
    fz = SG.case("mixed")["Z"][:, -1]
    fx = SG.case("mixed")["X"][:, -1]
    assert [fz[r] for r, _ in SG.MIXED_FRAC_ROWS] == [f for _, f in SG.MIXED_FRAC_ROWS]
    assert set(fz.tolist()) == {0.0, 1.0, 0.5, 0.9999999999999999} and (fz == 1).sum() >= 6
    for t in range(0, 190, 16):    # every 16-row block of X holds both fidelities
        assert {0.0, 1.0} == set(fx[t:t + 16].tolist())
    assert np.all(SG.case("lfz")["Z"][:, -1] == 0.0)
    assert set(SG.case("d10")["Z"][:, -1].tolist()) == {0.0, 1.0}
    sh = SG.case("shift")
    assert sh["X"][:, :-1].min() >= 999.9 and sh["Z"][:, :-1].min() >= 999.9 and set(sh["X"][:, -1].tolist()) == {0.0, 1.0}
    an = SG.case("aniso")["theta"]
    assert np.all(an[:, 1] == SG.ANISO_L) and np.all(an[:, 7] == SG.ANISO_L) and an[:, 2:6].max() <= 1.5
    k = SG.case("klm")
    assert k["kl_mult"] == 0.3 and k["scale"] == 3.0 and np.array_equal(k["Z"], SG.case("d3")["Z"])
    h = SG.case("het")
    assert h["U"].shape == h["Yobs"].shape and h["Y"].shape[1] == 12 and h["noise"].shape == (1,)
    m = SG.case("msk")
    miss = np.isnan(m["Yobs"])
    assert miss[:, SG.MSK_EMPTY_COL].all() and 0.10 < np.delete(miss, SG.MSK_EMPTY_COL, 1).mean() < 0.20
    assert m["noise"].shape == (6,) and np.unique(m["noise"]).size == 6
    ref = SG.case_reference("msk")
    assert ref["g_ref"]["noise"][SG.MSK_EMPTY_COL] == 0.0 and ref["S"]["noise"][SG.MSK_EMPTY_COL] == 0.0
    assert np.all(ref["S"]["W"][SG.MSK_EMPTY_COL] == 0.0)


@pytest.mark.slow
def test_mpmath_fallback_agrees():
    """Hosts whose long double is a double compute the references with mpmath at 40 digits: the same
    code on object arrays.  At d3 it gives the long-double result to under c / 100."""
    pytest.importorskip("mpmath")
    B = GR.backend(force="mpmath")
    assert B.name.startswith("mpmath")
    ref = SG.case_reference("d3")
    e, g, Sm = SG.svgp_grad_ref(SG.case("d3"), B)
    r = SG.ratios(g, ref["g_ref"], ref["S"], ref["c"])
    print("d3: mpmath against the wide reference, |dg| / (c S) per key " + ", ".join(f"{k} {v.max():.1e}" for k, v in r.items()))
    assert abs(e - ref["e_ref"]) <= 1e-14 * abs(ref["e_ref"])
    assert _worst(r) <= 1e-2
    for k in Sm:
        np.testing.assert_allclose(Sm[k], ref["S"][k], rtol=1e-12)


# ---------------------------------------------------------------- the gate has teeth
def _kuf_moment_terms(c, lat, centre):
    """float64: the K_uf part of d/dlL, d/dlD [L, D] and of dZ [M, D] from the moments
    [S0 | S1 | S2](a) = sum_i w(a, i) [1 | x_i | x_i^2] as k_kgrad forms them,
    sum_i w (z - x)^2 = z^2 S0 - 2 z S1 + S2 and sum_i w (z - x) = z S0 - S1, with the coordinates taken
    relative to `centre` [D]; and the same sums in the direct-difference form."""
    X, Z = c["X"][:, :-1] - centre, c["Z"][:, :-1] - centre
    D = X.shape[1]
    L = len(lat)
    mom, direct = np.zeros((2, L, D)), np.zeros((2, L, D))
    zmom, zdir = np.zeros(Z.shape), np.zeros(Z.shape)
    for l, s in enumerate(lat):
        uf, th = s["uf"], s["th"]
        for k, (w, ls) in enumerate(((s["Kbar"] * uf["ss"] * uf["kL"], th["lL"]), (s["Kbar"] * uf["hh"] * uf["kD"], th["lD"]))):
            S0, S1, S2 = w.sum(1), w @ X, w @ (X * X)
            mom[k, l] = (Z * Z * S0[:, None] - 2 * Z * S1 + S2).sum(0) / ls ** 3
            zmom -= (Z * S0[:, None] - S1) / ls ** 2
            direct[k, l] = [(w * uf["d2"][d]).sum() / ls[d] ** 3 for d in range(D)]
            zdir -= np.stack([(w * uf["diff"][d]).sum(1) / ls[d] ** 2 for d in range(D)], 1)
    return mom, zmom, direct, zdir


def test_uncentred_moment_form_violates_the_bound_at_shift(f64):
    """k_kgrad takes its coordinates relative to the block's first Z row.  The float64 restatement with
    the K_uf lengthscale and Z sums in that moment form keeps the bound when centred on Z[0] and
    misses it uncentred."""
    c, ref = SG.case("shift"), SG.case_reference("shift")
    D = c["X"].shape[1] - 1
    _, g, _, lat = f64("shift")
    worst = {}
    for tag, centre in (("centred", c["Z"][0, :-1]), ("uncentred", np.zeros(D))):
        mom, zmom, direct, zdir = _kuf_moment_terms(c, lat, centre)
        gd = {k: v.copy() for k, v in g.items()}
        gd["theta"][:, 1:1 + D] += mom[0] - direct[0]
        gd["theta"][:, 2 + D:2 + 2 * D] += mom[1] - direct[1]
        gd["Z"][:, :-1] += zmom - zdir
        r = SG.ratios(gd, ref["g_ref"], ref["S"], ref["c"])
        worst[tag] = {k: float(r[k].max()) for k in ("theta", "Z")}
        print(f"shift, K_uf sums in the {tag} moment form: |g - g_ref| / (c S) theta {worst[tag]['theta']:.3g} "
              f"({worst[tag]['theta'] * ref['c']:.1e} S), Z {worst[tag]['Z']:.3g} ({worst[tag]['Z'] * ref['c']:.1e} S)")
    clean = SG.ratios(g, ref["g_ref"], ref["S"], ref["c"])
    assert _worst(clean) <= SG.FACTOR
    assert max(worst["centred"].values()) <= SG.FACTOR
    assert max(worst["uncentred"].values()) > SG.FACTOR   # the lengthscale sums z^2 S0 - 2 z S1 + S2


def test_one_dropped_hf_pair_violates_the_bound_at_mixed(f64):
    """One HF x HF pair (a, b) of Z, of median size among its kind, loses its delta term in the K_uu
    sums of latent 0: vD, every lD(d) and the two Z rows then miss 8 c S_q."""
    c, ref = SG.case("mixed"), SG.case_reference("mixed")
    D = c["X"].shape[1] - 1
    s = f64("mixed")[3][0]
    uu, th, Sig = s["uu"], s["th"], s["Sig"]
    H = np.flatnonzero(c["Z"][:, -1] == 1)
    cand = sorted((abs(Sig[a, b] * uu["eD"][a, b]), a, b) for a in H for b in H if a < b)
    _, a, b = cand[len(cand) // 2]
    g = {k: v.copy() for k, v in ref["g64"].items()}
    g["theta"][0, 1 + D] -= 2 * Sig[a, b] * uu["eD"][a, b]
    for d in range(D):
        g["theta"][0, 2 + D + d] -= 2 * Sig[a, b] * uu["kD"][a, b] * uu["d2"][d][a, b] / th["lD"][d] ** 3
        t = -2 * Sig[a, b] * uu["diff"][d][a, b] * uu["kD"][a, b] / th["lD"][d] ** 2
        g["Z"][a, d] -= t
        g["Z"][b, d] += t
    r = SG.ratios(g, ref["g_ref"], ref["S"], ref["c"])
    clean = SG.ratios(ref["g64"], ref["g_ref"], ref["S"], ref["c"])
    print(f"mixed: HF x HF pair ({a}, {b}) of Z dropped from latent 0's K_uu sums: |g - g_ref| / (c S) vD "
          f"{r['theta'][0, 1 + D]:.3g} ({r['theta'][0, 1 + D] * ref['c']:.1e} S), lD {r['theta'][0, 2 + D:2 + 2 * D].min():.3g} to "
          f"{r['theta'][0, 2 + D:2 + 2 * D].max():.3g}, Z rows {r['Z'][[a, b], :-1].min():.3g} to {r['Z'][[a, b], :-1].max():.3g}")
    assert _worst(clean) <= 1.0   # the untouched oracle is within c by construction
    assert r["theta"][0, 1 + D] > SG.FACTOR and r["theta"][0, 2 + D:2 + 2 * D].min() > SG.FACTOR
    assert r["Z"][[a, b], :-1].max() > SG.FACTOR
    assert r["theta"][1:].max() <= 1.0 and r["q_mu"].max() <= 1.0   # untouched components


def test_small_component_error_passes_the_old_gate_and_violates_the_bound_at_aniso():
    """lL[0] = 20: d/dlL[0] is far below the largest entry of d theta.  A relative error of 1e-6 in it
    alone (latent 0) is invisible to max |g - ref| / max |ref| < 1e-10 and misses 8 c S_q."""
    ref = SG.case_reference("aniso")
    g = {k: v.copy() for k, v in ref["g64"].items()}
    g["theta"][0, 1] *= 1.0 + 1e-6
    old = SG.old_gate(g, ref["g64"])
    r = SG.ratios(g, ref["g_ref"], ref["S"], ref["c"])
    th = ref["g64"]["theta"]
    print(f"aniso: d/dlL[0] = {th[0, 1]:.3e} against max |d theta| = {np.abs(th).max():.3e}; a 1e-6 error in it: "
          f"old gate {old['theta']:.1e} (bound 1e-10), |g - g_ref| / (c S) {r['theta'][0, 1]:.3g} (bound {SG.FACTOR:g}), "
          f"S / |g| {ref['S']['theta'][0, 1] / abs(ref['g_ref']['theta'][0, 1]):.1f}")
    assert all(v < 1e-10 for v in old.values())
    assert r["theta"][0, 1] > SG.FACTOR
    r["theta"][0, 1] = 0.0
    assert _worst(r) <= 1.0
