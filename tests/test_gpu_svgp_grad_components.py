"""Every component of the SVGP ELBO gradient (csrc/mfgp_svgp_grad.hip: k_kgrad, k_kff_grad, k_ve_bwd,
k_ve_bwd_het, k_ve_bwd_masked, k_gw, k_glq_final, k_grad_reduce) against an extended-precision
reference, on the scale of the component's own absolute mass.

Bound.  tests/test_gpu_svgp.py, test_gpu_svgp_het.py, test_gpu_svgp_masked.py and
test_gpu_svgp_tile64.py hold max |g - g64| to 1e-10 of max |g64| per key, and theta [L, 2d+4] and
Z [M, d+1] are one key each: the largest entry is 600 to 1200 times the smallest of d theta and 2e3 to
5e5 times the smallest of dZ, and every entry is a cancelling sum.  Here, for every component q of
every key,

    |g_q - g_ref_q| <= 8 c S_q,     c = max(max_q |g64_q - g_ref_q| / S_q, N 2^-53)

with g_ref the wide restatement of the oracle and S_q the component's absolute mass
(tests/_svgp_grad_oracle.py), g64 fp64 torch autograd through the oracle; a component of mass 0 (the
fidelity column of dZ among them) must be exactly 0.  tests/test_svgp_grad_oracle_host.py keeps
c <= 1e-11 (2.1e-14 to 2.0e-12 at these cases) and shows that the bound fails for an uncentred k_kgrad,
for one dropped HF x HF pair and for a 1e-6 error in one small component that the older gate passes.
The factor 8 is the project's allowance for another summation order, not a measurement; the achieved
ratios are printed (-s) and recorded in DESIGN.md section 4 (largest on the MI355X: q_sqrt 4.19, q_mu
1.57, Z 0.14, W 0.12, theta 0.06, noise 0.02).  The ELBO is held to 1e-13 relative of the wide value.
`shift` is the case that found something: k_gram_dense expanded r^2 on the raw coordinates, and every
key stood at 2.6e3 (noise) to 4.5e6 (q_sqrt) times c, the ELBO at 4.1e-10, until the kernel centred
its operands (csrc/mfgp_kernels.hip); k_kgrad's own centring held.

Cases (_svgp_grad_oracle.SHAPES; N = 190 = 150 LF + 40 HF, M = 40, L = 3, P = 6, d = 5 unless said):
d3 (d = 3: DC 4, a ragged second 32-row tile), sb33 (single bin, M = 33, L = P = 4, W = NULL), d10
(d = 10, N = 300, M = 70, L = 2: DC 12, two K_uf column blocks), d14 / d20 (DC 16 / 32), wide
(M = 270, L = 2: two K_uu column blocks), shift (every coordinate + 1000: k_kgrad's centring), aniso
(lL[0] = lD[0] = 20), mixed (HF rows interleaved in X and Z, two Z rows of fractional fidelity), lfz
(every Z row LF), klm (d3 with kl_multiplier 0.3, num_data = 3 N), het and msk (the other two
likelihoods, through the engine-level call; msk: 15 % NaN, one output without observations, a (P,)
variance).  d3, d10 and wide also run at tile 64; sb33 also runs through the engine with q_sqrt dense
and packed (elbo_and_grad itself always passes packed triangles)."""
import numpy as np
import pytest
import torch

import _grad_oracle as GR
import _svgp_grad_oracle as SG
from multi_fidelity_gpflow_amd.engine import Engine, theta_size, to_dev
from multi_fidelity_gpflow_amd.svgp import DEFAULT_JITTER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    e = Engine.get()
    e.set_tile(32)
    yield e
    e.set_tile(32)


def _reference(name):
    GR.require_wide()
    if name == "wide" and not GR.backend().name.startswith("np.longdouble"):
        pytest.skip("the mpmath fallback is too slow at M = 270")
    return SG.case_reference(name)


def _engine_grad(eng, c, qs_packed):
    """One Engine.svgp_elbo_grad call at the case's state (tests/test_gpu_svgp_het._engine_grad): the
    homoscedastic, heteroscedastic or masked entry point by the case's kind."""
    m = c["model"]
    _, Z, thetas, q_mu, q_sqrt, W = m._dev_state()
    dev = eng.device
    Xd, Yd = to_dev(np.array(c["X"]), dev), to_dev(np.array(c["Yobs"]), dev)   # the case's arrays are read-only
    Ud = None if c["U"] is None else to_dev(np.array(c["U"]), dev)
    n, mi, L, p, d = Xd.shape[0], Z.shape[0], thetas.shape[0], Yd.shape[1], Xd.shape[1] - 1
    f64 = dict(dtype=torch.float64, device=dev)
    ti, tj = np.tril_indices(mi)
    tid, tjd = torch.as_tensor(ti, device=dev), torch.as_tensor(tj, device=dev)
    qs = q_sqrt[:, tid, tjd].contiguous() if qs_packed else q_sqrt
    noise = torch.tensor(np.array(c["noise"]), **f64)
    out, g_mu, g_var = torch.zeros(3, **f64), torch.empty((L, n), **f64), torch.empty((L, n), **f64)
    g = dict(Z=torch.zeros((mi, d + 1), **f64), theta=torch.zeros((L, theta_size(d)), **f64),
             q_mu=torch.zeros((mi, L), **f64), q_sqrt=torch.zeros_like(qs),
             noise=torch.full((noise.numel(),), float("nan"), **f64))
    if W is not None:
        g["W"] = torch.zeros((p, L), **f64)
    info = torch.zeros((L,), dtype=torch.int32, device=dev)
    eng.svgp_elbo_grad(Xd, Yd, Z, thetas, q_mu, qs, W, noise, c["scale"], c["kl_mult"], DEFAULT_JITTER, out, g_mu,
                       g_var, g["Z"], g["theta"], g["q_mu"], g["q_sqrt"], g.get("W"), g["noise"], info,
                       qs_packed=qs_packed, Yunc=Ud, masked=c["kind"] == "msk")
    torch.cuda.synchronize()
    assert int(info.abs().max().item()) == 0
    if qs_packed:
        dense = torch.zeros((L, mi, mi), **f64)
        dense[:, tid, tjd] = g["q_sqrt"]
        g["q_sqrt"] = dense
    return float(out[0].item()), {k: v.cpu().numpy() for k, v in g.items()}


def _guarded(fn):
    """A failed launch or a device error ends the run: nothing more starts on that device."""
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        pytest.exit(f"GPU call failed, ending the run: {e}", returncode=3)


LEGS = [(name, 32) for name in SG.SHAPES] + [(name, 64) for name in SG.TILE64_CASES]


@pytest.mark.parametrize("name,nb", LEGS, ids=[f"{n}-nb{nb}" for n, nb in LEGS])
def test_svgp_grad_components(eng, name, nb):
    """elbo_and_grad (het and msk: the engine-level call of their own tests) at tile 32, and at tile 64
    where the case crosses a 64-tile edge."""
    _reference(name)
    c = SG.case(name)
    try:
        eng.set_tile(nb)
        assert eng.tile() == nb
        if c["kind"] in ("het", "msk"):
            e, g = _guarded(lambda: _engine_grad(eng, c, qs_packed=False))
        else:
            e, g = _guarded(lambda: c["model"].elbo_and_grad((c["X"], c["Y"]), kl_multiplier=c["kl_mult"]))
    finally:
        eng.set_tile(32)
    SG.check_components(name, e, g, tag=f" nb{nb}")
    if name == "msk":
        assert g["noise"].shape == (6,) and g["noise"][SG.MSK_EMPTY_COL] == 0.0
        assert np.all(g["W"][SG.MSK_EMPTY_COL] == 0.0)


@pytest.mark.parametrize("qs_packed", [False, True], ids=["dense", "packed"])
def test_svgp_grad_components_engine_q_sqrt_layouts(eng, qs_packed):
    """sb33 through Engine.svgp_elbo_grad with q_sqrt / gq_sqrt dense [L, M, M] and as packed triangles
    (mfgp_set_svgp_qs_packed(1)): every key under the same bound, q_sqrt among them."""
    _reference("sb33")
    e, g = _guarded(lambda: _engine_grad(eng, SG.case("sb33"), qs_packed))
    r = SG.check_components("sb33", e, g, tag=" engine, q_sqrt " + ("packed" if qs_packed else "dense"))
    assert r["q_sqrt"] <= SG.FACTOR
    assert np.all(np.triu(g["q_sqrt"], 1) == 0.0)
