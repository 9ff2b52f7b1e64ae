"""MaskedGaussian (missing_outputs=True on the SVGP emulators): the fp64 restatement against the
KAT-pinned oracle, and the host logic that runs before any device call.  No GPU."""
import numpy as np
import pytest
import torch

import multi_fidelity_gpflow_amd as M
from multi_fidelity_gpflow_amd import engine as E
from multi_fidelity_gpflow_amd.svgp import _transform_code
from oracle import svgp_oracle as S

from _masked_oracle import apply_mask, masked_elbo_t, synthetic_mask


def _state(rng, N, P, D, L, Mi, with_W):
    X = np.hstack([rng.random((N, D)), (rng.random((N, 1)) < 0.3).astype(float)])
    Y = rng.standard_normal((N, P))
    Z = np.hstack([rng.random((Mi, D)), (rng.random((Mi, 1)) < 0.3).astype(float)])
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)   # a python float would make an fp32 tensor
    kps = [dict(vL=t64(0.5 + rng.random()), lL=t64(0.5 + rng.random(D)), vD=t64(0.2 + rng.random()),
                lD=t64(0.5 + rng.random(D)), rho=t64(0.5 + rng.random())) for _ in range(L)]
    q_mu = torch.tensor(rng.standard_normal((Mi, L)) * 0.3)
    q_sqrt = torch.tensor(np.tril(rng.standard_normal((L, Mi, Mi)) * 0.05) + np.eye(Mi)[None] * 0.4)
    W = torch.tensor(rng.standard_normal((P, L)) * 0.4) if with_W else None
    noise = torch.tensor(0.05 + rng.random() * 0.1, dtype=torch.float64)
    return torch.tensor(X), torch.tensor(Y), torch.tensor(Z), kps, q_mu, q_sqrt, W, noise


def _leaves(Z, kps, q_mu, q_sqrt, W, noise):
    leaves = [Z, q_mu, q_sqrt, noise] + ([W] if W is not None else []) + [t for kp in kps for t in kp.values()]
    for t in leaves:
        t.requires_grad_(True)
    return leaves


@pytest.mark.parametrize("with_W", [True, False])
def test_masked_oracle_without_nan_is_the_pinned_oracle(with_W):
    """masked_elbo_t (no NaN, scalar noise) == oracle.svgp_oracle.elbo_t, value and autograd
    gradients, 1e-14 relative."""
    P, L = (6, 3) if with_W else (4, 4)
    res = []
    for masked in (False, True):
        X, Y, Z, kps, q_mu, q_sqrt, W, noise = _state(np.random.default_rng(7), 23, P, 3, L, 9, with_W)
        leaves = _leaves(Z, kps, q_mu, q_sqrt, W, noise)
        fn = masked_elbo_t if masked else S.elbo_t
        e, kl, ve = fn(X, Y, Z, kps, q_mu, q_sqrt, W, noise, num_data=40)
        e.backward()
        res.append((float(e.detach()), float(kl.detach()), float(ve.detach()),
                    [t.grad.numpy().copy() for t in leaves]))
    (e0, kl0, ve0, g0), (e1, kl1, ve1, g1) = res
    for a, b in ((e0, e1), (kl0, kl1), (ve0, ve1)):
        assert abs(a - b) <= 1e-14 * abs(a), (a, b)
    for a, b in zip(g0, g1):
        assert np.abs(a - b).max() <= 1e-14 * max(np.abs(a).max(), 1e-300), (a, b)


def test_fully_masked_column_is_the_problem_without_it():
    """Column c of Y entirely NaN: masked_elbo_t with a (P,) noise equals elbo_t on the problem with that
    column of Y, that row of W and that noise entry removed (elbo_t broadcasts a (P - 1,) noise over the
    columns), 1e-13 relative, gradients included; the masked column's own noise gradient is exactly 0."""
    P, L, c = 6, 3, 2
    rng = np.random.default_rng(8)
    X, Y, Z, kps, q_mu, q_sqrt, W, _ = _state(rng, 23, P, 3, L, 9, True)
    noise = torch.tensor(0.05 + rng.random(P) * 0.1)
    keep = [j for j in range(P) if j != c]
    Yn = Y.clone()
    Yn[:, c] = float("nan")
    leaves = _leaves(Z, kps, q_mu, q_sqrt, W, noise)
    e1, kl1, ve1 = masked_elbo_t(X, Yn, Z, kps, q_mu, q_sqrt, W, noise, num_data=40)
    e1.backward()
    g1 = [t.grad.numpy().copy() for t in leaves]
    for t in leaves:
        t.grad = None
    e0, kl0, ve0 = S.elbo_t(X, Y[:, keep], Z, kps, q_mu, q_sqrt, W[keep], noise[keep], num_data=40)
    e0.backward()
    g0 = [t.grad.numpy().copy() for t in leaves]
    for a, b in ((e0, e1), (kl0, kl1), (ve0, ve1)):
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-13 * abs(float(a.detach())), (a, b)
    for a, b in zip(g0, g1):
        assert np.all(np.isfinite(b))
        assert np.abs(a - b).max() <= 1e-13 * max(np.abs(a).max(), 1e-300), (a, b)
    gn, gW = g1[3], g1[4]
    assert gn[c] == 0.0 and np.all(gn[keep] != 0.0)
    assert np.all(gW[c] == 0.0)


def test_masked_entries_have_exact_zero_gradients():
    """The seeded mask (scatter, a full row, a full column, the LF block): finite value and gradients, an
    exact 0 for the fully masked column's noise gradient, and VE equal to the per-entry terms summed
    over the observed entries alone."""
    rng = np.random.default_rng(9)
    X, Y, Z, kps, q_mu, q_sqrt, W, _ = _state(rng, 23, 6, 3, 3, 9, True)
    noise = torch.tensor(0.05 + rng.random(6) * 0.1)
    miss, row, col = synthetic_mask(X.numpy(), 6, 3)
    assert miss[row].all() and miss[:, col].all() and 0.3 < miss.mean() < 0.8
    obs = ~miss
    assert all(obs[:, c].sum() >= 2 for c in range(6) if c != col)
    Yn = torch.tensor(apply_mask(Y.numpy(), miss))
    leaves = _leaves(Z, kps, q_mu, q_sqrt, W, noise)
    e, kl, ve = masked_elbo_t(X, Yn, Z, kps, q_mu, q_sqrt, W, noise)
    e.backward()
    ve = ve.detach()
    assert np.isfinite(float(e.detach())) and all(np.all(np.isfinite(t.grad.numpy())) for t in leaves)
    assert noise.grad[col] == 0.0
    # the value is the per-entry sum over the observed entries
    with torch.no_grad():
        gm, gv = S.latent_moments(X, Z, kps, q_mu, q_sqrt)
        fm, fv = (gm @ W.T).numpy(), (gv @ (W * W).T).numpy()
    s2 = noise.detach().numpy()[None, :] * np.ones_like(fm)
    Yh = Y.numpy()
    terms = -0.5 * S.LOG2PI - 0.5 * np.log(s2) - 0.5 * ((Yh - fm) ** 2 + fv) / s2
    assert abs(terms[obs].sum() - float(ve)) <= 1e-13 * abs(float(ve))


def test_likelihood_shapes_transform_and_lower_bound():
    lik = M.MaskedGaussian(np.ones(5))
    assert isinstance(lik, M.Gaussian) and not isinstance(lik, M.HeteroscedasticGaussian)
    v = lik.variance
    assert v.shape == (5,) and v.trainable
    assert _transform_code(v) == 2                       # Gaussian's own Shift(1e-6) o Softplus
    np.testing.assert_array_equal(v.numpy(), np.ones(5))
    s = M.MaskedGaussian(0.25).variance
    assert s.shape == () and s.trainable and _transform_code(s) == 2
    assert abs(float(s.numpy()) - 0.25) < 1e-15          # forward(inverse(v)): an ulp
    assert M.MaskedGaussian().variance.shape == ()
    # the lower bound: the most negative unconstrained value still maps above 1e-6
    v.unconstrained_variable = np.full(5, -800.0)
    assert np.all(v.numpy() >= 1e-6) and np.all(v.numpy() < 1.1e-6)
    with pytest.raises(ValueError, match="shape"):
        M.MaskedGaussian(np.ones((2, 3)))


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the host-side check")
    monkeypatch.setattr(E.Engine, "get", staticmethod(boom))


def _k():
    return M.SquaredExponential(lengthscales=np.ones(5))


def test_constructor_keyword(hbs, monkeypatch):
    _no_device(monkeypatch)
    X, Y = hbs["X"], hbs["Y"]
    P = Y.shape[1]
    miss, _, _ = synthetic_mask(X, P, 4)
    Yn = apply_mask(Y, miss)
    m = M.LatentMFCoregionalizationSVGP(X, Yn, _k(), _k(), 3, 8, P, missing_outputs=True)
    assert type(m.likelihood) is M.MaskedGaussian and m._masked() and not m._heteroscedastic()
    assert m.likelihood.variance.shape == (P,) and m.likelihood.variance.trainable
    np.testing.assert_array_equal(m.likelihood.variance.numpy(), np.ones(P))
    s = M.SingleBinSVGP(X, Yn[:, :4], _k(), _k(), 4, np.zeros((6, 6)), missing_outputs=True)
    assert type(s.likelihood) is M.MaskedGaussian and s.likelihood.variance.shape == (4,)
    # the default is what it was
    h = M.LatentMFCoregionalizationSVGP(X, Y, _k(), _k(), 3, 8, P)
    assert type(h.likelihood) is M.Gaussian and h.likelihood.variance.shape == () and not h._masked()
    assert type(M.SingleBinSVGP(X, Y[:, :4], _k(), _k(), 4, np.zeros((6, 6))).likelihood) is M.Gaussian
    with pytest.raises(ValueError, match="heterosed"):
        M.LatentMFCoregionalizationSVGP(X, np.hstack([Y, Y]), _k(), _k(), 3, 8, P, True, True, missing_outputs=True)
    with pytest.raises(ValueError, match="heterosed"):
        M.LatentMFCoregionalizationSVGP(X, Yn, _k(), _k(), 3, 8, P, heterosed=True, missing_outputs=True)
    with pytest.raises(ValueError, match="pca"):
        M.LatentMFCoregionalizationSVGP(X, Yn, _k(), _k(), 3, 8, P, w_type='pca', missing_outputs=True)


@pytest.mark.parametrize("call", ["elbo", "elbo_and_grad", "optimize"])
def test_host_checks_come_before_the_device(hbs, monkeypatch, call):
    _no_device(monkeypatch)
    X, Y = hbs["X"], hbs["Y"]
    P = Y.shape[1]
    m = M.LatentMFCoregionalizationSVGP(X, Y, _k(), _k(), 3, 8, P, missing_outputs=True)

    def run(model, data):
        if call == "optimize":
            model.optimize(data, max_iters=2)
        else:
            getattr(model, call)(data)

    with pytest.raises(ValueError, match=rf"\[N, {P}\]"):
        run(m, (X, Y[:, :P - 1]))
    m.likelihood = M.MaskedGaussian(np.ones(P - 1))      # an assigned likelihood of the wrong size
    with pytest.raises(ValueError, match=r"\(num_outputs,\)"):
        run(m, (X, Y))


def test_parameter_dict_round_trip(hbs, monkeypatch, tmp_path):
    _no_device(monkeypatch)
    X, Y = hbs["X"], hbs["Y"]
    P = Y.shape[1]
    m = M.LatentMFCoregionalizationSVGP(X, Y, _k(), _k(), 3, 8, P, missing_outputs=True)
    rng = np.random.default_rng(1)
    for p in m.parameters:
        if p.transform is not None:
            p.unconstrained_variable = rng.normal(0.3, 1.0, p.shape)
    d = M.parameter_dict(m)
    assert d[".likelihood.variance"].shape == (P,)
    path = str(tmp_path / "masked.pkl")
    m.save_model(path)
    m2 = M.LatentMFCoregionalizationSVGP.load_model(path, X, Y, _k(), _k(), 3, 8, P, missing_outputs=True)
    assert type(m2.likelihood) is M.MaskedGaussian
    d2 = M.parameter_dict(m2)
    assert d2.keys() == d.keys()
    for k in d:
        np.testing.assert_array_equal(d2[k], d[k], err_msg=k)
    s = M.SingleBinSVGP(X, Y[:, :4], _k(), _k(), 4, np.zeros((6, 6)), missing_outputs=True)
    s.likelihood.variance.unconstrained_variable = rng.normal(0.3, 1.0, 4)
    path = str(tmp_path / "masked_sb.pkl")
    s.save_model(path)
    s2 = M.SingleBinSVGP.load_model(path, X, Y[:, :4], _k(), _k(), 4, np.zeros((6, 6)), missing_outputs=True)
    np.testing.assert_array_equal(s2.likelihood.variance.numpy(), s.likelihood.variance.numpy())


def test_c_entries_reject_a_bad_pn_before_any_device_work():
    """pn other than 1 or p is the bad-argument code (-1).  The pointers are non-null dummies: the
    argument checks come before anything reads them (include/mfgp.h, tests/test_capi.py)."""
    import ctypes as C
    from multi_fidelity_gpflow_amd import _lib
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mfgp_create(0, C.byref(h)) == 0
    try:
        q = 64   # never dereferenced
        n, m, l, p, d = 8, 4, 3, 3, 2
        for pn in (0, 2, 4, -1):
            assert lib.mfgp_svgp_elbo_masked(h, n, m, l, p, d, q, d + 1, q, p, q, d + 1, q, q, q, None, q, pn, 1.0,
                                             1e-6, q, 1 << 20, q, q, q, q) == -1
            assert lib.mfgp_svgp_elbo_grad_masked(h, n, m, l, p, d, q, d + 1, q, p, q, d + 1, q, q, q, 1, None, q, pn,
                                                  1.0, 1.0, 1e-6, q, 1 << 20, q, q, q, q, q, q, q, None, q, q) == -1
        # a NULL noise vector, and identity mixing with l != p, are bad arguments too
        assert lib.mfgp_svgp_elbo_masked(h, n, m, l, p, d, q, d + 1, q, p, q, d + 1, q, q, q, None, None, p, 1.0, 1e-6,
                                         q, 1 << 20, q, q, q, q) == -1
        assert lib.mfgp_svgp_elbo_masked(h, n, m, 2, p, d, q, d + 1, q, p, q, d + 1, q, q, q, None, q, p, 1.0, 1e-6,
                                         q, 1 << 20, q, q, q, q) == -1
    finally:
        lib.mfgp_destroy(h)


def test_c_entries_reject_a_short_leading_dimension_before_any_device_work():
    """All six ELBO entries, value and gradient alike, return the bad-argument code (-1) for ldx < d + 1,
    ldz < d + 1, ldy < p and, with a non-null Yunc, ldu < p (include/mfgp.h): such a call would read
    past its rows.  Non-null dummy pointers, never read, as above."""
    import ctypes as C
    from multi_fidelity_gpflow_amd import _lib
    from multi_fidelity_gpflow_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mfgp_create(0, C.byref(h)) == 0
    try:
        q = 64   # never dereferenced
        n, m, l, p, d = 8, 4, 3, 3, 2
        val = (1.0, 1e-6, q, 1 << 20, q, q, q, q)                             # scale .. info
        grad = (1.0, 1.0, 1e-6, q, 1 << 20, q, q, q, q, q, q, q, None, q, q)  # scale, kl_mult .. info

        def entries(ldx, ldy, ldz, yunc=None, ldu=p):
            head = (h, n, m, l, p, d, q, ldx, q, ldy)
            z = (q, ldz, q, q, q)   # Z, ldz, thetas, q_mu, q_sqrt
            return {   # called one by one: only a call with a bad argument may be made on these pointers
                "elbo": lambda: lib.mfgp_svgp_elbo(*head, *z, None, 0.1, *val),
                "elbo_grad": lambda: lib.mfgp_svgp_elbo_grad(*head, *z, None, q, *grad),
                "elbo_het": lambda: lib.mfgp_svgp_elbo_het(*head, yunc, ldu, *z, None, 0.1, *val),
                "elbo_grad_het": lambda: lib.mfgp_svgp_elbo_grad_het(*head, yunc, ldu, *z, 0, None, q, *grad),
                "elbo_masked": lambda: lib.mfgp_svgp_elbo_masked(*head, *z, None, q, p, *val),
                "elbo_grad_masked": lambda: lib.mfgp_svgp_elbo_grad_masked(*head, *z, 0, None, q, p, *grad),
            }

        for lds in ((d, p, d + 1), (d + 1, p, d), (d + 1, p - 1, d + 1)):   # ldx, ldy, ldz: one short each
            for yunc in (None, q):
                for name, call in entries(*lds, yunc=yunc).items():
                    assert call() == -1, (name, lds, yunc)
        short_ldu = entries(d + 1, p, d + 1, yunc=q, ldu=p - 1)
        assert short_ldu["elbo_het"]() == -1 and short_ldu["elbo_grad_het"]() == -1
    finally:
        lib.mfgp_destroy(h)


def test_multiple_assign_restores_values_whose_unconstrained_value_is_near_zero():
    """A Softplus value near log 2 has u ~ 0, where an ulp of u is a hundredth of an ulp of the value:
    trained (P,) variances around 0.7 are such values.  multiple_assign restores every one bit for bit."""
    rng = np.random.default_rng(2)
    src = M.MaskedGaussian(np.ones(4000))
    src.variance.unconstrained_variable = rng.normal(0.0, 0.02, 4000)
    saved = M.parameter_dict(src)
    assert 0.6 < saved[".variance"].min() and saved[".variance"].max() < 0.8
    dst = M.MaskedGaussian(np.ones(4000))
    M.multiple_assign(dst, saved)
    np.testing.assert_array_equal(dst.variance.numpy(), saved[".variance"])
