"""oracle/graph_oracle.py pinned to oracle/mfgp_oracle.py at m = 1 (CPU, fp64 against fp64).

With one LF source the graph kernel (graph.py:59-91) IS the linear kernel (linear.py:93-102) plus
its 1e-6 I jitter: rho_LF drops out at i == j, rho[:, 0] is rho.  So graph_oracle at noise 1e-3
must reproduce mfgp_oracle -- whose LML, gradient and predictions are pinned by the reference's
recorded values (tests/golden/kats.json) -- at noise 1e-3 + 1e-6: LML, the autograd gradient
(mapped (v_0, l_0, v_delta, l_delta, rho_0, noise) <-> (vL, lL, vD, lD, rho0, noise); rho_LF's
only entry is the unused diagonal, gradient None or 0) and predict_f.

Observed agreement of the two references (relative LML; gradient relative to its largest entry;
predictions absolute), random constrained parameters, seed fixed below:

    quantity            HBS      Goku
    LML                 9e-15    6e-14
    gradient            2e-14    5e-13
    predicted mean      8e-15    6e-13
    predicted variance  2e-15    3e-15

(another draw of the parameters gave 3e-14 / 1e-13 / 2e-15 on HBS and 6e-15 / 7e-13 / 3e-13 on
Goku).  Asserted: 1e-12 (LML), 1e-11 (gradient), 1e-11 (predict), about ten times the worst
observed value."""
import numpy as np
import pytest
import torch

from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O

NOISE = 1e-3


def _params(D, P, seed):
    rng = np.random.default_rng(seed)
    p = O.MFParams(0.8 + 0.7 * rng.random(), 0.6 + 1.4 * rng.random(D), 0.2 + 0.6 * rng.random(),
                   0.5 + 1.2 * rng.random(D), np.full((P, 1), 0.7 + 0.6 * rng.random()), NOISE + GO.JITTER)
    f64 = dict(dtype=torch.float64)
    prm = dict(v=torch.tensor([p.vL, p.vD], **f64), l=torch.tensor(np.stack([p.lL, p.lD]), **f64),
               rho=torch.tensor([p.rho0], **f64), rhoLF=torch.tensor([[0.2 + 0.6 * rng.random()]], **f64))
    return p, prm


@pytest.mark.parametrize("which", ["hbs", "goku"])
def test_graph_oracle_is_linear_oracle_at_one_source(which, hbs, goku):
    d = hbs if which == "hbs" else goku
    X, Y, Xs = d["X"], d["Y"], d["Xtest"][:10]
    D, P = X.shape[1] - 1, Y.shape[1]
    p, prm = _params(D, P, seed=11)
    for v in prm.values():
        v.requires_grad_(True)
    noise = torch.tensor(NOISE, dtype=torch.float64, requires_grad=True)
    Xt, Yt = torch.tensor(X), torch.tensor(Y)

    lo = GO.lml(Xt, Yt, prm, noise)
    lo.backward()
    lml, g = O.gpr_lml_and_grad(X, Y, p)
    e_lml = abs(float(lo.detach()) - lml) / abs(lml)
    gg = np.concatenate([[prm["v"].grad[0]], prm["l"].grad[0].numpy(), [prm["v"].grad[1]], prm["l"].grad[1].numpy(),
                         prm["rho"].grad.numpy(), [noise.grad]])
    gl = np.concatenate([[g["vL"]], g["lL"], [g["vD"]], g["lD"], [g["rho0"]], [g["noise"]]])
    assert gg.shape == (2 * D + 4,)
    e_g = np.abs(gg - gl).max() / np.abs(gl).max()

    with torch.no_grad():
        mo, vo = GO.predict_f(Xt, Yt, torch.tensor(Xs), prm, noise)
    ml, vl = O.gpr_predict_f(X, Y, Xs, p)
    e_m = np.abs(mo.numpy() - ml).max()
    e_v = np.abs(vo.numpy() - vl[:, 0]).max()
    print(f"{which}: lml {e_lml:.1e} grad {e_g:.1e} mean {e_m:.1e} var {e_v:.1e}")

    assert e_lml < 1e-12
    assert e_g < 1e-11
    glf = prm["rhoLF"].grad
    assert glf is None or not glf.numpy().any()
    assert e_m < 1e-11
    assert e_v < 1e-11
