"""Leave-group-out cross-validation, the parts that need no GPU: the closed form the device evaluates
against brute-force refits (tests/_leave_out_oracle.py), groups_by_input, and the group normaliser."""
import numpy as np
import pytest

import _leave_out_oracle as LO
from multi_fidelity_gpflow_amd.posteriors import groups_by_input, normalize_groups


@pytest.mark.parametrize("which,name", [("hbs", "singles"), ("hbs", "pairs"), ("n79", "sizes"), ("n79", "labels")])
def test_closed_form_is_the_refit(which, name):
    """The identity: the closed form from one factorization equals a refit without the group, to
    1e-12 max(1, |ref|), for the mean, the variance, the group covariance and the log density."""
    ref, closed, dev = LO.reference(which, name)
    print(f"{which} {name}: closed form vs refit {dev}")
    for k in ("mean", "var", "cov", "log_density"):
        assert ref[k].shape == closed[k].shape
        assert dev[k] <= 1e-12 * max(1.0, np.abs(ref[k]).max()), (which, name, k, dev[k])
    np.testing.assert_array_equal(ref["rows"], closed["rows"])
    P = ref["mean"].shape[1]
    assert ref["var"].shape == ref["mean"].shape and ref["log_density"].shape == (ref["cov"].shape[0], P)
    assert np.all(ref["var"] > 0)


def test_graph_kernel_identity():
    """The graph kernel with the asymmetric rho_LF of the graph tests: the closed form equals the
    oracle's refit at the rows of LF source 0 and at the HF rows, and the refit of the joint model as
    the factorization reads it (lower triangle mirrored) at every row, groups across sources included;
    at a tenth of the GPU tests' bounds (the references themselves: cond(K + s2 I) ~ 1e5 at noise 1e-3).
    At a row of LF source 1 the oracle's refit is another model (graph_refit_valid): its variance at
    training row 40 is negative."""
    from oracle import graph_oracle as GO
    import torch
    from test_gpu_graph import _data, _model, _oracle_params
    m, D = 2, 3
    X, Y = _data(m, D)
    mod = _model(X, Y, m, D, asym=True)
    prm, s2 = _oracle_params(mod, D), float(mod.likelihood.variance.numpy())
    valid = [[int(i)] for i in np.flatnonzero(LO.graph_refit_valid(X, m))]
    assert len(valid) == 52
    groups = [[i] for i in range(82)] + [[41, 75], [3, 50, 80]]
    for name, ref, closed in (("source 0 and HF", LO.brute(X, Y, prm, valid, noise=s2),
                               LO.closed_numpy(X, Y, prm, valid, noise=s2)),
                              ("joint", LO.brute_joint(X, Y, prm, groups, s2),
                               LO.closed_numpy(X, Y, prm, groups, noise=s2))):
        dev = LO.deviation(ref, closed)
        print(f"graph {name}: closed form vs refit {dev}")
        for k in dev:
            assert dev[k] <= 1e-10 * max(1.0, np.abs(ref[k]).max()), (name, k, dev[k])
    keep = np.setdiff1d(np.arange(82), [40])
    _, c = GO.predict_f_full_cov(torch.tensor(X[keep]), torch.tensor(Y[keep]), torch.tensor(X[[40]]), prm, s2)
    assert float(c[0, 0]) + s2 < 0.0


def test_groups_by_input_hbs(hbs):
    X = hbs["X"]
    labels = groups_by_input(X)
    assert labels.shape == (53,) and labels.dtype == np.int64
    assert len(set(labels.tolist())) == 50 and labels.min() == 0 and labels.max() == 49
    hf = groups_by_input(X, only_hf=True)
    pairs = [tuple(np.flatnonzero(hf == k)) for k in range(hf.max() + 1)]
    assert sorted(pairs) == [(0, 52), (9, 50), (46, 51)]
    assert np.count_nonzero(hf == -1) == 47
    for a, b in pairs:   # bit-identical inputs, fidelities 0 and 1
        assert X[a, :-1].tobytes() == X[b, :-1].tobytes() and X[a, -1] == 0.0 and X[b, -1] == 1.0
    offsets, rows, gmax = normalize_groups(hf, 53)
    assert gmax == 2 and offsets.tolist() == [0, 2, 4, 6] and rows.tolist() == [0, 52, 9, 50, 46, 51]


def test_groups_by_input_hand_made():
    X = np.array([[0.5, 0.25, 0.0],
                  [0.1, 0.25, 0.0],
                  [0.5, 0.25, 1.0],      # = row 0
                  [0.5, 0.25 + 2.0 ** -54, 0.0],   # one ulp from row 0: its own group
                  [0.1, 0.25, 0.0],      # = row 1, no HF row in the group
                  [-0.0, 0.0, 1.0],
                  [0.0, 0.0, 0.0]])      # -0.0 and 0.0 differ in their bits
    assert groups_by_input(X).tolist() == [0, 1, 0, 2, 1, 3, 4]
    assert groups_by_input(X, only_hf=True).tolist() == [0, -1, 0, -1, -1, 1, -1]
    assert groups_by_input(X[:, 2:]).tolist() == [0] * 7          # D = 0: one group
    with pytest.raises(ValueError):
        groups_by_input(np.zeros(5))


def test_normalize_groups_forms():
    off, rows, gmax = normalize_groups(None, 5)
    assert off.dtype == np.int32 and rows.dtype == np.int32
    assert off.tolist() == [0, 1, 2, 3, 4, 5] and rows.tolist() == [0, 1, 2, 3, 4] and gmax == 1
    # labels: order of first appearance, ascending inside a group, -1 left in
    for labels in (np.array([7, -1, 2, 7, 2, 2]), [7, -1, 2, 7, 2, 2]):
        off, rows, gmax = normalize_groups(labels, 6)
        assert off.tolist() == [0, 2, 5] and rows.tolist() == [0, 3, 2, 4, 5] and gmax == 3
    off, rows, gmax = normalize_groups(np.full(4, -1), 4)
    assert off.tolist() == [0] and rows.size == 0 and gmax == 0
    # index arrays: sorted inside a group, a row in several groups, a group listed twice
    off, rows, gmax = normalize_groups([[4, 1], np.array([1]), (4, 1), range(2, 5)], 6)
    assert off.tolist() == [0, 2, 3, 5, 8] and rows.tolist() == [1, 4, 1, 1, 4, 2, 3, 4] and gmax == 3
    off, rows, gmax = normalize_groups(np.array([[0, 5], [3, 2]]), 6)   # a 2-D array: one group per row
    assert off.tolist() == [0, 2, 4] and rows.tolist() == [0, 5, 2, 3]
    off, rows, gmax = normalize_groups([np.arange(32)], 40)
    assert gmax == 32
    off, rows, gmax = normalize_groups([], 6)
    assert off.tolist() == [0] and gmax == 0


@pytest.mark.parametrize("groups,match", [
    ([[1], []], "empty"),
    ([np.arange(33)], "at most 32"),
    ([[2, 5, 2]], "twice"),
    ([[0, 6]], "outside"),
    ([[-1, 2]], "outside"),
    (np.array([0, 0, 1]), "one label per training row"),
    (np.array([0, -2, 1, 1, 1, 1]), "labels are >= 0"),
    (np.zeros(40, dtype=np.int64), "at most 32"),
    ([[0.5, 1.0]], "integers"),
    ([np.array([[0, 1], [2, 3]])], "1-D"),
])
def test_normalize_groups_rejects(groups, match):
    n = 40 if isinstance(groups, np.ndarray) and groups.shape == (40,) else 6
    if isinstance(groups, list) and len(groups) == 1 and np.size(groups[0]) == 33:
        n = 40
    with pytest.raises(ValueError, match=match):
        normalize_groups(groups, n)
