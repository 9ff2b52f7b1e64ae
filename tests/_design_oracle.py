"""fp64 CPU references for simulation design from the cached GPR posterior -- TEST INFRASTRUCTURE ONLY.

  closed   the closed form the device evaluates, from the oracle's OWN predict functions on the stacked
           points [Xref ; Xcand]: C = the [ref, cand] block of predict_f(full_cov=True)
           (oracle.mfgp_oracle.gpr_predict_f_full_cov; graph models: oracle.graph_oracle.predict_f_full_cov),
           v = the marginal predict_f variance of the candidates,
           score[c] = sum_r w_r C(r, c)^2 / (v(c) + s2).  THE reference of the GPU tests.
  brute    one oracle refit per candidate with the candidate appended to the training set (the targets
           do not enter a variance: zeros): score[c] = sum_r w_r (var_before(r) - var_after(r)).  What a
           user does today.  Graph models: rescaled to the likelihood variance alone (see the comment there).
  greedy   q rounds of `brute`: argmax(score / cost), lowest index on a tie, the pick appended for good.
           Also returns each step's relative margin between the best and the second-best score / cost.

tests/test_design_host.py holds closed to brute at 1e-12 |ref|max (the identity).  The cases are built here
once and shared by both test files; nothing here runs the code under test.
"""
import functools

import numpy as np
import torch

from oracle import graph_oracle as GO
from oracle import mfgp_oracle as O


def _s2(prm, noise):
    return float(noise) if isinstance(prm, dict) else float(prm.noise)


def _marginal_var(X, Y, Xs, prm, s2):
    if isinstance(prm, dict):
        var = GO.predict_f(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), prm, s2)[1].numpy()
        return var.reshape(Xs.shape[0], -1)[:, 0]
    return O.gpr_predict_f(X, Y, Xs, prm)[1][:, 0]


def _full_cov(X, Y, Xs, prm, s2):
    if isinstance(prm, dict):
        return GO.predict_f_full_cov(torch.tensor(X), torch.tensor(Y), torch.tensor(Xs), prm, s2)[1].numpy()
    return O.gpr_predict_f_full_cov(X, Y, Xs, prm)[1][0]


def _weights(w, nr):
    return np.ones(nr) if w is None else np.asarray(w, dtype=np.float64)


def closed(X, Y, prm, Xref, Xcand, w=None, noise=None):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    s2, nr = _s2(prm, noise), Xref.shape[0]
    Xall = np.vstack([Xref, Xcand])
    C = _full_cov(X, Y, Xall, prm, s2)[:nr, nr:]
    v = _marginal_var(X, Y, Xall, prm, s2)[nr:]
    return (_weights(w, nr)[:, None] * C * C).sum(axis=0) / (v + s2)


def brute(X, Y, prm, Xref, Xcand, w=None, noise=None):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    s2, w = _s2(prm, noise), _weights(w, Xref.shape[0])
    before = _marginal_var(X, Y, Xref, prm, s2)
    zero = np.zeros((1, Y.shape[1]))
    out = np.empty(Xcand.shape[0])
    for c in range(Xcand.shape[0]):
        after = _marginal_var(np.vstack([X, Xcand[c:c + 1]]), np.vstack([Y, zero]), Xref, prm, s2)
        out[c] = np.sum(w * (before - after))
    if isinstance(prm, dict):
        # The graph kernel puts its 1e-6 jitter on the diagonal of K(X, X), so the appended row is observed
        # with variance s2 + 1e-6 in the refit, while the score is defined with the likelihood variance s2
        # alone.  Only the appended row's own diagonal entry is touched, so the refit's drop is the defined
        # one times (v + s2) / (v + s2 + 1e-6) exactly; undo that factor.
        v = _marginal_var(X, Y, Xcand, prm, s2)
        out *= (v + s2 + GO.JITTER) / (v + s2)
    return out


def greedy(X, Y, prm, Xref, Xcand, q, w=None, cost=None, noise=None):
    """(picks [q], gain [q], margin [q]): margin = (best - second best) / best of score / cost at each step
    (inf with a single candidate)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    cost = np.ones(Xcand.shape[0]) if cost is None else np.asarray(cost, dtype=np.float64)
    picks, gain, margin = [], [], []
    for _ in range(q):
        score = brute(X, Y, prm, Xref, Xcand, w, noise)
        ratio = score / cost
        k = int(np.argmax(ratio))
        rest = np.delete(ratio, k)
        margin.append(float((ratio[k] - rest.max()) / ratio[k]) if rest.size else np.inf)
        picks.append(k)
        gain.append(score[k])
        X, Y = np.vstack([X, Xcand[k:k + 1]]), np.vstack([Y, np.zeros((1, Y.shape[1]))])
    return np.array(picks), np.array(gain), np.array(margin)


# ---------------------------------------------------------------- the shared cases
def _points(rng, n, D, first):
    """n points of U[0, 1]^D, the fidelities 0 / 1 alternating from `first`."""
    return np.hstack([rng.random((n, D)), ((np.arange(n) + first) % 2)[:, None].astype(np.float64)])


def costs(Xcand):
    """The select tests' costs: 4 for an HF run, 1 for anything else."""
    return np.where(Xcand[:, -1] == 1.0, 4.0, 1.0)


@functools.lru_cache(maxsize=None)
def case(which):
    """(X, Y, prm, Xref, Xcand, w): the leave-out cases' data and parameters (cond(K + s2 I) < 1e6) with
    seeded reference / candidate sets and U[0, 1) weights.
      n25    Nr = Nc = 1: one tile, one column
      n25s   the same model with Nr = 4, Nc = 5 (the select test needs a choice)
      n79    Nr = Nc = 33: a one-row tail in a second tile on both sides; candidate 5 is bit-equal to
             training row 12; candidate 7 and reference 9 have fidelity 0.5 (contribute exactly 0)
      n180   Nr = 70, Nc = 40 (P = 65, D = 32)
      hbs    HBS at the initial parameters, 33 mixed-fidelity rows near training inputs on both sides"""
    import _input_grad_oracle as G
    import _leave_out_oracle as LO
    X, Y, prm = LO._data("n25" if which == "n25s" else which)
    D = X.shape[1] - 1
    rng = np.random.default_rng({"n25": 25, "n25s": 26, "n79": 79, "n180": 180, "hbs": 53}[which])
    if which == "hbs":
        Xref, Xcand = G.mixed_rows(X, 33, 3), G.mixed_rows(X, 33, 5)
    else:
        nr, nc = {"n25": (1, 1), "n25s": (4, 5), "n79": (33, 33), "n180": (70, 40)}[which]
        Xref, Xcand = _points(rng, nr, D, 1), _points(rng, nc, D, 0)
    if which == "n25":
        # one HF candidate 0.01 from the one HF reference: a score of the order of the variance itself, so
        # that the refit's difference of two variances (absolute error ~ eps var) resolves it to 1e-12
        Xcand = Xref.copy()
        Xcand[0, 0] += 0.01
    if which == "n79":
        Xcand[5] = X[12]
        Xcand[7, -1] = 0.5
        Xref[9, -1] = 0.5
    return X, Y, prm, Xref, Xcand, rng.random(Xref.shape[0])


@functools.lru_cache(maxsize=None)
def reference(which, weighted=True):
    """closed of one case, computed once (read-only for its users)."""
    X, Y, prm, Xref, Xcand, w = case(which)
    return closed(X, Y, prm, Xref, Xcand, w if weighted else None)


@functools.lru_cache(maxsize=None)
def greedy_reference(which, q=4):
    X, Y, prm, Xref, Xcand, w = case(which)
    return greedy(X, Y, prm, Xref, Xcand, q, w, costs(Xcand))


def graph_points(m, D, nr=20, nc=21, seed=11):
    """Reference / candidate sets of the graph tests: sources 0..m cycling, one candidate of fidelity 0.5."""
    rng = np.random.default_rng(seed)
    Xref = np.hstack([rng.random((nr, D)), (np.arange(nr) % (m + 1))[:, None].astype(np.float64)])
    Xcand = np.hstack([rng.random((nc, D)), ((np.arange(nc) + 1) % (m + 1))[:, None].astype(np.float64)])
    Xcand[4, -1] = 0.5
    return Xref, Xcand, rng.random(nr)
