"""Cached posteriors: GPflow's ``model.posterior()`` for the four fp64 models.

``model.posterior()`` freezes the model's parameters and training data and does the work of
``predict_f`` that does not depend on ``Xnew`` once (include/mfgp.h ``mfgp_gpr_posterior_build`` /
``mfgp_svgp_posterior_build``: Gram, factorization, inverse factor, projected targets).  The returned
object's ``predict_f`` then runs only ``mfgp_*_posterior_predict`` against that device block: two
launches, no Gram of X, no factorization, no parameter upload and no host read of a device word.

The cache is a *snapshot*: assigning to the model or training it does not change what the cached
``predict_f`` returns until ``update_cache()`` is called.  ``fused_predict_f`` never uses the cache:
it is the model's own ``predict_f`` at the model's current parameters.

Input gradients: ``predict_f_vjp(Xnew, grad_mean, grad_var)`` returns the marginal prediction and the
vector-Jacobian product with respect to ``Xnew`` from one call (``mfgp_*_posterior_predict_vjp``: the
predict call's two launches and one more), and the cached marginal ``predict_f`` of a torch ``Xnew``
with ``requires_grad=True`` is attached to autograd through it.  The fidelity column of ``Xnew``
enters the kernels only through exact ``== 0`` / ``== 1`` tests, so its gradient is exactly zero.

Simulation design: ``GPRPosterior.variance_reduction(Xcand, Xref, weights)`` scores every candidate run by
the posterior variance it buys down over a reference set, and ``GPRPosterior.select`` picks a greedy batch
by ``argmax(score / cost)``, both in closed form from the cached factors (``mfgp_gpr_posterior_design_score``
/ ``_append``: the reference x candidate covariance block is formed on chip, never in memory).

New simulations: ``GPRPosterior.condition_on(Xadd, Yadd)`` returns the posterior of the stacked data at the
snapshot's hyper-parameters from the cached factors (``mfgp_gpr_posterior_append``: a block append in
O(N^2 k), no Gram, no factorization of K); ``fantasize(Xadd)`` conditions on rows that have no value yet.

Joint draws: ``predict_f_samples(Xnew, num_samples)`` is GPflow's ``sample_mvn`` on the device
(``mfgp_mvn_sample``: a tile Cholesky of the predictive covariance that keeps L, then ``mean + L eps`` on
the matrix core).  A GPR posterior factors its one [N*, N*] block once for all P outputs; an SVGP posterior
factors the snapshot's [P, N*, N*].  ``eps=`` passes the standard-normal input (a deterministic call);
the four models have the same method at their current parameters.

Inference: ``log_density(Xnew, Y, obs_cov, obs_var, grad)`` is the emulator log-likelihood of one data vector
(or one per row) at every row of ``Xnew`` -- a batch of MCMC / HMC walkers -- and its exact input gradient, from
one call (``mfgp_*_posterior_logdens``: the forward once, a batched [P, P] density kernel in LDS
(``mfgp_mvn_logpdf``), then the VJP kernel fed the density's own gradients).  ``predict_log_density`` is GPflow's
method of that name on the marginal prediction, for the four models and both posterior classes.

First-order objects: ``mean_jacobian(Xnew)`` is the Jacobian of the emulated data vector w.r.t. the input
parameters, [N*, P, D], from one call (``mfgp_*_jacobian``: the forward once, then one product against
``alpha = K^{-1} Y`` with dK/dx generated on chip), and ``fisher(Xnew, obs_cov, obs_var)`` the Fisher
(Gauss-Newton) matrix ``J^T Sigma^{-1} J`` per row built from it (``mfgp_mvn_fisher``: the [P, P] factorization in
LDS carries the rows of J^T along, so F falls out of it): what forecasts, Laplace approximations and HMC
preconditioning are built from.
"""
from __future__ import annotations

import enum
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import MFGPError, info_error
from .engine import Engine, to_dev
from .params import as_result
from .session import CholeskyError


class PrecomputeCacheType(enum.Enum):
    """How a posterior keeps its precomputed quantities (the GPflow names).

    TENSOR: ``update_cache()`` may allocate new device buffers.  VARIABLE: ``update_cache()``
    rewrites the same device buffers (stable pointers, no reallocation while the shapes are
    unchanged).  NOCACHE: nothing is precomputed and ``predict_f`` is ``fused_predict_f``."""
    TENSOR = "tensor"
    VARIABLE = "variable"
    NOCACHE = "nocache"


def _cache_type(value) -> PrecomputeCacheType:
    if value is None:
        return PrecomputeCacheType.NOCACHE
    if isinstance(value, PrecomputeCacheType):
        return value
    return PrecomputeCacheType(str(value).lower())


def _wants_grad(Xnew) -> bool:
    return isinstance(Xnew, torch.Tensor) and Xnew.requires_grad and torch.is_grad_enabled()


def _upstream(g, shape, device, what):
    """An upstream gradient as a dense device tensor of `shape` (None stays None: zero)."""
    if g is None:
        return None
    g = to_dev(g, device)
    if tuple(g.shape) != tuple(shape):
        raise ValueError(f"predict_f_vjp: {what} has shape {tuple(g.shape)}, expected {tuple(shape)}")
    return g


DEFAULT_SAMPLE_JITTER = 1e-6   # gpflow.default_jitter(), what sample_mvn adds before its Cholesky


def sample_plan(what, Xnew, p, num_samples, full_cov, full_output_cov, eps, jitter):
    """The argument checks of predict_f_samples, all on the host before any device work:
    ``(S, N*)`` with S the number of draws computed (1 for ``num_samples=None``).  NotImplementedError
    for the output-covariance forms, ValueError for a bad ``num_samples`` / ``eps`` shape / ``jitter``."""
    if full_cov and full_output_cov:
        raise NotImplementedError(f"{what}: the combination of both full_cov and full_output_cov is not "
                                  "permitted.")
    if full_output_cov:
        raise NotImplementedError(f"{what}(full_output_cov=True): draws from the [N*, P, P] output covariance "
                                  "are not built; use full_cov=True or the marginal form")
    if num_samples is not None:
        if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)):
            raise ValueError(f"{what}: num_samples must be an integer >= 1 or None, got {num_samples!r}")
        if num_samples < 1:
            raise ValueError(f"{what}: num_samples must be >= 1, got {num_samples}")
    if isinstance(jitter, bool) or not isinstance(jitter, (int, float, np.integer, np.floating)) or not jitter >= 0:
        raise ValueError(f"{what}: jitter must be a number >= 0, got {jitter!r}")
    shape = tuple(Xnew.shape) if isinstance(Xnew, torch.Tensor) else np.shape(Xnew)
    if len(shape) != 2:
        raise ValueError(f"{what}: Xnew has shape {shape}, expected [N*, D + 1]")
    ns = int(shape[0])
    S = 1 if num_samples is None else int(num_samples)
    if eps is not None:
        eshape = tuple(eps.shape) if isinstance(eps, torch.Tensor) else np.shape(eps)
        if num_samples is None:
            if eshape != (ns, p):
                raise ValueError(f"{what}: eps has shape {eshape}, expected ({ns}, {p}) with num_samples=None")
        elif len(eshape) != 3 or eshape[1:] != (ns, p):
            raise ValueError(f"{what}: eps has shape {eshape}, expected ({S}, {ns}, {p})")
        elif eshape[0] != S:
            raise ValueError(f"{what}: eps holds {eshape[0]} draws, num_samples is {S}")
    return S, ns


def sample_eps(eng: Engine, eps, S, ns, p, generator):
    """The standard-normal input [S, N*, P] on the engine's device: the caller's, or torch.randn."""
    if eps is None:
        return torch.randn((S, ns, p), dtype=torch.float64, device=eng.device, generator=generator)
    return to_dev(eps, eng.device).reshape(S, ns, p)


def sample_marginal(mean, var, eps, squeeze):
    """sample_mvn(full_cov=False): mean + sqrt(var) eps (no jitter, no clamp of var)."""
    out = mean.as_subclass(torch.Tensor)[None] + torch.sqrt(var.as_subclass(torch.Tensor))[None] * eps
    return as_result(out[0] if squeeze else out)


def sample_joint(eng: Engine, what, mean, cov, eps, ncol, jitter, squeeze, pre=None):
    """sample_mvn(full_cov=True) on the device (Engine.mvn_sample): cov [B, N*, N*], B * ncol = P.  The
    call's one host read is info, after everything is enqueued (`pre`: the info words of the call that
    produced cov, read with it)."""
    out, info = eng.mvn_sample(cov, mean, eps, ncol, jitter)
    nb = info.shape[0]
    bad = (info if pre is None else torch.cat([info, pre.reshape(-1)])).cpu().numpy()
    if np.any(bad[nb:] != 0):
        err = info_error(int(bad[nb:][np.flatnonzero(bad[nb:])[0]]), what)
        raise err if pre.numel() == 1 else CholeskyError(f"{what}: Cholesky of K_uu was not successful")
    bad = bad[:nb]
    if np.any(bad != 0):
        b = int(np.flatnonzero(bad)[0])
        where = f" of output {b}" if cov.shape[0] > 1 else ""
        raise CholeskyError(f"{what}: Cholesky decomposition of the predictive covariance{where} was not "
                            f"successful (non-positive pivot at row {int(bad[b])}); the input might not be valid.")
    return as_result(out[0] if squeeze else out)


def draw_f_samples(p, inputs, marginal, joint, Xnew, num_samples, full_cov, full_output_cov, eps, generator, jitter):
    """predict_f_samples of a posterior or a model with P = p outputs.  ``inputs() -> (engine, Xnew on the
    device, detached)`` is called after the argument checks; ``marginal(Xs) -> (mean, var)`` is its marginal
    predict_f; ``joint(engine, Xs) -> (mean [N*, P], cov [B, N*, N*], ncol, info words of that call or
    None)`` its covariance entry point with B * ncol = P."""
    what = "predict_f_samples"
    S, ns = sample_plan(what, Xnew, p, num_samples, full_cov, full_output_cov, eps, jitter)
    eng, Xs = inputs()   # every ValueError of the arguments is raised above
    e = sample_eps(eng, eps, S, ns, p, generator)
    if not full_cov:
        mean, var = marginal(Xs)
        return sample_marginal(mean, var, e, num_samples is None)
    mean, cov, ncol, pre = joint(eng, Xs)
    return sample_joint(eng, what, mean, cov, e, ncol, jitter, num_samples is None, pre)


MAX_DENSE_OUTPUTS = 128   # outputs of the dense log-density form (include/mfgp.h mfgp_mvn_logpdf: p <= 128)


class LogDensityResult(NamedTuple):
    """What ``log_density`` returns (device tensors, detached)."""
    logp: torch.Tensor                      # [N*] log N(Y | mean, diag(var + obs_var) + obs_cov)
    mean: torch.Tensor                      # [N*, P] predict_f's mean (the same bits)
    var: torch.Tensor                       # [N*, P] predict_f's marginal variance (the same bits)
    grad_X: Optional[torch.Tensor] = None   # [N*, D + 1] d logp / d Xnew (fidelity column 0), with grad=True


def _shape_of(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)


def _on_host(x) -> bool:
    return not (isinstance(x, torch.Tensor) and x.device.type != "cpu")


def density_plan(what, ns, p, Y, obs_var, obs_cov):
    """The argument checks of log_density's Y / obs_var / obs_cov, all on the host before any device work.
    ValueError for a Y that is not [P] or [N*, P], an obs_var that is no scalar, [P] or
    [N*, P] or holds a negative (or NaN) entry, an obs_cov that is not [P, P], or P > 128 with obs_cov.
    (The sign of an obs_var that already lives on the device is not read back: a non-positive total
    variance shows in the call's info.)"""
    ys = _shape_of(Y)
    if ys != (p,) and ys != (ns, p):
        raise ValueError(f"{what}: Y has shape {ys}, expected ({p},) or ({ns}, {p})")
    if obs_var is not None:
        vs = _shape_of(obs_var)
        if vs not in ((), (p,), (ns, p)):
            raise ValueError(f"{what}: obs_var has shape {vs}, expected a scalar, ({p},) or ({ns}, {p})")
        if _on_host(obs_var):
            v = obs_var.detach().numpy() if isinstance(obs_var, torch.Tensor) else np.asarray(obs_var, dtype=np.float64)
            if not np.all(v >= 0):
                raise ValueError(f"{what}: obs_var must be non-negative (and not NaN)")
    if obs_cov is not None:
        cs = _shape_of(obs_cov)
        if cs != (p, p):
            raise ValueError(f"{what}: obs_cov has shape {cs}, expected ({p}, {p})")
        if p > MAX_DENSE_OUTPUTS:
            raise ValueError(f"{what}: the dense form (obs_cov) is built for P <= {MAX_DENSE_OUTPUTS} outputs, "
                             f"got {p}; pass a diagonal obs_var instead")


def density_inputs(eng: Engine, p, Y, obs_var, obs_cov):
    """(Y, obs_var, obs_cov) as fp64 device tensors (a scalar obs_var becomes [P]; an fp64 device obs_cov is
    passed as it is, strides and all)."""
    Yd = to_dev(Y, eng.device)
    ov = None
    if obs_var is not None:
        ov = to_dev(obs_var, eng.device)
        if ov.dim() == 0:
            ov = ov.expand(p).contiguous()
    oc = None
    if obs_cov is not None:
        if isinstance(obs_cov, torch.Tensor) and obs_cov.device == eng.device and obs_cov.dtype == torch.float64:
            oc = obs_cov.detach()
        else:
            oc = to_dev(obs_cov, eng.device)
    return Yd, ov, oc


def raise_density_info(what, info, dense):
    """The one host read of a log-density call, after everything is enqueued."""
    bad = info.cpu().numpy()
    if np.any(bad != 0):
        s = int(np.flatnonzero(bad)[0])
        kind = ("the Cholesky decomposition of its covariance was not successful" if dense
                else "its total variance is not positive")
        raise CholeskyError(f"{what}: row {s}: {kind} (or its residual is not finite) at output {int(bad[s]) - 1}; "
                            "the input might not be valid.")


def predict_log_density_of(model, predict_f, data, full_cov=False, full_output_cov=False):
    """GPflow ``GPModel.predict_log_density`` with the Gaussian likelihoods of this package: the marginal
    ``predict_f`` at Xnew, then ``sum_c log N(Y[s, c] | mean[s, c], var[s, c] + s2[s, c])`` on the device
    (mfgp_mvn_logpdf, the diagonal form), [N*].  s2 is the likelihood variance of ``model`` now:
    ``Gaussian`` its scalar; ``HeteroscedasticGaussian`` the baseline for [N*, P] targets and baseline +
    Y_unc**2 for [N*, 2P] targets [Y_obs | Y_unc]; ``MaskedGaussian`` each output's own, NaN targets left
    out (any other likelihood: a NaN target gives a NaN row, as GPflow's does)."""
    from .models import HeteroscedasticGaussian, MaskedGaussian
    what = "predict_log_density"
    if full_cov or full_output_cov:
        raise NotImplementedError("The predict_log_density method currently supports only the argument values "
                                  "full_cov=False and full_output_cov=False")
    try:
        Xnew, Ynew = data
    except (TypeError, ValueError):
        raise ValueError(f"{what}: data must be the pair (Xnew, Ynew)") from None
    lik = model.likelihood
    p = int(getattr(model, "num_outputs", None) or model.num_output_dims)
    xs, ys = _shape_of(Xnew), _shape_of(Ynew)
    if len(xs) != 2:
        raise ValueError(f"{what}: Xnew has shape {xs}, expected [N*, D + 1]")
    ns = int(xs[0])
    het = isinstance(lik, HeteroscedasticGaussian)
    masked = isinstance(lik, MaskedGaussian)
    if ys != (ns, p) and not (het and ys == (ns, 2 * p)) and not (p == 1 and ys == (ns,)):
        want = f"({ns}, {p})" + (f" or ({ns}, {2 * p})" if het else "")
        raise ValueError(f"{what}: Ynew has shape {ys}, expected {want}")
    s2 = np.ascontiguousarray(np.reshape(lik.variance.numpy(), -1), dtype=np.float64)
    if s2.size not in (1, p):
        raise ValueError(f"{what}: the likelihood variance has {s2.size} entries, expected 1 or {p}")
    mean, var = predict_f(Xnew)   # every ValueError of the arguments is raised above
    mean = mean.as_subclass(torch.Tensor).detach().to(torch.float64)   # (an fp32 model: cast for this call)
    var = var.as_subclass(torch.Tensor).detach().to(torch.float64)
    eng = Engine.get(mean.device)
    Yd = to_dev(Ynew, eng.device).reshape(ns, -1)
    ov = to_dev(np.broadcast_to(s2, (p,)).copy(), eng.device)
    if het and Yd.shape[1] == 2 * p:
        ov = ov[None, :] + Yd[:, p:] ** 2
        Yd = Yd[:, :p]
    logp, _, _, info = eng.mvn_logpdf(mean, Yd, var, obs_var=ov)
    if not masked:
        logp = torch.where(torch.isnan(Yd).any(dim=1), torch.full_like(logp, float("nan")), logp)
    raise_density_info(what, info, False)
    return as_result(logp)


FISHER_LDS_BYTES = 160 * 1024   # the dense Fisher form's LDS image must fit one compute unit (include/mfgp.h mfgp_mvn_fisher)


class FisherResult(NamedTuple):
    """What ``fisher`` returns (device tensors, detached)."""
    fisher: torch.Tensor      # [N*, D, D] J_s^T (diag(var_s + obs_var_s) + obs_cov)^{-1} J_s, exactly symmetric
    mean: torch.Tensor        # [N*, P] predict_f's mean (the same bits)
    var: torch.Tensor         # [N*, P] predict_f's marginal variance (the same bits)
    jacobian: torch.Tensor    # [N*, P, D] d mean / d Xnew, what mean_jacobian returns


def fisher_dense_fits(p: int, d: int) -> bool:
    """Whether the dense Fisher form is built for P = p outputs and D = d inputs: P <= 128 and the LDS image of
    (P8 + D) x ((P8 + D) | 1) doubles, P8 = P rounded up to 8, within the 160 KiB of a compute unit
    (P8 + D <= 143: D <= 15 at P = 128, any D <= 32 up to P = 104)."""
    r = ((int(p) + 7) & ~7) + int(d)
    return p <= MAX_DENSE_OUTPUTS and r * (r | 1) * 8 <= FISHER_LDS_BYTES


def fisher_plan(what, ns, p, d, obs_var, obs_cov):
    """The argument checks of fisher's obs_var / obs_cov, on the host before any device work: density_plan's
    (the same forms as log_density), then the dense form's limit."""
    density_plan(what, ns, p, np.empty((p,)), obs_var, obs_cov)
    if obs_cov is not None and not fisher_dense_fits(p, d):
        raise ValueError(f"{what}: the dense form (obs_cov) is built for P <= {MAX_DENSE_OUTPUTS} outputs and "
                         f"P8 + D <= 143 (P8 = P rounded up to 8; the [P8 + D]^2 image must fit the 160 KiB of LDS), "
                         f"got P = {p}, D = {d}; pass a diagonal obs_var instead")


MAX_GROUP = 32   # rows of one left-out group (include/mfgp.h mfgp_gpr_posterior_leave_out: gmax <= 32)


class LeaveOutResult(NamedTuple):
    """What ``GPRPosterior.leave_out`` returns: R rows over G groups, group after group."""
    rows: np.ndarray            # int64 [R] training-row indices, ascending within a group
    group: np.ndarray           # int64 [R] the group each returned row belongs to
    mean: torch.Tensor          # [R, P] held-out mean
    var: torch.Tensor           # [R, P] marginal variance of f, tiled over P as predict_f tiles it
    log_density: torch.Tensor   # [G, P] joint log predictive density of each group's observations
    cov: Optional[torch.Tensor] = None   # [G, gmax, gmax] covariance of f_S, zero outside each group's block


MAX_BATCH = 32   # picks of one greedy batch (include/mfgp.h mfgp_gpr_posterior_design_score: k <= 32)


MAX_APPEND = 32  # rows of one condition_on call (include/mfgp.h mfgp_gpr_posterior_append: k <= 32)


class DesignResult(NamedTuple):
    """What ``GPRPosterior.select`` returns: the greedy batch, pick after pick (device tensors)."""
    picks: torch.Tensor   # int64 [q] rows of Xcand, in the order they were picked (a row may repeat)
    gain: torch.Tensor    # [q] the score (not divided by the cost) of each pick at its step


def _design_rows(X, d, what):
    """Row count of an [N, d + 1] input (numpy / list / torch), ValueError otherwise; host only."""
    shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
    if len(shape) != 2 or shape[1] != d + 1:
        raise ValueError(f"{what} has shape {shape}, expected [N, {d + 1}] (D inputs and the fidelity column)")
    return int(shape[0])


def _design_vector(v, n, what, positive):
    """weights (>= 0) / cost (> 0) as a float64 tensor of n entries where it lives, checked before any
    device work of the call (for a device tensor that check is the call's one host read)."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        t = v.detach().to(torch.float64)
    else:
        t = torch.as_tensor(np.asarray(v, dtype=np.float64))
    if tuple(t.shape) != (n,):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected ({n},)")
    if not bool(((t > 0) if positive else (t >= 0)).all()):
        raise ValueError(f"{what} must be {'positive' if positive else 'non-negative'} (and not NaN)")
    return t


def _index_array(g, what):
    a = np.asarray(g)
    if a.size and (a.dtype == bool or not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"leave_out: {what} must hold integers, got dtype {a.dtype}")
    return a.astype(np.int64)


def _too_large(k, size):
    return ValueError(f"leave_out: group {k} has {size} rows; at most {MAX_GROUP} rows can be left out together")


def _groups_from_labels(labels, n):
    """Rows with equal labels >= 0, in order of first appearance (vectorised: at Goku a Python loop over
    the 1164 labels cost more than the device call)."""
    labels = _index_array(labels, "the label array").reshape(-1)
    if labels.shape[0] != n:
        raise ValueError(f"leave_out: a label array needs one label per training row ({n}), got {labels.shape[0]}")
    if labels.size and labels.min() < -1:
        raise ValueError("leave_out: labels are >= 0, or -1 for a row that is never left out")
    idx = np.flatnonzero(labels >= 0)
    if idx.size == 0:
        return np.zeros((1,), dtype=np.int32), np.zeros((0,), dtype=np.int32), 0
    _, first, inv = np.unique(labels[idx], return_index=True, return_inverse=True)
    rank = np.empty_like(first)
    rank[np.argsort(first)] = np.arange(first.size)   # label -> its place by first appearance
    gid = rank[inv.reshape(-1)]
    sizes = np.bincount(gid)
    if sizes.max() > MAX_GROUP:
        k = int(np.argmax(sizes > MAX_GROUP))
        raise _too_large(k, int(sizes[k]))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return offsets, idx[np.argsort(gid, kind="stable")].astype(np.int32), int(sizes.max())


def _groups_from_lists(groups, n):
    lists = []
    for k, g in enumerate(groups):
        a = _index_array(g, f"group {k}")
        if a.ndim != 1:
            raise ValueError(f"leave_out: group {k} is not a 1-D index array")
        a = np.sort(a)
        if a.size == 0:
            raise ValueError(f"leave_out: group {k} is empty")
        if a.size > MAX_GROUP:
            raise _too_large(k, a.size)
        if a[0] < 0 or a[-1] >= n:
            raise ValueError(f"leave_out: group {k} holds an index outside 0..{n - 1}")
        if np.any(a[1:] == a[:-1]):
            raise ValueError(f"leave_out: group {k} lists a row twice")
        lists.append(a)
    if not lists:
        return np.zeros((1,), dtype=np.int32), np.zeros((0,), dtype=np.int32), 0
    sizes = np.array([a.size for a in lists], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return offsets, np.concatenate(lists).astype(np.int32), int(sizes.max())


def normalize_groups(groups, n: int):
    """The three accepted forms of ``groups`` as ``(offsets [G + 1], rows [R], gmax)``, int32 host
    arrays laid out as mfgp_gpr_posterior_leave_out reads them: group g is ``rows[offsets[g]:
    offsets[g + 1]]``, ascending.  None: every one of the n rows is its own group.  A 1-D integer
    array (or flat list) of n labels: rows with equal labels >= 0 form a group, in order of first
    appearance; -1 keeps a row out of every group.  A sequence of index arrays (or a 2-D array, one
    group a row): one group each; a row may appear in several groups.  ValueError for an empty group,
    more than 32 rows in a group, a duplicate index inside a group or an index outside 0..n-1.  Pure
    host code."""
    n = int(n)
    if groups is None:
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1 if n else 0
    if isinstance(groups, torch.Tensor):
        groups = groups.detach().cpu().numpy()
    if isinstance(groups, np.ndarray) and groups.dtype != object:
        flat = groups.ndim == 1
    else:
        flat = len(groups) > 0 and all(np.ndim(g) == 0 for g in groups)
    return _groups_from_labels(groups, n) if flat else _groups_from_lists(groups, n)


def groups_by_input(X, only_hf: bool = False) -> np.ndarray:
    """Labels [N] that group the rows of X ([N, D + 1], fidelity in the last column) whose D input
    columns are bit-identical, numbered in order of first appearance: the ``groups`` argument of
    ``GPRPosterior.leave_out`` that leaves a high-fidelity simulation out together with the
    low-fidelity runs at the same input.  only_hf: groups without a row of fidelity 1 get label -1
    (never left out), the others are numbered in order of first appearance.  Host numpy code."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("groups_by_input: X must be [N, D + 1]")
    seen, raw = {}, np.empty((X.shape[0],), dtype=np.int64)
    for i in range(X.shape[0]):
        raw[i] = seen.setdefault(X[i, :-1].tobytes(), len(seen))
    if not only_hf:
        return raw
    keep = np.zeros((len(seen),), dtype=bool)
    keep[raw[X[:, -1] == 1.0]] = True
    renum = np.full((len(seen),), -1, dtype=np.int64)
    renum[keep] = np.arange(int(keep.sum()))
    return renum[raw]


class _PredictFn(torch.autograd.Function):
    """The cached marginal predict_f as an autograd node: backward is the VJP call on the cache block
    the forward ran on (a TENSOR cache replaced by update_cache() in between stays alive here)."""

    @staticmethod
    def forward(ctx, Xnew, post):
        ctx.post, ctx.cache = post, post.cache
        ctx.save_for_backward(Xnew)
        mean, var = post._marginal(Xnew)
        return mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mean, grad_var):
        (Xnew,) = ctx.saved_tensors
        _, _, gX = ctx.post._predict(ctx.cache, Xnew, grad=(grad_mean, grad_var))
        return gX.to(device=Xnew.device, dtype=Xnew.dtype), None


class _Posterior:
    """Shared surface: predict_f / predict_f_vjp / fused_predict_f / update_cache and the cache buffer
    policy."""

    def __init__(self, model, precompute_cache):
        self.model = model
        self._precompute_cache = None
        self.cache = None        # the device block (uint8 tensor), None without a cache
        self._valid = False
        self.update_cache(_cache_type(precompute_cache))

    def fused_predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """The model's own predict_f at the model's CURRENT parameters (never the cache)."""
        return self.model.predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)

    def update_cache(self, precompute_cache=None):
        """Re-snapshot the model's parameters and data (None: keep the cache type).  A failed
        factorization raises CholeskyError here; a VARIABLE cache is then unusable until an
        update succeeds, a TENSOR one keeps its previous contents."""
        if precompute_cache is not None:
            self._precompute_cache = _cache_type(precompute_cache)
        self._jac_weights = None   # they belong to the block's contents: a VARIABLE cache is rewritten in place
        if self._precompute_cache is PrecomputeCacheType.NOCACHE:
            self.cache, self._valid = None, False
            return
        self._build()

    def _cache_buffer(self, eng: Engine, nbytes: int) -> torch.Tensor:
        """VARIABLE: the existing block while it is large enough; otherwise a new one."""
        if (self._precompute_cache is PrecomputeCacheType.VARIABLE and self.cache is not None
                and self.cache.numel() >= nbytes and self.cache.device == eng.device):
            return self.cache
        return torch.empty(int(nbytes), dtype=torch.uint8, device=eng.device)

    def _commit(self, buf: torch.Tensor, info: torch.Tensor, what: str):
        """Build-time check of the factorization (the only host read of info): raise, or adopt buf."""
        bad = int(info.max().item()) if info.numel() > 1 else int(info.reshape(-1)[0].item())
        if bad != 0:
            if buf is self.cache:
                self._valid = False
            if info.numel() > 1:
                raise CholeskyError(f"{what}: Cholesky of K_uu was not successful")
            raise info_error(bad, what)
        self.cache, self._valid = buf, True
        self._jac_weights = None

    def predict_f_vjp(self, Xnew, grad_mean, grad_var=None):
        """The marginal predict_f at the snapshot and its vector-Jacobian product w.r.t. Xnew:
        ``(mean, var, grad_X)`` with ``grad_X[s, k] = sum_c grad_mean[s, c] dmean[s, c] / dXnew[s, k]
        + sum_c grad_var[s, c] dvar[s, c] / dXnew[s, k]``, shape [N*, D + 1], fidelity column exactly 0.
        ``grad_mean`` / ``grad_var`` are [N*, P] (None: zero; GPR also takes ``grad_var`` [N*], the
        gradient w.r.t. the one variance column that predict_f tiles over P).  mean / var carry
        predict_f's bits.  Like predict_f it is the snapshot's until update_cache()."""
        self._need_cache("predict_f_vjp: a NOCACHE posterior has no cached factors to differentiate through; use a "
                         "TENSOR or VARIABLE cache")
        self._check_vjp()
        mean, var, gX = self._predict(self.cache, Xnew, grad=(grad_mean, grad_var))
        return as_result(mean), as_result(var), as_result(gX)

    def predict_f_samples(self, Xnew, num_samples=None, full_cov: bool = True, full_output_cov: bool = False, *,
                          eps=None, generator=None, jitter: float = DEFAULT_SAMPLE_JITTER):
        """GPflow ``GPModel.predict_f_samples`` at the snapshot: joint draws of f(Xnew), [S, N*, P], or one
        draw [N*, P] with ``num_samples=None``.

        ``full_cov=True``: ``sample[s, :, p] = mean[:, p] + cholesky(cov_p + jitter I) @ eps[s, :, p]``
        (``sample_mvn``; the lower factor of the lower triangle, ``jitter = default_jitter() = 1e-6``),
        factored and multiplied on the device by mfgp_mvn_sample: no [P, N*, N*] copy of a GPR's one block,
        no rocSOLVER call.  ``full_cov=False``: ``mean + sqrt(var) * eps`` on the marginal predict_f (no
        jitter, no clamp of var).  ``full_output_cov=True`` raises NotImplementedError (with ``full_cov``
        as GPflow does; alone because draws from the [N*, P, P] form are not built).

        ``eps`` is the standard-normal input, [S, N*, P] ([N*, P] with ``num_samples=None``; numpy, list or
        device tensor): a given ``eps`` makes the call deterministic.  ``None``: ``torch.randn`` on the
        engine's device with ``generator``.  ValueError before any device work for a wrong ``eps`` shape,
        a ``num_samples`` that is no integer >= 1 or disagrees with ``eps``, ``jitter < 0``.  The call's
        one host read is the factorization's info, after everything is enqueued: CholeskyError with the
        pivot (SVGP: and the output) when a covariance is not positive definite, e.g. a NaN input row.

        The samples carry no autograd history: an Xnew with ``requires_grad`` returns detached samples.
        A NOCACHE posterior delegates to the model (its current parameters)."""
        if self._precompute_cache is PrecomputeCacheType.NOCACHE:
            return self.model.predict_f_samples(Xnew, num_samples, full_cov, full_output_cov, eps=eps,
                                                generator=generator, jitter=jitter)
        def inputs():
            eng = self._engine()
            return eng, to_dev(Xnew, eng.device)
        return draw_f_samples(self._num_outputs(), inputs, self.predict_f, self._joint, Xnew, num_samples, full_cov,
                              full_output_cov, eps, generator, jitter)

    def log_density(self, Xnew, Y, obs_cov=None, obs_var=None, grad: bool = False) -> LogDensityResult:
        """The emulator log-likelihood at the snapshot, one value per row of Xnew (one walker each):
        ``logp[s] = log N(Y_s | mean(Xnew_s), diag(var(Xnew_s) + obs_var_s) + obs_cov)``, and with
        ``grad=True`` its exact gradient w.r.t. Xnew, all from one call on the cache block
        (mfgp_*_posterior_logdens: the predict call's two launches, one density launch that factors the
        [P, P] covariance of every row in LDS, and k_post_grad fed the density's own gradients; the forward
        runs once, no [N*, P, P] tensor, no rocSOLVER call, no autograd graph).

        ``Y`` is [P] (one data vector for every row) or [N*, P]; ``obs_var`` a scalar, [P] or [N*, P];
        ``obs_cov`` [P, P] symmetric positive definite (its lower triangle is read), P <= 128.  Both may
        be given and are added.  The emulator's own likelihood noise is NOT added: this is the density of
        f, pass what the data carry in ``obs_var``.  Without ``obs_cov`` the diagonal form runs (any P);
        there a NaN target is a missing output and is left out.

        Returns ``LogDensityResult(logp [N*], mean [N*, P], var [N*, P], grad_X [N*, D + 1] or None)``,
        detached; mean / var carry predict_f's bits, grad_X is bitwise ``predict_f_vjp`` fed the density's
        gradients, its fidelity column exactly 0.  ValueError before any device work for a wrong shape,
        P > 128 with obs_cov or a negative obs_var; NotImplementedError for a NOCACHE posterior and for
        ``grad=True`` on the graph model, as predict_f_vjp.  The call's one host read is info, after
        everything is enqueued: CholeskyError naming the row whose covariance is not positive definite or
        whose residual is not finite (e.g. a NaN input row)."""
        what = "log_density"
        self._need_cache(f"{what}: a NOCACHE posterior has no cached factors; use a TENSOR or VARIABLE cache")
        if grad:
            self._check_vjp()
        p, d = self._num_outputs(), self._input_dim()
        ns = _design_rows(Xnew, d, f"{what}: Xnew")
        density_plan(what, ns, p, Y, obs_var, obs_cov)
        eng = self._engine()   # every ValueError of the arguments is raised above
        Xs = to_dev(Xnew, eng.device)
        Yd, ov, oc = density_inputs(eng, p, Y, obs_var, obs_cov)
        mean, var, logp, gX, info = self._logdens(eng, Xs, Yd, ov, oc, bool(grad))
        raise_density_info(what, info, oc is not None)
        return LogDensityResult(as_result(logp), as_result(mean), as_result(var),
                                None if gX is None else as_result(gX))

    def mean_jacobian(self, Xnew):
        """The marginal predict_f at the snapshot and the Jacobian of its mean w.r.t. Xnew, from one call:
        ``(mean [N*, P], var [N*, P], jac [N*, P, D])`` with ``jac[s, c, k] = d mean[s, c] / d Xnew[s, k]`` over
        the D input columns only (the fidelity column enters through exact ``== 0`` / ``== 1`` tests, has no
        derivative and no slot).  mfgp_*_jacobian: the predict call's own forward (mean / var carry predict_f's
        bits; it runs once) and one product against ``alpha = K^{-1} Y`` (SVGP: ``Lm^{-T} q_mu`` per latent)
        with dK/dx generated on chip -- not P one-hot ``predict_f_vjp`` calls.  ``jac`` is a transposed VIEW
        of the device layout [N*, D, P] (outputs fastest, what the kernel writes coalesced and ``fisher``
        reads): call ``.contiguous()`` for a dense [N*, P, D].  ``alpha`` is computed on first use and kept
        beside the cache block until ``update_cache()``.  Detached, deterministic (the same inputs give the
        same bits); no host read of a device word.  ValueError for a wrong Xnew shape, NotImplementedError for
        a NOCACHE posterior and for the graph model (as predict_f_vjp), all before any device work.  N* = 0
        returns empty tensors without a launch."""
        what = "mean_jacobian"
        self._need_cache(f"{what}: a NOCACHE posterior has no cached factors; use a TENSOR or VARIABLE cache")
        self._check_vjp()
        _design_rows(Xnew, self._input_dim(), f"{what}: Xnew")
        eng = self._engine()   # every ValueError of the arguments is raised above
        mean, var, J = self._jacobian(eng, to_dev(Xnew, eng.device))
        return as_result(mean), as_result(var), as_result(J.transpose(1, 2))

    def fisher(self, Xnew, obs_cov=None, obs_var=None) -> FisherResult:
        """The Fisher (Gauss-Newton) matrix of the emulated data vector at every row of Xnew:
        ``F[s] = J_s^T (diag(var(Xnew_s) + obs_var_s) + obs_cov)^{-1} J_s`` [N*, D, D], with ``J_s`` the
        ``mean_jacobian`` and the covariance exactly the one ``log_density`` uses: ``obs_var`` a scalar, [P] or
        [N*, P], ``obs_cov`` [P, P] symmetric positive definite (its lower triangle is read); both may be given
        and are added; the emulator's own likelihood noise is NOT added.  One Jacobian call and one launch of
        mfgp_mvn_fisher: with ``obs_cov`` the [P, P] covariance of every row is factored in LDS with the rows
        of J^T carried along, so F falls out of the factorization (no [N*, P, P] tensor, no rocSOLVER call);
        without it the diagonal form runs (any P).  F is exactly symmetric (one triangle is computed and
        mirrored).  This is the MEAN term of the Gaussian Fisher information; the
        ``1/2 tr(Sigma^-1 dSigma Sigma^-1 dSigma)`` term that dvar/dx adds is not formed.

        Returns ``FisherResult(fisher, mean, var, jacobian)``, detached.  ValueError before any device work
        for a wrong shape, a negative obs_var, or an obs_cov beyond the dense form's limit (P <= 128 and
        P8 + D <= 143, ``fisher_dense_fits``); NotImplementedError for a NOCACHE posterior and the graph model.
        The call's one host read is info, after everything is enqueued: CholeskyError naming the row whose
        covariance is not positive definite (e.g. a NaN input row)."""
        what = "fisher"
        self._need_cache(f"{what}: a NOCACHE posterior has no cached factors; use a TENSOR or VARIABLE cache")
        self._check_vjp()
        p, d = self._num_outputs(), self._input_dim()
        ns = _design_rows(Xnew, d, f"{what}: Xnew")
        fisher_plan(what, ns, p, d, obs_var, obs_cov)
        eng = self._engine()   # every ValueError of the arguments is raised above
        _, ov, oc = density_inputs(eng, p, np.zeros((p,)), obs_var, obs_cov)
        mean, var, J = self._jacobian(eng, to_dev(Xnew, eng.device), tiled=False)
        F, info = eng.mvn_fisher(J, var, ov, oc)
        if var.dim() == 1:
            var = var[:, None].expand(-1, p).contiguous()
        raise_density_info(what, info, oc is not None)
        return FisherResult(as_result(F), as_result(mean), as_result(var), as_result(J.transpose(1, 2)))

    def _weights(self, eng: Engine):
        """alpha of the current cache block (Engine.*_jacobian_weights), built on first use; update_cache() and
        _commit() drop it.  (Posteriors are also made with object.__new__: read with a default.)"""
        w = getattr(self, "_jac_weights", None)
        if w is None or w[0] is not self.cache:
            w = (self.cache, self._make_weights(eng))
            self._jac_weights = w
        return w[1]

    def predict_log_density(self, data, full_cov: bool = False, full_output_cov: bool = False):
        """GPflow ``GPModel.predict_log_density((Xnew, Ynew))`` on this posterior's marginal predict_f:
        [N*], summed over the outputs, the model's likelihood variance added (posteriors.predict_log_density_of;
        the likelihood is not part of the snapshot: it does not enter predict_f).  Either covariance flag
        raises NotImplementedError, as GPflow does."""
        return predict_log_density_of(self.model, self.predict_f, data, full_cov, full_output_cov)

    def _check_vjp(self):
        pass

    def _attached(self, Xnew):
        """predict_f of a requires_grad Xnew: outputs attached to autograd (backward = the VJP call)."""
        self._need_cache("predict_f of an Xnew that requires grad needs a cached posterior (TENSOR or VARIABLE)")
        self._check_vjp()
        mean, var = _PredictFn.apply(Xnew, self)
        return as_result(mean), as_result(var)

    def _marginal(self, Xnew):
        mean, var = self.predict_f(Xnew.detach())
        return mean.as_subclass(torch.Tensor), var.as_subclass(torch.Tensor)

    def _need_cache(self, nocache: str):
        """The first line of every call that only a cache can serve."""
        if self._precompute_cache is PrecomputeCacheType.NOCACHE:
            raise NotImplementedError(nocache)

    def _engine(self, cache=None) -> Engine:
        """The engine of the device the cache block lives on (`cache`: the block an autograd node kept;
        None: the current one), after the check that the block can be used."""
        cache = self.cache if cache is None else cache
        eng = Engine.get(cache.device if cache is not None else None)
        self._require_cache(eng)
        return eng

    def _require_cache(self, eng: Engine):
        if not self._valid:
            raise MFGPError("posterior: the cache is not valid (its last update failed); call update_cache()")
        if eng.tile() != self._nb:
            raise MFGPError(f"posterior: the cache was built for tile size {self._nb}, the engine now runs "
                            f"{eng.tile()}; call update_cache()")


class GPRPosterior(_Posterior):
    """Posterior of MultiFidelityGPModel (nlf = 0) / GraphMultiFidelityGPModel (nlf = its LF sources).

    The cache holds X, theta, L^{-1} and Z = L^{-1} Y; ``predict_f`` (marginal and ``full_cov=True``)
    is computed from it alone: A = L^{-1} K(X, X*) with K generated inside the product kernel,
    mean = A^T Z, var = K_diag(X*) - colsum(A^2), cov = K(X*, X*) - A^T A."""

    def __init__(self, model, nlf: int, theta_fn, precompute_cache):
        self._nlf = int(nlf)
        self._theta_fn = theta_fn
        self._stacked = None   # a conditioned posterior's own (X, Y, theta) device tensors
        self._theta = None     # the theta tensor of the last build
        super().__init__(model, precompute_cache)

    def _data(self):
        """(engine, X, Y) the cache stands for: the model's construction-time data (they cannot be
        reassigned), or the stacked rows of a conditioned posterior."""
        if self._stacked is None:
            return self.model._device_data()
        X, Y, _ = self._stacked
        return Engine.get(X.device), X, Y

    def _build(self):
        eng, X, Y = self._data()
        if self._stacked is None:
            theta = torch.tensor(self._theta_fn(), dtype=torch.float64, device=eng.device)
        else:
            theta = self._stacked[2]   # frozen: the rebuild of a conditioned posterior is exact at its snapshot
        n, p, d = X.shape[0], Y.shape[1], X.shape[1] - 1
        buf = self._cache_buffer(eng, eng.gpr_posterior_bytes(self._nlf, n, p, d))
        info = eng.gpr_posterior_build(self._nlf, X, Y, theta, buf)
        self._shape, self._nb = (n, p, d), eng.tile()
        self._commit(buf, info, "posterior")
        self._theta = theta   # (after the commit: a TENSOR cache that keeps its contents keeps their theta)

    def fused_predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        if self._stacked is not None:
            raise NotImplementedError("fused_predict_f: a conditioned posterior's rows are not in the model; "
                                      "use predict_f")
        return super().fused_predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)

    def condition_on(self, Xadd, Yadd=None) -> "GPRPosterior":
        """The posterior after k more simulations (1 <= k <= 32), at the snapshot's hyper-parameters: a NEW
        posterior of ``vstack(X, Xadd)``, ``vstack(Y, Yadd)`` in that row order, from the cached factors by
        a block append (mfgp_gpr_posterior_append: O(N^2 k), no Gram of X, no factorization of K).  Xadd
        [k, D + 1] (fidelity in the last column), Yadd [k, P] (or [k] when P = 1); numpy, lists or device
        tensors.  This posterior and its cache block are not written.  Everything that runs from a cache
        runs on the result (predict_f, predict_f_vjp, leave_out, variance_reduction / select,
        condition_on); it keeps the stacked data and the frozen theta, inherits the cache type, and its
        ``update_cache()`` is the exact rebuild from the stacked data at the frozen theta (the way to shed
        the rounding of many appends).  ``.model`` stays the original model, which does not hold the new
        rows: ``fused_predict_f`` raises NotImplementedError.

        ``Yadd=None`` (``fantasize``): the rows are observed at this posterior's own mean, so the mean is
        unchanged and the variance is that of the refit: the exact look-ahead on runs not yet made.

        ValueError before any device work: a wrong shape, k outside 1..32.  The call's one host read is
        info: ValueError for a row whose fidelity is no source of the kernel, CholeskyError when the new
        rows' conditional covariance is not positive definite (e.g. a NaN input); no posterior is returned.

        Graph model: the cross block is the one a factorization of the stacked rows reads (the new row is
        the row argument of the kernel's entry function), so the result is the refit's for any ``rho_LF``."""
        self._need_cache("condition_on: a NOCACHE posterior has no cached factors to append to; use a TENSOR or "
                         "VARIABLE cache")
        n, p, d = self._shape
        k = _design_rows(Xadd, d, "condition_on: Xadd")
        if k < 1 or k > MAX_APPEND:
            raise ValueError(f"condition_on: Xadd has {k} rows; 1..{MAX_APPEND} rows can be appended in one call")
        if Yadd is not None:
            shape = tuple(Yadd.shape) if isinstance(Yadd, torch.Tensor) else np.shape(Yadd)
            if shape != (k, p) and not (p == 1 and shape == (k,)):
                raise ValueError(f"condition_on: Yadd has shape {shape}, expected ({k}, {p})")
        eng = self._engine()   # every ValueError of the arguments is raised above
        Xa = to_dev(Xadd, eng.device)
        Ya = None if Yadd is None else to_dev(Yadd, eng.device).reshape(k, p)
        buf = torch.empty(int(eng.gpr_posterior_bytes(self._nlf, n + k, p, d)), dtype=torch.uint8, device=eng.device)
        mean, info = eng.gpr_posterior_append(self._nlf, self._shape, self.cache, Xa, Ya, buf)
        _, X, Y = self._data()
        stacked = (torch.cat([X, Xa]), torch.cat([Y, mean if Ya is None else Ya]), self._theta)
        bad = int(info.item())   # the one host read of a device word
        if bad < 0:
            raise ValueError(f"condition_on: row {-bad - 1} of Xadd has a fidelity that is no source of the kernel")
        if bad > 0:
            raise CholeskyError(f"condition_on: the conditional covariance of the new rows is not positive "
                                f"definite (pivot {bad}); the input might not be valid.")
        post = object.__new__(GPRPosterior)
        post.model, post._nlf, post._theta_fn = self.model, self._nlf, self._theta_fn
        post._precompute_cache = self._precompute_cache
        post._stacked, post._theta = stacked, self._theta
        post._shape, post._nb = (n + k, p, d), self._nb
        post.cache, post._valid = buf, True
        return post

    def fantasize(self, Xadd) -> "GPRPosterior":
        """``condition_on(Xadd)`` without values: the posterior after runs at Xadd whose results are not in
        yet (same mean, the refit's variance)."""
        return self.condition_on(Xadd, None)

    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """The model's predict_f at the snapshot (same shapes: mean [N*, P]; var [N*, P] or, with
        full_cov, [P, N*, N*]).  Uploads Xnew when it is not a device tensor, enqueues, returns."""
        if full_output_cov:
            raise NotImplementedError("predict_f(full_output_cov=True): GPR has no output covariance to return")
        if _wants_grad(Xnew):
            if full_cov:
                raise NotImplementedError("predict_f(full_cov=True) of an Xnew that requires grad: only the "
                                          "marginal form has an input gradient")
            return self._attached(Xnew)
        if self._precompute_cache is PrecomputeCacheType.NOCACHE:
            return self.fused_predict_f(Xnew, full_cov=full_cov)
        mean, var, _ = self._predict(self.cache, Xnew, full_cov=full_cov)
        return as_result(mean), as_result(var)

    def _predict(self, cache, Xnew, full_cov=False, grad=None):
        """predict_f on `cache`: (mean, var or cov tiled over P, None); with grad = (grad_mean, grad_var) the
        VJP call: (mean, var, grad_X)."""
        eng = self._engine(cache)
        p = self._shape[1]
        Xs = to_dev(Xnew, eng.device)
        if grad is not None:
            ns = Xs.shape[0]
            gm, gv = _upstream(grad[0], (ns, p), eng.device, "grad_mean"), grad[1]
            if gv is not None:
                gv = to_dev(gv, eng.device)
                if gv.dim() == 2:   # the variance is one column tiled over P: its upstream gradients add up
                    gv = _upstream(gv, (ns, p), eng.device, "grad_var").sum(dim=1)
                gv = _upstream(gv, (ns,), eng.device, "grad_var")
            grad = (gm, gv)
        mean, var, third = eng.gpr_posterior_predict(self._nlf, self._shape, cache, Xs, full_cov, grad)
        if full_cov:
            return mean, third[None].expand(p, -1, -1).contiguous(), None
        return mean, var[:, None].expand(-1, p).contiguous(), third

    def _num_outputs(self) -> int:
        return self._shape[1]

    def _input_dim(self) -> int:
        return self._shape[2]

    def _logdens(self, eng, Xs, Y, obs_var, obs_cov, grad):
        mean, var, logp, gX, info = eng.gpr_posterior_logdens(self._nlf, self._shape, self.cache, Xs, Y, obs_var,
                                                              obs_cov, grad)
        return mean, var[:, None].expand(-1, self._shape[1]).contiguous(), logp, gX, info

    def _make_weights(self, eng):
        return eng.gpr_jacobian_weights(self._shape, self.cache)

    def _jacobian(self, eng, Xs, tiled=True):
        """(mean, var [N*, P] -- [N*] with tiled=False --, J [N*, D, P]) on the current cache block."""
        w = self._weights(eng) if Xs.shape[0] else None   # (an empty call launches nothing)
        mean, var, J = eng.gpr_jacobian(self._shape, self.cache, w, Xs)
        return mean, (var[:, None].expand(-1, self._shape[1]).contiguous() if tiled else var), J

    def _joint(self, eng, Xs):
        """(mean [N*, P], the ONE [1, N*, N*] block, ncol = P): never tiled over P, factored once."""
        mean, _, cov = eng.gpr_posterior_predict(self._nlf, self._shape, self.cache, Xs, True)
        return mean, cov[None], self._shape[1], None

    def leave_out(self, groups=None, full_cov: bool = False) -> LeaveOutResult:
        """Leave-group-out cross-validation at the snapshot's hyper-parameters: for every group of
        training rows, what a model built without those rows predicts for them (``predict_f`` of that
        model at the rows' own inputs), in closed form from the cached factors (mfgp_gpr_posterior_leave_out:
        no Gram, no factorization of K, no Xnew).  ``groups``: see ``normalize_groups`` (None: every row
        on its own; a label array, e.g. ``groups_by_input(X, only_hf=True)``; a sequence of index
        arrays of at most 32 rows).  Returns a ``LeaveOutResult``; ``cov`` only with ``full_cov``.
        ``log_density`` is the joint density of the group's *observations* (the likelihood variance
        included).  Like predict_f it is the snapshot's until update_cache().

        Graph model: the joint covariance is the one the factorization reads (the lower triangle of K;
        the kernel's 1e-6 jitter is part of K and stays in the covariance).  With an asymmetric
        ``rho_LF`` a refit's ``predict_f`` at a row of LF source j >= 1 takes its cross-covariance from
        the other triangle and is another model there; rows of source 0 and HF rows agree with it."""
        self._need_cache("leave_out: a NOCACHE posterior has no cached factors; use a TENSOR or VARIABLE cache")
        n, p, d = self._shape
        offsets, rows, gmax = normalize_groups(groups, n)   # every ValueError is raised before the device is touched
        eng = self._engine()
        ng, nr = offsets.shape[0] - 1, rows.shape[0]
        group = np.repeat(np.arange(ng, dtype=np.int64), np.diff(offsets))
        pos = np.arange(nr, dtype=np.int64) - offsets[:-1].astype(np.int64)[group]   # place inside the group
        f64 = dict(dtype=torch.float64, device=eng.device)
        if ng == 0:
            z = lambda *s: as_result(torch.zeros(s, **f64))
            return LeaveOutResult(rows.astype(np.int64), group, z(0, p), z(0, p), z(0, p),
                                  z(0, 0, 0) if full_cov else None)
        idx = torch.from_numpy(np.concatenate([offsets, rows, pos.astype(np.int32)])).to(eng.device)
        d_off, d_rows, d_pos = idx[:ng + 1], idx[ng + 1:ng + 1 + nr], idx[ng + 1 + nr:].long()
        resid, cov, logd, info = eng.gpr_posterior_leave_out(self._nlf, self._shape, self.cache, d_off, d_rows, gmax)
        Y = self._data()[2]
        mean = Y.index_select(0, d_rows) - resid
        var = cov.gather(1, d_pos[:, None]).expand(-1, p).contiguous()
        full = None
        if full_cov:   # [G, gmax, gmax]: row r of the call's cov is row pos[r] of its group's block
            full = torch.zeros((ng, gmax, gmax), **f64)
            full[torch.from_numpy(group).to(eng.device), d_pos] = cov
        bad = info.cpu().numpy()   # the one host read of a device word
        if np.any(bad < 0):
            raise MFGPError("leave_out: the device rejected the group table")
        if np.any(bad > 0):
            g = int(np.flatnonzero(bad)[0])
            raise CholeskyError(f"leave_out: the held-out precision of group {g} (rows {rows[offsets[g]:offsets[g + 1]]}) "
                                f"is not positive definite (pivot {int(bad[g])})")
        return LeaveOutResult(rows.astype(np.int64), group, as_result(mean), as_result(var), as_result(logd),
                              None if full is None else as_result(full))

    def variance_reduction(self, Xcand, Xref, weights=None):
        """How much one more simulation at each candidate lowers the posterior variance of f over a
        reference set, at the snapshot's hyper-parameters (the ALC / integrated-variance criterion):
        ``score[c] = sum_r weights[r] cov(f(Xref_r), f(Xcand_c))^2 / (var f(Xcand_c) + s2)``, shape [Nc].
        Xcand [Nc, D + 1] and Xref [Nr, D + 1] carry the fidelity in the last column: the candidate's says
        which simulation is run, the reference's whose error is bought down.  ``weights`` [Nr] >= 0
        (None: ones).  cov and var are those of ``predict_f(vstack(Xref, Xcand), full_cov=True)``, s2 the
        likelihood variance; the variance is shared by the P outputs, so there is no P axis.  The
        Nr x Nc block is formed on chip by one fused kernel (mfgp_gpr_posterior_design_score), never in
        memory.  A row whose fidelity is no source of the kernel scores / adds exactly 0.  Like
        predict_f it is the snapshot's until update_cache().

        Graph model: the block is the one full_cov returns (the kernel's entry function with the
        reference as its row).  With an asymmetric ``rho_LF`` its reading as "the variance after a refit"
        holds only at references of LF source 0 and HF references (see ``leave_out``)."""
        return self._design(Xcand, Xref, weights, None, None, "variance_reduction")

    def select(self, Xcand, Xref, q, weights=None, cost=None) -> DesignResult:
        """A greedy batch of q simulations (q <= 32): each step takes ``argmax(score / cost)`` of
        ``variance_reduction`` (the lowest index wins a tie), then conditions every later covariance on
        the pick, in closed form (one more row under the cached A: mfgp_gpr_posterior_design_append).
        ``cost`` [Nc] > 0 (None: ones), e.g. 1 for an LF and 4 for an HF run.  A candidate may be picked
        again: a replicate is a legitimate design.  Returns ``DesignResult(picks, gain)``; ``gain[k]`` is
        the score (not divided by the cost) of pick k at its step.  After the argument checks the whole
        batch is enqueued without a host read of a device word: the pick is copied and its score gathered
        on the device."""
        return self._design(Xcand, Xref, weights, cost, q, "select")

    def _design(self, Xcand, Xref, weights, cost, q, what):
        self._need_cache(f"{what}: a NOCACHE posterior has no cached factors; use a TENSOR or VARIABLE cache")
        d = self._shape[2]
        nc, nr = _design_rows(Xcand, d, f"{what}: Xcand"), _design_rows(Xref, d, f"{what}: Xref")
        w = _design_vector(weights, nr, f"{what}: weights", False)
        cost = _design_vector(cost, nc, f"{what}: cost", True)
        if q is not None:
            if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 1 or q > MAX_BATCH:
                raise ValueError(f"{what}: q must be an integer in 1..{MAX_BATCH}, got {q!r}")
            if nc == 0:
                raise ValueError(f"{what}: no candidate to pick from (Xcand has no rows)")
            q = int(q)
        eng = self._engine()   # every ValueError is raised above
        f64 = dict(dtype=torch.float64, device=eng.device)
        if cost is not None:
            cost = cost.to(eng.device)
        if nc == 0 or nr == 0:   # nothing to score / nothing to buy down: zeros, no launch
            score = torch.zeros((nc,), **f64)
            if q is None:
                return as_result(score)
            idx = torch.argmax(score if cost is None else score / cost)
            return DesignResult(as_result(idx.repeat(q)), as_result(torch.zeros((q,), **f64)))
        Xall = torch.cat([to_dev(Xref, eng.device), to_dev(Xcand, eng.device)]).contiguous()
        w = None if w is None else w.to(eng.device).contiguous()
        nall, steps = nr + nc, 1 if q is None else q
        call = (self._nlf, self._shape, self.cache, Xall, nr)
        ws = eng.gpr_posterior_design_workspace(self._nlf, self._shape, nr, nc, steps)
        E = torch.empty((steps - 1, nall), **f64) if steps > 1 else None
        picks = torch.empty((steps,), dtype=torch.int64, device=eng.device)
        gain = torch.empty((steps,), **f64)
        for k in range(steps):
            score = eng.gpr_posterior_design_score(*call, w, E, k, ws)
            if q is None:
                return as_result(score)
            idx = torch.argmax(score if cost is None else score / cost)
            picks[k] = idx
            gain[k:k + 1] = score.index_select(0, idx.reshape(1))   # score[idx] would read idx on the host
            if k + 1 < steps:
                eng.gpr_posterior_design_append(*call, idx.to(torch.int32), E, k, ws)
        return DesignResult(as_result(picks), as_result(gain))

    def _check_vjp(self):
        if self._nlf:
            raise NotImplementedError("predict_f_vjp: the graph kernel's input gradient (a derivative per source) "
                                      "is not built; only the linear multi-fidelity kernel has one")


class SVGPPosterior(_Posterior):
    """Posterior of SingleBinSVGP / LatentMFCoregionalizationSVGP (any likelihood: it does not enter
    predict_f).

    The cache holds Z, the per-latent kernel parameters, W, q_mu, Lm^{-1} and Lq^T Lm^{-1}; the
    marginal ``predict_f`` is computed from it alone.  The covariance forms (``full_cov`` /
    ``full_output_cov``) are NOT cached: they run the model's covariance entry point
    (mfgp_svgp_predict_cov, factorization included) on the snapshot's parameters, which keeps the
    snapshot semantics."""

    def __init__(self, model, jitter: float, precompute_cache):
        self._jitter = float(jitter)
        self._state = None
        super().__init__(model, precompute_cache)

    def _build(self):
        eng, Z, thetas, q_mu, q_sqrt, W = self.model._dev_state()
        m, d, L, p = Z.shape[0], Z.shape[1] - 1, thetas.shape[0], int(self.model.num_outputs)
        buf = self._cache_buffer(eng, eng.svgp_posterior_bytes(m, L, p, d))
        info = eng.svgp_posterior_build(Z, thetas, q_mu, q_sqrt, W, p, self._jitter, buf)
        self._shape, self._nb = (m, L, p, d, W is not None), eng.tile()
        self._state = (Z, thetas, q_mu, q_sqrt, W)   # the snapshot the covariance forms run on
        self._commit(buf, info, "posterior")

    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """The model's predict_f at the snapshot: mean [N*, P]; var [N*, P], or the model's
        covariance forms (not cached, see the class docstring)."""
        if _wants_grad(Xnew):
            if full_cov or full_output_cov:
                raise NotImplementedError("predict_f(full_cov / full_output_cov) of an Xnew that requires grad: "
                                          "only the marginal form has an input gradient")
            return self._attached(Xnew)
        if self._precompute_cache is PrecomputeCacheType.NOCACHE:
            return self.fused_predict_f(Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
        if full_cov or full_output_cov:
            eng = self._engine()
            mode = 3 if (full_cov and full_output_cov) else (1 if full_cov else 2)
            Z, thetas, q_mu, q_sqrt, W = self._state
            f_mu, f_cov, info = eng.svgp_predict_cov(mode, to_dev(Xnew, eng.device), Z, thetas, q_mu, q_sqrt, W,
                                                     self._shape[2], self._jitter)
            if int(info.max().item()) != 0:
                raise CholeskyError("predict_f: Cholesky of K_uu was not successful")
            return as_result(f_mu), as_result(f_cov)
        f_mu, f_var, _ = self._predict(self.cache, Xnew)
        return as_result(f_mu), as_result(f_var)

    def _num_outputs(self) -> int:
        return self._shape[2]

    def _input_dim(self) -> int:
        return self._shape[3]

    def _logdens(self, eng, Xs, Y, obs_var, obs_cov, grad):
        return eng.svgp_posterior_logdens(self._shape, self.cache, Xs, Y, obs_var, obs_cov, grad)

    def _make_weights(self, eng):
        return eng.svgp_jacobian_weights(self._shape, self.cache)

    def _jacobian(self, eng, Xs, tiled=True):
        w = self._weights(eng) if Xs.shape[0] else None
        return eng.svgp_jacobian(self._shape, self.cache, w, Xs)

    def _joint(self, eng, Xs):
        """(mean [N*, P], cov [P, N*, N*] of the snapshot, ncol = 1): one factor per output."""
        Z, thetas, q_mu, q_sqrt, W = self._state
        mean, cov, kuu = eng.svgp_predict_cov(1, Xs, Z, thetas, q_mu, q_sqrt, W, self._shape[2], self._jitter)
        return mean, cov, 1, kuu

    def _predict(self, cache, Xnew, grad=None):
        """The marginal predict_f on `cache`: (f_mu, f_var, None); with grad = (grad_mean, grad_var) the VJP
        call: (f_mu, f_var, grad_X)."""
        eng = self._engine(cache)
        Xs = to_dev(Xnew, eng.device)
        if grad is not None:
            shape = (Xs.shape[0], self._shape[2])
            grad = (_upstream(grad[0], shape, eng.device, "grad_mean"),
                    _upstream(grad[1], shape, eng.device, "grad_var"))
        return eng.svgp_posterior_predict(self._shape, cache, Xs, grad)
