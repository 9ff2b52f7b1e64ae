"""Device engine: torch-ROCm buffers + calls into libmfgp.so (include/mfgp.h).

PyTorch only provides device memory, streams and graphs here; every FLOP of the
hot path runs in the hand-written HIP kernels of ``csrc/``.  There is no CPU
fallback — on a machine without a GPU every compute call raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

import torch

from . import _lib
from ._lib import MFGPError, check, ptr


def theta_size(d: int) -> int:
    return 2 * d + 4


def default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise MFGPError("no GPU visible: the MI355X engine has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x, device: torch.device, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """`dtype` (default float64), contiguous, on `device` (numpy / list / torch accepted)."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.as_tensor(np.asarray(x, dtype=np.float64))
    return t.to(device=device, dtype=dtype).contiguous()


def dtype_code(t: torch.Tensor) -> int:
    """include/mfgp.h dtype of a data tensor: MFGP_F32 for float32, MFGP_F64 for float64."""
    if t.dtype == torch.float32:
        return _lib.MFGP_F32
    if t.dtype == torch.float64:
        return _lib.MFGP_F64
    raise MFGPError(f"unsupported data dtype {t.dtype} (float64 or float32)")


def resolve_dtype(dtype) -> torch.dtype:
    """Model compute dtype: None / 'float64' / torch.float64 -> float64; 'float32' / torch.float32 -> float32."""
    if dtype is None or dtype in ("float64", "f64", torch.float64, np.float64):
        return torch.float64
    if dtype in ("float32", "f32", torch.float32, np.float32):
        return torch.float32
    raise MFGPError(f"unsupported compute dtype {dtype!r} (float64 or float32)")


class Engine:
    """One per device: owns the library handle binding and grow-only workspaces."""

    _engines: dict = {}

    def __init__(self, device: torch.device):
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()
        self._ws: dict = {}
        self.lib = _lib.load()

    @classmethod
    def get(cls, device=None) -> "Engine":
        device = torch.device(device) if device is not None else default_device()
        if device.type != "cuda":
            raise MFGPError(f"MI355X engine needs a GPU device, got {device}")
        key = device.index if device.index is not None else torch.cuda.current_device()
        eng = cls._engines.get(key)
        if eng is None:
            eng = cls(torch.device("cuda", key))
            cls._engines[key] = eng
        return eng

    # ------------------------------------------------------------ session ordering
    @contextlib.contextmanager
    def ordered(self, stream: torch.cuda.Stream):
        """Work enqueued on `stream` inside the block starts after the previous flow-bearing work
        on this device ended (whatever its stream, handle or host thread), and the block's end
        becomes the new last one: the library's device-wide flow fence (include/mfgp.h
        mfgp_flow_fence).  Two persistent k_chol_flow launches must never share the device: each
        needs every CU resident, and one that cannot get them stalls until its hand-off bound
        expires (a lost step).  The library fences every eager flow launch itself; this block is
        for graph replays, whose flows were captured unfenced.  Between WAIT and RECORD this host
        thread holds the fence: a flow launched from another host thread blocks (on the host) until
        the block ends.  No device synchronisation."""
        with torch.cuda.stream(stream):
            check(self.lib.mfgp_flow_fence(self.h, _lib.MFGP_FENCE_WAIT), "mfgp_flow_fence")
        try:
            yield
        finally:
            with torch.cuda.stream(stream):
                check(self.lib.mfgp_flow_fence(self.h, _lib.MFGP_FENCE_RECORD), "mfgp_flow_fence")

    # ------------------------------------------------------------ plumbing
    @property
    def h(self):
        return _lib.handle(self.index)

    def workspace(self, key: str, nbytes: int) -> torch.Tensor:
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[key] = buf
        return buf

    def _size(self, fn, *args) -> int:
        out = C.c_size_t(0)
        check(fn(self.h, *args, C.byref(out)), fn.__name__)
        return out.value

    # callables run after any change of the handle's execution settings (tile, flow, tiny): the
    # session pool (models.py) drops the cores whose captured graphs recorded the old settings
    _mode_listeners: list = []

    def _set_mode(self, fn, *args):
        before = self.mode()
        check(fn(self.h, *args), fn.__name__)
        if self.mode() != before:
            for cb in list(Engine._mode_listeners):
                cb(self)

    def mode(self) -> tuple:
        """The handle's execution settings that captured step graphs and workspace sizes depend
        on: (flow mode, tile size, one-launch small-problem path, k_grad chunk, step fusion)."""
        h = self.h
        fusion = self.lib.mfgp_get_step_fusion(h) if hasattr(self.lib, "mfgp_get_step_fusion") else 0
        return (self.lib.mfgp_get_flow(h), self.lib.mfgp_get_tile(h), self.lib.mfgp_get_tiny(h),
                self.lib.mfgp_get_grad_chunk(h), fusion)

    def tile(self) -> int:
        return self.lib.mfgp_get_tile(self.h)

    def set_tile(self, nb: int):
        self._set_mode(self.lib.mfgp_set_tile, nb)

    def flow(self) -> bool:
        return self.lib.mfgp_get_flow(self.h) in (1, 3)

    FLOW_MIN_TILES = 8   # mfgp_host.h: below this many 32-tiles mode 1 runs the step launches

    def flow_runs(self, n: int) -> bool:
        """Whether an n-point fp64 factorization takes the persistent flow under the current mode."""
        mode = self.lib.mfgp_get_flow(self.h)
        return self.tile() == 32 and (mode == 3 or (mode == 1 and -(-n // 32) >= self.FLOW_MIN_TILES))

    def set_flow(self, enable: bool, any_size: bool = False):
        """Cholesky schedule of the LML path: persistent dataflow launch (True; for factorizations of
        8 or more 32-tiles unless any_size) or one launch per step (False)."""
        self._set_mode(self.lib.mfgp_set_flow, (3 if any_size else 1) if enable else 0)

    def set_tiny(self, enable: bool):
        """One-launch LML step for small problems (n, p <= 64, D <= 16; True, the default) or the
        step sequence of the general path (False)."""
        self._set_mode(self.lib.mfgp_set_tiny, 1 if enable else 0)

    @contextlib.contextmanager
    def resident(self):
        """Value+grad LML calls inside the block may skip the flow's set-up launch when the previous
        fp64 LML call on this thread's handle left their workspace set up for the same problem
        (include/mfgp.h mfgp_set_resident).  For training sessions, whose private workspace nothing
        else writes."""
        if not hasattr(self.lib, "mfgp_set_resident"):   # an older diagnostic build (MFGP_LIB_PATH)
            yield
            return
        check(self.lib.mfgp_set_resident(self.h, 1), "mfgp_set_resident")
        try:
            yield
        finally:
            check(self.lib.mfgp_set_resident(self.h, 0), "mfgp_set_resident")

    def set_flow_timeout_us(self, us: int):
        """Bound of every k_chol_flow hand-off wait (default 50000 us; 0: diagnostic abort path)."""
        check(self.lib.mfgp_set_flow_timeout_us(self.h, int(us)), "mfgp_set_flow_timeout_us")

    # ------------------------------------------------------------ kernels
    def rbf_gram(self, X1: torch.Tensor, X2: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
        n1, d = X1.shape
        n2 = X2.shape[0]
        K = torch.empty((n1, n2), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_rbf_gram(self.h, n1, n2, d, ptr(X1), d, ptr(X2), X2.shape[1], ptr(params), ptr(K), n2),
              "mfgp_rbf_gram")
        return K

    def mf_gram(self, X1: torch.Tensor, X2: torch.Tensor, theta: torch.Tensor, diag_add: float = 0.0) -> torch.Tensor:
        """K(X1, X2) in X1's dtype (float64: mfgp_mf_gram; float32: mfgp_mf_gram_ex)."""
        n1, dp1 = X1.shape
        n2 = X2.shape[0]
        K = torch.empty((n1, n2), dtype=X1.dtype, device=self.device)
        check(self.lib.mfgp_mf_gram_ex(self.h, dtype_code(X1), n1, n2, dp1 - 1, ptr(X1), dp1, ptr(X2), X2.shape[1],
                                       ptr(theta), float(diag_add), ptr(K), n2), "mfgp_mf_gram_ex")
        return K

    def mf_kdiag(self, X: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
        n, dp1 = X.shape
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_mf_kdiag(self.h, n, dp1 - 1, ptr(X), dp1, ptr(theta), ptr(out)), "mfgp_mf_kdiag")
        return out

    def gpr_workspace_bytes(self, n: int, p: int, d: int, dtype: torch.dtype = torch.float64) -> int:
        return self._size(self.lib.mfgp_gpr_workspace_size_ex, dtype_code(torch.empty(0, dtype=dtype)), n, p, d)

    def set_f32_panel(self, tiles: int):
        """fp32 path: 128-wide tile columns per outer Cholesky panel (trailing-update K = 128 * tiles)."""
        check(self.lib.mfgp_set_f32_panel(self.h, int(tiles)), "mfgp_set_f32_panel")

    def set_f32_refine(self, steps):
        """fp32 path: fp64 iterative refinement of the value-only LML (one step) and the predictive
        mean (`steps` steps: True / 2 = the default two, 1, False / 0 = off); gradients and Adam
        steps are never refined.  mfgp_set_f32_refine."""
        steps = 2 if steps is True else 0 if steps is False else int(steps)
        check(self.lib.mfgp_set_f32_refine(self.h, steps), "mfgp_set_f32_refine")

    def set_f32_lookahead(self, enable: bool):
        """fp32 path: factor the next panel on a side stream beside the trailing update (default on)."""
        check(self.lib.mfgp_set_f32_lookahead(self.h, 1 if enable else 0), "mfgp_set_f32_lookahead")

    def set_f32_reserve(self, cus: int):
        """fp32 lookahead: CUs the trailing update leaves to the side stream (0: uncapped)."""
        check(self.lib.mfgp_set_f32_reserve(self.h, int(cus)), "mfgp_set_f32_reserve")

    def private_workspace(self, nbytes: int) -> torch.Tensor:
        """A workspace owned by its caller (a training session keeps it for the life of its
        recorded graphs; the shared grow-only buffers may be replaced under them)."""
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def gpr_lml(self, X, Y, theta, want_grad=False, ws=None, out=None, info=None):
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        nbytes = self.gpr_workspace_bytes(n, p, d, X.dtype)
        if ws is None:
            ws = self.workspace("gpr" if X.dtype == torch.float64 else "gpr32", nbytes)
        elif ws.numel() < nbytes:
            raise MFGPError("gpr_lml: private workspace too small")
        if Y.dtype != X.dtype:
            raise MFGPError("gpr_lml: X and Y must share a dtype")
        if out is None:
            out = torch.empty((1 + theta_size(d),), dtype=torch.float64, device=self.device)
        if info is None:
            info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gpr_lml_ex(self.h, dtype_code(X), n, p, d, ptr(X), dp1, ptr(Y), p, ptr(theta),
                                       int(want_grad), ptr(ws), ws.numel(), ptr(out), ptr(info)), "mfgp_gpr_lml_ex")
        return out, info

    def gpr_adam_step(self, X, Y, st: "AdamState", loss_hist: torch.Tensor, out: torch.Tensor, info: torch.Tensor,
                      ws: torch.Tensor = None):
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        nbytes = self.gpr_workspace_bytes(n, p, d, X.dtype)
        if ws is None:
            ws = self.workspace("gpr" if X.dtype == torch.float64 else "gpr32", nbytes)
        elif ws.numel() < nbytes:
            raise MFGPError("gpr_adam_step: private workspace too small")
        check(self.lib.mfgp_gpr_adam_step_ex(self.h, dtype_code(X), n, p, d, ptr(X), dp1, ptr(Y), p, ptr(st.theta),
                                             ptr(st.u), ptr(st.m), ptr(st.v), ptr(st.trainable), ptr(st.tie),
                                             ptr(st.step), st.lr, st.b1, st.b2, st.eps, ptr(loss_hist), ptr(ws),
                                             ws.numel(), ptr(out), ptr(info)), "mfgp_gpr_adam_step_ex")

    def gpr_adam_steps(self, X, Y, st: "AdamState", loss_hist: torch.Tensor, out: torch.Tensor, info: torch.Tensor,
                       ws: torch.Tensor = None, nsteps: int = 1):
        """`nsteps` Adam steps in one call (mfgp_gpr_adam_steps): the same bits as `nsteps` calls of
        gpr_adam_step; on the fp64 flow path every step's reduction but the last runs in the head of
        the next flow launch.  float32 inputs take the single-step entry `nsteps` times."""
        if X.dtype != torch.float64 or not hasattr(self.lib, "mfgp_gpr_adam_steps"):   # (or an older diagnostic build)
            for _ in range(nsteps):
                self.gpr_adam_step(X, Y, st, loss_hist, out, info, ws=ws)
            return
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        nbytes = self.gpr_workspace_bytes(n, p, d, X.dtype)
        if ws is None:
            ws = self.workspace("gpr", nbytes)
        elif ws.numel() < nbytes:
            raise MFGPError("gpr_adam_steps: private workspace too small")
        check(self.lib.mfgp_gpr_adam_steps(self.h, n, p, d, ptr(X), dp1, ptr(Y), p, ptr(st.theta), ptr(st.u),
                                           ptr(st.m), ptr(st.v), ptr(st.trainable), ptr(st.tie), ptr(st.step),
                                           st.lr, st.b1, st.b2, st.eps, ptr(loss_hist), ptr(ws), ws.numel(),
                                           ptr(out), ptr(info), int(nsteps)), "mfgp_gpr_adam_steps")

    def set_step_fusion(self, enable: bool):
        """gpr_adam_steps: defer each step's reduction into the next flow launch (default on; env
        MFGP_STEP_FUSION=0 turns it off for handles created afterwards)."""
        self._set_mode(self.lib.mfgp_set_step_fusion, 1 if enable else 0)

    def theta_from_u(self, u: torch.Tensor, theta: torch.Tensor, noise_index: int):
        check(self.lib.mfgp_theta_from_u(self.h, ptr(u), ptr(theta), u.numel(), noise_index), "mfgp_theta_from_u")

    def gpr_predict(self, X, Y, Xs, theta):
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        ns = Xs.shape[0]
        dt = dtype_code(X)
        nbytes = self._size(self.lib.mfgp_gpr_predict_workspace_size_ex, dt, n, p, d, ns)
        ws = self.workspace("pred" if X.dtype == torch.float64 else "pred32", nbytes)
        mean = torch.empty((ns, p), dtype=X.dtype, device=self.device)
        var = torch.empty((ns,), dtype=X.dtype, device=self.device)
        info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gpr_predict_ex(self.h, dt, n, p, d, ns, ptr(X), dp1, ptr(Y), p, ptr(Xs), Xs.shape[1],
                                           ptr(theta), ptr(ws), ws.numel(), ptr(mean), p, ptr(var), ptr(info)),
              "mfgp_gpr_predict_ex")
        return mean, var, info

    def gpr_predict_cov(self, nlf, X, Y, Xs, theta):
        """predict_f(full_cov=True): mean [ns, p], var [ns], cov [ns, ns] in X's dtype (nlf 0: linear
        MF kernel; float32 only for nlf 0)."""
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        ns = Xs.shape[0]
        dt = dtype_code(X)
        nbytes = self._size(self.lib.mfgp_gpr_predict_cov_workspace_size_ex, dt, nlf, n, p, d, ns)
        ws = self.workspace("pred_cov" if X.dtype == torch.float64 else "pred_cov32", nbytes)
        mean = torch.empty((ns, p), dtype=X.dtype, device=self.device)
        var = torch.empty((ns,), dtype=X.dtype, device=self.device)
        cov = torch.empty((ns, ns), dtype=X.dtype, device=self.device)
        info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gpr_predict_cov_ex(self.h, dt, nlf, n, p, d, ns, ptr(X), dp1, ptr(Y), p, ptr(Xs),
                                               Xs.shape[1], ptr(theta), ptr(ws), ws.numel(), ptr(mean), p, ptr(var),
                                               ptr(cov), ns, ptr(info)), "mfgp_gpr_predict_cov_ex")
        return mean, var, cov, info

    # ---- GraphMultiFidelityKernel (graph.py) with nlf LF sources
    def gmf_gram(self, nlf, X1, X2, theta, diag_add=0.0):
        n1, dp1 = X1.shape
        n2 = X2.shape[0]
        K = torch.empty((n1, n2), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_gmf_gram(self.h, nlf, n1, n2, dp1 - 1, ptr(X1), dp1, ptr(X2), X2.shape[1], ptr(theta),
                                     float(diag_add), ptr(K), n2), "mfgp_gmf_gram")
        return K

    def gmf_kdiag(self, nlf, X, theta):
        n, dp1 = X.shape
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_gmf_kdiag(self.h, nlf, n, dp1 - 1, ptr(X), dp1, ptr(theta), ptr(out)), "mfgp_gmf_kdiag")
        return out

    def gmf_workspace_bytes(self, nlf, n, p, d) -> int:
        return self._size(self.lib.mfgp_gmf_gpr_workspace_size, nlf, n, p, d)

    def gmf_lml(self, nlf, X, Y, theta, want_grad=False, out=None, info=None, ws=None):
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        nbytes = self.gmf_workspace_bytes(nlf, n, p, d)
        if ws is None:
            ws = self.workspace("gmf", nbytes)
        elif ws.numel() < nbytes:
            raise MFGPError("gmf_lml: private workspace too small")
        if out is None:
            out = torch.empty((1 + theta.numel(),), dtype=torch.float64, device=self.device)
        if info is None:
            info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gmf_gpr_lml(self.h, nlf, n, p, d, ptr(X), dp1, ptr(Y), p, ptr(theta), int(want_grad),
                                        ptr(ws), ws.numel(), ptr(out), ptr(info)), "mfgp_gmf_gpr_lml")
        return out, info

    def gmf_predict(self, nlf, X, Y, Xs, theta):
        n, dp1 = X.shape
        p = Y.shape[1]
        d = dp1 - 1
        ns = Xs.shape[0]
        nbytes = self._size(self.lib.mfgp_gmf_gpr_predict_workspace_size, nlf, n, p, d, ns)
        ws = self.workspace("gmf_pred", nbytes)
        mean = torch.empty((ns, p), dtype=torch.float64, device=self.device)
        var = torch.empty((ns,), dtype=torch.float64, device=self.device)
        info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gmf_gpr_predict(self.h, nlf, n, p, d, ns, ptr(X), dp1, ptr(Y), p, ptr(Xs), Xs.shape[1],
                                            ptr(theta), ptr(ws), ws.numel(), ptr(mean), p, ptr(var), ptr(info)),
              "mfgp_gmf_gpr_predict")
        return mean, var, info

    def potrf_inv(self, A: torch.Tensor):
        """A: [n, n] or [b, n, n] SPD -> (Linv, diag(L), info[b])."""
        batched = A.dim() == 3
        A3 = A if batched else A.unsqueeze(0)
        A3 = A3.contiguous()
        b, n, _ = A3.shape
        nbytes = self._size(self.lib.mfgp_potrf_inv_workspace_size, n, b)
        ws = self.workspace("potrf", nbytes)
        Linv = torch.empty_like(A3)
        ld = torch.empty((b, n), dtype=torch.float64, device=self.device)
        info = torch.empty((b,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_potrf_inv(self.h, n, b, ptr(A3), n, n * n, ptr(ws), ws.numel(), ptr(Linv), n, n * n,
                                      ptr(ld), ptr(info)), "mfgp_potrf_inv")
        if not batched:
            return Linv[0], ld[0], info
        return Linv, ld, info

    def mvn_sample(self, cov: torch.Tensor, mean: torch.Tensor, eps: torch.Tensor, ncol: int, jitter: float = 1e-6):
        """Joint draws (include/mfgp.h mfgp_mvn_sample): cov [B, n, n] (any row / batch stride, unit
        inner stride; only the lower triangles are read), mean [n, B * ncol], eps [S, n, B * ncol] ->
        (out [S, n, B * ncol], info [B]), out[s, :, b * ncol + c] = mean[:, b * ncol + c] +
        chol(cov[b] + jitter I) @ eps[s, :, b * ncol + c].  One factor per batch entry serves its ncol
        columns: GPR is B = 1, ncol = P; SVGP is B = P, ncol = 1.  No host read of a device word."""
        if cov.dim() != 3 or cov.shape[1] != cov.shape[2]:
            raise ValueError(f"mvn_sample: cov has shape {tuple(cov.shape)}, expected [B, n, n]")
        b, n, _ = cov.shape
        w = b * int(ncol)
        if mean.shape != (n, w) or eps.dim() != 3 or tuple(eps.shape[1:]) != (n, w):
            raise ValueError(f"mvn_sample: mean {tuple(mean.shape)} / eps {tuple(eps.shape)} do not match "
                             f"[{n}, {w}] / [S, {n}, {w}]")
        if n > 1 and (cov.stride(2) != 1 or cov.stride(1) < n):
            cov = cov.contiguous()
        ldc = max(cov.stride(1), n, 1)
        sC = cov.stride(0) if b > 1 else 0
        mean, eps = mean.contiguous(), eps.contiguous()
        ns = eps.shape[0]
        out = torch.empty_like(eps)
        info = torch.zeros((b,), dtype=torch.int32, device=self.device)
        ws = self.workspace("mvn_sample", self._size(self.lib.mfgp_mvn_sample_workspace_size, n, b))
        check(self.lib.mfgp_mvn_sample(self.h, n, b, ns, int(ncol), ptr(cov), ldc, sC, float(jitter), ptr(mean), w,
                                       int(ncol), ptr(eps), ptr(out), w, n * w, int(ncol), ptr(ws), ws.numel(),
                                       ptr(info)), "mfgp_mvn_sample")
        return out, info

    def _density_args(self, what, ns, p, Y, obs_var, obs_cov):
        """The Y / obs_var / obs_cov arguments of mfgp_mvn_logpdf and the fused posterior entries as
        (tensors kept alive, (Y, y_rs, obs_var, ov_rs, obs_cov, ldc)): fp64 device tensors, Y [p] or [ns, p],
        obs_var None / [p] / [ns, p], obs_cov None / [p, p] (unit inner stride; a row stride >= p is passed
        on as ldc, so a block of a wider matrix is read in place)."""
        def rows(t, name):
            if t.dim() == 1 and t.shape[0] == p:
                return t.contiguous(), 0
            if t.dim() == 2 and tuple(t.shape) == (ns, p):
                return t.contiguous(), p
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected ({p},) or ({ns}, {p})")
        Y, y_rs = rows(Y, "Y")
        ov, ov_rs = (None, 0) if obs_var is None else rows(obs_var, "obs_var")
        ldc = 0
        if obs_cov is not None:
            if tuple(obs_cov.shape) != (p, p):
                raise ValueError(f"{what}: obs_cov has shape {tuple(obs_cov.shape)}, expected ({p}, {p})")
            if p > 128:
                raise ValueError(f"{what}: the dense form (obs_cov) is built for P <= 128 outputs, got {p}")
            if (p > 1 and obs_cov.stride(1) != 1) or obs_cov.stride(0) < p:
                obs_cov = obs_cov.contiguous()
            ldc = max(obs_cov.stride(0), p)
        return (Y, ov, obs_cov), (ptr(Y), y_rs, ptr(ov), ov_rs, ptr(obs_cov), ldc)

    def mvn_logpdf(self, mean, Y, var, obs_var=None, obs_cov=None, grad=False, sum_gvar=False):
        """Batched Gaussian log-density (include/mfgp.h mfgp_mvn_logpdf): mean [ns, p], Y [p] (shared) or
        [ns, p], var [ns] (one variance per row, GPR) or [ns, p], obs_var / obs_cov as _density_args ->
        (logp [ns], gmean, gvar, info [ns] int32).  grad: gmean [ns, p] = d logp / d mean and gvar [ns, p]
        = d logp / d var per output; sum_gvar (var [ns] only): gvar [ns], the kernel's own fixed-order sum
        over the outputs (what the GPR VJP takes).  Without grad both are None.  obs_cov None: the diagonal
        form, NaN targets left out.  No host read of a device word."""
        if mean.dim() != 2:
            raise ValueError(f"mvn_logpdf: mean has shape {tuple(mean.shape)}, expected [ns, p]")
        ns, p = mean.shape
        if var.dim() == 1 and var.shape[0] == ns:
            var_rs, var_cs = 1, 0
        elif tuple(var.shape) == (ns, p):
            var_rs, var_cs = p, 1
        else:
            raise ValueError(f"mvn_logpdf: var has shape {tuple(var.shape)}, expected ({ns},) or ({ns}, {p})")
        if sum_gvar and var_cs != 0:
            raise ValueError("mvn_logpdf: sum_gvar needs var [ns] (one variance per row)")
        keep, dargs = self._density_args("mvn_logpdf", ns, p, Y, obs_var, obs_cov)
        mean, var = mean.contiguous(), var.contiguous()
        f64 = dict(dtype=torch.float64, device=self.device)
        logp = torch.empty((ns,), **f64)
        info = torch.zeros((ns,), dtype=torch.int32, device=self.device)
        gmean = torch.empty((ns, p), **f64) if grad else None
        gvar = torch.empty((ns,) if sum_gvar else (ns, p), **f64) if grad else None
        ws = self.workspace("mvn_logpdf", self._size(self.lib.mfgp_mvn_logpdf_workspace_size, ns, p))
        check(self.lib.mfgp_mvn_logpdf(self.h, ns, p, ptr(mean), p, dargs[0], dargs[1], ptr(var), var_rs, var_cs,
                                       *dargs[2:], ptr(ws), ws.numel(), ptr(logp), ptr(gmean), p, ptr(gvar),
                                       1 if sum_gvar else p, ptr(info)), "mfgp_mvn_logpdf")
        return logp, gmean, gvar, info

    @staticmethod
    def _check_yunc(Yunc, Y, n, p):
        """The heteroscedastic entry points' Yunc: fp64 [n, >= p] on Y's device, unit inner stride."""
        assert Yunc.dtype == torch.float64, "Yunc must be float64"
        assert Yunc.device == Y.device, "Yunc must live on Y's device"
        assert Yunc.dim() == 2 and Yunc.shape[0] == n and Yunc.shape[1] >= p, f"Yunc must be [{n}, >= {p}]"
        assert Yunc.stride(1) == 1 and Yunc.stride(0) >= p, "Yunc needs a unit inner stride"

    @staticmethod
    def _check_masked(noise, Y, Yunc, p):
        """The masked entry points' noise: an fp64 device vector of 1 or p entries; no Yunc with a mask."""
        assert Yunc is None, "Yunc together with a mask is not supported"
        assert torch.is_tensor(noise) and noise.dtype == torch.float64, "masked: noise must be a float64 tensor"
        assert noise.device == Y.device and noise.is_contiguous(), "masked: noise must be contiguous on Y's device"
        assert noise.numel() in (1, p), f"masked: noise must have 1 or {p} entries, got {noise.numel()}"
        assert Y.stride(1) == 1 and Y.stride(0) >= p, "Y needs a unit inner stride"

    def svgp_elbo(self, X, Y, Z, thetas, q_mu, q_sqrt, W, noise, scale, jitter=1e-6, Yunc=None, masked=False):
        """SVGP ELBO value; with Yunc [n, >= p] the HeteroscedasticGaussian one (noise + Yunc**2 per
        observation, mfgp_svgp_elbo_het), where Y may be a row-strided view (the [N, 2P] targets' halves).
        masked: the MaskedGaussian one (mfgp_svgp_elbo_masked): NaN targets are missing observations and
        noise is a DEVICE tensor of 1 or p variances; Y may be a row-strided view."""
        n, dp1 = X.shape
        d = dp1 - 1
        p = Y.shape[1]
        m = Z.shape[0]
        L = thetas.shape[0]
        nbytes = self._size(self.lib.mfgp_svgp_workspace_size, n, m, L, p, d)
        ws = self.workspace("svgp", nbytes)
        out = torch.empty((3,), dtype=torch.float64, device=self.device)
        g_mu = torch.empty((L, n), dtype=torch.float64, device=self.device)
        g_var = torch.empty((L, n), dtype=torch.float64, device=self.device)
        info = torch.empty((L,), dtype=torch.int32, device=self.device)
        if masked:
            self._check_masked(noise, Y, Yunc, p)
            check(self.lib.mfgp_svgp_elbo_masked(self.h, n, m, L, p, d, ptr(X), dp1, ptr(Y), Y.stride(0), ptr(Z),
                                                 Z.shape[1], ptr(thetas), ptr(q_mu), ptr(q_sqrt), ptr(W), ptr(noise),
                                                 noise.numel(), float(scale), float(jitter), ptr(ws), ws.numel(),
                                                 ptr(out), ptr(g_mu), ptr(g_var), ptr(info)),
                  "mfgp_svgp_elbo_masked")
            return out, g_mu, g_var, info
        if Yunc is not None:
            self._check_yunc(Yunc, Y, n, p)
            assert Y.stride(1) == 1, "Y needs a unit inner stride"
            check(self.lib.mfgp_svgp_elbo_het(self.h, n, m, L, p, d, ptr(X), dp1, ptr(Y), Y.stride(0), ptr(Yunc),
                                              Yunc.stride(0), ptr(Z), Z.shape[1], ptr(thetas), ptr(q_mu),
                                              ptr(q_sqrt), ptr(W), float(noise), float(scale), float(jitter),
                                              ptr(ws), ws.numel(), ptr(out), ptr(g_mu), ptr(g_var), ptr(info)),
                  "mfgp_svgp_elbo_het")
            return out, g_mu, g_var, info
        check(self.lib.mfgp_svgp_elbo(self.h, n, m, L, p, d, ptr(X), dp1, ptr(Y), p, ptr(Z), Z.shape[1],
                                      ptr(thetas), ptr(q_mu), ptr(q_sqrt), ptr(W), float(noise), float(scale),
                                      float(jitter), ptr(ws), ws.numel(), ptr(out), ptr(g_mu), ptr(g_var),
                                      ptr(info)), "mfgp_svgp_elbo")
        return out, g_mu, g_var, info

    def svgp_grad_workspace_bytes(self, n, m, L, p, d) -> int:
        return self._size(self.lib.mfgp_svgp_grad_workspace_size, n, m, L, p, d)

    def svgp_elbo_grad(self, X, Y, Z, thetas, q_mu, q_sqrt, W, noise, scale, kl_mult, jitter, out, g_mu, g_var,
                       gZ, gtheta, gq_mu, gq_sqrt, gW, gnoise, info, ws=None, qs_packed=False, Yunc=None,
                       masked=False):
        """Gradient of VE*scale - kl_mult*KL w.r.t. the constrained SVGP parameters (all device
        tensors, written in place; noise is a device scalar).  qs_packed: q_sqrt and gq_sqrt are
        packed lower triangles [L, M(M+1)/2] (mfgp_set_svgp_qs_packed), else [L, M, M].  Yunc
        [n, >= p]: the HeteroscedasticGaussian likelihood (mfgp_svgp_elbo_grad_het, which takes
        qs_packed as an argument, not from the handle).  masked: the MaskedGaussian likelihood
        (mfgp_svgp_elbo_grad_masked, qs_packed likewise an argument): NaN targets are missing
        observations, noise and gnoise have 1 or p entries."""
        n, dp1 = X.shape
        d = dp1 - 1
        p = Y.shape[1]
        m = Z.shape[0]
        L = thetas.shape[0]
        nbytes = self.svgp_grad_workspace_bytes(n, m, L, p, d)
        if ws is None:
            ws = self.workspace("svgp_grad", nbytes)
        elif ws.numel() < nbytes:
            raise MFGPError("svgp_elbo_grad: private workspace too small")
        h = self.h
        if masked:
            self._check_masked(noise, Y, Yunc, p)
            assert gnoise.numel() == noise.numel() and gnoise.is_contiguous(), "masked: gnoise must match noise"
            check(self.lib.mfgp_svgp_elbo_grad_masked(h, n, m, L, p, d, ptr(X), dp1, ptr(Y), Y.stride(0), ptr(Z), dp1,
                                                      ptr(thetas), ptr(q_mu), ptr(q_sqrt), 1 if qs_packed else 0,
                                                      ptr(W), ptr(noise), noise.numel(), float(scale), float(kl_mult),
                                                      float(jitter), ptr(ws), ws.numel(), ptr(out), ptr(g_mu),
                                                      ptr(g_var), ptr(gZ), ptr(gtheta), ptr(gq_mu), ptr(gq_sqrt),
                                                      ptr(gW), ptr(gnoise), ptr(info)),
                  "mfgp_svgp_elbo_grad_masked")
            return
        if Yunc is not None:
            self._check_yunc(Yunc, Y, n, p)
            assert Y.stride(1) == 1, "Y needs a unit inner stride"
            check(self.lib.mfgp_svgp_elbo_grad_het(h, n, m, L, p, d, ptr(X), dp1, ptr(Y), Y.stride(0), ptr(Yunc),
                                                   Yunc.stride(0), ptr(Z), dp1, ptr(thetas), ptr(q_mu), ptr(q_sqrt),
                                                   1 if qs_packed else 0, ptr(W), ptr(noise), float(scale),
                                                   float(kl_mult), float(jitter), ptr(ws), ws.numel(), ptr(out),
                                                   ptr(g_mu), ptr(g_var), ptr(gZ), ptr(gtheta), ptr(gq_mu),
                                                   ptr(gq_sqrt), ptr(gW), ptr(gnoise), ptr(info)),
                  "mfgp_svgp_elbo_grad_het")
            return
        check(self.lib.mfgp_set_svgp_qs_packed(h, 1 if qs_packed else 0), "mfgp_set_svgp_qs_packed")
        try:
            check(self.lib.mfgp_svgp_elbo_grad(h, n, m, L, p, d, ptr(X), dp1, ptr(Y), Y.stride(0), ptr(Z), dp1,
                                               ptr(thetas), ptr(q_mu), ptr(q_sqrt), ptr(W), ptr(noise), float(scale),
                                               float(kl_mult), float(jitter), ptr(ws), ws.numel(), ptr(out),
                                               ptr(g_mu), ptr(g_var), ptr(gZ), ptr(gtheta), ptr(gq_mu), ptr(gq_sqrt),
                                               ptr(gW), ptr(gnoise), ptr(info)), "mfgp_svgp_elbo_grad")
        finally:
            check(self.lib.mfgp_set_svgp_qs_packed(h, 0), "mfgp_set_svgp_qs_packed")

    def adam_packed(self, u, c, g, m, v, trainable, transform, span, step, lr_sched, b1, b2, eps, out, kl_mult,
                    loss_hist, kl_hist, info=None):
        """One packed Keras-Adam step; with `info` (the evaluation's int32 info words) a failed
        evaluation leaves the parameters and the step counter unchanged (mfgp_adam_packed_ex)."""
        check(self.lib.mfgp_adam_packed_ex(self.h, u.numel(), ptr(u), ptr(c), ptr(g), ptr(m), ptr(v), ptr(trainable),
                                           ptr(transform), ptr(span), ptr(step), ptr(lr_sched), float(b1), float(b2),
                                           float(eps), ptr(out), float(kl_mult), ptr(loss_hist), ptr(kl_hist),
                                           ptr(info), 0 if info is None else info.numel()),
              "mfgp_adam_packed_ex")

    def svgp_predict(self, Xs, Z, thetas, q_mu, q_sqrt, W, p, jitter=1e-6):
        ns, dp1 = Xs.shape
        d = dp1 - 1
        m = Z.shape[0]
        L = thetas.shape[0]
        nbytes = self._size(self.lib.mfgp_svgp_workspace_size, ns, m, L, p, d)
        ws = self.workspace("svgp_pred", nbytes)
        g_mu = torch.empty((L, ns), dtype=torch.float64, device=self.device)
        g_var = torch.empty((L, ns), dtype=torch.float64, device=self.device)
        f_mu = torch.empty((ns, p), dtype=torch.float64, device=self.device)
        f_var = torch.empty((ns, p), dtype=torch.float64, device=self.device)
        info = torch.empty((L,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_svgp_predict(self.h, ns, m, L, p, d, ptr(Xs), dp1, ptr(Z), Z.shape[1], ptr(thetas),
                                         ptr(q_mu), ptr(q_sqrt), ptr(W), float(jitter), ptr(ws), ws.numel(),
                                         ptr(g_mu), ptr(g_var), ptr(f_mu), ptr(f_var), ptr(info)),
              "mfgp_svgp_predict")
        return f_mu, f_var, g_mu, g_var, info

    def svgp_predict_cov(self, mode, Xs, Z, thetas, q_mu, q_sqrt, W, p, jitter=1e-6):
        """SVGP predict_f covariance forms (include/mfgp.h mfgp_svgp_predict_cov): mode 1 full_cov
        -> f_cov [p, ns, ns]; 2 full_output_cov -> [ns, p, p]; 3 both -> [ns, p, ns, p]."""
        ns, dp1 = Xs.shape
        d = dp1 - 1
        m = Z.shape[0]
        L = thetas.shape[0]
        nbytes = self._size(self.lib.mfgp_svgp_predict_cov_workspace_size, ns, m, L, p, d)
        ws = self.workspace("svgp_pred_cov", nbytes)
        f64 = dict(dtype=torch.float64, device=self.device)
        g_mu, g_var = torch.empty((L, ns), **f64), torch.empty((L, ns), **f64)
        f_mu, f_var = torch.empty((ns, p), **f64), torch.empty((ns, p), **f64)
        shape = {1: (p, ns, ns), 2: (ns, p, p), 3: (ns, p, ns, p)}[mode]
        f_cov = torch.empty(shape, **f64)
        info = torch.empty((L,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_svgp_predict_cov(self.h, mode, ns, m, L, p, d, ptr(Xs), dp1, ptr(Z), Z.shape[1],
                                             ptr(thetas), ptr(q_mu), ptr(q_sqrt), ptr(W), float(jitter), ptr(ws),
                                             ws.numel(), ptr(g_mu), ptr(g_var), ptr(f_mu), ptr(f_var), ptr(f_cov),
                                             ptr(info)), "mfgp_svgp_predict_cov")
        return f_mu, f_cov, info

    # ---- cached posterior (posteriors.py).  `cache` is the uint8 device block its caller owns, `shape`
    # what it was built for: GPR (n, p, d), SVGP (m, L, p, d, mixed).  The calls behind the two builds
    # read only that block and their arguments: no parameter upload, no host read of a device word.
    def gpr_posterior_bytes(self, nlf, n, p, d) -> int:
        return self._size(self.lib.mfgp_gpr_posterior_size, nlf, n, p, d)

    def gpr_posterior_build(self, nlf, X, Y, theta, cache):
        """Fill `cache` (>= gpr_posterior_bytes) from the data and theta; returns the factorization's info [1]."""
        n, dp1 = X.shape
        p, d = Y.shape[1], dp1 - 1
        ws = self.workspace("pred_cov", self._size(self.lib.mfgp_gpr_predict_cov_workspace_size, nlf, n, p, d, 1))
        info = torch.empty((1,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_gpr_posterior_build(self.h, nlf, n, p, d, ptr(X), dp1, ptr(Y), p, ptr(theta), ptr(ws),
                                                ws.numel(), ptr(cache), cache.numel(), ptr(info)),
              "mfgp_gpr_posterior_build")
        return info

    def _posterior_run(self, name, key, dims, head, tail):
        """name(h, *head, ws, ws_bytes, *tail) on the workspace `key`, sized by name_workspace_size(h, *dims)."""
        h, nbytes = self.h, C.c_size_t(0)
        check(getattr(self.lib, name + "_workspace_size")(h, *dims, C.byref(nbytes)), name + "_workspace_size")
        ws = self.workspace(key, nbytes.value)
        check(getattr(self.lib, name)(h, *head, ptr(ws), ws.numel(), *tail), name)

    # The forward entries (predict, predict_vjp, logdens) of the two families share their shape: the integers
    # `dims` of their size query first -- GPR (nlf, n, p, d, ns), SVGP (ns, m, L, p, d) -- then `flags` (SVGP:
    # mixed), the cache, Xs, the workspace, mean (GPR: with its leading dimension), var (GPR [ns], SVGP [ns, p]).
    def _posterior_predict(self, fam, dims, flags, p, d, cache, Xs, full_cov, grad, out):
        gpr = fam == "gpr"
        ns = Xs.shape[0]
        if out is None:
            f64 = dict(dtype=torch.float64, device=self.device)
            third = (ns, d + 1) if grad is not None else (ns, ns) if full_cov else None
            out = (torch.empty((ns, p), **f64), torch.empty((ns,) if gpr else (ns, p), **f64),
                   None if third is None else torch.empty(third, **f64))
        mean, var, third = out
        if ns == 0:
            return out
        head = (*dims, *flags, ptr(cache), cache.numel(), ptr(Xs), Xs.shape[1])
        outs = (ptr(mean), p, ptr(var)) if gpr else (ptr(mean), ptr(var))
        # the two entries share their arguments up to var; then (GPR) cov, ldc / gmean, ldgm, gvar, gX, ldgx
        if grad is None:
            self._posterior_run(f"mfgp_{fam}_posterior_predict", "post_pred", dims, head,
                                outs + (ptr(third), ns) if gpr else outs)
        else:
            self._posterior_run(f"mfgp_{fam}_posterior_predict_vjp", "post_vjp", dims, head,
                                outs + (ptr(grad[0]), p, ptr(grad[1]), ptr(third), d + 1))
        return out

    def _posterior_logdens(self, fam, dims, flags, p, d, cache, Xs, Y, obs_var, obs_cov, grad):
        gpr = fam == "gpr"
        ns = Xs.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        mean, var = torch.empty((ns, p), **f64), torch.empty((ns,) if gpr else (ns, p), **f64)
        logp = torch.empty((ns,), **f64)
        gX = torch.empty((ns, d + 1), **f64) if grad else None
        info = torch.zeros((ns,), dtype=torch.int32, device=self.device)
        keep, dargs = self._density_args("log_density", ns, p, Y, obs_var, obs_cov)
        if ns:
            head = (*dims, *flags, ptr(cache), cache.numel(), ptr(Xs), Xs.shape[1])
            outs = (ptr(mean), p, ptr(var)) if gpr else (ptr(mean), ptr(var))
            self._posterior_run(f"mfgp_{fam}_posterior_logdens", "post_logdens", dims, head,
                                (*outs, *dargs, ptr(logp), ptr(gX), d + 1, ptr(info)))
        return mean, var, logp, gX, info

    def gpr_posterior_predict(self, nlf, shape, cache, Xs, full_cov=False, grad=None, out=None):
        """(mean [ns, p], var [ns], third): third is cov [ns, ns] with full_cov, else None.  grad =
        (grad_mean [ns, p], grad_var [ns]), either may be None (zero): the VJP call, third is the gradient
        w.r.t. Xs [ns, d + 1].  out: the three result tensors, preallocated."""
        n, p, d = shape
        return self._posterior_predict("gpr", (nlf, n, p, d, Xs.shape[0]), (), p, d, cache, Xs, full_cov, grad, out)

    def gpr_posterior_leave_out(self, nlf, shape, cache, offsets, rows, gmax, out=None):
        """Leave-group-out from the cache: int32 device offsets [G + 1] and rows [R] (group g is
        rows[offsets[g]:offsets[g + 1]], at most gmax rows) -> (resid [R, p], cov [R, gmax], logdens [G, p],
        info [G]).  out: those four, preallocated."""
        n, p, d = shape
        ng, nr = offsets.shape[0] - 1, rows.shape[0]
        if out is None:
            f64 = dict(dtype=torch.float64, device=self.device)
            out = (torch.empty((nr, p), **f64), torch.empty((nr, gmax), **f64), torch.empty((ng, p), **f64),
                   torch.empty((ng,), dtype=torch.int32, device=self.device))
        resid, cov, logd, info = out
        self._posterior_run("mfgp_gpr_posterior_leave_out", "post_lo", (nlf, n, p, d, ng, nr),
                            (nlf, n, p, d, ptr(cache), cache.numel(), ng, ptr(offsets), ptr(rows), nr, gmax),
                            (ptr(resid), p, ptr(cov), gmax, ptr(logd), ptr(info)))
        return out

    def gpr_posterior_design_workspace(self, nlf, shape, nref, ncand, qmax) -> torch.Tensor:
        """The workspace of one batch of design calls (it carries the forward's A from score step 0 on)."""
        n, p, d = shape
        return self.workspace("post_design", self._size(self.lib.mfgp_gpr_posterior_design_workspace_size, nlf, n, p,
                                                        d, nref, ncand, qmax))

    def gpr_posterior_design_score(self, nlf, shape, cache, Xall, nref, w, E, k, ws):
        """score [ncand] of the candidates Xall[nref:] over the references Xall[:nref] (weights w or None),
        conditioned on the k rows of E; k == 0 runs the forward on Xall first."""
        n, p, d = shape
        nall = Xall.shape[0]
        score = torch.empty((nall - nref,), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_gpr_posterior_design_score(self.h, nlf, n, p, d, ptr(cache), cache.numel(), ptr(Xall),
                                                       d + 1, nref, nall - nref, ptr(w), ptr(E), nall, k, ptr(ws),
                                                       ws.numel(), ptr(score), 1 if k == 0 else 0),
              "mfgp_gpr_posterior_design_score")
        return score

    def gpr_posterior_design_append(self, nlf, shape, cache, Xall, nref, pick, E, k, ws):
        """Row k of E: the conditioning row of the candidate whose index the int32 device word `pick` holds."""
        n, p, d = shape
        nall = Xall.shape[0]
        check(self.lib.mfgp_gpr_posterior_design_append(self.h, nlf, n, p, d, ptr(cache), cache.numel(), ptr(Xall),
                                                        d + 1, nref, nall - nref, ptr(ws), ws.numel(), ptr(pick),
                                                        ptr(E), nall, k), "mfgp_gpr_posterior_design_append")

    def gpr_posterior_append(self, nlf, shape, cache, Xadd, Yadd, out_cache):
        """Fill `out_cache` (>= gpr_posterior_bytes of n + k rows) with the cache of [X ; Xadd], [Y ; Yadd] from
        the factors in `cache` (Yadd None: the rows are observed at their own mean).  Returns the mean of
        `cache` at Xadd [k, p] and info [1] (int32, device)."""
        n, p, d = shape
        k = Xadd.shape[0]
        mean = torch.empty((k, p), dtype=torch.float64, device=self.device)
        info = torch.empty((1,), dtype=torch.int32, device=self.device)
        self._posterior_run("mfgp_gpr_posterior_append", "post_append", (nlf, n, p, d, k),
                            (nlf, n, p, d, k, ptr(cache), cache.numel(), ptr(Xadd), Xadd.shape[1], ptr(Yadd), p),
                            (ptr(out_cache), out_cache.numel(), ptr(mean), p, ptr(info)))
        return mean, info

    def svgp_posterior_bytes(self, m, L, p, d) -> int:
        return self._size(self.lib.mfgp_svgp_posterior_size, m, L, p, d)

    def svgp_posterior_build(self, Z, thetas, q_mu, q_sqrt, W, p, jitter, cache):
        """Fill `cache` (>= svgp_posterior_bytes) from the variational state; returns the K_uu factorizations' info [L]."""
        m, dp1 = Z.shape
        d, L = dp1 - 1, thetas.shape[0]
        ws = self.workspace("svgp_pred", self._size(self.lib.mfgp_svgp_workspace_size, 1, m, L, p, d))
        info = torch.empty((L,), dtype=torch.int32, device=self.device)
        check(self.lib.mfgp_svgp_posterior_build(self.h, m, L, p, d, ptr(Z), dp1, ptr(thetas), ptr(q_mu), ptr(q_sqrt),
                                                 ptr(W), float(jitter), ptr(ws), ws.numel(), ptr(cache), cache.numel(),
                                                 ptr(info)), "mfgp_svgp_posterior_build")
        return info

    def svgp_posterior_predict(self, shape, cache, Xs, grad=None):
        """(f_mu [ns, p], f_var [ns, p], None); grad = (grad_mean, grad_var), each [ns, p] or None (zero):
        the VJP call, third is the gradient w.r.t. Xs [ns, d + 1]."""
        m, L, p, d, mixed = shape
        return self._posterior_predict("svgp", (Xs.shape[0], m, L, p, d), (1 if mixed else 0,), p, d, cache, Xs,
                                       False, grad, None)

    def gpr_posterior_logdens(self, nlf, shape, cache, Xs, Y, obs_var=None, obs_cov=None, grad=False):
        """mfgp_gpr_posterior_logdens: the forward, the density launch and (grad) k_post_grad in one call ->
        (mean [ns, p], var [ns], logp [ns], grad_X [ns, d + 1] or None, info [ns] int32).  Y / obs_var /
        obs_cov as _density_args.  No host read of a device word."""
        n, p, d = shape
        return self._posterior_logdens("gpr", (nlf, n, p, d, Xs.shape[0]), (), p, d, cache, Xs, Y, obs_var, obs_cov,
                                       grad)

    def svgp_posterior_logdens(self, shape, cache, Xs, Y, obs_var=None, obs_cov=None, grad=False):
        """mfgp_svgp_posterior_logdens -> (f_mu [ns, p], f_var [ns, p], logp [ns], grad_X or None, info [ns])."""
        m, L, p, d, mixed = shape
        return self._posterior_logdens("svgp", (Xs.shape[0], m, L, p, d), (1 if mixed else 0,), p, d, cache, Xs, Y,
                                       obs_var, obs_cov, grad)

    # ---- emulator Jacobian and Fisher matrix (include/mfgp.h mfgp_*_jacobian, mfgp_mvn_fisher)
    def _jacobian_weights(self, fam, dims, flags, cache):
        """alpha of `cache` in a new device buffer (mfgp_*_jacobian_weights: one launch, once per cache block)."""
        nbytes = self._size(getattr(self.lib, f"mfgp_{fam}_jacobian_weights_workspace_size"), *dims)
        w = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        name = f"mfgp_{fam}_jacobian_weights"
        check(getattr(self.lib, name)(self.h, *dims, *flags, ptr(cache), cache.numel(), ptr(w), w.numel()), name)
        return w

    def _jacobian(self, fam, dims, flags, p, d, cache, weights, Xs):
        gpr = fam == "gpr"
        ns = Xs.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        mean, var = torch.empty((ns, p), **f64), torch.empty((ns,) if gpr else (ns, p), **f64)
        J = torch.empty((ns, d, p), **f64)
        if ns:
            head = (*dims, *flags, ptr(cache), cache.numel(), ptr(weights), weights.numel(), ptr(Xs), Xs.shape[1])
            outs = (ptr(mean), p, ptr(var)) if gpr else (ptr(mean), ptr(var))
            self._posterior_run(f"mfgp_{fam}_jacobian", "post_jac", dims, head, (*outs, ptr(J), p))
        return mean, var, J

    def gpr_jacobian_weights(self, shape, cache):
        n, p, d = shape
        return self._jacobian_weights("gpr", (0, n, p, d), (), cache)

    def gpr_jacobian(self, shape, cache, weights, Xs):
        """mfgp_gpr_jacobian: the predict forward and the Jacobian kernel -> (mean [ns, p], var [ns],
        J [ns, d, p], the device layout: outputs fastest).  No host read of a device word."""
        n, p, d = shape
        return self._jacobian("gpr", (0, n, p, d, Xs.shape[0]), (), p, d, cache, weights, Xs)

    def svgp_jacobian_weights(self, shape, cache):
        m, L, p, d, mixed = shape
        return self._jacobian_weights("svgp", (m, L, p, d), (1 if mixed else 0,), cache)

    def svgp_jacobian(self, shape, cache, weights, Xs):
        """mfgp_svgp_jacobian -> (f_mu [ns, p], f_var [ns, p], J [ns, d, p])."""
        m, L, p, d, mixed = shape
        return self._jacobian("svgp", (Xs.shape[0], m, L, p, d), (1 if mixed else 0,), p, d, cache, weights, Xs)

    def mvn_fisher(self, J, var, obs_var=None, obs_cov=None):
        """Batched Fisher matrix (include/mfgp.h mfgp_mvn_fisher): J [ns, d, p] (the Jacobian's device layout),
        var [ns] (one variance per row, GPR) or [ns, p], obs_var None / [p] / [ns, p], obs_cov None / [p, p] ->
        (F [ns, d, d], info [ns] int32).  No host read of a device word."""
        ns, d, p = J.shape
        if var.dim() == 1 and var.shape[0] == ns:
            var_rs, var_cs = 1, 0
        elif tuple(var.shape) == (ns, p):
            var_rs, var_cs = p, 1
        else:
            raise ValueError(f"mvn_fisher: var has shape {tuple(var.shape)}, expected ({ns},) or ({ns}, {p})")
        ov, ov_rs = None, 0
        if obs_var is not None:
            if tuple(obs_var.shape) not in ((p,), (ns, p)):
                raise ValueError(f"mvn_fisher: obs_var has shape {tuple(obs_var.shape)}, expected ({p},) or ({ns}, {p})")
            ov, ov_rs = obs_var.contiguous(), (p if obs_var.dim() == 2 else 0)
        ldc = 0
        if obs_cov is not None:
            if tuple(obs_cov.shape) != (p, p):
                raise ValueError(f"mvn_fisher: obs_cov has shape {tuple(obs_cov.shape)}, expected ({p}, {p})")
            r = ((p + 7) & ~7) + d
            if p > 128 or r * (r | 1) * 8 > 160 * 1024:
                raise ValueError(f"mvn_fisher: the dense form (obs_cov) is built for P <= 128 outputs and P8 + D <= 143, "
                                 f"got P = {p}, D = {d}; use the diagonal form")
            if (p > 1 and obs_cov.stride(1) != 1) or obs_cov.stride(0) < p:
                obs_cov = obs_cov.contiguous()
            ldc = max(obs_cov.stride(0), p)
        J, var = J.contiguous(), var.contiguous()
        F = torch.empty((ns, d, d), dtype=torch.float64, device=self.device)
        info = torch.zeros((ns,), dtype=torch.int32, device=self.device)
        ws = self.workspace("mvn_fisher", self._size(self.lib.mfgp_mvn_fisher_workspace_size, ns, p, d))
        check(self.lib.mfgp_mvn_fisher(self.h, ns, p, d, ptr(J), p, ptr(var), var_rs, var_cs, ptr(ov), ov_rs,
                                       ptr(obs_cov), ldc, ptr(ws), ws.numel(), ptr(F), ptr(info)), "mfgp_mvn_fisher")
        return F, info

    def selftest_mfma(self) -> np.ndarray:
        out = torch.zeros((16, 16), dtype=torch.float64, device=self.device)
        check(self.lib.mfgp_selftest_mfma(self.h, ptr(out)), "mfgp_selftest_mfma")
        return out.cpu().numpy()


class AdamState:
    """Device-resident Keras-Adam state over the unconstrained theta vector."""

    def __init__(self, device, u: np.ndarray, trainable: np.ndarray, tie: np.ndarray, lr: float, b1=0.9, b2=0.999,
                 eps=1e-7):
        f32 = lambda x: float(np.float32(x))   # TF 2.10 OptimizerV2 hyper variables are float32
        self.u = torch.tensor(u, dtype=torch.float64, device=device)
        self.theta = torch.empty_like(self.u)
        self.m = torch.zeros_like(self.u)
        self.v = torch.zeros_like(self.u)
        self.trainable = torch.tensor(trainable.astype(np.uint8), device=device)
        self.tie = torch.tensor(tie.astype(np.int32), device=device)
        self.step = torch.zeros((1,), dtype=torch.int32, device=device)
        self.lr, self.b1, self.b2, self.eps = f32(lr), f32(b1), f32(b2), float(eps)


F32_PHASES = ["gram", "diag", "panel", "update_in", "update_out", "alpha", "grad", "finalize"]


def gpr_phase_times_ex(eng: Engine, X, Y, theta):
    """One value+grad evaluation with hipEvents around every launch (diagnostic).  Returns
    {phase: (ms, flops performed, launches)}: fp32 phases F32_PHASES; fp64 the five of gpr_phase_times."""
    n, dp1 = X.shape
    p = Y.shape[1]
    d = dp1 - 1
    nbytes = eng.gpr_workspace_bytes(n, p, d, X.dtype)
    ws = eng.workspace("gpr" if X.dtype == torch.float64 else "gpr32", nbytes)
    out = torch.empty((1 + theta_size(d),), dtype=torch.float64, device=eng.device)
    info = torch.empty((1,), dtype=torch.int32, device=eng.device)
    k = len(F32_PHASES)
    ms, fl, la = (C.c_float * k)(), (C.c_double * k)(), (C.c_int * k)()
    check(eng.lib.mfgp_gpr_phase_times_ex(eng.h, dtype_code(X), n, p, d, ptr(X), dp1, ptr(Y), p, ptr(theta), ptr(ws),
                                          ws.numel(), ptr(out), ptr(info), ms, fl, la, k), "mfgp_gpr_phase_times_ex")
    names = F32_PHASES if X.dtype == torch.float32 else ["pre", "gram", "chol_steps", "grad", "finalize"]
    return {nm: (float(ms[i]), float(fl[i]), int(la[i])) for i, nm in enumerate(names)}


def gpr_phase_times(eng: Engine, X, Y, theta):
    """Per-phase device times (ms) of one value+grad evaluation, measured with
    hipEvents on the launch stream: [pre, gram, chol_steps (+alpha), grad, finalize]."""
    n, dp1 = X.shape
    p = Y.shape[1]
    d = dp1 - 1
    nbytes = eng._size(eng.lib.mfgp_gpr_workspace_size, n, p, d)
    ws = eng.workspace("gpr", nbytes)
    out = torch.empty((1 + theta_size(d),), dtype=torch.float64, device=eng.device)
    info = torch.empty((1,), dtype=torch.int32, device=eng.device)
    ms = (C.c_float * 5)()
    check(eng.lib.mfgp_gpr_lml_phase_times(eng.h, n, p, d, ptr(X), dp1, ptr(Y), p, ptr(theta), ptr(ws), ws.numel(),
                                           ptr(out), ptr(info), ms), "mfgp_gpr_lml_phase_times")
    return [float(v) for v in ms]
