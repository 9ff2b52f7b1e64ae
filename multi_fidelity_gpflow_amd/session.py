"""What every device-resident training session shares: the dedicated stream, the hipGraph step
runner, the lifetime of the captured graphs, the packed Keras-Adam state and the diagnosis of a
finished run.  This is the one place where a session's stream, capture and graph lifetime are
decided; models.py, graph.py, svgp.py and distributed.py keep only their own buffers, step and
read-back.  Imports nothing from those four.
"""
from __future__ import annotations

import atexit
import contextlib
import weakref

import numpy as np
import torch

from ._lib import MFGP_FLOW_TIMEOUT, MFGPError, info_error


class CholeskyError(MFGPError):
    """Analogue of TF's InvalidArgumentError('Cholesky decomposition was not successful')."""


# ---------------------------------------------------------------- retired step graphs
# The captured step graphs of a closed, released or dropped session are not destroyed before the
# interpreter exits; they are kept here (no buffers: a graph holds no reference to the tensors it
# was captured on).  Reason: in the HIP runtime this image ships (libamdhip64 of
# ROCm 7.0.2, GPU_MAX_HW_QUEUES = 4), instantiating a graph with parallel branches (the fp32
# lookahead's and the SVGP gradient's fork / join) acquires hardware queues for its internal branch
# streams, shared by reference count with user streams; destroying such a graph exec after a later
# user stream came to share one of those queues made the next hipGraphLaunch on it segfault
# (tools/graph_lifetime_probe.py small_graphs_after: the fifth session's first replay, every run,
# with AMD_LOG_LEVEL=3 showing the exec's releaseQueue on the queue the new session's stream
# holds; never with the graphs kept).  A retired graph costs its exec's host nodes and kernel
# arguments (a few hundred KB at the Synth size); release_retired_graphs() frees them when the
# caller knows that no captured graph will be launched again in the process.
_retired_graphs: list = []   # models.py re-exports this very list: mutate it, never rebind it


def _retire_graphs(graphs: dict):
    if graphs:
        _retired_graphs.extend(graphs.values())
        graphs.clear()


def release_retired_graphs():
    """Destroy the retired step graphs now (see above: only when no captured graph is launched in
    this process afterwards).  Returns how many were destroyed."""
    n = len(_retired_graphs)
    if n and torch.cuda.is_available():
        torch.cuda.synchronize()
    _retired_graphs.clear()
    return n


# atexit runs the last registered handler first: models.py imports this module before it registers
# clear_session_pool, so at exit the pool is cleared first and the retired graphs are released last
atexit.register(lambda: release_retired_graphs())


class _StepRunner:
    """Runs a step function n times: eagerly, or replaying a hipGraph of `chunk`
    captured steps (torch.cuda.CUDAGraph is the HIP graph API on ROCm).

    Graph lifetime is deterministic: the runner holds its session's step method weakly (no
    session <-> runner reference cycle), so a session and its hipGraphExecs are freed by
    reference counting the moment the last reference goes, or at close() -- never by a cyclic
    collection that could run in the middle of another session's capture (destroying a graph
    while a stream captures is illegal and aborts the process)."""

    def __init__(self, step, chunk: int, graphs: dict = None, steps=None):
        hold = lambda fn: weakref.WeakMethod(fn) if hasattr(fn, "__self__") else (lambda f=fn: f)
        self._step = hold(step)
        # optional steps(n): n steps in ONE call (a session whose library entry runs several);
        # called once per captured chunk and once for an eager remainder instead of step() n times
        self._steps = hold(steps) if steps is not None else None
        self.chunk = chunk
        self._owns = graphs is None
        self.graphs = {} if graphs is None else graphs

    def step(self):
        fn = self._step()
        if fn is None:
            raise MFGPError("the training session of this step runner was released")
        fn()

    def steps(self, n: int):
        if self._steps is None:
            for _ in range(n):
                self.step()
            return
        fn = self._steps()
        if fn is None:
            raise MFGPError("the training session of this step runner was released")
        fn(n)

    def close(self):
        """Release the captured graphs now (retired until exit, see release_retired_graphs)."""
        _retire_graphs(self.graphs)

    def __del__(self):
        # a dropped runner's own graphs are retired too, not destroyed by reference counting (a
        # session's graphs belong to its _AdamCore, which retires them itself)
        if getattr(self, "_owns", False):
            _retire_graphs(self.graphs)

    def _graph(self, n):
        g = self.graphs.get(n)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.steps(n)
            self.graphs[n] = g
        return g

    def prepare(self, n: int):
        """Capture (without running) every graph that run(n) will replay, so a later
        run(n) is replay-only (bench.py captures before its timed region)."""
        if self.chunk <= 0 or n < 4:
            return
        full, rem = divmod(n, self.chunk)
        if full:
            self._graph(self.chunk)
        if rem >= 4:
            self._graph(rem)

    def run(self, n: int):
        if self.chunk <= 0 or n < 4:
            self.steps(n)
            return
        full, rem = divmod(n, self.chunk)
        for _ in range(full):
            self._graph(self.chunk).replay()
        if rem:
            if rem < 4:
                self.steps(rem)
            else:
                self._graph(rem).replay()


def new_stream(device) -> torch.cuda.Stream:
    """A session's stream: new, and ordered after the work already on the caller's current one."""
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    return stream


class _Session:
    """Base of every training session: `max_iters` steps of the subclass's _step(), run on the
    session's stream and replayed from hipGraphs of `chunk` steps (0: eagerly).

    stream: None makes a new one on eng's device (new_stream); an existing stream is used as it is
    (SharedInducingTrainer runs on its inner trainer's); with no eng either there is no stream (the
    CPU rehearsal of the shared trainers with injected hooks).  warm=False: the first step of the
    first run() runs eagerly before anything is captured."""

    fence = False   # whether run() holds the device-wide flow fence (Engine.ordered) for its steps

    def __init__(self, eng, max_iters, chunk, stream=None, graphs=None, warm=True):
        self.eng = eng
        self.max_iters = max(int(max_iters), 1)
        self.stream = new_stream(eng.device) if stream is None and eng is not None else stream
        self.runner = _StepRunner(self._step, chunk, graphs=graphs, steps=getattr(self, "_steps", None))
        self.done = 0
        self._warm = warm

    def _ctx(self, fence=None):
        """The session's stream, and the flow fence where the class launches flows (fence=False:
        the stream alone, for set-up and capture)."""
        if self.stream is None:
            return contextlib.nullcontext()
        if self.fence if fence is None else fence:
            return self._fenced()
        return torch.cuda.stream(self.stream)

    @contextlib.contextmanager
    def _fenced(self):
        with torch.cuda.stream(self.stream), self.eng.ordered(self.stream):
            yield

    def _count(self, n):
        self.done += n

    def run(self, n: int):
        if self.done + n > self.max_iters:
            raise ValueError(f"{type(self).__name__}: more iterations than max_iters")
        if n <= 0:
            return
        with self._ctx():
            if not self._warm:
                # the first step runs eagerly: the communicator, the workspace set-up and the
                # kernels' launch attributes exist before any capture
                self._step()
                self._warm = True
                self._count(1)
                n -= 1
            self.runner.run(n)
        self._count(n)

    def prepare(self, n: int):
        """Capture the step graphs a later run(n) replays (nothing executes; after the eager first
        step where the session has one)."""
        if self.stream is not None and self._warm:
            with self._ctx(fence=False):
                self.runner.prepare(n)

    def sync(self):
        if self.stream is not None:
            self.stream.synchronize()

    def close(self):
        """Release the recorded step graphs now (a later run re-captures)."""
        self.runner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def span_from_tie(tie) -> np.ndarray:
    """Tie groups (equal numbers name one shared value) -> the packed Adam step's span bytes: the
    first entry of a group carries the group's size, its followers 0."""
    tie = np.asarray(tie)
    _, first, counts = np.unique(tie, return_index=True, return_counts=True)
    span = np.zeros(tie.size, np.uint8)
    span[first] = counts
    return span


class _PackedAdam:
    """Device tensors of one packed Keras-Adam state (mfgp_adam_packed), built from host arrays on
    the current stream: unconstrained u, constrained c, both moments, per-entry trainable /
    transform / span bytes, the step counter, the learning-rate schedule (one entry per step) and
    the loss history (with kl_hist=True a KL history too)."""

    def __init__(self, device, u, c, trainable, transform, span, lr_sched, kl_hist=False):
        f64 = dict(dtype=torch.float64, device=device)
        u8 = lambda a: torch.tensor(np.asarray(a).astype(np.uint8), device=device)
        self.u = torch.tensor(np.asarray(u, np.float64), **f64)
        self.c = torch.tensor(np.asarray(c, np.float64), **f64)
        self.m = torch.zeros_like(self.u)
        self.v = torch.zeros_like(self.u)
        self.trainable, self.transform, self.span = u8(trainable), u8(transform), u8(span)
        self.step = torch.zeros((1,), dtype=torch.int32, device=device)
        self.lr = torch.tensor(np.asarray(lr_sched, np.float64), **f64)
        self.hist = torch.zeros_like(self.lr)
        self.kl_hist = torch.zeros_like(self.lr) if kl_hist else None
        self.b1, self.b2 = float(np.float32(0.9)), float(np.float32(0.999))

    def apply(self, eng, g, out, kl_mult, info):
        """One step on the gradient g and the evaluation's `out`; a non-zero `info` word skips it."""
        eng.adam_packed(self.u, self.c, g, self.m, self.v, self.trainable, self.transform, self.span, self.step,
                        self.lr, self.b1, self.b2, 1e-7, out, kl_mult, self.hist, self.kl_hist, info=info)


def check_outcome(prefix, info, steps, done, hist, timeout=True, cause="", chol="Cholesky failed", history=None):
    """Diagnose a finished run from the info word(s) of its evaluations, the device step counter,
    the steps issued and the loss history read back.  A failed step leaves the step counter behind
    and the next one retries it, so a failure followed by good steps shows only as steps < done
    (trailing loss entries never written).  MFGP_FLOW_TIMEOUT is a non-zero word, so the three
    cases are disjoint.  timeout=False: the words carry no timeout code (SVGP).  history: the
    model's loss_history list, cut after the first bad entry and named in the message (optimize)."""
    v = int(info if isinstance(info, int) else np.max(info))
    finite = np.isfinite(hist)
    if v == 0 and finite.all():
        if steps != done:
            raise MFGPError(f"{prefix}: {done - steps} of {done} steps failed{cause} and were retried; "
                            f"the trajectory is incomplete")
        return
    at = by = ""
    if history is not None:
        bad = len(hist) - 1 if finite.all() else int(np.argmin(finite))
        del history[bad + 1:]
        at, by = f" at iteration {bad}", f" (by iteration {bad})"
    if timeout and v == MFGP_FLOW_TIMEOUT:
        raise info_error(v, prefix + by)
    raise CholeskyError(f"{prefix}: {chol}{at}")
