"""_StepRunner's optional steps(n) callable (host logic, no GPU): an eager run hands its whole
count to ONE steps(n) call; without the callable it falls back to n step() calls."""
from multi_fidelity_gpflow_amd.session import _StepRunner


class _Sess:
    def __init__(self):
        self.calls = []

    def _step(self):
        self.calls.append(1)

    def _steps(self, n):
        self.calls.append(("n", n))


def test_eager_run_calls_steps_once():
    s = _Sess()
    _StepRunner(s._step, 0, steps=s._steps).run(5)
    assert s.calls == [("n", 5)]


def test_short_run_of_a_chunked_runner_is_eager():
    s = _Sess()
    _StepRunner(s._step, 50, steps=s._steps).run(3)   # fewer than 4 steps are never captured
    assert s.calls == [("n", 3)]


def test_without_steps_every_step_is_a_call():
    s = _Sess()
    _StepRunner(s._step, 0).run(4)
    assert s.calls == [1, 1, 1, 1]
