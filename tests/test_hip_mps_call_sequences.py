"""GPU: the committed call sequences of tests/mps_seq_model.py on the real DeviceMPS / LockstepLanes objects.

A pool of long-lived states, some made by the device, some edited in place, listed together (and twice) in batched calls, with
holders of copies alive across the edits: every step is predicted by the project's NumPy statements from the tensors the device held,
compared at the bound of that feature's own test, and followed by an audit of every live slot.  tests/test_mps_seq_model.py holds the
same runner, the sequences' conditions and five planted faults on the CPU.  The tests print the largest error per step kind;
DESIGN.md 6zc records them."""
import pytest

from tests import mps_seq_model as sm

pytestmark = pytest.mark.gpu


def _run(register, seed):
    """One sequence; it builds its pool and closes it, leaves the lockstep cache as it found it and ``live_buffers()`` unchanged (the
    runner's last step asserts both)."""
    from aqc_research_amd import mps_engine
    from aqc_research_amd.engine import live_buffers

    live, cache = live_buffers(), dict(mps_engine._LOCKSTEP_CACHE)
    runner = sm.run_sequence(sm.device_backend(), register, seed, min_gap=sm.MIN_GAP)
    print(f"{register}-{seed}: {sum(runner.counts.values())} steps, smallest gap {runner.smallest_gap:.3g}; " + sm.report(runner))
    assert live_buffers() == live
    assert mps_engine._LOCKSTEP_CACHE == cache
    return runner


@pytest.mark.parametrize("register,seed", sm.SEQUENCES, ids=[f"{r}-{s}" for r, s in sm.SEQUENCES])
def test_call_sequence(register, seed):
    _run(register, seed)


@pytest.mark.parametrize("apply", (None, "single"))
@pytest.mark.parametrize("register,seed", sm.APPLY_SWITCH_SEQUENCES, ids=[f"{r}-{s}" for r, s in sm.APPLY_SWITCH_SEQUENCES])
def test_call_sequence_under_the_apply_switch(monkeypatch, register, seed, apply):
    """AQC_MPS_APPLY unset and set to ``single``: every read agrees with the model at the same bounds."""
    if apply is None:
        monkeypatch.delenv("AQC_MPS_APPLY", raising=False)
    else:
        monkeypatch.setenv("AQC_MPS_APPLY", apply)
    _run(register, seed)


@pytest.mark.parametrize("name", sm.REGRESSIONS)
def test_regression(name):
    """The shortest sequence that showed each bug the sequences found."""
    register, steps = sm.regression(name)
    sm.run_steps(sm.device_backend(), register, steps)
