"""CPU: the loss scaler's state machine as restated in loss_scale_reference.py, against sequences
computed by hand and against torch's own GradScaler kernel where this build has it on the CPU; the
host-side refusals of emsanet_amd.optim.LossScaler."""
import math

import pytest
import torch

from loss_scale_reference import ScalerState


def _run(state, founds):
    return [(float(state.update(f).scale), state.growth_tracker, state.skip, state.skipped, state.steps)
            for f in founds]


def test_backoff_halves_the_scale_and_resets_the_tracker():
    s = ScalerState(init_scale=2.0 ** 16, growth_interval=3)
    #                 scale     tracker skip skipped steps
    assert _run(s, [False, False, True, True, False]) == [
        (2.0 ** 16, 1, 0, 0, 1),
        (2.0 ** 16, 2, 0, 0, 2),
        (2.0 ** 15, 0, 1, 1, 3),       # two clean steps are forgotten
        (2.0 ** 14, 0, 1, 2, 4),
        (2.0 ** 14, 1, 0, 2, 5),
    ]
    assert s.found == 0


def test_growth_exactly_at_the_interval():
    s = ScalerState(init_scale=4.0, growth_interval=3)
    assert _run(s, [False] * 7) == [
        (4.0, 1, 0, 0, 1), (4.0, 2, 0, 0, 2), (8.0, 0, 0, 0, 3),
        (8.0, 1, 0, 0, 4), (8.0, 2, 0, 0, 5), (16.0, 0, 0, 0, 6), (16.0, 1, 0, 0, 7),
    ]
    one = ScalerState(init_scale=1.0, growth_interval=1)
    assert [r[0] for r in _run(one, [False, False, True, False])] == [2.0, 4.0, 2.0, 4.0]


def test_growth_is_suppressed_when_it_would_overflow():
    s = ScalerState(init_scale=2.0 ** 127, growth_interval=2)
    rows = _run(s, [False, False, False, False])
    # 2^128 is not a float32: the scale stays, the tracker starts over all the same
    assert rows == [(2.0 ** 127, 1, 0, 0, 1), (2.0 ** 127, 0, 0, 0, 2),
                    (2.0 ** 127, 1, 0, 0, 3), (2.0 ** 127, 0, 0, 0, 4)]
    assert math.isfinite(float(s.scale))


def test_inv_scale_belongs_to_the_scale_the_step_ran_with():
    s = ScalerState(init_scale=8.0, growth_interval=1)
    s.update(False)                     # ran with 8, the next step runs with 16
    assert (float(s.scale), float(s.inv_scale)) == (16.0, 1.0 / 8.0)
    s.update(True)                      # ran with 16, skipped, the next runs with 8
    assert (float(s.scale), float(s.inv_scale), s.skip) == (8.0, 1.0 / 16.0, 1)


def test_restatement_against_torch_amp_update_scale():
    """torch's kernel (aten::_amp_update_scale_) over the same sequences, where this build has a CPU
    form of it; scale and growth tracker must agree after every step"""
    scale = torch.tensor(2.0 ** 10)
    tracker = torch.zeros((), dtype=torch.int32)
    try:
        torch._amp_update_scale_(scale.clone(), tracker.clone(), torch.zeros(()), 2.0, 0.5, 3)
    except (NotImplementedError, RuntimeError, AttributeError):
        return                          # no CPU form in this build: the hand-computed rows stand alone
    for g, b, interval, init in ((2.0, 0.5, 3, 2.0 ** 10), (3.0, 0.25, 1, 1.5), (2.0, 0.5, 2, 2.0 ** 127)):
        ref = ScalerState(init, g, b, interval)
        scale, tracker = torch.tensor(init, dtype=torch.float32), torch.zeros((), dtype=torch.int32)
        for f in [False, False, True, False, False, False, True, True, False, False, False, False]:
            torch._amp_update_scale_(scale, tracker, torch.tensor(1.0 if f else 0.0), g, b, interval)
            ref.update(f)
            assert float(scale) == float(ref.scale) and int(tracker) == ref.growth_tracker


@pytest.mark.parametrize('kw', [
    dict(growth_factor=1.0), dict(growth_factor=0.5), dict(growth_factor=float('nan')),
    dict(backoff_factor=0.0), dict(backoff_factor=1.0), dict(backoff_factor=1.5), dict(backoff_factor=-0.5),
    dict(growth_interval=0), dict(growth_interval=-3),
    dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=float('inf')), dict(init_scale=float('nan')),
    dict(init_scale=1e39),          # finite as a Python float, not as the float32 the device holds
])
def test_constructor_refuses_on_the_host(kw):
    """the arguments are checked before the optimizer or the device is touched"""
    from emsanet_amd.optim import LossScaler
    with pytest.raises(ValueError):
        LossScaler(None, **kw)


def test_constructor_wants_a_fused_optimizer():
    from emsanet_amd.optim import LossScaler
    with pytest.raises(TypeError):
        LossScaler(object())
