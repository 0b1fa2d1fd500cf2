"""CPU: the restatement of the surface-normal rules (tests/normal_reference.py) against torch autograd and
against the acos form of the angle, and the host-side surface of the normal task: arguments, loss
weights and refusals.  The GPU kernels are held to the restatement in tests/test_normal_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normal_reference as R   # noqa: E402

TASKS = ('semantic', 'instance', 'orientation', 'scene', 'normal')


def _args(**kw):
    from emsanet_amd import full_args
    kw.setdefault('tasks', TASKS)
    return full_args(**kw)


# ---- the reference itself ----------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 3, 1, 1), (3, 3, 4, 4)])
def test_reference_l1_equals_autograd(shape):
    rng = np.random.default_rng(3)
    n, _, h, w = shape
    target = R.random_normals(n, h, w, seed=5, invalid=0.3)
    if shape == (1, 3, 1, 1):
        target[:] = (0.0, 0.6, -0.8)                  # one valid pixel with a zero component
    pred = rng.standard_normal(shape).astype(np.float32)
    loss, grad = R.l1_loss(pred, target, grad_out=0.7)
    loss_a, grad_a = R.l1_loss_autograd(pred, target, grad_out=0.7)
    assert loss == pytest.approx(loss_a, rel=1e-14)
    assert np.allclose(grad, grad_a, rtol=1e-14, atol=0)
    m = R.valid_mask(target)
    assert (grad[~np.broadcast_to(m[:, None], grad.shape)] == 0).all()
    assert np.abs(grad[np.broadcast_to(m[:, None], grad.shape)]).min() == pytest.approx(0.7 / (3 * m.sum()))


def test_reference_l1_edges():
    target = np.zeros((1, 2, 2, 3), np.float32)
    target[0, 0, 1, 0] = -0.0                         # still (0, 0, 0)
    pred = np.ones((1, 3, 2, 2), np.float32)
    assert not R.valid_mask(target).any()
    loss, grad = R.l1_loss(pred, target)
    assert loss == 0.0 and not grad.any()
    target[0, 1, 1] = (0.0, 0.0, 1.0)                 # sign(0) = 0 where the prediction equals the target
    pred[0, :, 1, 1] = (0.5, 0.0, 1.0)
    loss, grad = R.l1_loss(pred, target)
    assert loss == pytest.approx(0.5 / 3)
    assert grad[0, :, 1, 1].tolist() == [1 / 3, 0.0, 0.0] and np.count_nonzero(grad) == 1


def test_reference_angle_equals_acos():
    """away from 0 and pi (where acos loses half of its digits) the two forms agree to rounding"""
    rng = np.random.default_rng(11)
    target = R.random_normals(2, 9, 11, seed=2)
    pred = (rng.standard_normal((2, 3, 9, 11)) * 3).astype(np.float32)        # not unit length
    a, b = R.angles(pred, target), R.angles_acos(pred, target)
    keep = (a > 0.05) & (a < np.pi - 0.05)
    assert keep.sum() > 50 and a.size == R.valid_mask(target).sum()
    assert np.abs(a - b)[keep].max() < 1e-13
    t = np.zeros((1, 1, 3, 3), np.float32)
    t[0, 0] = [(0, 0, 1), (0, 0, 2), (1, 0, 0)]
    p = np.zeros((1, 3, 1, 3), np.float32)
    p[0, :, 0] = [[0, 0, 0], [0, 0, 0], [5, -3, 0.5]]                        # (0,0,5), (0,0,-3), (0,0,.5)
    assert np.allclose(R.angles(p, t), [0.0, np.pi, np.pi / 2], atol=1e-15)
    mean, count = R.angular_error([])
    assert np.isnan(mean) and count == 0


def test_reference_targets_and_nearest():
    t = R.random_normals(2, 96, 128, seed=1)
    out = R.multiscale_targets(t)
    assert [o.shape for o in out] == [(2, 96, 128, 3), (2, 3, 4, 3), (2, 6, 8, 3), (2, 12, 16, 3)]
    assert np.array_equal(out[1][1, 2, 3], t[1, 64, 96])
    assert R.nearest_source(8, 4).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    got = torch.nn.functional.interpolate(torch.arange(5.)[None, None, None], size=(1, 7), mode='nearest')
    assert R.nearest_source(7, 5).tolist() == got.flatten().long().tolist()


def test_reference_augment_flip_negates_x():
    t = R.random_normals(2, 6, 8, seed=4)
    table = np.array([[6, 8, 0, 0, 0, 0, 0, 0], [6, 8, 0, 0, 1, 0, 0, 0]], np.int32)
    out = R.augment(t, table, 6, 8)
    assert np.array_equal(out[0], t[0])
    assert np.array_equal(out[1][..., 0], -t[1][:, ::-1, 0]) and np.array_equal(out[1][..., 1:], t[1][:, ::-1, 1:])
    assert np.array_equal(R.valid_mask(out)[1], R.valid_mask(t)[1][:, ::-1])


# ---- arguments and weights ---------------------------------------------------------------------------
def test_args_expose_the_normal_fields():
    from emsanet_amd import default_args
    args = default_args(tasks=('semantic', 'normal'))
    assert args.normal_loss == 'l1' and args.normal_no_multiscale_supervision is False
    assert default_args(normal_no_multiscale_supervision=True).normal_no_multiscale_supervision is True


def test_loss_weights_carry_normal():
    from emsanet_amd.loss import loss_weights, reduce_losses
    args = _args(tasks_weighting=(1.0, 3.0, 1.0, 0.25, 0.5))
    w = loss_weights(args)
    assert w['normal'] == 0.5 and w['scene'] == 0.25 and w['instance_center'] == 6.0
    total = reduce_losses({'normal': torch.tensor(2.0), 'scene': torch.tensor(4.0)}, w)
    assert float(total) == 2.0


# ---- refusals ----------------------------------------------------------------------------------------
def test_loss_name_other_than_l1_is_refused():
    from emsanet_amd.loss import NormalLoss, TrainingLosses
    assert NormalLoss().loss_name == 'l1'
    with pytest.raises(NotImplementedError, match='l1'):
        NormalLoss('l2')
    with pytest.raises(NotImplementedError, match='l1'):
        TrainingLosses(_args(normal_loss='cosine'), torch.ones(40), 10)
    assert not hasattr(TrainingLosses(_args(tasks=('semantic', 'scene')), torch.ones(40), 10), 'normal')


def test_normal_map_refusals():
    from emsanet_amd.postprocessing import normal_map
    good = torch.zeros(2, 4, 6, 3)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        normal_map(good, 'who', 'what')
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        normal_map(torch.zeros(2, 3, 4, 6), 'who', 'what')
    with pytest.raises(TypeError, match='float32'):
        normal_map(good.double(), 'who', 'what')
    with pytest.raises(TypeError, match='float32'):
        normal_map(good.half(), 'who', 'what')
    with pytest.raises(TypeError, match='tensor'):
        normal_map(None, 'who', 'what')
    for bad in (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6, 2), torch.zeros(2, 2, 4, 6)):
        with pytest.raises(ValueError, match='shape'):
            normal_map(bad, 'who', 'what')
    with pytest.raises(ValueError, match='4 x 7'):
        normal_map(good, 'who', 'what', hw=(4, 7))


def test_loss_refuses_cpu_wrong_dtype_and_wrong_shape():
    from emsanet_amd.loss import NormalLoss
    crit = NormalLoss()
    pred = torch.zeros(2, 3, 4, 6)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        crit([pred], [torch.zeros(2, 4, 6, 3)])
    with pytest.raises(TypeError, match='float32'):
        crit([pred], [torch.zeros(2, 4, 6, 3, dtype=torch.float64)])
    with pytest.raises(ValueError, match='shape'):
        crit([pred], [torch.zeros(2, 4, 5, 3)])
    with pytest.raises(ValueError, match='prediction'):
        crit([torch.zeros(2, 2, 4, 6)], [torch.zeros(2, 4, 6, 3)])


def test_metric_refuses_cpu_wrong_dtype_and_wrong_shape():
    from emsanet_amd import MeanAbsoluteNormalError
    m = MeanAbsoluteNormalError()
    r = m.compute()
    assert np.isnan(r['mae_rad']) and np.isnan(r['mae_deg']) and m.counts() == (0, 0)
    pred = torch.zeros(2, 3, 4, 6)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        m.update(pred, torch.zeros(2, 4, 6, 3))
    with pytest.raises(TypeError, match='float32'):
        m.update(pred, torch.zeros(2, 4, 6, 3, dtype=torch.int64))
    with pytest.raises(TypeError, match='floating'):
        m.update(pred.long(), torch.zeros(2, 4, 6, 3))
    with pytest.raises(ValueError, match='shape'):
        m.update(torch.zeros(2, 4, 6), torch.zeros(2, 4, 6, 3))
    with pytest.raises(ValueError, match='shape'):
        m.update(pred, torch.zeros(2, 4, 6))


def test_target_generator_scales_follow_the_switch():
    """(the generator's refusals of a bad batch['normal'] need device label maps: tests/test_normal_gpu.py)"""
    from emsanet_amd import TrainingTargetGenerator
    from emsanet_amd.targets import DEFAULT_SCALES, N_LAUNCHES, N_NORMAL_LAUNCHES
    gen = TrainingTargetGenerator(_args(), [False] + [True] * 40, [False] * 41)
    assert gen.with_normal and gen.normal_scales == DEFAULT_SCALES == R.DEFAULT_SCALES
    assert (N_LAUNCHES, N_NORMAL_LAUNCHES) == (3, 1)
    one = TrainingTargetGenerator(_args(normal_no_multiscale_supervision=True), [False] + [True] * 40)
    assert one.normal_scales == (1,)
    assert TrainingTargetGenerator(_args(tasks=('semantic',)), [False] * 41).normal_scales == ()


def test_augmenter_refuses_without_the_switch_and_constructs_with_it():
    from emsanet_amd import TrainingAugmenter
    args = _args(input_height=32, input_width=48)
    with pytest.raises(NotImplementedError, match='normal'):
        TrainingAugmenter(args)
    with pytest.raises(NotImplementedError, match='normal'):
        TrainingAugmenter(args, with_normal=False)
    aug = TrainingAugmenter(args, with_normal=True)
    assert aug.with_normal
    assert not TrainingAugmenter(_args(tasks=('semantic',), input_height=32, input_width=48),
                                 with_normal=True).with_normal
    batch = {'rgb': torch.zeros(2, 40, 60, 3, dtype=torch.uint8),
             'depth': torch.zeros(2, 40, 60, dtype=torch.int16).view(torch.uint16),
             'semantic': torch.zeros(2, 40, 60, dtype=torch.uint8),
             'instance': torch.zeros(2, 40, 60, dtype=torch.uint8),
             'orientations': torch.zeros(2, 16), 'scene': torch.zeros(2, dtype=torch.int64)}
    with pytest.raises(TypeError, match="batch\\['normal'\\]"):
        aug.apply(batch)
    with pytest.raises(TypeError, match='float32'):
        aug.apply(dict(batch, normal=torch.zeros(2, 40, 60, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match='shape'):
        aug.apply(dict(batch, normal=torch.zeros(2, 40, 61, 3)))
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        aug.apply(dict(batch, normal=torch.zeros(2, 40, 60, 3)))


def test_evaluator_keys_follow_the_task():
    from emsanet_amd import ValidationEvaluator, nyuv2_config
    ev = ValidationEvaluator(_args(), nyuv2_config())
    assert ev.with_normal and ev.normal_mae is not None
    ev = ValidationEvaluator(_args(tasks=('semantic', 'scene')), nyuv2_config())
    assert not ev.with_normal and ev.normal_mae is None and 'normal_mae_deg' not in ev.compute()


def test_entry_points_validate_on_the_host():
    """negative codes before any launch (no device memory is touched: null and odd arguments only)"""
    from emsanet_amd import _lib
    L = _lib.lib()
    assert L.emsa_normal_l1_fwd(None, 8, None, 0, 4, 4, None, None, None) == -2
    assert L.emsa_normal_l1_fwd(8, 2, 8, 0, 4, 4, 8, 8, None) == -1                  # ld < 3
    assert L.emsa_normal_l1_fwd(8, 8, 8, 0, 3, 4, 8, 8, None) == -1                  # pixels % hw
    assert L.emsa_normal_l1_bwd(8, 8, 8, 0, 4, 4, 8, 8, 8, 2, None) == -1            # ld_d < 3
    assert L.emsa_normal_l1_bwd(8, 8, 8, 0, 4, 4, None, 8, 8, 4, None) == -2
    assert L.emsa_normal_targets(None, 0, 1, 4, 4, None, 1, None) == -2
    scales = (_lib.EmsaNormalScale * 1)()
    scales[0].scale, scales[0].out = 3, 16
    assert L.emsa_normal_targets(8, 0, 1, 4, 4, scales, 1, None) == -1               # 4 % 3
    assert L.emsa_normal_targets(8, 0, 1, 4, 4, scales, 9, None) == -1
    scales[0].scale, scales[0].out = 2, 4
    assert L.emsa_normal_targets(8, 0, 1, 4, 4, scales, 1, None) == -2               # unaligned output
    assert L.emsa_augment_normal(8, 0, None, 1, 4, 4, 4, 4, 16, None) == -2
    assert L.emsa_augment_normal(8, 0, 8, 1, 4, 5000, 4, 4, 16, None) == -1
    assert L.emsa_normal_unit(8, 2, 4, 16, None) == -1
    assert L.emsa_normal_unit(8, 8, 4, None, None) == -2
    assert L.emsa_normal_angular_error(8, 8, 1, 4, 4, 8, 0, 4, 40000, 8, 8, None) == -1
    assert L.emsa_normal_angular_error(8, 8, 1, 4, 4, 8, 0, 4, 4, None, 8, None) == -2
