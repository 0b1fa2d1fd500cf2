"""The surface-normal task on the device (csrc/normal.hip; loss, targets, augmentation, unit vectors, metric,
evaluator) against the NumPy / plain-torch restatement in tests/normal_reference.py.

Tolerances: the loss and its gradient as tests/test_loss_gpu.py (loss 1e-5 relative, gradient max-abs
error <= 1e-5 * max |reference| + 1e-12, against fp64 on the fp32 values the kernel reads); targets and
augmentation are copies: bit-equal; unit vectors |d| <= 1e-6 per component against F.normalize on the CPU
(components are at most 1, a handful of fp32 roundings of at most 6e-8 each); the metric's count is exact
and its mean within 1e-5 rad of the float64 reference (fp32 cross / dot / atan2: order 3e-6 at angles up
to pi, plus the 2^-21 rad of the fixed point).  Every comparison prints its figures before it asserts.

Every test but the two whole-model ones runs on the guarded arena of tests/guard.py (payload 0xFF = NaN:
the compared outputs are floating point): target and augmentation ring slots, the unit vectors and the
metric state lie between two bands of 0xFF, and normal maps, predictions and parameter rows are placed
with `guard.put`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard   # noqa: E402
import normal_reference as R   # noqa: E402
import targets_reference as T   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, deterministic_state_dict   # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL, GRAD_ATOL = 1e-5, 1e-12
UNIT_ATOL = 1e-6
MAE_ATOL = 1e-5
TASKS5 = ('semantic', 'instance', 'orientation', 'scene', 'normal')
_CACHE = {}


def _dev(a):
    return guard.put(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))    # flush between two bands of 0xFF


def _target(hwc, layout):
    """the (N,H,W,3) array on the device as a loader's HWC tensor, as contiguous CHW planes, or as a
    channels-last (N,3,H,W) view"""
    if layout == 'hwc':
        return _dev(hwc)
    if layout == 'chw':
        return _dev(np.moveaxis(hwc, -1, 1))
    return _dev(hwc).permute(0, 3, 1, 2)


def _pred8(n, h, w, seed, target=None, equal=0.1, scale=1.0):
    """-> (the (N,3,H,W) slice of an ld = 8 NHWC activation on the device, as the head returns it; its
    fp32 values on the host).  With `target`, about `equal` of the pixels predict it exactly."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, 8)) * scale).astype(np.float32)
    if target is not None:
        eq = rng.random((n, h, w)) < equal
        x[..., :3][eq] = target[eq]
    x8 = _dev(x).permute(0, 3, 1, 2)
    assert x8.stride(1) == 1 and (w == 1 or x8.stride(3) == 8)
    return x8[:, :3], np.ascontiguousarray(np.moveaxis(x[..., :3], -1, 1))


def _check_loss(got, ref, what):
    got, ref = float(got.detach() if torch.is_tensor(got) else got), float(ref)
    rel = abs(got - ref) / abs(ref) if ref != 0.0 else abs(got)
    print(f"{what}: loss {got:.9e} ref {ref:.9e} rel err {rel:.2e}")
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), (what, got, ref, rel)


def _check_grad(got, ref, what):
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, mag = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: grad max err {err:.2e} max |ref| {mag:.2e} ratio {err / mag if mag else 0:.2e}")
    assert err <= GRAD_RTOL * mag + GRAD_ATOL, (what, err, mag)


def _loss_and_grad(pred, target, gscale=1.0):
    from emsanet_amd.loss import NormalLoss
    x = pred.detach().requires_grad_(True)
    loss = NormalLoss()([x], [target])[0][0]
    grad, = torch.autograd.grad(loss * gscale, x)
    return loss.detach(), grad


# ---- loss --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['hwc', 'chw', 'channels_last'])
@pytest.mark.parametrize('shape', [(2, 3, 15, 20), (2, 3, 60, 80), (1, 3, 1, 1)])
def test_l1_loss_and_gradient(shape, layout):
    n, _, h, w = shape
    t = R.random_normals(n, h, w, seed=h, invalid=0.3)
    if h == 1:
        t[:] = (0.0, 0.6, -0.8)
    pred, host = _pred8(n, h, w, seed=7 + w, target=t)
    m = R.valid_mask(t)
    n_equal = int(((host == np.moveaxis(t, -1, 1)).all(1) & m).sum())
    print(f"{shape} {layout}: {int(m.sum())} of {m.size} pixels valid, {n_equal} valid predictions exact")
    if h > 1:
        assert 0.2 < 1 - m.mean() < 0.4 and n_equal > 0
    ref_loss, ref_grad = R.l1_loss(host, t, grad_out=0.7)
    loss, grad = _loss_and_grad(pred, _target(t, layout), 0.7)
    _check_loss(loss, ref_loss, f"{shape} {layout}")
    _check_grad(grad, ref_grad, f"{shape} {layout}")
    g = grad.cpu().numpy()
    assert (g[~np.broadcast_to(m[:, None], g.shape)] == 0).all()
    assert (g[np.broadcast_to(m[:, None], g.shape) & (host == np.moveaxis(t, -1, 1))] == 0).all()   # sign(0)


def test_l1_all_invalid_map_gives_zero():
    t = np.zeros((2, 15, 20, 3), np.float32)
    t[0, 3, 4, 1] = -0.0
    pred, _ = _pred8(2, 15, 20, seed=1)
    loss, grad = _loss_and_grad(pred, _dev(t))
    print(f"all invalid: loss {float(loss)!r}, grad max {float(grad.abs().max())!r}")
    assert float(loss) == 0.0 and torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize('ld_d', [4, 8, 5])
def test_l1_gradient_rows_are_written_whole(monkeypatch, ld_d):
    """what EMSA_POISON=1 does: fresh buffers are NaN.  Through the module nothing of the gradient is NaN;
    through the C entry point every element of the ld_d-wide rows is written, the padding exactly 0."""
    from emsanet_amd import _lib, functional as Fn
    monkeypatch.setattr(Fn, '_POISON', True)
    n, h, w = 2, 15, 20
    t = R.random_normals(n, h, w, seed=3)
    pred, host = _pred8(n, h, w, seed=4, target=t)
    ref_loss, ref_grad = R.l1_loss(host, t)
    assert bool(torch.isnan(Fn._empty((4,), DEV)).all())
    loss, grad = _loss_and_grad(pred, _dev(t))
    assert not bool(torch.isnan(grad).any())
    _check_loss(loss, ref_loss, 'poisoned')
    _check_grad(grad, ref_grad, 'poisoned')
    L, td, pixels = _lib.lib(), _dev(t), n * h * w
    partial = Fn._empty((2 * L.emsa_normal_l1_blocks(pixels),), DEV)
    out, rows = Fn._empty((2,), DEV), Fn._empty((pixels, ld_d), DEV)
    one = torch.ones(1, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.emsa_normal_l1_fwd(pred.data_ptr(), 8, td.data_ptr(), 0, h * w, pixels, partial.data_ptr(),
                                out.data_ptr(), st) == 0
    assert L.emsa_normal_l1_bwd(pred.data_ptr(), 8, td.data_ptr(), 0, h * w, pixels, out.data_ptr(),
                                one.data_ptr(), rows.data_ptr(), ld_d, st) == 0
    print(f"ld_d {ld_d}: out {out.tolist()}, NaNs {int(torch.isnan(rows).sum())}, padding max "
          f"{float(rows[:, 3:].abs().max())!r}")
    assert float(out[0]) == float(loss) and float(out[1]) == float(R.valid_mask(t).sum())
    assert torch.equal(rows[:, 3:], torch.zeros_like(rows[:, 3:])) and not bool(torch.isnan(rows).any())
    _check_grad(rows[:, :3].reshape(n, h, w, 3).permute(0, 3, 1, 2), ref_grad, f'rows of {ld_d}')


def test_l1_is_reproducible():
    n, h, w = 2, 60, 80
    t = R.random_normals(n, h, w, seed=9)
    pred, _ = _pred8(n, h, w, seed=10, target=t)
    td = _dev(t)
    l1, g1 = _loss_and_grad(pred, td)
    l2, g2 = _loss_and_grad(pred, td)
    print(f"two runs: {float(l1)!r} {float(l2)!r}")
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_l1_refuses_a_target_of_another_size():
    pred, _ = _pred8(2, 15, 20, seed=1)
    with pytest.raises(ValueError, match='shape'):
        _loss_and_grad(pred, _dev(np.zeros((2, 15, 21, 3), np.float32)))
    with pytest.raises(ValueError, match='images'):
        _loss_and_grad(pred, _dev(np.zeros((3, 15, 20, 3), np.float32)))


# ---- targets -----------------------------------------------------------------------------------------
def _generator(**kw):
    from emsanet_amd import TrainingTargetGenerator, default_args
    args = default_args(tasks=('semantic', 'normal'), **kw)
    return TrainingTargetGenerator(args, [False] + [True] * 40)


def _assert_targets(got, ref):
    assert len(got) == len(ref)
    for z, (g, want) in enumerate(zip(got, ref)):
        assert g.dtype == torch.float32 and tuple(g.shape) == (want.shape[0], 3) + want.shape[1:3], z
        assert g.permute(0, 2, 3, 1).is_contiguous(), z
        assert np.array_equal(g.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), want.view(np.uint32)), \
            f"normal target, scale {z}"


@pytest.mark.parametrize('layout', ['hwc', 'chw', 'channels_last'])
def test_targets_equal_the_reference(layout):
    t = R.random_normals(2, 96, 128, seed=21)
    t[0, 32, 64] = (-0.0, 0.0, 0.0)
    ref = R.multiscale_targets(t)
    assert ref[1].shape == (2, 3, 4, 3) and not R.valid_mask(ref[1]).all() and R.valid_mask(ref[1]).any()
    gen = _generator()
    batch = {'semantic': torch.zeros(2, 96, 128, dtype=torch.uint8, device=DEV), 'normal': _target(t, layout)}
    got = gen.generate(batch)
    guard.check()
    assert sorted(got) == ['normal', 'semantic']
    _assert_targets(got['normal'], ref)
    first = [g.data_ptr() for g in got['normal']]
    again = gen.generate(batch)['normal']                  # ring of 2: other buffers, then the first again
    assert [g.data_ptr() for g in again] != first
    assert [g.data_ptr() for g in gen.generate(batch)['normal']] == first
    _assert_targets(again, ref)
    assert 'normal' not in gen.generate({'semantic': batch['semantic']})


def test_targets_without_multiscale_supervision():
    t = R.random_normals(2, 96, 128, seed=22)
    gen = _generator(normal_no_multiscale_supervision=True)
    got = gen.generate({'semantic': torch.zeros(2, 96, 128, dtype=torch.uint8, device=DEV), 'normal': _dev(t)})
    assert len(got['normal']) == 1 and len(got['semantic']) == 4
    _assert_targets(got['normal'], R.multiscale_targets(t, (1,)))


def test_targets_capture_into_a_graph():
    t1, t2 = R.random_normals(2, 96, 128, seed=23), R.random_normals(2, 96, 128, seed=24)
    gen = _generator()
    batch = {'semantic': torch.zeros(2, 96, 128, dtype=torch.uint8, device=DEV), 'normal': _dev(t1)}
    eager = [g.clone() for g in gen.generate(batch)['normal']]
    gen.generate(batch)                                    # (both slots of the ring exist)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            got = gen.generate(batch)['normal']
    torch.cuda.current_stream().wait_stream(stream)
    batch['normal'].copy_(_dev(t2))
    graph.replay()
    torch.cuda.synchronize()
    _assert_targets(got, R.multiscale_targets(t2))
    batch['normal'].copy_(_dev(t1))
    graph.replay()
    torch.cuda.synchronize()
    for g, e in zip(got, eager):
        assert torch.equal(g, e)
    guard.check()                                          # (both ring slots were made before the capture)


def test_targets_refuse_a_bad_normal_map():
    gen = _generator()
    sem = torch.zeros(2, 96, 128, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='normal'):
        gen.generate({'semantic': sem, 'normal': _dev(np.zeros((2, 96, 64, 3), np.float32))})
    with pytest.raises(ValueError, match='shape'):
        gen.generate({'semantic': sem, 'normal': _dev(np.zeros((2, 96, 128), np.float32))})
    with pytest.raises(TypeError, match='float32'):
        gen.generate({'semantic': sem, 'normal': _dev(np.zeros((2, 96, 128, 3), np.float64))})
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        gen.generate({'semantic': sem, 'normal': torch.zeros(2, 96, 128, 3)})
    with pytest.raises(TypeError, match='tensor'):
        gen.generate({'semantic': sem, 'normal': np.zeros((2, 96, 128, 3), np.float32)})
    with pytest.raises(ValueError, match='contiguous'):
        gen.generate({'semantic': sem, 'normal': _dev(np.zeros((2, 96, 256, 3), np.float32))[:, :, ::2]})


# ---- augmentation ------------------------------------------------------------------------------------
HS, WS, H, W = 120, 160, 96, 128


def _augmenter(**kw):
    from emsanet_amd import TrainingAugmenter, default_args
    args = default_args(tasks=('semantic', 'normal'), input_height=H, input_width=W)
    return TrainingAugmenter(args, (2000.0, 900.0), with_normal=True, **kw)


def _raw_batch(n, layout='hwc', seed=0):
    g = np.random.default_rng(seed)
    t = R.random_normals(n, HS, WS, seed=seed + 1)
    return {'rgb': _dev(g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)),
            'depth': _dev(g.integers(300, 8000, (n, HS, WS)).astype(np.int16)).view(torch.uint16),
            'semantic': _dev(g.integers(0, 41, (n, HS, WS)).astype(np.uint8)),
            'normal': _target(t, layout)}, t


def _assert_augmented(got, t, table, what):
    want = R.augment(t, table, H, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(t), 3, H, W), what
    assert got.permute(0, 2, 3, 1).is_contiguous(), what
    g = got.permute(0, 2, 3, 1).cpu().numpy()
    print(f"{what}: flips {table[:, 4].tolist()}, {int((g != want).any(-1).sum())} pixels differ")
    assert np.array_equal(g, want), what
    assert np.array_equal(R.valid_mask(g), R.valid_mask(want)), what
    return g


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_augment_explicit_rows(layout):
    """scale 1 without a flip (the identity crop at the origin); the largest scale in the far corner,
    flipped; the largest scale unflipped; scale 1 flipped, inside"""
    hr, wr = (HS * 1434 + 512) >> 10, (WS * 1434 + 512) >> 10
    assert (hr, wr) == (168, 224)
    table = np.array([[HS, WS, 0, 0, 0, 0, 0, 0], [hr, wr, hr - H, wr - W, 1, 0, 0, 0],
                      [hr, wr, 17, 31, 0, 0, 0, 0], [HS, WS, HS - H, WS - W, 1, 0, 0, 0]], np.int32)
    batch, t = _raw_batch(4, layout)
    aug = _augmenter()
    out = aug.apply(batch, params=_dev(table))
    guard.check()
    assert sorted(out) == ['depth', 'normal', 'rgb', 'semantic']
    g = _assert_augmented(out['normal'], t, table, f'explicit rows, {layout}')
    assert np.array_equal(g[0], t[0, :H, :W])
    assert np.array_equal(g[3][..., 0], -t[3, HS - H:, WS - W:][:, ::-1, 0])
    assert np.array_equal(g[3][..., 1:], t[3, HS - H:, WS - W:][:, ::-1, 1:])
    assert np.array_equal(g[2][0, 0], t[2, (17 * HS) // hr, (31 * WS) // wr])


def test_augment_drawn_rows_and_the_validation_twin():
    batch, t = _raw_batch(4, seed=5)
    aug = _augmenter(seed=3)
    seen = set()
    for call in range(3):
        out = aug.apply(batch)
        table = aug.last_params().numpy()
        seen |= set(table[:, 4].tolist())
        _assert_augmented(out['normal'], t, table, f'drawn rows, call {call}')
    assert seen == {0, 1}
    first = aug.apply(batch)['normal'].data_ptr()
    aug.apply(batch)
    assert aug.apply(batch)['normal'].data_ptr() == first              # ring of 2: no new buffers
    out = aug.resize_normalize(batch, H, W)
    _assert_augmented(out['normal'], t, np.array([[H, W, 0, 0, 0, 0, 0, 0]] * 4, np.int32), 'resize_normalize')


# ---- unit vectors ------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dense', [((2, 3, 15, 20), False), ((1, 3, 1, 1), False), ((2, 3, 7, 9), True),
                                         ((1, 3, 16, 16), False)])
def test_unit_vectors(shape, dense):
    from emsanet_amd import NormalPostprocessing
    n, _, h, w = shape
    pred, host = _pred8(n, h, w, seed=31, scale=3.0)
    host = host.copy()
    if h > 1:
        host[0, :, 0, 0] = 0.0                                # a zero vector
        host[0, :, 0, 1] = (1e-20, 0.0, 0.0)                  # shorter than the epsilon... squares underflow
        host[0, :, 1, 0] = (3e18, -4e18, 0.0)                 # long
        host[0, :, 1, 1] = (0.0, 0.0, -2.5)
        pred[0, :, 0, 0] = 0.0
        pred[0, :, 0, 1] = torch.tensor([1e-20, 0.0, 0.0], device=DEV)
        pred[0, :, 1, 0] = torch.tensor([3e18, -4e18, 0.0], device=DEV)
        pred[0, :, 1, 1] = torch.tensor([0.0, 0.0, -2.5], device=DEV)
    if dense:
        pred = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # ld = 3: scalar loads
    prediction = {'normal_output': pred, 'normal_side_outputs': ()}
    out = NormalPostprocessing()(prediction)
    guard.check()
    assert out is prediction and sorted(out) == ['normal_output', 'normal_side_outputs', 'normal_vectors']
    v = out['normal_vectors']
    assert v.dtype == torch.float32 and tuple(v.shape) == shape and v.permute(0, 2, 3, 1).is_contiguous()
    got, want = v.cpu().numpy(), R.unit_vectors(host)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    print(f"{shape} dense={dense}: max |d| {err:.2e}, lengths {length.min():.7f} ... {length.max():.7f}")
    assert np.isfinite(got).all() and err <= UNIT_ATOL
    if h > 1:
        assert (got[0, :, 0, 0] == 0).all() and got[0, :, 1, 1].tolist() == [0.0, 0.0, -1.0]
        assert np.allclose(got[0, :, 1, 0], (0.6, -0.8, 0.0), atol=1e-6)


# ---- metric ------------------------------------------------------------------------------------------
def _metric_inputs(n, h, w, seed, scale=2):
    """(pred (N,3,h,w) host values with special pairs, target (N,H,W,3)) with H = scale * h"""
    rng = np.random.default_rng(seed)
    t = R.random_normals(n, h * scale, w * scale, seed=seed + 1)
    p = (rng.standard_normal((n, 3, h, w)) * rng.uniform(0.1, 5.0, (n, 1, h, w))).astype(np.float32)
    s = scale
    for k, (vec, factor) in enumerate((((0.25, 0.0, 0.5), 2.5), ((0.0, -1.0, 0.0), -0.5), ((1.0, 0.0, 0.0), None))):
        t[0, 0, k * s] = vec                                    # parallel, antiparallel, orthogonal pairs
        p[0, :, 0, k] = np.array(vec) * factor if factor else (0.0, 3.0, -4.0)
    t[0, 0, 3 * s] = 0.0                                        # an invalid target
    return p, t


def _pred_dev(p):
    x = np.zeros(p.shape[:1] + p.shape[2:] + (8,), np.float32)
    x[..., :3] = np.moveaxis(p, 1, -1)
    return _dev(x).permute(0, 3, 1, 2)[:, :3]


def _check_metric(m, pairs, what):
    ref_mean, ref_count = R.angular_error(pairs)
    total, count = m.counts()
    got = m.compute()
    err = abs(got['mae_rad'] - ref_mean)
    print(f"{what}: count {count} ref {ref_count}, mean {got['mae_rad']:.9f} ref {ref_mean:.9f} rad, "
          f"|err| {err:.2e} rad (bound {MAE_ATOL:.0e})")
    assert count == ref_count
    assert err <= MAE_ATOL
    assert got['mae_deg'] == math.degrees(got['mae_rad']) and total == round(got['mae_rad'] * count * R.ANGLE_ONE)


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_metric_same_size_and_update_order(layout):
    from emsanet_amd import MeanAbsoluteNormalError
    from emsanet_amd.metrics import NORMAL_ANGLE_ONE
    assert NORMAL_ANGLE_ONE == R.ANGLE_ONE
    pa, ta = _metric_inputs(2, 15, 20, seed=41, scale=1)
    pb, tb = _metric_inputs(1, 60, 80, seed=43, scale=1)
    a = R.angles(pa, ta)
    assert a.min() == 0.0 and abs(a.max() - np.pi) < 1e-12 and (np.abs(a - np.pi / 2) < 1e-12).any()
    m = MeanAbsoluteNormalError()
    r = m.compute()
    assert math.isnan(r['mae_rad']) and math.isnan(r['mae_deg'])
    m.update(_pred_dev(pa), _target(ta, layout))
    _check_metric(m, [(pa, ta)], f'one update, {layout}')
    m.update(_pred_dev(pb), _target(tb, layout))
    _check_metric(m, [(pa, ta), (pb, tb)], f'two updates, {layout}')
    other = MeanAbsoluteNormalError()
    other.update(_pred_dev(pb), _target(tb, layout))
    other.update(_pred_dev(pa), _target(ta, layout))
    assert torch.equal(m._state, other._state)
    m.reset()
    assert m.counts() == (0, 0) and math.isnan(m.compute()['mae_rad'])


def test_metric_with_a_target_twice_the_size():
    from emsanet_amd import MeanAbsoluteNormalError
    p, t = _metric_inputs(2, 15, 20, seed=47, scale=2)
    assert t.shape == (2, 30, 40, 3)
    m = MeanAbsoluteNormalError()
    m.update(_pred_dev(p), _dev(t))
    guard.check()
    _check_metric(m, [(p, t)], 'target 2x')
    dense = MeanAbsoluteNormalError()                        # a dense ld = 3 prediction: scalar loads
    dense.update(_dev(np.moveaxis(p, 1, -1)).permute(0, 3, 1, 2), _dev(t))
    assert torch.equal(m._state, dense._state)


def test_metric_flags_a_prediction_that_is_not_finite():
    from emsanet_amd import MeanAbsoluteNormalError
    p, t = _metric_inputs(1, 15, 20, seed=49, scale=1)
    t[0, 5, 5] = (0.0, 0.0, 1.0)
    p[0, :, 5, 5] = np.nan
    m = MeanAbsoluteNormalError()
    m.update(_pred_dev(p), _dev(t))
    with pytest.raises(ValueError, match='finite'):
        m.compute()


# ---- the whole model ---------------------------------------------------------------------------------
def _setup():
    """five-task model, a labelled batch, device targets -- built once, never modified"""
    if 'model' in _CACHE:
        return _CACHE['model']
    from emsanet_amd import TrainingTargetGenerator, full_args, nyuv2_config
    from emsanet_amd.model import EMSANet
    from oracle.emsanet_oracle import synthetic_batch
    cfg = nyuv2_config()
    args = full_args(input_height=96, input_width=128, tasks=TASKS5,
                     tasks_weighting=(1.0, 3.0, 1.0, 0.25, 0.5))
    model = EMSANet(args, cfg)
    model.load_state_dict(deterministic_state_dict(model))
    model.to(DEV)
    is_thing = (False,) + tuple(bool(i % 3) for i in range(40))
    use_o = tuple(t and i % 2 == 0 for i, t in enumerate(is_thing))
    esem, einst, eori, _ = T.edge_scene()
    sem = np.array([0, 6, 5, 7, 8, 9])[esem[1:]]
    normal = R.random_normals(2, 96, 128, seed=61)
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 96, 128).items()}
    batch.update(semantic=_dev(sem.astype(np.uint8)), instance=_dev(einst[1:].astype(np.int32)),
                 orientations=_dev(eori[1:]), scene=_dev(np.array([3, 0], np.int64)), normal=_dev(normal))
    gen = TrainingTargetGenerator(args, is_thing, use_o)
    targets = gen.generate(batch)
    gen.check()
    _CACHE['model'] = (args, cfg, model, batch, targets, normal)
    return _CACHE['model']


def test_training_step_with_the_normal_task():
    from emsanet_amd import full_args
    from emsanet_amd.loss import TrainingLosses, loss_weights
    args, cfg, model, batch, targets, normal = _setup()
    g = torch.Generator(device='cpu').manual_seed(99)
    class_weights = torch.rand(40, generator=g) * 2 + 0.3
    crit = TrainingLosses(args, class_weights, 10).to(DEV)
    model.train()
    model.zero_grad(set_to_none=True)
    model.dropout_step = 0
    out = model(batch)
    assert len(out) == 4 and len(out[2]) == 2 and len(out[2][1]) == 3
    total, losses = crit(out, targets)
    assert sorted(losses) == ['instance_center', 'instance_offset', 'instance_orientation', 'normal', 'scene',
                              'semantic']
    # the normal loss against the reference evaluated on the model's own outputs, scale by scale
    scales = [out[2][0]] + list(out[2][1])
    assert [tuple(s.shape[2:]) for s in scales] == [(96, 128), (3, 4), (6, 8), (12, 16)]
    ref = sum(R.l1_loss(s.detach().cpu().numpy(), t)[0] for s, t in zip(scales, R.multiscale_targets(normal)))
    _check_loss(losses['normal'], ref, 'normal loss of the model')
    weights = loss_weights(args)
    assert weights['normal'] == 0.5
    want = sum(weights[k] * float(v) for k, v in losses.items())
    print(f"total {float(total)!r}, weighted sum {want!r}")
    assert abs(float(total) - want) <= 1e-6 * abs(want)
    # without the task: every other loss bit for bit.  Not a second, four-task model (its Dropout2d layer
    # ids and streams differ, so its outputs are not comparable bit for bit): the five-task model's own
    # outputs minus the normal entry go through a four-task TrainingLosses, whose code path is the one a
    # configuration without 'normal' takes -- the loss path is what this change could have disturbed
    args4 = full_args(input_height=96, input_width=128, tasks_weighting=(1.0, 0.25, 3.0, 1.0))
    crit4 = TrainingLosses(args4, class_weights, 10).to(DEV)
    total4, losses4 = crit4([out[0], out[1], out[3]], {k: v for k, v in targets.items() if k != 'normal'})
    assert sorted(losses4) == sorted(k for k in losses if k != 'normal')
    for k, v in losses4.items():
        assert torch.equal(v, losses[k]), k
    merged = dict(semantic_output=out[0][0], semantic_side_outputs=out[0][1], instance_output=out[1][0],
                  instance_side_outputs=out[1][1], normal_output=out[2][0], normal_side_outputs=out[2][1],
                  scene_output=out[3][0])
    total_m, losses_m = crit(merged, targets)
    assert torch.equal(total_m, total) and torch.equal(losses_m['normal'], losses['normal'])
    total.backward()
    bad = []
    for name, p in model.decoders['normal_decoder'].named_parameters():
        if p.grad is None or not bool(torch.isfinite(p.grad).all()) or not bool(p.grad.any()):
            bad.append(name)
    n_par = len(list(model.decoders['normal_decoder'].parameters()))
    print(f"normal_decoder: {n_par} parameters, without a finite non-zero gradient: {bad}")
    assert n_par > 50 and not bad


def test_evaluator_reports_the_normal_error():
    from emsanet_amd import NormalPostprocessing, ValidationEvaluator, full_args
    args, cfg, model, batch, targets, normal = _setup()
    model.eval()
    with torch.no_grad():
        prediction = model(batch, do_postprocessing=True)
    raw = prediction['normal_output']
    assert tuple(raw.shape) == (2, 3, 96, 128) and 'normal_vectors' not in prediction
    ev = ValidationEvaluator(args, cfg)
    ev.update(prediction, batch)
    got = ev.compute()
    ref_mean, ref_count = R.angular_error([(raw.cpu().numpy(), normal)])
    err = abs(got['normal_mae_rad'] - ref_mean)
    print(f"normal_mae_deg {got['normal_mae_deg']:.6f} ref {math.degrees(ref_mean):.6f}, |err| {err:.2e} rad, "
          f"{ref_count} pixels")
    assert err <= MAE_ATOL and abs(got['normal_mae_deg'] - math.degrees(ref_mean)) <= math.degrees(MAE_ATOL)
    assert int(ev.state()['normal_mae'][1]) == ref_count
    # the angle needs no unit length: the unit vectors give the same error
    unit = ValidationEvaluator(args, cfg)
    unit.update(dict(prediction, normal_output=NormalPostprocessing()(dict(prediction))['normal_vectors']), batch)
    assert abs(unit.compute()['normal_mae_rad'] - ref_mean) <= MAE_ATOL
    # a full-resolution target twice the size of the output
    big = np.ascontiguousarray(normal.repeat(2, 1).repeat(2, 2))
    full = ValidationEvaluator(args, cfg)
    full.normal_mae.update(raw, _dev(big))
    assert full.normal_mae.counts()[1] == 4 * ref_count
    assert abs(full.normal_mae.compute()['mae_rad'] - ref_mean) <= MAE_ATOL
    # through the evaluator: batch['normal_fullres'] is the target when the batch has it
    chosen = ValidationEvaluator(args, cfg)
    chosen.update(prediction, dict(batch, normal_fullres=_dev(big)))
    assert int(chosen.state()['normal_mae'][1]) == 4 * ref_count
    assert torch.equal(chosen.normal_mae._state, full.normal_mae._state)
    # without the task the keys are absent
    ev4 = ValidationEvaluator(full_args(input_height=96, input_width=128), cfg)
    ev4.update(prediction, batch)
    assert not [k for k in ev4.compute() if 'normal' in k]
    assert sorted(set(got) - set(ev4.compute())) == ['normal_mae_deg', 'normal_mae_rad']
