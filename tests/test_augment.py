"""CPU: the NumPy restatement of the augmentation rules (tests/augment_reference.py) against values
computed by hand, against Pillow's bilinear resize and against its own invariants; and the host-side
refusals of emsanet_amd.augment.TrainingAugmenter.  The GPU kernels are held to this restatement in
tests/test_augment_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R   # noqa: E402


# ---- the hash and the draw ---------------------------------------------------------------------------
def test_hash_known_answers():
    """computed with plain Python integers from the constants in the docstring of emsanet_amd/augment.py"""
    assert [R.lowbias32(v) for v in (0, 1, 0xFFFFFFFF, 12345)] == [0x0, 0x688990C0, 0x6768824A, 0x912EFCF7]
    assert R.aug_hash(0, 0, 0, 0) == 0x41F39E5E
    assert R.aug_hash(0, 0, 0, 1) == 0x2B4B55BB
    assert R.aug_hash(7, 3, 2, 5) == 0x610E2C30
    assert R.aug_hash(0xFFFFFFFF, 0xFFFFFFFF, 1, 6) == 0x8470EB8D


def test_draw_known_answers():
    """seed 7, step 3, 37x53 -> 32x48, scales 1.0 ... 1.4 (q in [1024, 1434]), by hand from the hashes:
    sample 0 draws q = 1343 -> 49x70, crop (8, 6), flip, u = 7062347, 2827503, 14020457"""
    amps = (10 / 180, 20 / 255, 50 / 255)
    row = R.draw_row(7, 3, 0, 37, 53, 32, 48, 1024, 1434, 0.5, amps)
    assert row[:5] == (49, 70, 8, 6, 1)
    for got, k, amp in zip(row[5:], (-2652522, -11122210, 11263698), amps):
        assert got.dtype == np.float32 and got == np.float32(k) * np.float32(amp / 2 ** 24)
        assert abs(float(got) - k / 2 ** 24 * amp) < 1e-8
    row = R.draw_row(7, 3, 1, 37, 53, 32, 48, 1024, 1434, 0.5, amps)
    assert row[:5] == (49, 70, 17, 2, 0)
    t = R.draw_table(7, 3, 2, 37, 53, 32, 48)
    assert t.dtype == np.int32 and t.shape == (2, 8) and tuple(t[1, :5]) == (49, 70, 17, 2, 0)
    assert R.unpack_row(t[0])[5:] == R.draw_row(7, 3, 0, 37, 53, 32, 48, 1024, 1434, 0.5, amps)[5:]


def test_draws_stay_in_range_and_reach_both_ends():
    amps = (10 / 180, 20 / 255, 50 / 255)
    rows = [R.draw_row(1, step, s, 37, 53, 32, 48, 1024, 1434, 0.5, amps)
            for step in range(100) for s in range(100)]
    assert len(rows) == 10000
    lo_y = hi_y = lo_x = hi_x = flips = 0
    qs = set()
    for hr, wr, cy, cx, flip, dh, ds, dv in rows:
        assert 37 <= hr <= (37 * 1434 + 512) >> 10 and 53 <= wr <= (53 * 1434 + 512) >> 10
        assert 0 <= cy <= hr - 32 and 0 <= cx <= wr - 48 and flip in (0, 1)
        assert abs(dh) <= np.float32(amps[0]) and abs(ds) <= np.float32(amps[1]) and abs(dv) <= np.float32(amps[2])
        lo_y += cy == 0
        hi_y += cy == hr - 32
        lo_x += cx == 0
        hi_x += cx == wr - 48
        flips += flip
        qs.add((hr, wr))
    assert min(lo_y, hi_y, lo_x, hi_x) > 0
    assert 4500 < flips < 5500
    assert (37, 53) in qs and ((37 * 1434 + 512) >> 10, (53 * 1434 + 512) >> 10) in qs
    dh = np.array([r[5] for r in rows])
    assert dh.min() < -0.9 * amps[0] and dh.max() > 0.9 * amps[0] and abs(dh.mean()) < 0.05 * amps[0]
    assert all(R.draw_row(1, 0, s, 37, 53, 32, 48, 1024, 1434, 0.0, amps)[4] == 0 for s in range(64))
    assert all(R.draw_row(1, 0, s, 37, 53, 32, 48, 1024, 1434, 1.0, amps)[4] == 1 for s in range(64))


# ---- geometry ----------------------------------------------------------------------------------------
def _identity_table(n, h, w, flip=0):
    return R.pack_rows([(h, w, 0, 0, flip, 0.0, 0.0, 0.0)] * n)


def test_identity_parameters_reproduce_the_input():
    b = R.random_batch(2, 37, 53, seed=1)
    out = R.reference_apply(b, _identity_table(2, 37, 53), 37, 53, (2000.0, 900.0), hsv=False)
    assert np.array_equal(out['rgb_u8'], b['rgb'])
    assert np.array_equal(out['semantic'], b['semantic']) and np.array_equal(out['instance'], b['instance'])
    assert np.array_equal(out['rgb'], R.normalize_rgb_u8(b['rgb']).transpose(0, 3, 1, 2))
    assert np.array_equal(out['depth'][:, 0], R.normalize_depth(b['depth'], 2000.0, 900.0))
    assert (out['depth'][:, 0][b['depth'] == 0] == 0).all() and (b['depth'] == 0).any()
    assert np.array_equal(out['orientations'], b['orientations'], equal_nan=True)


def test_upscale_2x2_to_4x4_by_hand():
    """per axis the weights of (p0, p1) are (1, 0), (3/4, 1/4), (1/4, 3/4), (0, 1); .5 rounds up"""
    i0, i1, a = R.bilinear_axis(np.arange(4), 2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [0, 1, 1, 1] and a.tolist() == [1536, 512, 1536, 512]
    img = np.array([[0, 100], [200, 40]], np.uint8)[:, :, None]
    want = [[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]]
    assert R.resize_bilinear_u8(img, 4, 4)[:, :, 0].tolist() == want
    lab = np.array([[1, 2], [3, 4]], np.uint8)
    assert R.nearest(lab, 4, 4, np.arange(4), np.arange(4)).tolist() == [[1, 1, 2, 2], [1, 1, 2, 2],
                                                                        [3, 3, 4, 4], [3, 3, 4, 4]]


def test_flipped_row_by_hand():
    b = {'rgb': np.array([[[[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]]], np.uint8),
         'depth': np.array([[[0, 500, 600, 700]]], np.uint16),
         'semantic': np.array([[[1, 2, 3, 4]]], np.uint8)}
    out = R.reference_apply(b, _identity_table(1, 1, 4, flip=1), 1, 4, (0.0, 1.0), hsv=False)
    assert out['rgb_u8'][0, 0].tolist() == [[10, 11, 12], [7, 8, 9], [4, 5, 6], [1, 2, 3]]
    assert out['semantic'][0, 0].tolist() == [4, 3, 2, 1]
    assert out['depth'][0, 0, 0].tolist() == [700.0, 600.0, 500.0, 0.0]
    # a crop of two at cx = 1 of the flipped row reads source columns 2, 1
    t = R.pack_rows([(1, 4, 0, 1, 1, 0.0, 0.0, 0.0)])
    assert R.reference_apply(b, t, 1, 2, hsv=False)['semantic'][0, 0].tolist() == [3, 2]


@pytest.mark.parametrize('hs,ws', [(37, 53), (96, 128), (480, 640)])
def test_bilinear_within_one_grey_level_of_pillow(hs, ws):
    from PIL import Image
    img = np.random.default_rng(hs).integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    for q in (1024, 1025, 1100, 1229, 1434, 2048):
        hr, wr = (hs * q + 512) >> 10, (ws * q + 512) >> 10
        ours = R.resize_bilinear_u8(img, hr, wr)
        theirs = np.asarray(Image.fromarray(img).resize((wr, hr), Image.BILINEAR))
        diff = np.abs(ours.astype(np.int16) - theirs.astype(np.int16))
        if q == 1024:
            assert np.array_equal(ours, img) and not diff.any()
        assert diff.max() <= 1, (q, int(diff.max()))


# ---- colour ------------------------------------------------------------------------------------------
def _all_colours():
    g = np.random.default_rng(5)
    special = [[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [255, 255, 0], [0, 255, 0],
               [0, 255, 255], [0, 0, 255], [255, 0, 255], [1, 0, 0], [254, 255, 255], [200, 200, 199]]
    return np.concatenate([np.array(special, np.uint8), g.integers(0, 256, (4000, 3), dtype=np.uint8)])


def test_hsv_zero_deltas_return_the_input():
    c = _all_colours()
    out = R.hsv_jitter(c, 0.0, 0.0, 0.0)
    # the hue (< 6, ulp 8.9e-16) passes through about six roundings, the rest through a few of ulp(1)
    assert out.dtype == np.float64 and np.abs(out - c / 255.0).max() < 1e-14


def test_hsv_clips_at_both_ends():
    c = _all_colours()
    assert np.array_equal(R.hsv_jitter(c, 0.0, 0.0, -1.0), np.zeros(c.shape))          # value 0: black
    up = R.hsv_jitter(c, 0.0, 0.0, 1.0)                                                # value 1
    assert np.array_equal(up.max(-1), np.ones(len(c)))
    grey = R.hsv_jitter(c, 0.0, -1.0, 0.0)                                             # saturation 0
    assert np.abs(grey - (c.max(-1, keepdims=True) / 255.0)).max() < 1e-15
    full = R.hsv_jitter(c[3:], 0.3, 1.0, 0.0)                                          # saturation 1
    assert np.abs(full.min(-1)).max() < 1e-15
    assert 0.0 <= R.hsv_jitter(c, 0.2, 0.5, 0.5).min() and R.hsv_jitter(c, 0.2, 0.5, 0.5).max() <= 1.0


def test_hsv_wraps_hue_across_zero():
    red = np.array([[255, 0, 0]], np.uint8)
    assert np.abs(R.hsv_jitter(red, 1 / 6, 0, 0) - [1, 1, 0]).max() < 1e-12            # +60 degrees: yellow
    assert np.abs(R.hsv_jitter(red, -1 / 6, 0, 0) - [1, 0, 1]).max() < 1e-12           # -60 degrees: magenta
    assert np.abs(R.hsv_jitter(red, -1 / 12, 0, 0) - [1, 0, 0.5]).max() < 1e-12
    magenta = np.array([[255, 0, 255]], np.uint8)
    assert np.abs(R.hsv_jitter(magenta, 1 / 3, 0, 0) - [1, 1, 0]).max() < 1e-12        # 300 + 120 = 60
    c = _all_colours()
    assert np.abs(R.hsv_jitter(c, 1.0, 0, 0) - c / 255.0).max() < 1e-12                # a full turn
    there = R.hsv_jitter(c, 0.25, 0, 0)
    assert np.abs(there.max(-1) - c.max(-1) / 255.0).max() < 1e-12                     # value is kept
    assert np.abs(there.min(-1) - c.min(-1) / 255.0).max() < 1e-12                     # and so is chroma


def test_hsv_float32_twin_is_close_to_float64():
    """the bound the GPU gate leans on: the float32 arithmetic against float64, on the normalised values,
    over random and special colours at the extreme default deltas of both signs and at none"""
    c = _all_colours()
    worst = 0.0
    for dh, ds, dv in [(0, 0, 0), (10 / 180, 20 / 255, 50 / 255), (-10 / 180, -20 / 255, -50 / 255),
                       (10 / 180, -20 / 255, 50 / 255), (-10 / 180, 20 / 255, -50 / 255), (0.013, 0.02, -0.07)]:
        a = R.normalize_rgb_unit(R.hsv_jitter(c, np.float32(dh), np.float32(ds), np.float32(dv), np.float32),
                                 np.float32)
        b = R.normalize_rgb_unit(R.hsv_jitter(c, np.float32(dh), np.float32(ds), np.float32(dv)))
        assert a.dtype == np.float32
        worst = max(worst, float(np.abs(a - b).max()))
    print(f"float32 twin vs float64, normalised values: {worst:.3e}")
    assert worst <= 2.5e-5


# ---- orientations ------------------------------------------------------------------------------------
def test_orientation_flip():
    t = np.array([[0.0, np.pi / 2, np.nan, 6.0], [0.0, np.pi / 2, np.nan, 6.0]], np.float32)
    out = R.flip_orientations(t, [1, 0])
    assert out.dtype == np.float32
    assert out[0, 0] == 0.0 and np.isnan(out[0, 2])
    assert abs(out[0, 1] - 1.5 * np.pi) < 1e-6 and abs(out[0, 3] - (2 * np.pi - 6.0)) < 1e-6
    assert np.array_equal(out[1], t[1], equal_nan=True)
    assert ((out[0][[0, 1, 3]] >= 0) & (out[0][[0, 1, 3]] < 2 * np.pi)).all()
    assert np.abs(R.flip_orientations(out, [1, 0])[:, 1] - t[:, 1]).max() < 1e-6     # twice: back, to an ulp


# ---- the host side of the engine ---------------------------------------------------------------------
def _augmenter(**kw):
    from emsanet_amd import TrainingAugmenter, full_args
    ctor = {k: kw.pop(k) for k in ('seed', 'hsv_jitter', 'flip_p', 'ring') if k in kw}
    kw.setdefault('input_height', 32)
    kw.setdefault('input_width', 48)
    return TrainingAugmenter(full_args(**kw), (2000.0, 900.0), **ctor)


def _cpu_batch(n, hs, ws):
    b = R.random_batch(n, hs, ws, max_instances=16)
    return {k: torch.from_numpy(v) for k, v in b.items()}


def test_args_carry_the_reference_defaults():
    from emsanet_amd import default_args
    a = default_args()
    assert a.aug_scale_min == 1.0 and a.aug_scale_max == 1.4
    aug = _augmenter()
    assert (aug.q_min, aug.q_max) == (1024, 1434) and aug.flip_threshold == 2 ** 31
    assert aug.hsv_jitter == (10 / 180, 20 / 255, 50 / 255)
    assert aug.state_dict() == {'seed': 0, 'step': 0}
    aug.load_state_dict({'seed': 5, 'step': 9})
    assert aug.state_dict() == {'seed': 5, 'step': 9}


def test_refuses_a_crop_larger_than_the_smallest_resize():
    aug = _augmenter(aug_scale_min=0.5, aug_scale_max=1.0)
    with pytest.raises(ValueError, match='smaller than the 32x48 crop'):
        aug.apply(_cpu_batch(1, 37, 53))
    with pytest.raises(ValueError, match='smaller than'):
        _augmenter().check_size(31, 53)
    _augmenter().check_size(32, 48)
    _augmenter(aug_scale_min=0.6, aug_scale_max=1.0).check_size(60, 80)
    with pytest.raises(ValueError, match='smaller than'):
        _augmenter(aug_scale_min=0.6, aug_scale_max=1.0).check_size(52, 80)      # 31.2 -> 31 rows


def test_refuses_sizes_over_4096():
    with pytest.raises(ValueError, match='4096'):
        _augmenter(input_height=4097)
    aug = _augmenter()
    with pytest.raises(ValueError, match='4096'):
        aug.check_size(4097, 64)
    with pytest.raises(ValueError, match='4096'):
        aug.apply({'rgb': torch.zeros((1, 40, 4097, 3), dtype=torch.uint8),
                   'depth': torch.zeros((1, 40, 4097), dtype=torch.uint16),
                   'semantic': torch.zeros((1, 40, 4097), dtype=torch.uint8),
                   'instance': torch.zeros((1, 40, 4097), dtype=torch.uint8),
                   'orientations': torch.zeros((1, 16)), 'scene': torch.zeros(1, dtype=torch.int64)})
    with pytest.raises(ValueError, match='4096'):
        aug.resize_normalize(_cpu_batch(1, 37, 53), 5000, 32)
    aug.check_size(4096, 4096)
    with pytest.raises(ValueError, match='16384'):
        _augmenter(aug_scale_max=4.5).check_size(4096, 4096)


def test_refuses_the_normal_task():
    with pytest.raises(NotImplementedError, match='normal'):
        _augmenter(tasks=('semantic', 'normal'))


def test_refuses_cpu_tensors_and_wrong_types():
    aug = _augmenter()
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        aug.apply(_cpu_batch(2, 37, 53))
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        aug.resize_normalize(_cpu_batch(2, 37, 53), 24, 32)
    b = _cpu_batch(2, 37, 53)
    with pytest.raises(TypeError, match="'rgb'"):
        aug.apply(dict(b, rgb=b['rgb'].float()))
    with pytest.raises(TypeError, match="'instance'"):
        aug.apply(dict(b, instance=b['instance'].float()))
    with pytest.raises(ValueError, match="'depth'"):
        aug.apply(dict(b, depth=b['depth'][:, :30].contiguous()))
    with pytest.raises(TypeError, match="'semantic'"):
        aug.apply({k: v for k, v in b.items() if k != 'semantic'})
    with pytest.raises(ValueError):
        _augmenter(hsv_jitter=(0.1, 0.2))
    with pytest.raises(ValueError):
        _augmenter(flip_p=1.5)
