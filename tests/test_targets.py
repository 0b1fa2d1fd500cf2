"""CPU: the NumPy reference of the training-target rules (tests/targets_reference.py) against images
small enough to compute by hand, and the host side of emsanet_amd/targets.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_reference as R   # noqa: E402


def f32(v):
    return np.float32(v)


def test_reference_two_rectangles_by_hand():
    """8x8, sigma 1 (window radius 4), classes 1 and 2 are things:
         A: id 1, rows 1..2, columns 1..3: mean (1.5, 2)   -> centre (2, 2)  (1.5 rounds to even)
         B: id 5, rows 5..7, columns 4..7: mean (6, 5.5)   -> centre (6, 6)"""
    sem = np.zeros((1, 8, 8), np.int64)
    inst = np.zeros((1, 8, 8), np.int64)
    R.rect(sem[0], 1, 2, 1, 3, 1)
    R.rect(inst[0], 1, 2, 1, 3, 1)
    R.rect(sem[0], 5, 7, 4, 7, 2)
    R.rect(inst[0], 5, 7, 4, 7, 5)
    r = R.reference_targets(sem, inst, (False, True, True), scales=(1,), sigma=1, max_instances=8)
    assert r['centers'] == [[{1: (2, 2), 5: (6, 6)}]]
    assert not r['bad_id'] and not r['bad_label']
    c = r['instance'][0]['center'][0, 0]
    assert c.dtype == np.float32
    assert c[2, 2] == 1.0 and c[6, 6] == 1.0
    assert c[2, 3] == f32(math.exp(-0.5)) and c[1, 2] == f32(math.exp(-0.5))
    assert c[4, 4] == f32(math.exp(-4.0))            # d2 = 8 from both centres
    assert c[3, 5] == f32(math.exp(-5.0))            # d2 = 10 from both
    assert c[0, 0] == f32(math.exp(-4.0))            # A only (B: dy = -6, outside)
    assert c[2, 6] == f32(math.exp(-8.0))            # the window's edge: dx = 4 (A), dy = -4 (B)
    assert c[0, 7] == 0.0 and c[7, 1] == 0.0         # |dx| = 5 / |dy| = 5 from the nearer centre: outside
    assert c[7, 2] == f32(math.exp(-0.5 * (1 + 16)))  # B: dy = 1, dx = -4, just inside
    fg = r['instance'][0]['foreground'][0]
    assert fg.dtype == bool and fg.sum() == 6 + 12 and np.array_equal(fg, inst[0] != 0)
    o = r['instance'][0]['offset'][0]
    assert o.dtype == np.float32 and o.shape == (2, 8, 8)
    assert (o[0, 1, 1], o[1, 1, 1]) == (0.125, 0.125)          # (2 - 1) / 8
    assert (o[0, 2, 3], o[1, 2, 3]) == (0.0, -0.125)
    assert (o[0, 5, 4], o[1, 5, 4]) == (0.125, 0.25)           # (6 - 5) / 8, (6 - 4) / 8
    assert (o[0, 7, 7], o[1, 7, 7]) == (-0.125, -0.125)
    assert not o[:, ~fg].any()
    assert np.array_equal(r['semantic'][0], sem)
    # pixel offsets ('deeplab' encoding)
    p = R.reference_targets(sem, inst, (False, True, True), scales=(1,), sigma=1, max_instances=8,
                            normalized_offset=False)['instance'][0]['offset'][0]
    assert (p[0, 5, 4], p[1, 5, 4]) == (1.0, 2.0) and (p[0, 7, 7], p[1, 7, 7]) == (-1.0, -1.0)
    # B on a stuff class: cleared, its centre and its bump are gone, the label stays
    r = R.reference_targets(sem, inst, (False, True, False), scales=(1,), sigma=1, max_instances=8)
    assert r['centers'] == [[{1: (2, 2)}]] and r['instance'][0]['foreground'].sum() == 6
    assert r['instance'][0]['center'][0, 0, 6, 6] == f32(math.exp(-16.0)) and r['semantic'][0][0, 6, 6] == 2


def test_reference_half_way_centres_and_coarse_scale():
    """a 2x2 instance has the mean (r + .5, c + .5): half to even in both directions, with an even
    and with an odd integer part; at scale 2 only the pixels on even rows and columns are left"""
    sem = np.ones((2, 8, 8), np.int64)
    inst = np.zeros((2, 8, 8), np.int64)
    R.rect(inst[0], 2, 3, 4, 5, 3)        # mean (2.5, 4.5) -> (2, 4)
    R.rect(inst[1], 3, 4, 5, 6, 3)        # mean (3.5, 5.5) -> (4, 6)
    ori = np.full((2, 4), np.nan, np.float32)
    ori[0, 3] = 0.25
    r = R.reference_targets(sem, inst, (False, True), (False, True), ori, scene=[2, 0], scales=(1, 2),
                            sigma=1, max_instances=4)
    assert r['centers'][0] == [{3: (2, 4)}, {3: (4, 6)}]
    # scale 2 (sigma_2 = 4 * 1 // 2 = 2): image 0 keeps (2, 4) -> (1, 2); image 1 keeps (4, 6) -> (2, 3)
    assert r['centers'][1] == [{3: (1, 2)}, {3: (2, 3)}]
    assert r['instance'][1]['foreground'].sum() == 2
    assert r['instance'][1]['center'][0, 0, 1, 3] == f32(math.exp(-1.0 / 8.0))
    o = r['instance'][0]['offset']
    assert (o[0, 0, 3, 5], o[0, 1, 3, 5]) == (-0.125, -0.125) and (o[1, 0, 3, 5], o[1, 1, 3, 5]) == (0.125, 0.125)
    assert np.array_equal(r['instance'][0]['orientation'][0] == f32(0.25), inst[0] == 3)
    assert np.array_equal(r['instance'][0]['orientation_foreground'][0], inst[0] == 3)
    assert not r['instance'][0]['orientation'][1].any() and not r['instance'][0]['orientation_foreground'][1].any()
    assert r['scene'].dtype == np.int64 and r['scene'].tolist() == [2, 0]
    assert r['semantic'][1].shape == (2, 4, 4)


def test_reference_flags_labels_out_of_range():
    sem = np.ones((1, 4, 4), np.int64)
    inst = np.zeros((1, 4, 4), np.int64)
    inst[0, 1, 1:3] = 2
    inst[0, 3, 3] = 4                     # == max_instances
    r = R.reference_targets(sem, inst, (False, True), scales=(1,), sigma=1, max_instances=4)
    assert r['bad_id'] and not r['bad_label'] and r['centers'] == [[{2: (1, 2)}]]
    inst[0, 3, 3] = 0
    sem[0, 0, 0] = 2
    r = R.reference_targets(sem, inst, (False, True), scales=(1,), sigma=1, max_instances=4)
    assert r['bad_label'] and not r['bad_id'] and r['centers'] == [[{2: (1, 2)}]]


def test_edge_scene_holds_its_cases():
    """the scene of the GPU test contains what its docstring promises"""
    sem, inst, ori, scene = R.edge_scene()
    r = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene)
    full, s32, s16, s8 = r['centers']
    assert full[0] == {} and not inst[0].any() and len(np.unique(sem[0])) == 6
    assert full[1] == {3: (6, 114), 7: (50, 70), 20: (48, 18), 21: (52, 38), 40: (81, 114),
                       50: (64, 64), 51: (68, 82), 255: (20, 24)}        # 30 (stuff), 31 (void): cleared
    assert (inst[1] == 30).any() and (inst[1] == 31).any() and (inst[1] == 7).sum() == 1
    assert 40 in s16[1] and 40 not in s32[1] and 7 not in s8[1]
    assert abs(48 - 52) <= 25 and abs(18 - 38) <= 25                      # the two windows overlap
    fgo = r['instance'][0]['orientation_foreground'][1]
    assert fgo[inst[1] == 20].all() and not fgo[inst[1] == 21].any() and not fgo[inst[1] == 3].any()
    assert len(full[2]) > 10


def _args(**kw):
    from emsanet_amd import full_args
    return full_args(**kw)


def test_instance_center_sigma_default():
    assert _args().instance_center_sigma == 8


def test_gauss_table():
    from emsanet_amd.targets import gauss_table, scale_sigma
    assert [scale_sigma(8, s) for s in (1, 32, 16, 8)] == [8, 1, 2, 4]
    t = gauss_table(2)
    assert t.dtype == np.float32 and len(t) == 2 * 7 * 7 + 1 and t[0] == 1.0
    assert t[8] == f32(math.exp(-1.0)) and t[-1] == f32(math.exp(-98.0 / 8.0))


def test_orientation_table():
    from emsanet_amd import orientation_table
    t = orientation_table([{3: 0.5, 7: -1.0}, {}, {255: 3.0}], 256)
    assert t.shape == (3, 256) and t.dtype == torch.float32
    assert t[0, 3] == 0.5 and t[0, 7] == -1.0 and t[2, 255] == 3.0
    assert int(torch.isnan(t).sum()) == 3 * 256 - 3
    assert t.is_pinned() == torch.cuda.is_available()
    with pytest.raises(ValueError):
        orientation_table([{256: 0.1}], 256)
    with pytest.raises(ValueError):
        orientation_table([{0: 0.1}], 256)


def test_host_side_refusals():
    from emsanet_amd import TrainingTargetGenerator
    gen = TrainingTargetGenerator(_args(), R.IS_THING, R.USE_ORIENTATION)
    assert gen.normalized_offset and gen.sigma == 8
    assert [(s, sg) for s, sg, _sem, _inst in gen.plan] == [(1, 8), (32, 1), (16, 2), (8, 4)]
    assert not TrainingTargetGenerator(_args(instance_offset_encoding='deeplab'), R.IS_THING).normalized_offset
    with pytest.raises(ValueError, match='divisible'):
        gen.check_size(480, 650)
    gen.check_size(480, 640)
    with pytest.raises(ValueError, match='divisible'):        # before anything touches a device
        gen.generate({'semantic': torch.zeros(1, 100, 128, dtype=torch.int64),
                      'instance': torch.zeros(1, 100, 128, dtype=torch.int64)})
    with pytest.raises(ValueError, match='sigma_32 = 0'):
        TrainingTargetGenerator(_args(instance_center_sigma=7), R.IS_THING)      # 28 // 32
    with pytest.raises(ValueError, match='sigma'):
        TrainingTargetGenerator(_args(instance_center_sigma=0), R.IS_THING)
    # ... which is no refusal where that scale has no instance targets
    g1 = TrainingTargetGenerator(_args(instance_center_sigma=7, instance_no_multiscale_supervision=True),
                                 R.IS_THING)
    assert [(s, sg, inst) for s, sg, _sem, inst in g1.plan] == [(1, 7, True), (32, 0, False), (16, 0, False),
                                                                 (8, 0, False)]
    with pytest.raises(ValueError, match='max_instances'):
        TrainingTargetGenerator(_args(), R.IS_THING, max_instances=1025)
    TrainingTargetGenerator(_args(), R.IS_THING, max_instances=1024)
    with pytest.raises(ValueError):
        TrainingTargetGenerator(_args(), R.IS_THING, use_orientation=(True,))
    with pytest.raises(ValueError):
        TrainingTargetGenerator(_args(), R.IS_THING, scales=(8, 1))


def test_generate_refuses_cpu_tensors():
    from emsanet_amd import TrainingTargetGenerator
    gen = TrainingTargetGenerator(_args(), R.IS_THING, R.USE_ORIENTATION)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        gen.generate({'semantic': torch.zeros(1, 96, 128, dtype=torch.int64),
                      'instance': torch.zeros(1, 96, 128, dtype=torch.int64),
                      'orientations': torch.zeros(1, 256), 'scene': torch.zeros(1, dtype=torch.int64)})
    gen.check()                                   # nothing ran: nothing to report


def test_c_abi_rejects_bad_geometry_before_any_launch():
    from emsanet_amd import _lib
    L = _lib.lib()
    assert L.emsa_targets_workspace_bytes(2, 4, 256) == 4 * 2 * 256 * (24 + 4 + 4) + 4 * 2 * 4
    assert L.emsa_targets_workspace_bytes(2, 4, 1025) == -1 and L.emsa_targets_workspace_bytes(0, 4, 256) == -1
    assert L.emsa_targets_table_entries(8) == 2 * 25 * 25 + 1 and L.emsa_targets_table_entries(0) == -1
    sc = (_lib.EmsaTargetScale * 1)()
    sc[0].scale, sc[0].sigma, sc[0].semantic = 32, 1, 4096
    assert L.emsa_targets_finalize(1, 100, 128, sc, 1, 256, None, None) == -1       # 100 % 32
    assert L.emsa_targets_finalize(1, 96, 128, sc, 1, 256, None, None) == -2        # no workspace
    assert L.emsa_targets_stats(None, 0, None, 0, None, 6, 1, 96, 128, sc, 1, 256, None, None) == -2
    assert L.emsa_targets_render(None, 0, None, 0, None, None, None, 6, 1, 96, 128, sc, 1, 4096, 1, None,
                                 None, None, None) == -1                            # max_instances
    sc[0].center, sc[0].sigma = 4096, 0
    assert L.emsa_targets_stats(None, 0, None, 0, None, 6, 1, 96, 128, sc, 1, 256, None, None) == -1   # sigma 0


def test_corner_scene_holds_its_cases():
    sem, inst, ori, scene = R.corner_scene()
    r = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene)
    assert [t.shape[1:] for t in r['semantic']] == [(32, 32), (1, 1), (2, 2), (4, 4)]
    assert all(t[0].size % 64 for t in r['semantic'][1:])
    # the four corners at full scale, the last table entry among them; the side scales sample (0, 0) only
    assert r['centers'][0][0] == {1: (1, 1), 2: (1, 30), 254: (30, 1), 255: (30, 30)}
    assert [c[0] for c in r['centers'][1:]] == [{1: (0, 0)}] * 3
    assert [c[1] for c in r['centers']] == [{255: (16, 16)}, {255: (0, 0)}, {255: (0, 0)}, {255: (2, 2)}]
    c = r['instance'][0]['center'][0, 0]
    for y, x in ((0, 0), (0, 31), (31, 0), (31, 31)):       # the window (radius 25) leaves the image there
        assert 0 < c[y, x] < 1
    assert c[1, 1] == c[1, 30] == c[30, 1] == c[30, 30] == 1.0
    assert r['instance'][1]['center'].shape == (2, 1, 1, 1) and (r['instance'][1]['center'] == 1.0).all()
    assert not r['bad_id'] and not r['bad_label']
