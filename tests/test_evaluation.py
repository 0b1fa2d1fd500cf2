"""CPU: the NumPy reference of tests/evaluation_reference.py (scene accuracy, angular error, PQ match
lists) pinned by hand-computed cases, and the argument checks of the new metric classes, which run on
the host before any launch."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluation_reference as E   # noqa: E402
import test_metrics as R   # noqa: E402


def _unit(deg):
    """one pixel's (sin, cos) as the fixed-point sum of a one-pixel instance"""
    a = math.radians(deg)
    return [int(np.rint(np.float64(np.float32(math.sin(a))) * E.VEC_ONE)),
            int(np.rint(np.float64(np.float32(math.cos(a))) * E.VEC_ONE))]


# ---- angles ---------------------------------------------------------------------------------------
def test_angle_wraps_around_zero():
    assert abs(E.angular_error(math.radians(359), math.radians(1)) - math.radians(2)) < 1e-12
    assert abs(E.angular_error(math.radians(1), math.radians(359)) - math.radians(2)) < 1e-12
    # through the sums of a one-pixel instance: the 2^-24 grid of the vector moves the angle by < 1e-7
    m = E.AngularErrorReference()
    m.update(np.array([[[0, 0], _unit(359)]], np.int64), np.array([[0, 1]]),
             np.array([[np.nan, math.radians(1)]], np.float32))
    assert m.count == 1 and not m.flag
    assert abs(m.compute()['mae_deg'] - 2.0) < 1e-5


def test_opposite_angle_is_pi():
    assert E.angular_error(0.0, math.pi) == math.pi
    assert E.angular_error(math.pi / 2, 3 * math.pi / 2) == math.pi
    m = E.AngularErrorReference()
    m.update(np.array([[[0, 0], [0, E.VEC_ONE]]], np.int64), np.array([[0, 5]]),
             np.array([[np.nan, math.pi]], np.float32))              # float32(pi) is 8.7e-8 above pi
    assert abs(m.compute()['mae_rad'] - math.pi) < 1e-6 and m.compute()['mae_rad'] <= math.pi


def test_two_pixel_instance_averages_to_45_degrees():
    ori = np.zeros((1, 2, 1, 2), np.float32)
    ori[0, :, 0, 0] = (0.0, 1.0)                                        # 0 deg: (sin, cos)
    ori[0, :, 0, 1] = (1.0, 0.0)                                        # 90 deg
    vec, cnt = E.orientation_sums_reference(ori, np.array([[[1, 1]]]), 2)
    assert vec.tolist() == [[[0, 0], [E.VEC_ONE, E.VEC_ONE]]] and cnt.tolist() == [[0, 2]]
    assert E.angle_of(vec[0, 1]) == math.pi / 4
    m = E.AngularErrorReference()
    m.update(vec, cnt, np.array([[np.nan, 0.0]], np.float32))
    assert (m.total, m.count) == (int(np.rint(math.pi / 4 * E.ANGLE_ONE)), 1)
    assert abs(m.compute()['mae_deg'] - 45.0) < 1e-10


def test_zero_vector_sum_is_angle_zero():
    ori = np.zeros((1, 2, 1, 2), np.float32)
    ori[0, :, 0, 0] = (0.0, 1.0)
    ori[0, :, 0, 1] = (0.0, -1.0)
    vec, cnt = E.orientation_sums_reference(ori, np.array([[[1, 1]]]), 2)
    assert vec[0, 1].tolist() == [0, 0] and E.angle_of(vec[0, 1]) == 0.0
    m = E.AngularErrorReference()
    m.update(vec, cnt, np.array([[np.nan, 0.5]], np.float32))
    assert (m.total, m.count) == (1 << 39, 1)                         # 0.5 rad, exactly


def test_nan_ground_truth_mask_keep_and_empty_set():
    vec = np.array([[[0, 0], _unit(10), _unit(20), _unit(30)]], np.int64)
    cnt = np.array([[0, 1, 1, 0]])
    gt = np.array([[np.nan, np.nan, math.radians(50), math.radians(0)]], np.float32)
    m = E.AngularErrorReference()
    m.update(vec, cnt, gt)                     # 1: NaN ground truth; 3: no pixels; 2: 30 deg
    assert m.count == 1 and abs(m.compute()['mae_deg'] - 30.0) < 1e-5
    m = E.AngularErrorReference()
    m.update(vec, cnt, gt, keep=np.array([[1, 1, 0, 1]]))
    assert m.count == 0 and math.isnan(m.compute()['mae_deg']) and math.isnan(m.compute()['mae_rad'])
    # the mask of the sums: a masked-out pixel does not count
    ori = np.ones((1, 2, 1, 2), np.float32)
    _, c = E.orientation_sums_reference(ori, np.array([[[1, 2]]]), 3, mask=np.array([[[1, 0]]]))
    assert c.tolist() == [[0, 1, 0]]


def test_ids_outside_the_tables_are_flagged_not_compared():
    vec = np.array([[[0, 0], _unit(10), _unit(20)]], np.int64)
    cnt = np.array([[0, 1, 1]])
    m = E.AngularErrorReference()
    m.update(vec, cnt, np.array([[np.nan, 0.0]], np.float32))          # slot 2 has no ground-truth column
    assert m.flag and m.count == 1
    m = E.AngularErrorReference()                                        # matched: stuff pairs are skipped
    m.update_matched(vec, cnt, np.array([[np.nan, 0.0, 0.0]], np.float32),
                     [[(5000, 5000), (1002, 1001), (1001, 1000)]], 1000)
    assert not m.flag and m.count == 1 and abs(m.compute()['mae_deg'] - 20.0) < 1e-5
    m.update_matched(vec, cnt, np.array([[np.nan, 0.0, 0.0]], np.float32), [[(1003, 1001)]], 1000)
    assert m.flag and m.count == 1


# ---- scene ----------------------------------------------------------------------------------------
def test_scene_accuracy_by_hand():
    """3 classes + void; class 3 never occurs in the targets, one target is void.  Kept samples
    (target, pred): (1,1) (1,1) (1,2) (2,2) (1,3): acc = 3/5; recall 1: 2/4, recall 2: 1/1 -> bacc 3/4"""
    target = np.array([1, 1, 1, 2, 0, 1])
    pred = np.array([1, 1, 2, 2, 3, 3])
    cm, bad = R.confusion_reference(pred, target, 4)
    assert bad == 0
    acc, bacc = E.scene_reference(cm, True)
    assert acc == 0.6 and bacc == 0.75
    assert E.scene_reference(np.zeros((4, 4), np.int64), True) == (0.0, 0.0)


# ---- PQ match list --------------------------------------------------------------------------------
def test_match_list_by_hand():
    """image 0: thing 1/1 (IoU 3/4) and stuff 5 (IoU 1) match; prediction 2/1 is a false positive,
    prediction 2/2 lies in void.  image 1 (`void_overlap_image`): only stuff 5 matches."""
    t0 = np.array([[1001, 1001, 5000, 5000], [1001, 1001, 5000, 0]], np.int64)
    p0 = np.array([[1001, 1001, 5000, 5000], [1001, 2001, 5000, 2002]], np.int64)
    p1, t1 = R.void_overlap_image(1000)
    ref = E.PanopticQualityPairsReference(R.SCENE_CATEGORIES, 0, 1000, R.SCENE_IS_THING)
    ref.update(np.stack([p0, p1]), np.stack([t0, t1]))
    assert [sorted(x) for x in ref.pairs] == [[(1001, 1001), (5000, 5000)], [(5000, 5000)]]
    assert ref.tp == [0, 1, 0, 0, 0, 2, 0] and ref.fp == [0, 0, 1, 0, 0, 0, 0] and ref.fn == [0] * 7
    assert ref.void_skipped == 2
    assert [len(x) for x in ref.pairs] == [2, 1] and sum(ref.tp) == 3
    # the random scenes of the GPU test: as many pairs as true positives
    pred, target = R.rectangle_batch(2, 37, 53, 8, 1000, 2)
    ref = E.PanopticQualityPairsReference(R.SCENE_CATEGORIES, 0, 1000, R.SCENE_IS_THING)
    ref.update(pred, target)
    assert sum(len(x) for x in ref.pairs) == sum(ref.tp) >= 2


def test_pan_ids():
    sem = np.array([[0, 1, 4, 9]])
    inst = np.array([[3, 3, 3, 3]])
    assert E.pan_ids(sem, inst, R.SCENE_IS_THING, 1000).tolist() == [[0, 1003, 4000, 0]]


# ---- refusals -------------------------------------------------------------------------------------
def test_new_metrics_refuse_bad_arguments_by_name():
    import torch
    from emsanet_amd import MeanAbsoluteAngularError, PanopticQuality, SceneAccuracy
    vec, cnt = torch.zeros(2, 4, 2, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32)
    gt = torch.zeros(2, 5)
    m = MeanAbsoluteAngularError()
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        m.update(vec, cnt, gt)
    with pytest.raises(TypeError, match='vec has dtype'):
        m.update(vec.int(), cnt, gt)
    with pytest.raises(TypeError, match='gt_table has dtype'):
        m.update(vec, cnt, gt.double())
    with pytest.raises(TypeError, match='keep has dtype'):
        m.update(vec, cnt, gt, keep=cnt)
    with pytest.raises(ValueError, match='expected'):
        m.update(vec, cnt[:, :3], gt)
    with pytest.raises(ValueError, match='expected'):
        m.update(vec, cnt, gt[:1])
    with pytest.raises(ValueError, match='expected'):
        m.update(vec, cnt, gt, keep=torch.zeros(2, 3, dtype=torch.bool))
    matches, n_matches = torch.zeros(2, 8, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        m.update_matched(vec, cnt, gt, matches, n_matches, 1000)
    with pytest.raises(TypeError, match='n_matches has dtype'):
        m.update_matched(vec, cnt, gt, matches, n_matches.long(), 1000)
    with pytest.raises(ValueError, match='label_divisor'):
        m.update_matched(vec, cnt, gt, matches[:1], n_matches, 1000)
    with pytest.raises(ValueError, match='label_divisor'):
        m.update_matched(vec, cnt, gt, matches, n_matches, 0)
    assert math.isnan(m.compute()['mae_deg']) and math.isnan(m.compute()['mae_rad'])
    s = SceneAccuracy(4)
    x = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        s.update(x, x)
    with pytest.raises(TypeError, match='dtype'):
        s.update(x.float(), x)
    with pytest.raises(ValueError, match='equal shape'):
        s.update(x, x[:2])
    with pytest.raises(ValueError, match='equal shape'):
        s.update(x.view(3, 1), x.view(3, 1))
    assert s.compute() == {'acc': 0.0, 'bacc': 0.0}
    ids = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        PanopticQuality(7, 0, 1000, 256 ** 3, R.SCENE_IS_THING).update_with_matches(ids, ids)


def test_evaluator_refuses_cpu_batches_and_knows_its_keys():
    import torch
    from emsanet_amd import ValidationEvaluator, default_args, full_args, nyuv2_config
    ev = ValidationEvaluator(default_args(tasks=('semantic', 'scene')), nyuv2_config())
    assert ev.compute() == {'semantic_miou': 0.0, 'scene_acc': 0.0, 'scene_bacc': 0.0}
    sem = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        ev.update({'semantic_segmentation_idx': sem.long()}, {'semantic': sem, 'scene': sem[:, 0, 0]})
    ev = ValidationEvaluator(full_args(enable_panoptic=True), nyuv2_config())
    keys = set(ev.compute())
    assert {'semantic_miou', 'scene_bacc', 'orientation_mae_gt_deg', 'panoptic_all_deeplab_pq',
            'panoptic_deeplab_semantic_miou', 'panoptic_mae_deeplab_deg'} <= keys
    assert 'instance_all_with_gt_deeplab_pq' not in keys        # no such map seen yet
    assert not any('with_gt' in k and k.startswith('panoptic') for k in keys)
    assert math.isnan(ev.compute()['orientation_mae_gt_deg'])
    with pytest.raises(ValueError, match='max_instances'):
        ValidationEvaluator(full_args(), nyuv2_config(), max_instances=2000)


def test_new_entries_validate_on_the_host():
    """negative codes before any launch (no GPU needed)"""
    from emsanet_amd import _lib
    L = _lib.lib()
    assert L.emsa_panoptic_match_pairs(8, 1, 256, 7, 0, 1000, 8, 8, 8, 8, None, 8, 8, None) == -2
    assert L.emsa_panoptic_match_pairs(8, 1, 2048, 7, 0, 1000, 8, 8, 8, 8, 8, 8, 8, None) == -1
    assert L.emsa_angular_error(None, 8, None, 1, 4, 8, 4, None, None, 0, 1, 8, 8, None) == -2
    assert L.emsa_angular_error(8, 8, None, 1, 4, 8, 4, 8, None, 8, 1000, 8, 8, None) == -2   # half a list
    assert L.emsa_angular_error(8, 8, None, 1, 1, 8, 4, None, None, 0, 1, 8, 8, None) == -1
    assert L.emsa_angular_error(8, 8, None, 1, 4, 8, 4, 8, 8, 2048, 1000, 8, 8, None) == -1
    assert L.emsa_angular_error(8, 8, None, 1, 4, 8, 4, 8, 8, 8, 0, 8, 8, None) == -1
