"""Device-side validation (emsanet_amd/evaluation.py, the new entries of csrc/metrics.hip) against the
NumPy restatement of tests/evaluation_reference.py.

Bounds: every count is an integer and must match exactly.  The angular-error sum is int64 fixed point
(2^-40 rad) with each term rounded once: |dev - ref| <= count units (half a unit per term for the
rounding, doubled as margin; the device's double atan2 differs from NumPy's by ~1e-16, far below a
unit).  Results within 1e-9 (one unit is 5.2e-11 deg), the bar tests/test_metrics_gpu.py uses.

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (counts, match pairs and
confusion matrices are compared exactly): the evaluator's buffers, the metric states and workspaces lie
between two bands of 0xFF, hand-made inputs are placed with `guard.put`.  The model whose prediction the
evaluator tests read is built by a module fixture, before the arena is installed; the two tests that
run a model themselves are opted out (guard.OPT_OUT)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluation_reference as E   # noqa: E402
import guard   # noqa: E402
import test_metrics as R   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return guard.put(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))    # flush between two bands of 0xFF


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- match export ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name,images', [('2x37x53', 2), ('4x48x64', 3)])
def test_match_pairs_equal_match_and_export_the_reference_pairs(name, images):
    from emsanet_amd import _lib
    _, _, h, w, k, div, seed = next(s for s in R.SCENES if s[0] == name)
    pred, target = R.rectangle_batch(images, h, w, k, div, seed)
    ref = E.PanopticQualityPairsReference(R.SCENE_CATEGORIES, 0, div, R.SCENE_IS_THING)
    ref.update(pred, target)
    L, T, K = _lib.lib(), 256, R.SCENE_CATEGORIES
    p, t = _dev(pred), _dev(target)
    from emsanet_amd import functional as Fn
    ws = Fn._empty((L.emsa_panoptic_workspace_bytes(images, T),), DEV, torch.uint8)      # (the arena's)
    a = guard.put(torch.zeros(4 * K + 1, device=DEV, dtype=torch.int64))
    b = guard.put(torch.zeros(4 * K + 1, device=DEV, dtype=torch.int64))
    matches = guard.put(torch.full((images, T, 2), -7, device=DEV, dtype=torch.int64))
    n_matches = guard.put(torch.full((images,), -7, device=DEV, dtype=torch.int32))
    assert L.emsa_panoptic_pairs(p.data_ptr(), t.data_ptr(), images, h * w, T, ws.data_ptr(),
                                 a.data_ptr() + 32 * K, _stream()) == 0
    assert L.emsa_panoptic_match(ws.data_ptr(), images, T, K, 0, div, *(a.data_ptr() + 8 * K * j for j in range(4)),
                                 a.data_ptr() + 32 * K, _stream()) == 0
    assert L.emsa_panoptic_match_pairs(ws.data_ptr(), images, T, K, 0, div,
                                       *(b.data_ptr() + 8 * K * j for j in range(4)), matches.data_ptr(),
                                       n_matches.data_ptr(), b.data_ptr() + 32 * K, _stream()) == 0
    torch.cuda.synchronize()
    guard.check()
    assert int(a[:K].sum()) == sum(ref.tp) >= images
    assert torch.equal(a, b)                                            # tp / fn / fp / iou_sum, flags
    assert a[:K].tolist() == ref.tp and a[K:2 * K].tolist() == ref.fn and a[2 * K:3 * K].tolist() == ref.fp
    m, nm = matches.cpu().numpy(), n_matches.cpu().numpy()
    for i in range(images):
        one = R.PanopticQualityReference(K, 0, div, R.SCENE_IS_THING)
        one.update(pred[i], target[i])
        assert nm[i] == sum(one.tp) == len(ref.pairs[i])
        got = [tuple(int(v) for v in row) for row in m[i, :nm[i]]]
        assert len(set(got)) == len(got) and set(got) == set(ref.pairs[i]), (i, got, ref.pairs[i])
        assert (m[i, nm[i]:] == -7).all()                               # nothing written behind the list


def test_update_with_matches_is_update_and_survives_overflow():
    from emsanet_amd import PanopticQuality

    def pq(**kw):
        return PanopticQuality(R.SCENE_CATEGORIES, 0, 1000, 256 ** 3, R.SCENE_IS_THING, **kw)
    pred, target = R.rectangle_batch(2, 37, 53, 8, 1000, 2)
    a, b = pq(), pq()
    a.update(_dev(pred), _dev(target))
    matches, n_matches = b.update_with_matches(_dev(pred), _dev(target))
    assert torch.equal(a._state, b._state) and a.compute() == b.compute()
    assert matches.shape == (2, 256, 2) and matches.dtype == torch.int64 and matches.is_cuda
    assert n_matches.dtype == torch.int32 and int(n_matches.sum()) == sum(b.counts()['tp'])
    again = b.update_with_matches(_dev(pred), _dev(target))
    assert again[0] is matches and again[1] is n_matches               # owned by the object
    # 20 segments against max_segments = 8: flagged, and at most 8 pairs written
    grid = (np.arange(20).reshape(4, 5) + 1).repeat(6, 0).repeat(7, 1)
    crowded = (4000 + grid).astype(np.int64)[None]
    m = pq(max_segments=8)
    matches, n_matches = m.update_with_matches(_dev(crowded), _dev(crowded))
    guard.check()                                                       # the pairs too many were stored nowhere
    assert matches.shape == (1, 8, 2) and 0 <= int(n_matches[0]) <= 8
    with pytest.raises(ValueError, match='overflow'):
        m.compute()
    few = (4000 + (grid - 1) % 8).astype(np.int64)[None]               # a table exactly full
    m.reset()
    matches, n_matches = m.update_with_matches(_dev(few), _dev(few))
    guard.check()
    assert int(n_matches[0]) == 8 and m.counts()['tp'][4] == 8
    got = sorted(tuple(r) for r in matches[0].tolist())
    assert got == [(4000 + j, 4000 + j) for j in range(8)]


# ---- angular error --------------------------------------------------------------------------------
MAX_INST = 24


def _angle_case(n, h, w, seed):
    """blocky ids in [0, MAX_INST) (MAX_INST - 1 among them), orientation channels, a foreground mask
    that leaves instance 5 of image 0 without a pixel, a ground-truth table with NaN entries"""
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, MAX_INST, (n, (h + 7) // 8, (w + 7) // 8)).repeat(8, 1).repeat(8, 2)[:, :h, :w]
    ids[:, :3, :3] = MAX_INST - 1
    ids[0, 3:6, :3] = 5
    ori = rng.randn(n, 2, h, w).astype(np.float32)
    fg = rng.rand(n, h, w) < 0.8
    fg[0][ids[0] == 5] = False
    fg[:, :3, :3] = True
    gt = (rng.rand(n, MAX_INST) * E.TWO_PI).astype(np.float32)
    gt[:, 0] = np.nan
    gt[rng.rand(n, MAX_INST) < 0.2] = np.nan
    gt[:, MAX_INST - 1] = 1.0
    return ids.astype(np.int32), ori, fg, gt


def _match_lists(n, slots, seed, T=32):
    """hand-made match lists: thing pairs, stuff pairs (instance part 0), an empty list; the rows behind
    n_matches hold valid-looking pairs that must not be read"""
    rng = np.random.RandomState(seed)
    m = np.zeros((n, T, 2), np.int64)
    m[..., 0] = rng.randint(1, 4, (n, T)) * 1000 + rng.randint(1, slots, (n, T))
    m[..., 1] = rng.randint(1, 4, (n, T)) * 1000 + rng.randint(1, MAX_INST, (n, T))
    m[:, ::5, 0] = 5000
    m[:, ::5, 1] = 5000
    m[:, 1::7, 1] = 6000                                                # a thing against a stuff id
    nm = rng.randint(8, T + 1, n).astype(np.int32)
    nm[-1] = 0
    nm[0] = T
    return m, nm


def _check_angle(metric, ref, what):
    total, count = metric.counts()
    print(what, 'count', count, 'sum', total, 'reference', ref.total, 'difference', total - ref.total)
    assert count == ref.count >= 3, (what, count, ref.count)
    assert abs(total - ref.total) <= count, (what, total, ref.total)
    got, want = metric.compute(), ref.compute()
    assert abs(got['mae_deg'] - want['mae_deg']) <= 1e-9 and abs(got['mae_rad'] - want['mae_rad']) <= 1e-9
    assert abs(got['mae_deg'] - math.degrees(got['mae_rad'])) <= 1e-12
    assert 0.0 < got['mae_rad'] < math.pi


@pytest.mark.parametrize('n,h,w', [(3, 37, 53), (2, 96, 128)])
@pytest.mark.parametrize('layout', ['f32', 'bf16_nhwc'])
def test_angular_error_both_modes(n, h, w, layout):
    from emsanet_amd import MeanAbsoluteAngularError
    from emsanet_amd.postprocessing import instance_orientation_sums
    ids, ori, fg, gt = _angle_case(n, h, w, seed=h)
    o = _dev(ori)
    if layout == 'bf16_nhwc':
        o = o.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        ori = o.float().cpu().numpy()
    vec, cnt = instance_orientation_sums(o, _dev(ids), MAX_INST, _dev(fg))
    rvec, rcnt = E.orientation_sums_reference(ori, ids, MAX_INST, fg)
    assert np.array_equal(vec.cpu().numpy(), rvec) and np.array_equal(cnt.cpu().numpy(), rcnt)
    assert rcnt[0, 5] == 0 and rcnt[:, MAX_INST - 1].min() >= 9 and np.isnan(gt[:, 1:]).any()
    # identity mode
    m, ref = MeanAbsoluteAngularError(), E.AngularErrorReference()
    m.update(vec, cnt, _dev(gt))
    ref.update(rvec, rcnt, gt)
    assert not ref.flag
    _check_angle(m, ref, f'identity {n}x{h}x{w} {layout}')
    keep = np.random.RandomState(1).rand(n, MAX_INST) < 0.7
    m.update(vec, cnt, _dev(gt), keep=_dev(keep))                       # accumulates; bool keep table
    ref.update(rvec, rcnt, gt, keep)
    _check_angle(m, ref, 'identity + keep')
    m.reset()
    assert m.counts() == (0, 0) and math.isnan(m.compute()['mae_deg'])
    # matched mode, sums with fewer slots than the ground truth has ids
    slots = 17
    vec, cnt = instance_orientation_sums(o, _dev(ids), slots)
    rvec, rcnt = E.orientation_sums_reference(ori, ids, slots)
    matches, nm = _match_lists(n, slots, seed=w)
    pairs = [[tuple(r) for r in matches[i, :nm[i]].tolist()] for i in range(n)]
    keep8 = keep[:, :slots].astype(np.uint8)
    m, ref = MeanAbsoluteAngularError(), E.AngularErrorReference()
    m.update_matched(vec, cnt, _dev(gt), _dev(matches), _dev(nm), 1000, keep=_dev(keep8))
    guard.check()
    ref.update_matched(rvec, rcnt, gt, pairs, 1000, keep8)
    assert not ref.flag
    _check_angle(m, ref, f'matched {n}x{h}x{w} {layout}')


def test_angular_error_flags_an_id_equal_to_max_instances():
    from emsanet_amd import MeanAbsoluteAngularError
    from emsanet_amd.postprocessing import instance_orientation_sums
    n, h, w = 3, 37, 53
    ids, ori, fg, gt = _angle_case(n, h, w, seed=11)
    ids[1, 10:12, 10:12] = MAX_INST
    fg[1, 10:12, 10:12] = True
    ids[2, 20:22, 20:22] = 1                                             # (compared in the matched case)
    fg[2, 20:22, 20:22] = True
    vec, cnt = instance_orientation_sums(_dev(ori), _dev(ids), MAX_INST + 1, _dev(fg))
    rvec, rcnt = E.orientation_sums_reference(ori, ids, MAX_INST + 1, fg)
    m, ref = MeanAbsoluteAngularError(), E.AngularErrorReference()
    m.update(vec, cnt, _dev(gt))
    guard.check()                                                        # id == MAX_INST: flagged, stored nowhere
    ref.update(rvec, rcnt, gt)
    assert ref.flag
    with pytest.raises(ValueError, match='outside the orientation tables'):
        m.compute()
    s = m._state.cpu()
    assert int(s[1]) == ref.count and abs(int(s[0]) - ref.total) <= ref.count   # the rest was counted
    m.reset()
    m.update(vec[:, :MAX_INST].contiguous(), cnt[:, :MAX_INST].contiguous(), _dev(gt))
    assert m.counts()[1] == ref.count
    # matched mode: a target id whose instance part is MAX_INST, a predicted one beyond the sums
    for bad in ((1001, 1000 + MAX_INST), (1000 + MAX_INST + 1, 1001)):
        matches = np.zeros((n, 8, 2), np.int64)
        matches[:, 0] = (1002, 1002)
        matches[2, 1] = bad
        nm = np.array([1, 1, 2], np.int32)
        m, ref = MeanAbsoluteAngularError(), E.AngularErrorReference()
        m.update_matched(vec, cnt, _dev(gt), _dev(matches), _dev(nm), 1000)
        ref.update_matched(rvec, rcnt, gt, [[tuple(r) for r in matches[i, :nm[i]].tolist()] for i in range(n)],
                           1000)
        assert ref.flag
        with pytest.raises(ValueError, match='outside the orientation tables'):
            m.compute()
        assert int(m._state[1]) == ref.count


# ---- scene accuracy -------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 7, 300])
def test_scene_accuracy(n):
    from emsanet_amd import SceneAccuracy
    rng = np.random.RandomState(n)
    c = 11                                                               # 10 scene classes + void
    target = rng.randint(0, c - 2, n)                                    # void targets; class 9, 10 absent
    pred = np.where(rng.rand(n) < 0.6, np.maximum(target, 1), rng.randint(1, c, n))
    m = SceneAccuracy(c)
    m.update(_dev(pred), _dev(target.astype(np.uint8)))
    m.update(_dev(pred.astype(np.int32)), _dev(target))
    cm, bad = R.confusion_reference(pred, target, c)
    assert bad == 0 and np.array_equal(m.confusion_matrix.cpu().numpy(), 2 * cm)
    acc, bacc = E.scene_reference(2 * cm, True)
    got = m.compute()
    assert abs(got['acc'] - acc) <= 1e-12 and abs(got['bacc'] - bacc) <= 1e-12
    if n == 300:
        assert (target == 0).any() and 0 < acc < 1 and abs(acc - bacc) > 1e-6
    pred[0] = c                                                          # out of range
    m.update(_dev(pred), _dev(target))
    with pytest.raises(ValueError, match='n_invalid'):
        m.compute()
    m.reset()
    assert m.compute() == {'acc': 0.0, 'bacc': 0.0}


# ---- the evaluator --------------------------------------------------------------------------------
H, W, BS = 96, 128, 4
_CACHE = {}


def _config():
    from emsanet_amd import nyuv2_config
    cfg = nyuv2_config()
    labels = cfg.semantic_label_list_without_void
    labels.classes_is_thing = tuple(bool(i % 3) for i in range(len(labels)))
    labels.classes_use_orientations = tuple(bool(i % 3) and i % 5 != 1 for i in range(len(labels)))
    return cfg


def _setup():
    """model (full tasks, enable_panoptic), a labelled batch and its eval prediction -- built once, never
    modified.  Labels as in test_metrics_gpu.test_validation_loop_end_to_end: blocks, with image 0's
    labels set to the model's own prediction so that something matches."""
    if 'full' in _CACHE:
        return _CACHE['full']
    from util import deterministic_state_dict
    from emsanet_amd import full_args
    from emsanet_amd.model import EMSANet
    cfg = _config()
    args = full_args(input_height=H, input_width=W, enable_panoptic=True)
    model = EMSANet(args, cfg)
    model.load_state_dict(deterministic_state_dict(model))
    model.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    batch = {'rgb': torch.randn(BS, 3, H, W, generator=g).to(DEV),
             'depth': torch.randn(BS, 1, H, W, generator=g).to(DEV)}
    with torch.no_grad():
        first = model(batch, do_postprocessing=True)
    n_classes = len(cfg.semantic_label_list_without_void) + 1
    sem = torch.randint(0, n_classes, (BS, H // 16, W // 16), generator=g).repeat_interleave(16, 1) \
        .repeat_interleave(16, 2).to(torch.uint8)
    inst = torch.randint(0, 5, (BS, H // 32, W // 32), generator=g).repeat_interleave(32, 1) \
        .repeat_interleave(32, 2).to(torch.int32)
    sem[0] = first['panoptic_segmentation_deeplab_semantic_idx'][0].cpu().to(torch.uint8)
    inst[0] = first['panoptic_segmentation_deeplab_instance_idx'][0].cpu()
    scene = torch.randint(0, 11, (BS,), generator=g)
    scene[0] = int(first['scene_class_idx'][0]) + 1
    scene[1] = 0
    table = torch.rand(BS, 256, generator=g) * E.TWO_PI
    table[:, 0] = float('nan')
    table[:, 3] = float('nan')
    batch.update(semantic=sem.to(DEV), instance=inst.to(DEV), scene=scene.to(DEV),
                 orientations=table.to(DEV),
                 orientation_foreground=(torch.rand(BS, H, W, generator=g) < 0.9).to(DEV))
    with torch.no_grad():
        prediction = model(batch, do_postprocessing=True)
    _CACHE['full'] = (args, cfg, model, batch, prediction)
    return _CACHE['full']


@pytest.fixture(scope='module')
def full_setup():
    """`_setup()` ahead of the function-scoped guard fixture: the model and its eval forward passes (the
    whole model) run on the plain allocator, the evaluator under test on the arena"""
    return _setup()


def _host_inputs(prediction, batch, fullres=False):
    """the evaluator's inputs as host arrays for E.EvaluatorReference"""
    s = '_fullres' if fullres else ''
    c = lambda t: t.detach().cpu().numpy()                               # noqa: E731
    ori = c(prediction['instance_orientation'].float())
    if fullres:
        ori = ori.repeat(2, 2).repeat(2, 3)                              # nearest, factor 2
    b = {k: c(batch[k]) for k in ('semantic', 'instance', 'scene', 'orientations', 'orientation_foreground')
         if k in batch}
    p = {'orientation': ori, 'keep': c(prediction['orientations_panoptic_segmentation_deeplab_instance_keep'])}
    for name, key in (('semantic_idx', 'semantic_segmentation_idx'), ('panoptic', 'panoptic_segmentation_deeplab'),
                      ('panoptic_semantic', 'panoptic_segmentation_deeplab_semantic_idx'),
                      ('panoptic_instance', 'panoptic_segmentation_deeplab_instance_idx'),
                      ('grouping', 'instance_segmentation_idx')):
        p[name] = c(prediction[key + s])
    p['scene_idx'] = c(prediction['scene_class_idx'])
    p['instance_grouping'] = np.where(b['instance'] != 0, p['grouping'], 0)
    return p, b


def _reference(args, cfg, div=1000, max_instances=256):
    labels = cfg.semantic_label_list_without_void
    return E.EvaluatorReference(args.tasks, args.enable_panoptic, len(labels) + 1,
                                len(cfg.scene_label_list_without_void) + 1,
                                (False,) + tuple(labels.classes_is_thing), div, max_instances)


def _check_evaluator(ev, ref, what):
    got, want = ev.compute(), ref.compute()
    print(what, got)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9, (what, k, got[k], want[k])
    st = ev.state()
    k = ref.k
    assert np.array_equal(st['semantic_miou'][:-1].view(k, k).numpy(), ref.cm)
    assert np.array_equal(st['panoptic_miou'][:-1].view(k, k).numpy(), ref.cm_pan)
    assert np.array_equal(st['scene'][:-1].view(ref.k_scene, ref.k_scene).numpy(), ref.cm_scene)
    for name, r in (('panoptic_pq', ref.pq_pan), ('instance_pq', ref.pq_inst)):
        assert st[name][:3 * k].view(3, k).tolist() == [r.tp, r.fn, r.fp], name
    for name, r in (('orientation_mae_gt', ref.mae_gt), ('panoptic_mae', ref.mae_pan)):
        assert int(st[name][1]) == r.count and abs(int(st[name][0]) - r.total) <= r.count, name
        assert int(st[name][2]) == 0 and not r.flag


def _nothing_vacuous(ref):
    assert sum(ref.pq_pan.tp) >= 1 and sum(ref.pq_pan.fn) >= 1
    assert sum(ref.pq_inst.tp) + sum(ref.pq_inst.fn) >= 1
    assert ref.mae_gt.count >= 1 and ref.mae_pan.count >= 1
    assert ref.cm_scene[1:, 1:].sum() >= 1 and ref.cm_scene[0].sum() >= 1


@pytest.mark.usefixtures('full_setup')
def test_evaluator_against_the_numpy_composition():
    from emsanet_amd import ValidationEvaluator
    args, cfg, model, batch, prediction = _setup()
    div = model.decoders['panoptic_helper'].postprocessing.max_instances_per_category
    ev = ValidationEvaluator(args, cfg, label_divisor=div)
    ev.update(prediction, batch)
    guard.check()
    ref = _reference(args, cfg, div)
    ref.update(*_host_inputs(prediction, batch))
    _nothing_vacuous(ref)
    _check_evaluator(ev, ref, 'one update')
    assert 'instance_all_with_gt_deeplab_pq' in ev.compute()
    ev.update(prediction, batch)                                         # accumulates
    ref.update(*_host_inputs(prediction, batch))
    _check_evaluator(ev, ref, 'two updates')
    ev.reset()
    assert all(int(s.abs().sum()) == 0 for s in ev.state().values())


@pytest.mark.usefixtures('full_setup')
def test_evaluator_is_consistent_with_the_existing_outputs():
    """the two angular errors from the per-sample dictionaries the post-processing already yields;
    semantic_miou and panoptic_all_deeplab_pq from the existing classes on the same maps"""
    from emsanet_amd import MeanIntersectionOverUnion, PanopticQuality, ValidationEvaluator, panoptic_targets
    args, cfg, model, batch, prediction = _setup()
    div = model.decoders['panoptic_helper'].postprocessing.max_instances_per_category
    ev = ValidationEvaluator(args, cfg, label_divisor=div)
    ev.update(prediction, batch)
    got = ev.compute()
    table = batch['orientations'].cpu().numpy()

    errs = []
    for i, d in enumerate(prediction['orientations_gt_instance_gt_orientation_foreground']):
        errs += [E.angular_error(a, table[i, j]) for j, a in d.items() if not np.isnan(table[i, j])]
    assert len(errs) >= 1
    assert abs(got['orientation_mae_gt_deg'] - math.degrees(sum(errs) / len(errs))) <= 1e-9

    is_thing = (False,) + tuple(cfg.semantic_label_list_without_void.classes_is_thing)
    targets = panoptic_targets(batch['semantic'], batch['instance'], is_thing, div)
    ref = E.PanopticQualityPairsReference(len(is_thing), 0, div, is_thing)
    ref.update(prediction['panoptic_segmentation_deeplab'].cpu().numpy(), targets.cpu().numpy())
    errs = []
    for i, d in enumerate(prediction['orientations_panoptic_segmentation_deeplab_instance']):
        for p, t in ref.pairs[i]:
            if p % div and t % div and p % div in d and not np.isnan(table[i, t % div]):
                errs.append(E.angular_error(d[p % div], table[i, t % div]))
    assert len(errs) >= 1
    assert abs(got['panoptic_mae_deeplab_deg'] - math.degrees(sum(errs) / len(errs))) <= 1e-9

    miou = MeanIntersectionOverUnion(len(is_thing), ignore_first_class=True)
    miou.update(prediction['semantic_segmentation_idx'] + 1, batch['semantic'])
    pq = PanopticQuality(len(is_thing), 0, div, 256 ** 3, is_thing)
    pq.update(prediction['panoptic_segmentation_deeplab'], targets)
    assert got['semantic_miou'] == miou.compute() > 0
    want = pq.compute()
    for g in ('all', 'things', 'stuff'):
        for q in ('pq', 'sq', 'rq'):
            assert got[f'panoptic_{g}_deeplab_{q}'] == want[f'{g}_{q}']
    assert got['panoptic_all_deeplab_pq'] > 0


def _slice(d, sel):
    return {k: v[sel] for k, v in d.items() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == BS}


@pytest.mark.usefixtures('full_setup')
def test_evaluator_batch_equals_single_images_and_repeats():
    from emsanet_amd import ValidationEvaluator
    args, cfg, model, batch, prediction = _setup()
    a, b, c = (ValidationEvaluator(args, cfg) for _ in range(3))
    a.update(prediction, batch)
    for i in range(BS):
        b.update(_slice(prediction, slice(i, i + 1)), _slice(batch, slice(i, i + 1)))
    c.update(prediction, batch)
    sa, sb, sc = a.state(), b.state(), c.state()
    assert set(sa) == set(sb) == set(sc) and len(sa) == 7
    for k in sa:
        assert int(sa[k].abs().sum()) > 0, k
        assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sc[k]), k


@pytest.mark.usefixtures('full_setup')
def test_evaluator_update_captures_into_a_graph():
    """warm-up, capture one update() on static inputs, replay it on two further batches (the samples in
    another order) copied into them: the state is the eager one, compute() the reference's"""
    from emsanet_amd import ValidationEvaluator
    args, cfg, model, batch, prediction = _setup()
    rolled = [(_slice(prediction, torch.arange(BS, device=DEV).roll(r)), _slice(batch, torch.arange(BS, device=DEV).roll(r)))
              for r in (1, 2)]
    eager, ref = ValidationEvaluator(args, cfg), _reference(args, cfg)
    for p, b in rolled:
        eager.update(p, b)
        ref.update(*_host_inputs(p, b))
    static_p = {k: v.clone() for k, v in _slice(prediction, slice(None)).items()}
    static_b = {k: v.clone() for k, v in _slice(batch, slice(None)).items()}
    ev = ValidationEvaluator(args, cfg)
    ev.update(static_p, static_b)                                        # warm-up: buffers, tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            ev.update(static_p, static_b)
    torch.cuda.current_stream().wait_stream(stream)
    ev.reset()
    for p, b in rolled:
        for dst, src in ((static_p, p), (static_b, b)):
            for k in dst:
                dst[k].copy_(src[k])
        graph.replay()
    torch.cuda.synchronize()
    se, sg = eager.state(), ev.state()
    for k in se:
        assert int(se[k].abs().sum()) > 0 and torch.equal(se[k], sg[k]), k
    _check_evaluator(ev, ref, 'graph')
    guard.check()                                    # (every buffer of `ev` was made by the warm-up update)


@pytest.mark.usefixtures('full_setup')
def test_evaluator_reads_fullres_entries_for_larger_label_maps():
    from emsanet_amd import ValidationEvaluator
    args, cfg, model, batch, prediction = _setup()
    up = lambda t: t.repeat_interleave(2, -2).repeat_interleave(2, -1)   # noqa: E731
    big = dict(batch, rgb_fullres=torch.zeros(BS, 3, 2 * H, 2 * W, device=DEV),
               semantic=up(batch['semantic']), instance=up(batch['instance']),
               orientation_foreground=up(batch['orientation_foreground']))
    with torch.no_grad():
        p = model({k: big[k] for k in ('rgb', 'depth', 'rgb_fullres')}, do_postprocessing=True)
    assert p['panoptic_segmentation_deeplab_fullres'].shape == (BS, 2 * H, 2 * W)
    ev, ref = ValidationEvaluator(args, cfg), _reference(args, cfg)
    ev.update(p, big)
    ref.update(*_host_inputs(p, big, fullres=True))
    _check_evaluator(ev, ref, 'fullres')
    assert ref.mae_gt.count >= 1 and sum(ref.pq_pan.tp) >= 1
    small = dict(big, semantic=batch['semantic'][:, :50], instance=batch['instance'][:, :50])
    with pytest.raises(ValueError, match="has the label maps' shape"):
        ValidationEvaluator(args, cfg).update(p, small)


@pytest.mark.usefixtures('full_setup')
def test_evaluator_keys_follow_the_tasks():
    from util import deterministic_state_dict
    from emsanet_amd import ValidationEvaluator, full_args
    from emsanet_amd.model import EMSANet
    _, cfg, _, batch, _ = _setup()
    args = full_args(input_height=H, input_width=W, tasks=('semantic', 'scene'))
    model = EMSANet(args, cfg)
    model.load_state_dict(deterministic_state_dict(model))
    model.to(DEV).eval()
    with torch.no_grad():
        p = model({'rgb': batch['rgb'], 'depth': batch['depth']}, do_postprocessing=True)
    ev = ValidationEvaluator(args, cfg)
    ev.update(p, {'semantic': batch['semantic'], 'scene': batch['scene']})
    got = ev.compute()
    assert sorted(got) == ['scene_acc', 'scene_bacc', 'semantic_miou']
    ref = _reference(args, cfg)
    c = lambda t: t.cpu().numpy()                                        # noqa: E731
    ref.update({'semantic_idx': c(p['semantic_segmentation_idx']), 'scene_idx': c(p['scene_class_idx'])},
               {'semantic': c(batch['semantic']), 'scene': c(batch['scene'])})
    want = ref.compute()
    assert sorted(want) == sorted(got)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9, k
    assert sorted(ev.state()) == ['scene', 'semantic_miou']


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
