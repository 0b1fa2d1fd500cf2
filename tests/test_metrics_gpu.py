"""Device-side validation metrics (emsanet_amd/metrics.py, csrc/metrics.hip) against the brute-force
NumPy reference of tests/test_metrics.py.  Counts are integers and must match exactly; iou_sum is
int64 fixed point (2^-40), each term rounded once: |dev - ref| <= tp * 2^-40 per category (half a
unit per term, with a factor 2 of margin); the nine results within 1e-9, the bar the reference sets
its own metric against panopticapi (/root/reference/emsanet/tests/test_metrics_with_model.py:209-237).

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (all counts are integers
compared exactly): the state vectors, the hash-table workspace and the match tables lie between two
bands of 0xFF -- the confusion matrix is binned by `target * C + pred`, data the kernel reads -- and
the prediction and label maps are placed with `guard.put`."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard   # noqa: E402
import test_metrics as R   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_DTYPES = {torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}


# ---- confusion matrix ---------------------------------------------------------------------------
def _label_maps(c, shape, seed):
    """blocky maps (large equal-label regions, as real segmentations have) + per-pixel noise"""
    rng = np.random.RandomState(seed)
    n, h, w = shape
    coarse = rng.randint(0, c, (n, (h + 7) // 8, (w + 7) // 8))
    target = np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :h, :w]
    pred = np.where(rng.rand(n, h, w) < 0.7, target, rng.randint(0, c, (n, h, w)))
    return pred, target


@pytest.mark.parametrize('ignore_first', [False, True])
@pytest.mark.parametrize('c,shape,dt_pred,dt_target', [
    (5, (2, 37, 53), torch.int64, torch.int64),          # pixel count: no multiple of any width
    (5, (2, 37, 53), torch.int32, torch.uint8),
    (5, (2, 37, 53), torch.uint8, torch.int32),
    (41, (1, 480, 640), torch.int64, torch.uint8),       # LDS bins at the real class count
    (200, (1, 48, 64), torch.int64, torch.int32),        # global-atomics fallback
    (200, (1, 48, 64), torch.uint8, torch.uint8),
])
def test_confusion_matrix_and_miou(c, shape, dt_pred, dt_target, ignore_first):
    from emsanet_amd import MeanIntersectionOverUnion
    pred, target = _label_maps(c, shape, seed=c)
    m = MeanIntersectionOverUnion(c, ignore_first_class=ignore_first)
    m.update(_dev(pred.astype(NP_DTYPES[dt_pred])), _dev(target.astype(NP_DTYPES[dt_target])))
    guard.check()
    cm, bad = R.confusion_reference(pred, target, c)
    assert bad == 0 and cm.sum() == pred.size
    got = m.confusion_matrix
    assert got.is_cuda and got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), cm)
    assert abs(m.compute() - R.miou_reference(cm, ignore_first)) <= 1e-12
    # a second update accumulates, reset clears
    m.update(_dev(pred.astype(NP_DTYPES[dt_pred])), _dev(target.astype(NP_DTYPES[dt_target])))
    assert np.array_equal(m.confusion_matrix.cpu().numpy(), 2 * cm)
    m.reset()
    assert int(m.confusion_matrix.abs().sum()) == 0


@pytest.mark.parametrize('c,shape', [(5, (2, 37, 53)), (200, (1, 48, 64))])
@pytest.mark.parametrize('side', ['pred', 'target'])
def test_confusion_matrix_label_out_of_range(c, shape, side):
    """one label == C: compute() raises and names n_invalid; the matrix is the reference's without
    that pixel (nothing was written out of bounds: the matrix is the tail of the state buffer, with
    n_invalid right behind it)"""
    from emsanet_amd import MeanIntersectionOverUnion
    pred, target = _label_maps(c, shape, seed=7)
    (pred if side == 'pred' else target)[-1, -1, -1] = c
    m = MeanIntersectionOverUnion(c)
    m.update(_dev(pred), _dev(target))
    guard.check()
    cm, bad = R.confusion_reference(pred, target, c)
    assert bad == 1 and cm.sum() == pred.size - 1
    assert np.array_equal(m.confusion_matrix.cpu().numpy(), cm)
    with pytest.raises(ValueError, match='n_invalid'):
        m.compute()
    m.reset()
    m.update(_dev(np.minimum(pred, c - 1)), _dev(np.minimum(target, c - 1)))
    assert m.compute() > 0


@pytest.mark.parametrize('c,shape,dtype', [(5, (2, 37, 53), torch.uint8), (5, (1, 1, 1), torch.int64),
                                           (200, (2, 15, 13), torch.uint8), (200, (1, 48, 64), torch.int32)])
def test_confusion_matrix_last_bin_from_the_last_pixel(c, shape, dtype):
    """the last pixel of the last image carries (C - 1, C - 1): the last input element goes into the
    last bin of the matrix, at the small class count (LDS bins) and at 200 (global atomics; 199 as
    uint8 is above 127).  n_invalid, right behind the matrix, stays 0"""
    from emsanet_amd import MeanIntersectionOverUnion
    pred, target = _label_maps(c, shape, seed=c + 1)
    pred[...] = np.minimum(pred, c - 2)              # so that the last bin is that pixel's alone
    pred[-1, -1, -1] = target[-1, -1, -1] = c - 1
    m = MeanIntersectionOverUnion(c)
    m.update(_dev(pred.astype(NP_DTYPES[dtype])), _dev(target.astype(NP_DTYPES[dtype])))
    guard.check()
    cm, bad = R.confusion_reference(pred, target, c)
    assert bad == 0 and cm[c - 1, c - 1] == 1 and cm.sum() == pred.size
    assert np.array_equal(m.confusion_matrix.cpu().numpy(), cm)
    assert int(m._state[-1]) == 0
    assert abs(m.compute() - R.miou_reference(cm, False)) <= 1e-12


# ---- panoptic quality ---------------------------------------------------------------------------
def _pq(div, **kw):
    from emsanet_amd import PanopticQuality
    return PanopticQuality(num_categories=R.SCENE_CATEGORIES, ignored_label=0,
                           max_instances_per_category=div, offset=256 ** 3, is_thing=R.SCENE_IS_THING,
                           **kw)


def _ref(div):
    return R.PanopticQualityReference(R.SCENE_CATEGORIES, 0, div, R.SCENE_IS_THING)


_SCENE_CACHE = {}


def _scene(name):
    """(pred, target, divisor, reference after one update) -- computed once, never modified"""
    if name not in _SCENE_CACHE:
        if name == 'half_iou':
            div, (pred, target) = 1000, R.half_iou_image(1000)
            pred, target = pred[None], target[None]
        elif name == 'void_overlap':
            div, (pred, target) = 1 << 16, R.void_overlap_image(1 << 16)
            pred, target = pred[None], target[None]
        else:
            _, n, h, w, k, div, seed = next(s for s in R.SCENES if s[0] == name)
            pred, target = R.rectangle_batch(n, h, w, k, div, seed)
        ref = _ref(div)
        ref.update(pred, target)
        _SCENE_CACHE[name] = (pred, target, div, ref)
    return _SCENE_CACHE[name]


def _dev(a):
    return guard.put(torch.from_numpy(a).to(DEV))    # flush between two bands of 0xFF


def _assert_matches(metric, ref, what=''):
    c = metric.counts()
    print(what, 'tp', c['tp'], 'fn', c['fn'], 'fp', c['fp'])
    assert c['tp'] == ref.tp and c['fn'] == ref.fn and c['fp'] == ref.fp, (what, c, ref.tp, ref.fn, ref.fp)
    for cat in range(ref.k):
        err = abs(Fraction(c['iou_sum'][cat], 1 << 40) - ref.iou_sum[cat])
        print(what, 'category', cat, 'iou_sum error', float(err), 'bound', ref.tp[cat] * 2.0 ** -40)
        assert err <= Fraction(ref.tp[cat], 1 << 40), (what, cat, float(err))
    got, want = metric.compute(), ref.compute()
    assert tuple(got) == R.PQ_KEYS
    for k in R.PQ_KEYS:
        assert abs(got[k] - want[k]) <= 1e-9, (what, k, got[k], want[k])


@pytest.mark.parametrize('name', [s[0] for s in R.SCENES])
def test_panoptic_quality_random_scenes(name):
    pred, target, div, ref = _scene(name)
    for i in range(pred.shape[0]):                     # no passing on empty ground
        one = _ref(div)
        one.update(pred[i], target[i])
        assert min(sum(one.tp), sum(one.fp), sum(one.fn), one.void_skipped) >= 1
    m = _pq(div)
    m.update(_dev(pred), _dev(target))
    guard.check()
    _assert_matches(m, ref, name)


def test_panoptic_quality_half_iou_is_no_match():
    pred, target, div, ref = _scene('half_iou')
    m = _pq(div)
    m.update(_dev(pred), _dev(target))
    c = m.counts()
    assert c['tp'] == [0, 0, 0, 0, 0, 1, 0] and c['fn'] == [0, 1, 0, 0, 0, 0, 0] == c['fp']
    assert c['iou_sum'][5] == 1 << 40
    _assert_matches(m, ref, 'half_iou')


def test_panoptic_quality_prediction_in_void_is_no_fp():
    pred, target, div, ref = _scene('void_overlap')
    m = _pq(div)
    m.update(_dev(pred[0]), _dev(target[0]))           # (H, W) maps are one image
    c = m.counts()
    assert c['tp'] == [0, 0, 0, 0, 0, 1, 0] and c['fn'] == [0] * 7 == c['fp']
    assert c['iou_sum'][5] == round(Fraction(4, 5) * (1 << 40))
    _assert_matches(m, ref, 'void_overlap')


def test_panoptic_quality_batch_equals_single_images_and_repeats():
    """state after one update of 4 images == after four updates of one image, bit for bit; a repeat
    of the same update gives the same bits"""
    pred, target, div, _ = _scene('4x48x64')
    p, t = _dev(pred), _dev(target)
    a, b, c = _pq(div), _pq(div), _pq(div)
    a.update(p, t)
    for i in range(4):
        b.update(p[i:i + 1], t[i:i + 1])
    c.update(p, t)
    assert int(a._state[:-1].abs().sum()) > 0
    assert torch.equal(a._state, b._state) and torch.equal(a._state, c._state)


def test_updates_capture_into_a_graph():
    """after a warm-up call both update()s are captured on one stream; three replays leave exactly
    three times the counts of one call"""
    from emsanet_amd import MeanIntersectionOverUnion
    pred, target, div, ref = _scene('4x48x64')
    p, t = _dev(pred), _dev(target)
    sp, st = (p // div).to(torch.uint8), (t // div).to(torch.int32)
    pq, miou = _pq(div), MeanIntersectionOverUnion(R.SCENE_CATEGORIES, ignore_first_class=True)
    pq.update(p, t)
    miou.update(sp, st)
    torch.cuda.synchronize()
    once_pq, once_cm = pq._state.clone(), miou._state.clone()
    pq.reset()
    miou.reset()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            pq.update(p, t)
            miou.update(sp, st)
    torch.cuda.current_stream().wait_stream(stream)
    pq.reset()                                          # (capturing does not run the kernels)
    miou.reset()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(once_pq[:-1].abs().sum()) > 0 and int(once_cm.sum()) == pred.size
    assert torch.equal(pq._state, 3 * once_pq)          # (the flag word is 0)
    assert torch.equal(miou._state, 3 * once_cm)
    guard.check()                                       # (state and workspace were made by the warm-up calls)


def test_panoptic_quality_segment_table_overflow():
    """20 segments against max_segments=8: compute() raises and names the overflow; after reset() the
    same object counts a valid image correctly"""
    div = 1000
    grid = (np.arange(20).reshape(4, 5) + 1).repeat(6, 0).repeat(7, 1)          # 24 x 35, 20 segments
    crowded = (4 * div + grid).astype(np.int64)[None]
    m = _pq(div, max_segments=8)
    m.update(_dev(crowded), _dev(crowded))
    guard.check()                                       # the twelve segments too many were stored nowhere
    with pytest.raises(ValueError, match='overflow'):
        m.compute()
    m.reset()
    pred, target, _, ref = _scene('half_iou')
    m.update(_dev(pred), _dev(target))
    _assert_matches(m, ref, 'after overflow')
    # and a table that is exactly full is no overflow
    few = (4 * div + (grid - 1) % 8).astype(np.int64)[None]
    m.reset()
    m.update(_dev(few), _dev(few))
    guard.check()
    assert m.counts()['tp'][4] == 8 and m.compute()['all_pq'] == 1.0


def test_panoptic_quality_invalid_ids_are_reported():
    div = 1000
    pred, target, _, _ = _scene('half_iou')
    for bad in (-1, R.SCENE_CATEGORIES * div):
        p = pred.copy()
        p[0, 0, 0] = bad
        m = _pq(div)
        m.update(_dev(p), _dev(target))
        with pytest.raises(ValueError, match='invalid panoptic id'):
            m.compute()


def test_panoptic_targets():
    from emsanet_amd import panoptic_targets
    rng = np.random.RandomState(4)
    sem = rng.randint(0, R.SCENE_CATEGORIES, (2, 37, 53))
    inst = rng.randint(0, 9, (2, 37, 53))
    want = np.where(np.array(R.SCENE_IS_THING)[sem], sem * 1000 + inst, sem * 1000).astype(np.int64)
    assert (want[sem == 0] == 0).all()
    for ds, di in ((np.int64, np.int64), (np.uint8, np.int32), (np.int32, np.uint8)):
        got = panoptic_targets(_dev(sem.astype(ds)), _dev(inst.astype(di)), R.SCENE_IS_THING, 1000)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


# ---- end to end -----------------------------------------------------------------------------------
def test_validation_loop_end_to_end():
    """eval forward + post-processing of a small random-weight model -> panoptic_targets on synthetic
    labels -> both metrics; against the NumPy reference on the same maps copied to the host"""
    from util import deterministic_state_dict
    from emsanet_amd import (MeanIntersectionOverUnion, PanopticQuality, full_args, nyuv2_config,
                             panoptic_targets)
    from emsanet_amd.model import EMSANet
    h, w, bs = 96, 128, 4
    cfg = nyuv2_config()
    labels = cfg.semantic_label_list_without_void
    labels.classes_is_thing = tuple(bool(i % 3) for i in range(len(labels)))
    model = EMSANet(full_args(input_height=h, input_width=w, enable_panoptic=True), cfg)
    model.load_state_dict(deterministic_state_dict(model))
    model.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    batch = {'rgb': torch.randn(bs, 3, h, w, generator=g).to(DEV),
             'depth': torch.randn(bs, 1, h, w, generator=g).to(DEV)}
    with torch.no_grad():
        prediction = model(batch, do_postprocessing=True)
    n_classes = len(labels) + 1                                           # with void
    is_thing = (False,) + labels.classes_is_thing
    div = model.decoders['panoptic_helper'].postprocessing.max_instances_per_category
    # synthetic labels: blocks of one class, 0 = void; instance ids in blocks, 0 = no instance
    sem = torch.randint(0, n_classes, (bs, h // 16, w // 16), generator=g).repeat_interleave(16, 1) \
        .repeat_interleave(16, 2).to(torch.uint8)
    inst = torch.randint(0, 5, (bs, h // 32, w // 32), generator=g).repeat_interleave(32, 1) \
        .repeat_interleave(32, 2).to(torch.int32)
    # make sure something matches: the labels of image 0 are the model's own prediction
    sem[0] = prediction['panoptic_segmentation_deeplab_semantic_idx'][0].cpu().to(torch.uint8)
    inst[0] = prediction['panoptic_segmentation_deeplab_instance_idx'][0].cpu()
    targets = panoptic_targets(sem.to(DEV), inst.to(DEV), is_thing, div)

    miou = MeanIntersectionOverUnion(n_classes, ignore_first_class=True)
    pq = PanopticQuality(num_categories=n_classes, ignored_label=0, max_instances_per_category=div,
                         offset=256 ** 3, is_thing=is_thing)
    sem_pred = prediction['semantic_segmentation_idx'] + 1                # into the label list with void
    miou.update(sem_pred, sem.to(DEV))
    pq.update(prediction['panoptic_segmentation_deeplab'], targets)

    cm, bad = R.confusion_reference(sem_pred.cpu().numpy(), sem.numpy(), n_classes)
    assert bad == 0
    assert np.array_equal(miou.confusion_matrix.cpu().numpy(), cm)
    assert abs(miou.compute() - R.miou_reference(cm, True)) <= 1e-12
    ref = R.PanopticQualityReference(n_classes, 0, div, is_thing)
    ref.update(prediction['panoptic_segmentation_deeplab'].cpu().numpy(), targets.cpu().numpy())
    assert sum(ref.tp) >= 1 and sum(ref.fn) >= 1
    _assert_matches(pq, ref, 'end to end')
    assert pq.compute()['all_pq'] > 0 and miou.compute() > 0


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
