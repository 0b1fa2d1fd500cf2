"""CPU: the brute-force NumPy reference of the validation metrics (mIoU, panoptic quality) that
tests/test_metrics_gpu.py holds the device kernels to, checked here against hand-computed images.

The reference is written from the rules, independently of csrc/metrics.hip: `np.unique` over the
(target id, predicted id) pairs of an image, then Python loops over the segments.
  * a pair of equal category (not the ignored one) matches iff IoU > 1/2 (strictly), with
    union = area_t + area_p - inter - (overlap of the prediction with ignored target pixels)
  * match: tp, IoU added to iou_sum; unmatched target: fn; unmatched prediction: fp, unless more
    than half of it lies on ignored target pixels
(the DeepLab2 / panopticapi rules /root/reference/emsanet/tests/test_metrics_with_model.py:37-237
holds the reference's metric to).  IoU sums are kept as exact fractions."""
from fractions import Fraction

import numpy as np

PQ_KEYS = tuple(f'{g}_{k}' for g in ('all', 'things', 'stuff') for k in ('pq', 'sq', 'rq'))


# ---- confusion matrix / mIoU ------------------------------------------------------------------
def confusion_reference(pred, target, n_classes):
    """-> (cm[target][pred] int64, number of pixels with a label outside [0, n_classes))"""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    ok = (p >= 0) & (p < n_classes) & (t >= 0) & (t < n_classes)
    cm = np.bincount(t[ok] * n_classes + p[ok], minlength=n_classes ** 2)
    return cm.reshape(n_classes, n_classes).astype(np.int64), int((~ok).sum())


def miou_reference(cm, ignore_first_class):
    cm = cm[1:, 1:] if ignore_first_class else cm
    ious = []
    for c in range(cm.shape[0]):
        union = int(cm[c].sum() + cm[:, c].sum() - cm[c, c])
        if union > 0:
            ious.append(int(cm[c, c]) / union)
    return sum(ious) / len(ious) if ious else 0.0


# ---- panoptic quality -------------------------------------------------------------------------
class PanopticQualityReference:
    def __init__(self, num_categories, ignored_label, max_instances_per_category, is_thing):
        self.k, self.ignored, self.div = num_categories, ignored_label, max_instances_per_category
        self.is_thing = tuple(is_thing)
        self.tp = [0] * self.k
        self.fn = [0] * self.k
        self.fp = [0] * self.k
        self.iou_sum = [Fraction(0)] * self.k
        self.void_skipped = 0                   # unmatched predictions that were no fp

    def update(self, preds, targets):
        preds, targets = np.asarray(preds), np.asarray(targets)
        if preds.ndim == 2:
            preds, targets = preds[None], targets[None]
        for p, t in zip(preds, targets):
            self._image(p.reshape(-1).astype(np.int64), t.reshape(-1).astype(np.int64))

    def _image(self, p, t):
        pairs, counts = np.unique(np.stack([t, p], 1), axis=0, return_counts=True)
        inter = {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, counts)}
        area_t, area_p, void_p = {}, {}, {}
        for (a, b), c in inter.items():
            area_t[a] = area_t.get(a, 0) + c
            area_p[b] = area_p.get(b, 0) + c
            if a // self.div == self.ignored:
                void_p[b] = void_p.get(b, 0) + c
        hit_t, hit_p = set(), set()
        for (a, b), c in inter.items():
            cat = a // self.div
            if cat != b // self.div or cat == self.ignored:
                continue
            union = area_t[a] + area_p[b] - c - void_p.get(b, 0)
            if 2 * c > union:
                self.tp[cat] += 1
                self.iou_sum[cat] += Fraction(c, union)
                hit_t.add(a)
                hit_p.add(b)
        for a in area_t:
            if a // self.div != self.ignored and a not in hit_t:
                self.fn[a // self.div] += 1
        for b in area_p:
            if b // self.div == self.ignored or b in hit_p:
                continue
            if 2 * void_p.get(b, 0) > area_p[b]:
                self.void_skipped += 1
            else:
                self.fp[b // self.div] += 1

    def compute(self):
        rows = {'all': [], 'things': [], 'stuff': []}
        for c in range(self.k):
            tp, fn, fp = self.tp[c], self.fn[c], self.fp[c]
            if c == self.ignored or tp + fn + fp == 0:
                continue
            sq = float(self.iou_sum[c] / tp) if tp else 0.0
            rq = tp / (tp + 0.5 * fn + 0.5 * fp)
            for g in ('all', 'things' if self.is_thing[c] else 'stuff'):
                rows[g].append((sq * rq, sq, rq))
        return {f'{g}_{k}': (sum(r[j] for r in v) / len(v) if v else 0.0)
                for g, v in rows.items() for j, k in enumerate(('pq', 'sq', 'rq'))}


# ---- scenes -----------------------------------------------------------------------------------
# 6 categories + void: 0 = void (ignored), 1-3 things, 4-6 stuff
SCENE_CATEGORIES = 7
SCENE_IS_THING = (False, True, True, True, False, False, False)


def _paint(canvas, rect, value):
    y0, x0, y1, x1 = rect
    h, w = canvas.shape
    canvas[max(y0, 0):min(y1, h), max(x0, 0):min(x1, w)] = value


def rectangle_scene(h, w, n_things, divisor, seed):
    """one (pred, target) pair of int64 panoptic id maps.  Target: three stuff bands, `n_things`
    thing rectangles on top, one void rectangle.  Prediction: the same segments shifted by 1-3 px
    each, with two instances merged, one instance relabelled to another class, one segment turned to
    void and one spurious segment placed over the target's void rectangle."""
    rng = np.random.RandomState(seed)
    target = np.zeros((h, w), np.int64)
    pred = np.zeros((h, w), np.int64)

    def shift(r):
        dy, dx = (int(s) * int(m) for s, m in zip(rng.choice([-1, 1], 2), rng.randint(1, 4, 2)))
        return r[0] + dy, r[1] + dx, r[2] + dy, r[3] + dx

    bands = [(0, (w * i) // 3, h, (w * (i + 1)) // 3) for i in range(3)]
    for cat, r in zip((4, 5, 6), bands):
        _paint(target, r, cat * divisor)
        _paint(pred, shift(r), cat * divisor)
    lo, hi = max(6, min(h, w) // 8), max(10, min(h, w) // 4)
    things = []
    for i in range(n_things):
        rh, rw = rng.randint(lo, hi + 1, 2)
        y0, x0 = rng.randint(0, h - rh), rng.randint(0, w - rw)
        things.append(((y0, x0, y0 + rh, x0 + rw), 1 + i % 3, 1 + i // 3))
    for i, (r, cat, inst) in enumerate(things):
        _paint(target, r, cat * divisor + inst)
        if i == 0:                                   # turned to void
            label = 0
        elif i == 6:                                 # merged into the instance before it in its class
            label = cat * divisor + things[3][2]
        elif i == 4:                                 # relabelled to another class
            label = (1 + (cat % 3)) * divisor + 50
        else:
            label = cat * divisor + inst
        _paint(pred, shift(r), label)
    vh, vw = max(8, h // 5), max(8, w // 5)
    vy, vx = rng.randint(0, h - vh), rng.randint(0, w - vw)
    _paint(target, (vy, vx, vy + vh, vx + vw), 0)
    _paint(pred, (vy + 1, vx + 1, vy + vh - 1, vx + vw - 1), 2 * divisor + 60)   # spurious, over void
    return pred, target


def rectangle_batch(n, h, w, n_things, divisor, seed):
    scenes = [rectangle_scene(h, w, n_things, divisor, seed + 17 * i) for i in range(n)]
    return np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])


# (name, images, h, w, thing rectangles, max_instances_per_category, seed)
SCENES = (('4x48x64', 4, 48, 64, 9, 1 << 16, 1),
          ('2x37x53', 2, 37, 53, 8, 1000, 2),
          ('480x640', 1, 480, 640, 56, 1 << 16, 3))


def half_iou_image(divisor):
    """target: thing 1/1 of area 4, stuff 5 on the rest; prediction: 2 px of the thing (inside it), void
    on its other 2, the stuff alike.  inter 2, union 4 + 2 - 2 = 4: IoU exactly 1/2 is NO match."""
    a, s = divisor + 1, 5 * divisor
    target = np.array([[a, a, s, s], [a, a, s, s]], np.int64)
    pred = np.array([[a, 0, s, s], [a, 0, s, s]], np.int64)
    return pred, target


def void_overlap_image(divisor):
    """prediction thing 1/1 of area 4 with 3 px on void and 1 px on stuff 5: unmatched, but no fp
    (2 * 3 > 4).  Stuff 5: target area 5, prediction 4 inside it: IoU 4/5."""
    a, s = divisor + 1, 5 * divisor
    target = np.array([[0, 0, s, s], [0, s, s, s]], np.int64)
    pred = np.array([[a, a, s, s], [a, a, s, s]], np.int64)
    return pred, target


def _ref(divisor=1000):
    return PanopticQualityReference(SCENE_CATEGORIES, 0, divisor, SCENE_IS_THING)


def test_reference_half_iou_is_no_match():
    r = _ref()
    r.update(*half_iou_image(1000))
    assert r.tp == [0, 0, 0, 0, 0, 1, 0]
    assert r.fn == [0, 1, 0, 0, 0, 0, 0]
    assert r.fp == [0, 1, 0, 0, 0, 0, 0]
    assert r.iou_sum[5] == 1 and sum(r.iou_sum) == 1 and r.void_skipped == 0
    c = r.compute()
    # things: category 1 with pq = 0; stuff: category 5 with pq = 1
    assert c['things_pq'] == 0.0 and c['things_rq'] == 0.0 and c['stuff_pq'] == 1.0
    assert c['all_pq'] == 0.5 and c['all_sq'] == 0.5 and c['all_rq'] == 0.5


def test_reference_prediction_in_void_is_no_fp():
    r = _ref()
    r.update(*void_overlap_image(1000))
    assert r.tp == [0, 0, 0, 0, 0, 1, 0]
    assert r.fn == [0] * 7 and r.fp == [0] * 7
    assert r.iou_sum[5] == Fraction(4, 5) and r.void_skipped == 1
    c = r.compute()
    assert abs(c['all_pq'] - 0.8) < 1e-15 and c['all_rq'] == 1.0 and c['things_pq'] == 0.0
    # one pixel fewer in void: 2 * 2 > 4 fails, the prediction counts as fp
    pred, target = void_overlap_image(1000)
    target[0, 1] = 5000
    r = _ref()
    r.update(pred, target)
    assert r.fp == [0, 1, 0, 0, 0, 0, 0] and r.void_skipped == 0


def test_scenes_exercise_every_rule():
    """every random scene of the GPU test has a tp, a fp, a fn and a void-skipped prediction"""
    for name, n, h, w, k, div, seed in SCENES:
        pred, target = rectangle_batch(n, h, w, k, div, seed)
        for i in range(n):
            r = _ref(div)
            r.update(pred[i], target[i])
            assert min(sum(r.tp), sum(r.fp), sum(r.fn), r.void_skipped) >= 1, (name, i, r.tp, r.fp, r.fn)
            assert len(np.unique(target[i])) <= 256 and len(np.unique(pred[i])) <= 256
    assert len(np.unique(rectangle_batch(1, 480, 640, 56, 1 << 16, 3)[1])) >= 50


def test_confusion_reference_by_hand():
    pred = np.array([0, 1, 1, 2, 3, 2])
    target = np.array([0, 1, 2, 2, 2, 7])
    cm, bad = confusion_reference(pred, target, 3)
    assert bad == 2 and cm.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 1]]
    # IoU: class 0: 1/1, class 1: 1/2, class 2: 1/2
    assert abs(miou_reference(cm, False) - 2 / 3) < 1e-15
    assert abs(miou_reference(cm, True) - 0.5) < 1e-15


def test_metrics_refuse_cpu_tensors_by_name():
    import pytest
    import torch
    from emsanet_amd import MeanIntersectionOverUnion, PanopticQuality, panoptic_targets
    x = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        MeanIntersectionOverUnion(5).update(x, x)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        PanopticQuality(7, 0, 1000, 256 ** 3, SCENE_IS_THING).update(x, x)
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        panoptic_targets(x, x, SCENE_IS_THING, 1000)
    with pytest.raises(ValueError, match='max_segments'):
        PanopticQuality(7, 0, 1000, 256 ** 3, SCENE_IS_THING, max_segments=4096)


def test_metric_entries_validate_on_the_host():
    """negative codes before any launch (no GPU needed)"""
    from emsanet_amd import _lib
    L = _lib.lib()
    assert L.emsa_confusion_matrix(None, 0, None, 0, 10, 5, None, None, None) == -2
    assert L.emsa_confusion_matrix(8, 0, 8, 0, 0, 5, 8, 8, None) == -1
    assert L.emsa_confusion_matrix(8, 7, 8, 0, 10, 5, 8, 8, None) == -2
    assert L.emsa_panoptic_pairs(None, None, 1, 10, 256, None, None, None) == -2
    assert L.emsa_panoptic_pairs(8, 8, 1, 10, 2048, 8, 8, None) == -1
    assert L.emsa_panoptic_match(8, 1, 0, 7, 0, 1000, 8, 8, 8, 8, 8, None) == -1
    assert L.emsa_panoptic_targets(8, 0, 8, 0, 8, 7, 0, 10, 8, None) == -1
    assert L.emsa_panoptic_workspace_bytes(2, 256) == 2 * (2 * 256 * 8 + 256 * 256 * 4)
    assert L.emsa_panoptic_workspace_bytes(1, 1025) == 0
