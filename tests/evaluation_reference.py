"""Brute-force NumPy restatement of the validation metrics beyond mIoU / PQ and of the evaluator's
composition (emsanet_amd/evaluation.py), written from the rules and independently of the kernels:

  * scene acc / bacc from the confusion matrix cm[target][pred]: acc = trace / total, bacc = mean of
    cm[c][c] / row_c over the classes present in the targets; row and column 0 (void) dropped first
  * per-instance orientation sums: round-half-even(v * 2^24) per pixel and channel (|v| clamped to
    2^14, NaN -> 0), int64 -- what `emsa_instance_orientation` documents
  * angular error: angle = float64 arctan2(sum sin, sum cos) mod 2 pi; d = |angle - gt| mod 2 pi;
    err = min(d, 2 pi - d); sum of round-half-even(err * 2^40) as Python int, count
  * PQ matching that also returns the matched (predicted id, target id) pairs per image
  * the evaluator: which map goes into which metric

tests/test_evaluation.py pins these by hand-computed cases; tests/test_evaluation_gpu.py holds the
device to them."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_metrics as R   # noqa: E402

TWO_PI = 2.0 * math.pi
ANGLE_ONE = 1 << 40
VEC_ONE = 1 << 24


# ---- scene ----------------------------------------------------------------------------------------
def scene_reference(cm, ignore_first_class=True):
    """-> (acc, bacc); (0.0, 0.0) without a counted sample"""
    cm = np.asarray(cm)
    cm = cm[1:, 1:] if ignore_first_class else cm
    total = int(cm.sum())
    if total == 0:
        return 0.0, 0.0
    recalls = [int(cm[c, c]) / int(cm[c].sum()) for c in range(cm.shape[0]) if cm[c].sum() > 0]
    return int(np.trace(cm)) / total, sum(recalls) / len(recalls)


# ---- orientation ----------------------------------------------------------------------------------
def orientation_sums_reference(orientation, ids, slots, mask=None):
    """orientation (N, 2, H, W) float (sin, cos), ids (N, H, W) -> vec int64 (N, slots, 2), count int64
    (N, slots) over the pixels with 0 < id < slots (and mask != 0)"""
    o = np.asarray(orientation, np.float32).astype(np.float64)
    o = np.where(np.isnan(o), 0.0, np.clip(o, -16384.0, 16384.0))
    fixed = np.rint(o * VEC_ONE).astype(np.int64)
    ids = np.asarray(ids).astype(np.int64)
    n = ids.shape[0]
    vec = np.zeros((n, slots, 2), np.int64)
    cnt = np.zeros((n, slots), np.int64)
    ok = (ids > 0) & (ids < slots)
    if mask is not None:
        ok &= np.asarray(mask).reshape(ids.shape) != 0
    for i in range(n):
        sel = ids[i][ok[i]]
        cnt[i] = np.bincount(sel, minlength=slots)
        for ch in range(2):
            np.add.at(vec[i, :, ch], sel, fixed[i, ch][ok[i]])
    return vec, cnt


def angle_of(vec):
    return float(np.arctan2(np.float64(vec[0]), np.float64(vec[1]))) % TWO_PI


def angular_error(angle, gt):
    d = abs(angle - float(gt)) % TWO_PI
    return min(d, TWO_PI - d)


class AngularErrorReference:
    """mirror of metrics.MeanAbsoluteAngularError: `total` in units of 2^-40 rad (Python int), `count`,
    `flag` (an id outside the tables on an otherwise compared instance)"""

    def __init__(self):
        self.total, self.count, self.flag = 0, 0, False

    def _compare(self, vec, count, keep, gt, i, ps, gs):
        if ps >= vec.shape[1]:
            self.flag = True
            return
        if count[i, ps] <= 0 or (keep is not None and not keep[i, ps]):
            return
        if gs >= gt.shape[1]:
            self.flag = True
            return
        g = np.float32(gt[i, gs])
        if np.isnan(g):
            return
        self.total += int(np.rint(angular_error(angle_of(vec[i, ps]), g) * ANGLE_ONE))
        self.count += 1

    def update(self, vec, count, gt, keep=None):
        for i in range(vec.shape[0]):
            for j in range(1, vec.shape[1]):
                self._compare(vec, count, keep, gt, i, j, j)

    def update_matched(self, vec, count, gt, pairs, divisor, keep=None):
        """pairs: per image a list of (predicted id, target id)"""
        for i, image in enumerate(pairs):
            for p, t in image:
                ps, gs = int(p) % divisor, int(t) % divisor
                if ps > 0 and gs > 0:
                    self._compare(vec, count, keep, gt, i, ps, gs)

    def compute(self):
        if self.count == 0:
            return {'mae_rad': float('nan'), 'mae_deg': float('nan')}
        rad = self.total / ANGLE_ONE / self.count
        return {'mae_rad': rad, 'mae_deg': math.degrees(rad)}


# ---- PQ with the match list -----------------------------------------------------------------------
class PanopticQualityPairsReference(R.PanopticQualityReference):
    """`PanopticQualityReference` that also keeps, per image of the LAST update, the list of matched
    (predicted id, target id) pairs -- found by a second, separate pass over the (target, prediction)
    pairs with the same rule"""

    def update(self, preds, targets):
        preds, targets = np.asarray(preds), np.asarray(targets)
        if preds.ndim == 2:
            preds, targets = preds[None], targets[None]
        super().update(preds, targets)
        self.pairs = [self._matched(p.reshape(-1).astype(np.int64), t.reshape(-1).astype(np.int64))
                      for p, t in zip(preds, targets)]

    def _matched(self, p, t):
        out = []
        for a in np.unique(t):
            if a // self.div == self.ignored:
                continue
            for b in np.unique(p[t == a]):
                if b // self.div != a // self.div:
                    continue
                inter = int(((t == a) & (p == b)).sum())
                void = int(((p == b) & (t // self.div == self.ignored)).sum())
                union = int((t == a).sum()) + int((p == b).sum()) - inter - void
                if 2 * inter > union:
                    out.append((int(b), int(a)))
        return out


# ---- the evaluator --------------------------------------------------------------------------------
def pan_ids(semantic, instance, is_thing, divisor):
    sem = np.asarray(semantic).astype(np.int64)
    inst = np.asarray(instance).astype(np.int64)
    thing = np.asarray(is_thing, bool)[np.clip(sem, 0, len(is_thing) - 1)]
    ok = (sem > 0) & (sem < len(is_thing))
    return np.where(ok, sem * divisor + np.where(thing, inst, 0), 0).astype(np.int64)


class EvaluatorReference:
    """the composition of emsanet_amd.evaluation.ValidationEvaluator on host arrays.  `update` takes the
    maps already selected at the label maps' resolution: dict prediction with
      semantic_idx, scene_idx, orientation (N, 2, H, W), instance_grouping (the map of the
      `instance_all_with_gt` key, already restricted to the ground-truth foreground),
      panoptic, panoptic_semantic, panoptic_instance, keep (N, slots)
    and dict batch with semantic, instance, scene, orientations, orientation_foreground (or None);
    entries of tasks that are off may be missing."""

    def __init__(self, tasks, enable_panoptic, n_classes, n_scene_classes, is_thing, divisor,
                 max_instances):
        self.tasks, self.panoptic = tuple(tasks), bool(enable_panoptic)
        self.k, self.k_scene, self.is_thing, self.div = n_classes, n_scene_classes, tuple(is_thing), divisor
        self.max_instances = max_instances
        self.cm = np.zeros((n_classes, n_classes), np.int64)
        self.cm_pan = np.zeros((n_classes, n_classes), np.int64)
        self.cm_scene = np.zeros((n_scene_classes, n_scene_classes), np.int64)
        self.mae_gt, self.mae_pan = AngularErrorReference(), AngularErrorReference()
        self.pq_inst = R.PanopticQualityReference(n_classes, 0, divisor, self.is_thing)
        self.pq_pan = PanopticQualityPairsReference(n_classes, 0, divisor, self.is_thing)
        self.bad = 0
        self.instance_seen = False

    def _confusion(self, cm, pred, target):
        add, bad = R.confusion_reference(pred, target, cm.shape[0])
        cm += add
        self.bad += bad

    def update(self, prediction, batch):
        t = self.tasks
        if 'semantic' in t:
            self._confusion(self.cm, prediction['semantic_idx'] + 1, batch['semantic'])
        if 'scene' in t:
            self._confusion(self.cm_scene, prediction['scene_idx'] + 1, batch['scene'])
        if 'orientation' in t:
            ids = np.minimum(np.asarray(batch['instance']).astype(np.int64), self.max_instances)
            vec, cnt = orientation_sums_reference(prediction['orientation'], ids, self.max_instances + 1,
                                                  batch.get('orientation_foreground'))
            self.mae_gt.update(vec, cnt, batch['orientations'])
        targets = None
        if 'instance' in t or self.panoptic:
            targets = pan_ids(batch['semantic'], batch['instance'], self.is_thing, self.div)
        if 'instance' in t and prediction.get('instance_grouping') is not None:
            self.pq_inst.update(pan_ids(batch['semantic'], prediction['instance_grouping'], self.is_thing,
                                        self.div), targets)
            self.instance_seen = True
        if self.panoptic:
            self.pq_pan.update(prediction['panoptic'], targets)
            self._confusion(self.cm_pan, prediction['panoptic_semantic'], batch['semantic'])
            if 'orientation' in t:
                keep = prediction['keep']
                vec, cnt = orientation_sums_reference(prediction['orientation'],
                                                      prediction['panoptic_instance'], keep.shape[1])
                self.mae_pan.update_matched(vec, cnt, batch['orientations'], self.pq_pan.pairs, self.div,
                                            keep)

    def compute(self):
        assert self.bad == 0
        t, r = self.tasks, {}
        if 'semantic' in t:
            r['semantic_miou'] = R.miou_reference(self.cm, True)
        if 'scene' in t:
            r['scene_acc'], r['scene_bacc'] = scene_reference(self.cm_scene, True)
        if 'orientation' in t:
            m = self.mae_gt.compute()
            r['orientation_mae_gt_deg'], r['orientation_mae_gt_rad'] = m['mae_deg'], m['mae_rad']
        if 'instance' in t and self.instance_seen:
            q = self.pq_inst.compute()
            for k in ('pq', 'sq', 'rq'):
                r[f'instance_all_with_gt_deeplab_{k}'] = q[f'all_{k}']
        if self.panoptic:
            for k, v in self.pq_pan.compute().items():
                g, q = k.split('_')
                r[f'panoptic_{g}_deeplab_{q}'] = v
            r['panoptic_deeplab_semantic_miou'] = R.miou_reference(self.cm_pan, True)
            if 'orientation' in t:
                m = self.mae_pan.compute()
                r['panoptic_mae_deeplab_deg'], r['panoptic_mae_deeplab_rad'] = m['mae_deg'], m['mae_rad']
        return r
