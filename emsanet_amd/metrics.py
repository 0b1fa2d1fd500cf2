# -*- coding: utf-8 -*-
"""
Validation metrics on device: mean IoU and panoptic quality, the two values the reference keeps its
checkpoints by (`valid_semantic_miou`, `valid_panoptic_all_deeplab_pq`: /root/reference/main.py:229,
emsanet/args.py:1054), and the other checkpoint keys of the reference's evaluation commands: scene
accuracy (`bacc`), the mean absolute angular error of the orientations (`mae_gt_deg`,
`panoptic_mae_deeplab_deg`) and that of the surface normals (`normal_mae_deg`).  `emsanet_amd.evaluation.ValidationEvaluator` composes them.

The reference takes them from `metric.MeanIntersectionOverUnion` / `metric.PanopticQuality` of the
un-vendored `nicr_mt_scene_analysis` library.  The classes here keep that surface
(/root/reference/external/stuff/eval_miou.py:39-67, emsanet/tests/test_metrics_with_model.py:82-88,
186-237) and count on the GPU, where the post-processed maps already are: `update()` only launches
kernels on the current stream (no device-to-host copy, no synchronisation, no allocation after the
first call for a shape, so it can be captured into a graph); the one host read is in `compute()`.
Arithmetic: csrc/metrics.hip -- integer sums only, so results are independent of the execution order.
"""
import math

import torch

from . import _lib
from ._lib import check
from .functional import _stream
from . import functional as Fn
from .postprocessing import normal_map, thing_table

_LABEL_DTYPES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}       # EMSA_LABEL_*
IOU_ONE = 1 << 40                                                      # fixed point of iou_sum
NORMAL_ANGLE_ONE = 1 << 20          # EMSA_NORMAL_ANGLE_ONE: fixed point of the normal error sum, 1 / rad


def _label_map(t, name, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} must be a tensor")
    if not t.is_cuda:
        raise NotImplementedError(f"{name}: {what} is a CPU tensor; the metrics count on the GPU only")
    if t.dtype not in _LABEL_DTYPES:
        raise TypeError(f"{name}: {what} has dtype {t.dtype}; int64, int32 or uint8 label maps only")
    return t.contiguous()


class MeanIntersectionOverUnion:
    """[U] restatement of the library's `MeanIntersectionOverUnion(n_classes, ignore_first_class)`
    (the upstream class is not vendored; surface as /root/reference/external/stuff/eval_miou.py:39-67
    uses it).  `update(preds, targets)` adds the label maps (equal shapes; int64 / int32 / uint8) into
    the confusion matrix cm[target][pred]; `compute()` is the mean of
    IoU_c = cm[c][c] / (row_c + col_c - cm[c][c]) over the classes with a non-zero union, after row
    and column 0 (void) have been dropped when `ignore_first_class`.  A label outside [0, n_classes)
    is not counted and makes `compute()` raise."""

    def __init__(self, n_classes, ignore_first_class=False):
        if n_classes < 1 + int(bool(ignore_first_class)):
            raise ValueError(f"MeanIntersectionOverUnion: n_classes={n_classes}")
        self.n_classes = int(n_classes)
        self.ignore_first_class = bool(ignore_first_class)
        self._state = None                      # int64 [C*C + 1]: the matrix, then n_invalid

    def _buffers(self, device):
        if self._state is None or self._state.device != device:
            self._state = Fn._zeros((self.n_classes ** 2 + 1,), device, torch.int64)
        return self._state

    def update(self, preds, targets):
        p = _label_map(preds, 'MeanIntersectionOverUnion.update', 'preds')
        t = _label_map(targets, 'MeanIntersectionOverUnion.update', 'targets')
        if p.numel() != t.numel() or p.device != t.device:
            raise ValueError(f"MeanIntersectionOverUnion.update: preds {tuple(p.shape)} on {p.device} vs "
                             f"targets {tuple(t.shape)} on {t.device}")
        s = self._buffers(p.device)
        cc = self.n_classes ** 2
        check(_lib.lib().emsa_confusion_matrix(
            p.data_ptr(), _LABEL_DTYPES[p.dtype], t.data_ptr(), _LABEL_DTYPES[t.dtype], p.numel(),
            self.n_classes, s.data_ptr(), s.data_ptr() + 8 * cc, _stream()), 'emsa_confusion_matrix')

    @property
    def confusion_matrix(self):
        """(C, C) int64 on the device, [target][pred] (a view of the running state: no sync)"""
        if self._state is None:
            return torch.zeros((self.n_classes, self.n_classes), dtype=torch.int64)
        return self._state[:-1].view(self.n_classes, self.n_classes)

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def compute(self):
        if self._state is None:
            return 0.0
        s = self._state.cpu()
        if int(s[-1]) != 0:
            raise ValueError(f"MeanIntersectionOverUnion: n_invalid = {int(s[-1])} pixels carried a label "
                             f"outside [0, {self.n_classes}) and were not counted")
        cm = s[:-1].view(self.n_classes, self.n_classes)
        if self.ignore_first_class:
            cm = cm[1:, 1:]
        tp = cm.diagonal()
        union = cm.sum(0) + cm.sum(1) - tp
        keep = union > 0
        if not bool(keep.any()):
            return 0.0
        return float((tp[keep].double() / union[keep].double()).mean())


class PanopticQuality:
    """`metric.PanopticQuality(num_categories, ignored_label, max_instances_per_category, offset,
    is_thing)` as /root/reference/emsanet/tests/test_metrics_with_model.py:82-88 builds it, with the
    DeepLab2 / panopticapi rules that test holds the library to (at 9 decimals).

    `update(preds, targets)`: int64 panoptic id maps (N, H, W) on the GPU,
    id = category * max_instances_per_category + instance (`panoptic_segmentation_deeplab[_fullres]`
    and `panoptic_targets`).  Per image, a predicted and a target segment of one category (not the
    ignored one) match iff IoU > 1/2, where the prediction's overlap with ignored target pixels is
    left out of the union; a match is a tp, an unmatched target a fn, an unmatched prediction a fp
    unless more than half of it lies on ignored pixels.

    `compute()` -> dict all_pq / all_sq / all_rq, things_*, stuff_*: per category
    sq = iou_sum / tp, rq = tp / (tp + fn/2 + fp/2), pq = sq * rq, averaged over the categories of the
    group with tp + fn + fp > 0 (0.0 for a group without any).

    `offset` is accepted for interface compatibility and unused: the device never forms id products.
    `max_segments` bounds the distinct segments per side per image; more make `compute()` raise."""

    def __init__(self, num_categories, ignored_label, max_instances_per_category, offset=None,
                 is_thing=None, max_segments=256):
        if is_thing is None or len(is_thing) != num_categories:
            raise ValueError("PanopticQuality: is_thing must name every one of the num_categories")
        if max_instances_per_category < 1:
            raise ValueError("PanopticQuality: max_instances_per_category must be positive")
        self.num_categories = int(num_categories)
        self.ignored_label = int(ignored_label)
        self.max_instances_per_category = int(max_instances_per_category)
        self.offset = offset
        self.is_thing = tuple(bool(t) for t in is_thing)
        self.max_segments = int(max_segments)
        if _lib.lib().emsa_panoptic_workspace_bytes(1, self.max_segments) <= 0:
            raise ValueError(f"PanopticQuality: max_segments={max_segments} outside [1, 1024]")
        self._state = None                      # int64 [4*K + 1]: tp, fn, fp, iou_sum, then 2 int32 flags
        self._ws = {}                           # (device, images) -> workspace
        self._matches = {}                      # images -> (matches, n_matches)

    def _buffers(self, device, n):
        if self._state is None or self._state.device != device:
            self._state = Fn._zeros((4 * self.num_categories + 1,), device, torch.int64)
            self._ws = {}
            self._matches = {}
        ws = self._ws.get(n)
        if ws is None:
            nbytes = _lib.lib().emsa_panoptic_workspace_bytes(n, self.max_segments)
            ws = self._ws[n] = Fn._empty((nbytes,), device, torch.uint8)
        return self._state, ws

    def update(self, preds, targets):
        self._update(preds, targets, False)

    def update_with_matches(self, preds, targets):
        """`update(preds, targets)` through `emsa_panoptic_match_pairs`: the same counts, and
        -> (matches (N, max_segments, 2) int64, n_matches (N,) int32) on the device: the first
        n_matches[i] rows of matches[i] are the (predicted id, target id) pairs of image i that matched,
        in no particular order; the rows behind them are stale.  Both tensors belong to this object and
        are overwritten by its next `update_with_matches` of the same batch size."""
        return self._update(preds, targets, True)

    def _update(self, preds, targets, export):
        for what, t in (('preds', preds), ('targets', targets)):
            if not torch.is_tensor(t):
                raise TypeError(f"PanopticQuality.update: {what} must be a tensor")
            if not t.is_cuda:
                raise NotImplementedError(f"PanopticQuality.update: {what} is a CPU tensor; the metrics "
                                          "count on the GPU only")
            if t.dtype != torch.int64:
                raise TypeError(f"PanopticQuality.update: {what} has dtype {t.dtype}; int64 panoptic ids only")
        if preds.shape != targets.shape or preds.dim() not in (2, 3) or preds.device != targets.device:
            raise ValueError(f"PanopticQuality.update: preds {tuple(preds.shape)} vs targets "
                             f"{tuple(targets.shape)}; (N, H, W) or (H, W) maps of equal shape")
        p, t = preds.contiguous(), targets.contiguous()
        n = 1 if p.dim() == 2 else p.shape[0]
        hw = p.shape[-2] * p.shape[-1]
        s, ws = self._buffers(p.device, n)
        k = self.num_categories
        base, flags = s.data_ptr(), s.data_ptr() + 8 * 4 * k
        L = _lib.lib()
        check(L.emsa_panoptic_pairs(p.data_ptr(), t.data_ptr(), n, hw, self.max_segments, ws.data_ptr(),
                                    flags, _stream()), 'emsa_panoptic_pairs')
        if export:
            m = self._matches.get(n)
            if m is None:
                m = self._matches[n] = (
                    Fn._zeros((n, self.max_segments, 2), p.device, torch.int64),
                    Fn._zeros((n,), p.device, torch.int32))
            check(L.emsa_panoptic_match_pairs(ws.data_ptr(), n, self.max_segments, k, self.ignored_label,
                                              self.max_instances_per_category, base, base + 8 * k,
                                              base + 16 * k, base + 24 * k, m[0].data_ptr(),
                                              m[1].data_ptr(), flags, _stream()),
                  'emsa_panoptic_match_pairs')
            return m
        check(L.emsa_panoptic_match(ws.data_ptr(), n, self.max_segments, k, self.ignored_label,
                                    self.max_instances_per_category, base, base + 8 * k,
                                    base + 16 * k, base + 24 * k, flags, _stream()),
              'emsa_panoptic_match')
        return None

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def counts(self):
        """host copy of the state: dict tp / fn / fp / iou_sum (lists of Python ints, iou_sum in
        units of 2^-40) -- raises like `compute()`"""
        k = self.num_categories
        if self._state is None:
            return {key: [0] * k for key in ('tp', 'fn', 'fp', 'iou_sum')}
        s = self._state.cpu()
        overflow, invalid = (int(v) for v in s[4 * k:].view(torch.int32)[:2])
        if overflow:
            raise ValueError(f"PanopticQuality: segment table overflow -- an image had more than "
                             f"max_segments = {self.max_segments} distinct segments on one side")
        if invalid:
            raise ValueError("PanopticQuality: invalid panoptic id -- negative, or of a category outside "
                             f"[0, {k})")
        v = s[:4 * k].view(4, k).tolist()
        return {'tp': v[0], 'fn': v[1], 'fp': v[2], 'iou_sum': v[3]}

    def compute(self):
        c = self.counts()
        groups = {'all': [], 'things': [], 'stuff': []}
        for cat in range(self.num_categories):
            tp, fn, fp = c['tp'][cat], c['fn'][cat], c['fp'][cat]
            if cat == self.ignored_label or tp + fn + fp == 0:
                continue
            sq = (c['iou_sum'][cat] / IOU_ONE) / tp if tp else 0.0
            rq = tp / (tp + 0.5 * fn + 0.5 * fp)
            for g in ('all', 'things' if self.is_thing[cat] else 'stuff'):
                groups[g].append((sq * rq, sq, rq))
        out = {}
        for g, rows in groups.items():
            for j, key in enumerate(('pq', 'sq', 'rq')):
                out[f'{g}_{key}'] = sum(r[j] for r in rows) / len(rows) if rows else 0.0
        return out


class SceneAccuracy:
    """`valid_scene_acc` / `valid_scene_bacc` from the confusion matrix cm[target][pred] of (N,) scene
    labels (`emsa_confusion_matrix`; row and column 0 = void dropped when `ignore_first_class`).
    acc = trace / total of the kept matrix; bacc = mean of cm[c][c] / row_c over the classes that occur
    in the targets (row_c > 0) -- [U]: the library's balanced accuracy is not vendored; averaging
    the recall over the classes present in the targets is the usual definition.  0.0 without any
    counted sample.  A label outside [0, n_classes_with_void) is not counted and makes `compute()`
    raise."""

    def __init__(self, n_classes_with_void, ignore_first_class=True):
        self._cm = MeanIntersectionOverUnion(n_classes_with_void, ignore_first_class)
        self.n_classes = self._cm.n_classes
        self.ignore_first_class = self._cm.ignore_first_class

    def update(self, pred_idx_with_void, target):
        for what, x in (('pred_idx_with_void', pred_idx_with_void), ('target', target)):
            if not torch.is_tensor(x):
                raise TypeError(f"SceneAccuracy.update: {what} must be a tensor")
            if x.dtype not in _LABEL_DTYPES:
                raise TypeError(f"SceneAccuracy.update: {what} has dtype {x.dtype}; int64, int32 or uint8 "
                                "labels only")
        if pred_idx_with_void.dim() != 1 or pred_idx_with_void.shape != target.shape:
            raise ValueError(f"SceneAccuracy.update: pred {tuple(pred_idx_with_void.shape)} vs target "
                             f"{tuple(target.shape)}; (N,) labels of equal shape")
        p = _label_map(pred_idx_with_void, 'SceneAccuracy.update', 'pred_idx_with_void')
        t = _label_map(target, 'SceneAccuracy.update', 'target')
        self._cm.update(p, t)

    @property
    def confusion_matrix(self):
        return self._cm.confusion_matrix

    def reset(self):
        self._cm.reset()

    def compute(self):
        if self._cm._state is None:
            return {'acc': 0.0, 'bacc': 0.0}
        s = self._cm._state.cpu()
        if int(s[-1]) != 0:
            raise ValueError(f"SceneAccuracy: n_invalid = {int(s[-1])} samples carried a label outside "
                             f"[0, {self.n_classes}) and were not counted")
        cm = s[:-1].view(self.n_classes, self.n_classes)
        if self.ignore_first_class:
            cm = cm[1:, 1:]
        total, rows, tp = int(cm.sum()), cm.sum(1), cm.diagonal()
        present = rows > 0
        if total == 0:
            return {'acc': 0.0, 'bacc': 0.0}
        return {'acc': int(tp.sum()) / total,
                'bacc': float((tp[present].double() / rows[present].double()).mean())}


ANGLE_ONE = 1 << 40                                                    # fixed point of the error sum


def _angle_inputs(name, vec, count, gt_table, keep):
    for what, t, dtypes in (('vec', vec, (torch.int64,)), ('count', count, (torch.int32,)),
                            ('gt_table', gt_table, (torch.float32,)),
                            ('keep', keep, (torch.uint8, torch.bool))):
        if t is None and what == 'keep':
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"{name}: {what} must be a tensor")
        if t.dtype not in dtypes:
            raise TypeError(f"{name}: {what} has dtype {t.dtype}; expected {' or '.join(map(str, dtypes))}")
    if vec.dim() != 3 or vec.shape[2] != 2 or tuple(count.shape) != tuple(vec.shape[:2]) or \
            gt_table.dim() != 2 or gt_table.shape[0] != vec.shape[0] or \
            (keep is not None and keep.shape != count.shape):
        raise ValueError(f"{name}: vec {tuple(vec.shape)}, count {tuple(count.shape)}, gt_table "
                         f"{tuple(gt_table.shape)}, keep {None if keep is None else tuple(keep.shape)}; "
                         "expected (N, slots, 2), (N, slots), (N, gt_slots), (N, slots)")
    if vec.shape[1] < 2 or gt_table.shape[1] < 2:
        raise ValueError(f"{name}: at least 2 slots on either side (slot 0 is 'no instance')")
    for what, t in (('vec', vec), ('count', count), ('gt_table', gt_table), ('keep', keep)):
        if t is not None and not t.is_cuda:
            raise NotImplementedError(f"{name}: {what} is a CPU tensor; the metrics count on the GPU only")
        if t is not None and t.device != vec.device:
            raise ValueError(f"{name}: {what} on {t.device}, vec on {vec.device}")
    k = None if keep is None else keep.contiguous()
    if k is not None and k.dtype == torch.bool:
        k = k.view(torch.uint8)
    return vec.contiguous(), count.contiguous(), gt_table.contiguous(), k


class MeanAbsoluteAngularError:
    """`valid_orientation_mae_gt_*` / `valid_panoptic_mae_deeplab_*`: the mean over the compared
    instances of the absolute angular difference (in [0, pi]) between the instance's mean predicted
    orientation and its ground-truth angle (`emsa_angular_error`).

    vec (N, slots, 2) int64 / count (N, slots) int32: the per-instance sums of
    `postprocessing.instance_orientation_sums`; gt_table (N, gt_slots) float32: the angle in rad per
    ground-truth instance id, NaN = none (`targets.orientation_table`); keep (N, slots) uint8 / bool or
    None.  `update` compares slot j with ground-truth id j; `update_matched` compares, for every pair of
    `PanopticQuality.update_with_matches`, predicted slot pred_id % label_divisor with ground-truth id
    target_id % label_divisor (stuff pairs skipped).  An instance without pixels, with keep 0 or with a
    NaN ground truth is skipped.  Which instances the library compares and that it averages over
    instances rather than pixels is [U] (the library is not vendored).

    `compute()` -> {'mae_rad', 'mae_deg'}: NaN, not 0.0, when nothing was compared -- the value is ranked
    "lower is better", and a 0.0 would be kept as the best ever.  It is the one host read and raises
    ValueError when an id lay outside the tables (such an instance is not compared)."""

    def __init__(self):
        self._state = None                      # int64 [3]: error sum (2^-40 rad), count, int32 flag

    def _buffers(self, device):
        if self._state is None or self._state.device != device:
            self._state = Fn._zeros((3,), device, torch.int64)
        return self._state

    def _launch(self, name, vec, count, gt_table, keep, matches, n_matches, max_segments, divisor):
        v, c, g, k = _angle_inputs(name, vec, count, gt_table, keep)
        s = self._buffers(v.device)
        check(_lib.lib().emsa_angular_error(
            v.data_ptr(), c.data_ptr(), None if k is None else k.data_ptr(), v.shape[0], v.shape[1],
            g.data_ptr(), g.shape[1], None if matches is None else matches.data_ptr(),
            None if n_matches is None else n_matches.data_ptr(), max_segments, divisor, s.data_ptr(),
            s.data_ptr() + 16, _stream()), 'emsa_angular_error')

    def update(self, vec, count, gt_table, keep=None):
        self._launch('MeanAbsoluteAngularError.update', vec, count, gt_table, keep, None, None, 0, 1)

    def update_matched(self, vec, count, gt_table, matches, n_matches, label_divisor, keep=None):
        name = 'MeanAbsoluteAngularError.update_matched'
        for what, t, dtype in (('matches', matches, torch.int64), ('n_matches', n_matches, torch.int32)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name}: {what} must be a tensor")
            if t.dtype != dtype:
                raise TypeError(f"{name}: {what} has dtype {t.dtype}; expected {dtype}")
        if matches.dim() != 3 or matches.shape[2] != 2 or tuple(n_matches.shape) != (matches.shape[0],) or \
                not torch.is_tensor(vec) or matches.shape[0] != vec.shape[0] or int(label_divisor) < 1:
            raise ValueError(f"{name}: matches {tuple(matches.shape)}, n_matches {tuple(n_matches.shape)}; "
                             "expected (N, max_segments, 2) and (N,) for the N images of vec, and a "
                             "positive label_divisor")
        if not matches.is_contiguous() or not n_matches.is_contiguous():
            raise ValueError(f"{name}: matches / n_matches must be contiguous")
        if not matches.is_cuda or not n_matches.is_cuda:
            raise NotImplementedError(f"{name}: matches is a CPU tensor; the metrics count on the GPU only")
        self._launch(name, vec, count, gt_table, keep, matches, n_matches, matches.shape[1],
                     int(label_divisor))

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def counts(self):
        """host copy of the state -> (error sum in units of 2^-40 rad, compared instances); raises like
        `compute()`"""
        if self._state is None:
            return 0, 0
        s = self._state.cpu()
        if int(s[2:].view(torch.int32)[0]):
            raise ValueError("MeanAbsoluteAngularError: an instance id lay outside the orientation tables "
                             "(ground-truth id >= gt_slots, or predicted instance >= slots)")
        return int(s[0]), int(s[1])

    def compute(self):
        total, n = self.counts()
        if n == 0:
            return {'mae_rad': float('nan'), 'mae_deg': float('nan')}
        rad = total / ANGLE_ONE / n
        return {'mae_rad': rad, 'mae_deg': math.degrees(rad)}


class MeanAbsoluteNormalError:
    """[U] `valid_normal_mae_*`: the mean over all valid pixels of all updates of the angle between the
    predicted and the ground-truth normal, atan2(|p x t|, p . t) in [0, pi] -- well conditioned near 0 and
    pi, needs neither vector at unit length and equals acos of the cosine similarity.

    `update(pred, target)`: pred float (N,3,h,w) on the GPU, the raw `normal_output` (any length);
    target float32 (N,H,W,3) or (N,3,H,W), (0,0,0) = invalid (not compared).  Where the target is larger
    than the prediction, the prediction is read with nearest neighbour (source index floor(y * h / H), the
    rule of `evaluation`).  The angle is computed in fp32, rounded once to 2^-20 rad (at most 4.8e-7 rad
    per pixel; room for more than 10^12 pixels in the int64 sum) and added as an integer, so the state
    does not depend on the launch geometry or on the order of the updates; the count is exact.  One
    launch on the current stream, no host copy, no allocation after the first call.

    `compute()` -> {'mae_rad', 'mae_deg'}: NaN, not 0.0, when nothing was compared (ranked "lower is
    better").  It is the one host read and raises ValueError if a prediction was not finite (such a pixel
    is not compared)."""

    def __init__(self):
        self._state = None                      # int64 [3]: error sum (2^-20 rad), count, int32 flag

    def _buffers(self, device):
        if self._state is None or self._state.device != device:
            self._state = Fn._zeros((3,), device, torch.int64)
        return self._state

    def update(self, pred, target):
        name = 'MeanAbsoluteNormalError.update'
        if not torch.is_tensor(pred):
            raise TypeError(f"{name}: pred must be a tensor")
        if not pred.dtype.is_floating_point:
            raise TypeError(f"{name}: pred has dtype {pred.dtype}; a floating-point (N, 3, h, w) map")
        if pred.dim() != 4 or pred.shape[1] != 3:
            raise ValueError(f"{name}: pred has shape {tuple(pred.shape)}; expected (N, 3, h, w)")
        target, chw, (n, th, tw) = normal_map(target, name, 'target')
        if not pred.is_cuda:
            raise NotImplementedError(f"{name}: pred is a CPU tensor; the metrics count on the GPU only")
        if pred.shape[0] != n or pred.device != target.device:
            raise ValueError(f"{name}: pred {tuple(pred.shape)} on {pred.device} vs target of {n} images on "
                             f"{target.device}")
        pred = Fn.as_act(pred if pred.dtype == torch.float32 else pred.float())
        s = self._buffers(pred.device)
        check(_lib.lib().emsa_normal_angular_error(
            pred.data_ptr(), Fn.ld_of(pred), n, pred.shape[2], pred.shape[3], target.data_ptr(),
            1 if chw else 0, th, tw, s.data_ptr(), s.data_ptr() + 16, _stream()), 'emsa_normal_angular_error')

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def counts(self):
        """host copy of the state -> (error sum in units of 2^-20 rad, compared pixels); raises like
        `compute()`"""
        if self._state is None:
            return 0, 0
        s = self._state.cpu()
        if int(s[2:].view(torch.int32)[0]):
            raise ValueError("MeanAbsoluteNormalError: a predicted normal was not finite (the pixel was not "
                             "compared)")
        return int(s[0]), int(s[1])

    def compute(self):
        total, n = self.counts()
        if n == 0:
            return {'mae_rad': float('nan'), 'mae_deg': float('nan')}
        rad = total / NORMAL_ANGLE_ONE / n
        return {'mae_rad': rad, 'mae_deg': math.degrees(rad)}


def panoptic_targets(semantic, instance, is_thing, label_divisor):
    """ground-truth side of the panoptic merge, as `deeplab_merge_batch(semantic, instance, instance !=
    0, label_divisor, np.where(is_thing)[0], 0)` is called in
    /root/reference/emsanet/tests/test_metrics_with_model.py:155-163: semantic (labels WITH void,
    0 = void) and instance maps of equal shape (int64 / int32 / uint8) on the GPU -> int64 ids
    sem * label_divisor + inst for a thing class, sem * label_divisor for a stuff class, 0 for void.
    `is_thing` is indexed by the label with void.  One kernel on the current stream, no host sync (the
    is-thing table is uploaded once per class list: call it once before capturing a graph)."""
    s = _label_map(semantic, 'panoptic_targets', 'semantic')
    i = _label_map(instance, 'panoptic_targets', 'instance')
    if s.shape != i.shape or s.device != i.device:
        raise ValueError(f"panoptic_targets: semantic {tuple(s.shape)} vs instance {tuple(i.shape)}")
    table = thing_table(is_thing, s.device)
    out = Fn._empty(s.shape, s.device, torch.int64)
    check(_lib.lib().emsa_panoptic_targets(s.data_ptr(), _LABEL_DTYPES[s.dtype], i.data_ptr(),
                                           _LABEL_DTYPES[i.dtype], table.data_ptr(), len(is_thing),
                                           int(label_divisor), s.numel(), out.data_ptr(), _stream()),
          'emsa_panoptic_targets')
    return out
