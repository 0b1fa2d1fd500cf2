# -*- coding: utf-8 -*-
"""
Device-side validation: the metrics the reference logs after every validation epoch and keeps its
checkpoints by (its README's evaluation commands pass `--checkpointing-metrics valid_semantic_miou
bacc mae_gt_deg panoptic_deeplab_semantic_miou panoptic_all_deeplab_pq`; main.py ranks keys with
`acc` upwards and keys with `mae` downwards), from the post-processed prediction of an eval forward
and the labels of the batch -- both already on the GPU.

`ValidationEvaluator.update(prediction, batch)` only launches kernels on the current stream: no
device-to-host copy, no synchronisation, and every buffer of its own is created in the first call for
a shape (call it once before capturing it into a graph).  `compute()` is the one host read.

Keys of `compute()` (the reference's names without the `valid_` prefix):
  semantic_miou                          semantic_segmentation_idx + 1 against batch['semantic'] (void
                                         ignored)
  scene_acc, scene_bacc                  scene_class_idx + 1 against batch['scene'] (0 = void)
  orientation_mae_gt_deg / _rad          the predicted orientation averaged over the pixels of every
                                         GROUND-TRUTH instance (inside batch['orientation_foreground']
                                         when the batch has it) against batch['orientations']
  instance_all_with_gt_deeplab_pq/sq/rq  PQ of the grouping inside the ground-truth foreground, given
                                         the ground-truth classes, against the ground truth
  panoptic_{all,things,stuff}_deeplab_{pq,sq,rq}
                                         panoptic_segmentation_deeplab against panoptic_targets(...)
  panoptic_deeplab_semantic_miou         panoptic_segmentation_deeplab_semantic_idx (with void)
                                         against batch['semantic'], void ignored
  panoptic_mae_deeplab_deg / _rad        angular error over the segments the panoptic PQ matched
  normal_mae_deg / _rad                  mean angle between the raw `normal_output` and the valid vectors
                                         of batch['normal'] (`metrics.MeanAbsoluteNormalError`)
Only the keys whose task is in `args.tasks` / `args.enable_panoptic` are present.

[U] (the metric library is not vendored; each rule is restated in tests/evaluation_reference.py):
  * balanced accuracy: mean recall over the classes present in the targets (metrics.SceneAccuracy)
  * angular error: per instance, mean over instances (metrics.MeanAbsoluteAngularError); the predicted
    angle of an instance is atan2 of its summed (sin, cos) channels, as `orientation_dicts`
  * `instance_all_with_gt`: the predicted side is `instance_segmentation_gt_foreground`; for the
    panoptic model, which groups inside its own thing mask, `instance_segmentation_idx` restricted to
    the pixels with a ground-truth instance.  Both sides take the ground-truth class:
    panoptic_targets(semantic, <that grouping>) against panoptic_targets(semantic, instance)
  * `panoptic_mae_deeplab`: only instances of a class with `classes_use_orientations` are compared
    (the keep table of `PanopticPostprocessing`)
  * label maps larger than the network output: every map is read from its `<key>_fullres` entry; the
    orientation channels, which have none, are resampled with nearest neighbour.  The normal target is
    batch['normal_fullres'] when the batch has it, batch['normal'] otherwise; a smaller `normal_output`
    is read with nearest neighbour.
  * `normal_mae`: the mean over pixels of atan2(|p x t|, p . t), which needs no unit length.

Not built: `panoptic_*_with_gt_deeplab_*`.  Nothing in the reference's tree says what "with gt" means
for the panoptic helper, so no such key is guessed.  Validation losses are out of scope here.
"""
import torch

from . import _lib
from . import functional as Fn
from ._lib import check
from .metrics import (_LABEL_DTYPES, MeanAbsoluteAngularError, MeanAbsoluteNormalError,
                      MeanIntersectionOverUnion, PanopticQuality, SceneAccuracy, _label_map)
from .postprocessing import thing_table

_KEEP_KEY = 'orientations_panoptic_segmentation_deeplab_instance_keep'


def _squeeze_map(t):
    return t[:, 0] if torch.is_tensor(t) and t.dim() == 4 else t


class ValidationEvaluator:
    """see the module docstring.  `max_instances` bounds the ground-truth instance ids ([0,
    max_instances), the width of `targets.orientation_table`); `max_segments` the distinct panoptic
    segments per image and side; `label_divisor` is the one of the model's panoptic post-processing."""

    def __init__(self, args, dataset_config, max_instances=256, max_segments=256, label_divisor=1000):
        tasks = tuple(args.tasks)
        labels = dataset_config.semantic_label_list_without_void
        self.with_semantic = 'semantic' in tasks
        self.with_scene = 'scene' in tasks
        self.with_instance = 'instance' in tasks
        self.with_orientation = 'orientation' in tasks
        self.with_panoptic = bool(getattr(args, 'enable_panoptic', False))
        self.with_normal = 'normal' in tasks
        self.n_classes = len(labels) + 1                                  # with void
        self.is_thing = (False,) + tuple(bool(t) for t in labels.classes_is_thing)
        self.max_instances = int(max_instances)
        self.label_divisor = int(label_divisor)
        if not 2 <= self.max_instances <= self.label_divisor:
            raise ValueError(f"ValidationEvaluator: max_instances={max_instances} outside [2, label_divisor "
                             f"= {label_divisor}]")

        def pq():
            return PanopticQuality(self.n_classes, 0, self.label_divisor, None, self.is_thing, max_segments)
        self.semantic_miou = MeanIntersectionOverUnion(self.n_classes, True) if self.with_semantic else None
        self.scene = SceneAccuracy(len(dataset_config.scene_label_list_without_void) + 1, True) \
            if self.with_scene else None
        self.orientation_mae_gt = MeanAbsoluteAngularError() if self.with_orientation else None
        self.instance_pq = pq() if self.with_instance else None
        self.panoptic_pq = pq() if self.with_panoptic else None
        self.panoptic_miou = MeanIntersectionOverUnion(self.n_classes, True) if self.with_panoptic else None
        self.panoptic_mae = MeanAbsoluteAngularError() if self.with_panoptic and self.with_orientation \
            else None
        self.normal_mae = MeanAbsoluteNormalError() if self.with_normal else None
        # whether the prediction carries a grouping for `instance_all_with_gt`: a property of the model,
        # learnt in the first update and kept over reset() (a replayed graph runs no Python)
        self._instance_pq_seen = False
        self._buf = {}

    # ---- buffers -----------------------------------------------------------------------------------
    def _buffer(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype, str(device))
        t = self._buf.get(key)
        if t is None:
            t = self._buf[key] = Fn._zeros(tuple(shape), device, dtype)
        return t

    @staticmethod
    def _map(prediction, key, shape):
        """`<key>_fullres` when it has the label maps' shape, the plain entry otherwise"""
        full, plain = prediction.get(key + '_fullres'), prediction.get(key)
        if torch.is_tensor(full) and tuple(full.shape) == tuple(shape):
            return full.contiguous()
        if torch.is_tensor(plain) and tuple(plain.shape) == tuple(shape):
            return plain.contiguous()
        raise ValueError(f"ValidationEvaluator.update: neither prediction['{key}_fullres'] nor "
                         f"prediction['{key}'] has the label maps' shape {tuple(shape)}")

    def _orientation(self, prediction, shape):
        """(N, 2, H, W) fp32 NHWC at the label maps' resolution"""
        o = prediction.get('instance_orientation')
        if not torch.is_tensor(o) or o.dim() != 4 or o.shape[0] != shape[0] or o.shape[1] != 2:
            raise ValueError("ValidationEvaluator.update: prediction['instance_orientation'] must be the "
                             f"(N, 2, h, w) orientation output of the {shape[0]} images")
        o = Fn.as_act(o.float() if o.dtype != torch.float32 else o)
        if tuple(o.shape[2:]) == tuple(shape[1:]):
            return o
        big = self._buffer('orientation', (shape[0], shape[1], shape[2], 2), torch.float32, o.device)
        return Fn.nearest_fwd(Fn.as_act(o, dense=True), big.permute(0, 3, 1, 2))

    def _orientation_sums(self, name, ori, ids, mask, slots):
        n, _, h, w = ori.shape
        vec = self._buffer(name + '_vec', (n, slots, 2), torch.int64, ori.device)
        cnt = self._buffer(name + '_cnt', (n, slots), torch.int32, ori.device)
        check(_lib.lib().emsa_instance_orientation(
            ori.data_ptr(), Fn.ld_of(ori), ids.data_ptr(), None if mask is None else mask.data_ptr(), n,
            h * w, slots, vec.data_ptr(), cnt.data_ptr(), Fn._stream()), 'emsa_instance_orientation')
        return vec, cnt

    def _panoptic_ids(self, name, semantic, instance):
        """`metrics.panoptic_targets` into a buffer of this object"""
        out = self._buffer(name, semantic.shape, torch.int64, semantic.device)
        table = thing_table(self.is_thing, semantic.device)
        check(_lib.lib().emsa_panoptic_targets(
            semantic.data_ptr(), _LABEL_DTYPES[semantic.dtype], instance.data_ptr(),
            _LABEL_DTYPES[instance.dtype], table.data_ptr(), self.n_classes, self.label_divisor,
            semantic.numel(), out.data_ptr(), Fn._stream()), 'emsa_panoptic_targets')
        return out

    # ---- update ------------------------------------------------------------------------------------
    def update(self, prediction, batch):
        name = 'ValidationEvaluator.update'
        sem = inst = None
        if self.with_semantic or self.with_instance or self.with_panoptic:
            sem = _label_map(_squeeze_map(batch['semantic']), name, "batch['semantic']")
        if self.with_instance or self.with_orientation or self.with_panoptic:
            inst = _label_map(_squeeze_map(batch['instance']), name, "batch['instance']")
        shape = tuple((sem if sem is not None else inst).shape) if (sem is not None or inst is not None) \
            else None
        if shape is not None and (len(shape) != 3 or (sem is not None and inst is not None and
                                                      sem.shape != inst.shape)):
            raise ValueError(f"{name}: batch['semantic'] / batch['instance'] must be (N, H, W) label maps of "
                             "equal shape")
        dev = (sem if sem is not None else inst).device if shape is not None else None

        if self.with_semantic:
            idx = self._map(prediction, 'semantic_segmentation_idx', shape)
            pred = self._buffer('semantic', shape, idx.dtype, dev)
            torch.add(idx, 1, out=pred)                                  # into the label list with void
            self.semantic_miou.update(pred, sem)
        if self.with_scene:
            idx = prediction['scene_class_idx']
            pred = self._buffer('scene', idx.shape, idx.dtype, idx.device)
            torch.add(idx, 1, out=pred)
            self.scene.update(pred, batch['scene'])

        gt_table = ori = None
        if self.with_orientation:
            gt_table = batch['orientations']
            ori = self._orientation(prediction, shape)
            # ground-truth ids as the int32 the sums are indexed with; every id >= max_instances lands
            # in the extra slot max_instances, where emsa_angular_error flags it
            ids = self._buffer('gt_ids', shape, torch.int32, dev)
            ids.copy_(inst)
            ids.clamp_(max=self.max_instances)
            fg = _squeeze_map(batch.get('orientation_foreground'))
            if fg is not None:
                if fg.dtype not in (torch.bool, torch.uint8) or tuple(fg.shape) != shape:
                    raise TypeError(f"{name}: batch['orientation_foreground'] must be a bool / uint8 mask of "
                                    f"shape {shape}")
                fg = fg.contiguous()
                fg = fg.view(torch.uint8) if fg.dtype == torch.bool else fg
            vec, cnt = self._orientation_sums('gt', ori, ids, fg, self.max_instances + 1)
            self.orientation_mae_gt.update(vec, cnt, gt_table)

        targets = None
        if self.with_instance or self.with_panoptic:
            targets = self._panoptic_ids('targets', sem, inst)
        if self.with_instance:
            grouping = None
            try:
                grouping = self._map(prediction, 'instance_segmentation_gt_foreground', shape)
            except ValueError:
                if self.with_panoptic:
                    idx = self._map(prediction, 'instance_segmentation_idx', shape)
                    fg = self._buffer('gt_foreground', shape, torch.bool, dev)
                    torch.ne(inst, 0, out=fg)
                    grouping = self._buffer('grouping', shape, idx.dtype, dev)
                    torch.mul(idx, fg, out=grouping)
            if grouping is not None:
                grouping = _label_map(grouping, name, 'the instance grouping')
                self.instance_pq.update(self._panoptic_ids('grouping_ids', sem, grouping), targets)
                self._instance_pq_seen = True
        if self.with_panoptic:
            pan = self._map(prediction, 'panoptic_segmentation_deeplab', shape)
            matches, n_matches = self.panoptic_pq.update_with_matches(pan, targets)
            self.panoptic_miou.update(
                self._map(prediction, 'panoptic_segmentation_deeplab_semantic_idx', shape), sem)
            if self.panoptic_mae is not None:
                pan_inst = self._map(prediction, 'panoptic_segmentation_deeplab_instance_idx', shape)
                keep = prediction[_KEEP_KEY]
                if pan_inst.dtype != torch.int32:
                    raise TypeError(f"{name}: the panoptic instance map must be int32")
                vec, cnt = self._orientation_sums('panoptic', ori, pan_inst, None, keep.shape[1])
                self.panoptic_mae.update_matched(vec, cnt, gt_table, matches, n_matches,
                                                 self.label_divisor, keep)

        if self.with_normal:
            target = batch.get('normal_fullres')
            self.normal_mae.update(prediction['normal_output'],
                                   target if torch.is_tensor(target) else batch['normal'])

    # ---- results -----------------------------------------------------------------------------------
    def _metrics(self):
        return {'semantic_miou': self.semantic_miou, 'scene': self.scene,
                'orientation_mae_gt': self.orientation_mae_gt, 'instance_pq': self.instance_pq,
                'panoptic_pq': self.panoptic_pq, 'panoptic_miou': self.panoptic_miou,
                'panoptic_mae': self.panoptic_mae, 'normal_mae': self.normal_mae}

    def reset(self):
        for m in self._metrics().values():
            if m is not None:
                m.reset()

    def state(self):
        """host copy of every integer state (flag words included): {metric name: int64 tensor} -- for
        tests; two evaluators that counted the same hold equal states, bit for bit"""
        out = {}
        for k, m in self._metrics().items():
            s = None if m is None else (m._cm._state if isinstance(m, SceneAccuracy) else m._state)
            if s is not None:
                out[k] = s.cpu()
        return out

    def compute(self):
        r = {}
        if self.with_semantic:
            r['semantic_miou'] = self.semantic_miou.compute()
        if self.with_scene:
            s = self.scene.compute()
            r['scene_acc'], r['scene_bacc'] = s['acc'], s['bacc']
        if self.with_orientation:
            m = self.orientation_mae_gt.compute()
            r['orientation_mae_gt_deg'], r['orientation_mae_gt_rad'] = m['mae_deg'], m['mae_rad']
        if self.with_instance and self._instance_pq_seen:
            q = self.instance_pq.compute()
            for k in ('pq', 'sq', 'rq'):
                r[f'instance_all_with_gt_deeplab_{k}'] = q[f'all_{k}']
        if self.with_panoptic:
            for k, v in self.panoptic_pq.compute().items():
                g, q = k.split('_')
                r[f'panoptic_{g}_deeplab_{q}'] = v
            r['panoptic_deeplab_semantic_miou'] = self.panoptic_miou.compute()
            if self.panoptic_mae is not None:
                m = self.panoptic_mae.compute()
                r['panoptic_mae_deeplab_deg'], r['panoptic_mae_deeplab_rad'] = m['mae_deg'], m['mae_rad']
        if self.with_normal:
            m = self.normal_mae.compute()
            r['normal_mae_deg'], r['normal_mae_rad'] = m['mae_deg'], m['mae_rad']
        return r
