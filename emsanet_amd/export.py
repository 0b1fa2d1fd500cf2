# -*- coding: utf-8 -*-
"""
Inference outputs packed on the device: the four formats of the reference's dataset inference run
(/root/reference/inference_dataset.py:139-552) -- `scannet-semantic`, `scannet-instance`,
`scannet-panoptic`, `mapping` -- formed from the post-processed prediction of an eval forward where it
lies, in HBM.  The reference pulls about ten full-resolution int64 / int32 / fp32 maps per image to the
host and lets NumPy do the `+ 1`, the class re-mapping, the casts, the three-channel encoding and
`class + clamp(score)`; here only the packed bytes (1 - 4 per pixel and output) cross to the host.
Arithmetic: csrc/export.hip; NumPy restatement: tests/export_reference.py.

    packer = InferenceOutputPacker(formats, max_instances_per_category, ...)
    packed = packer.pack(prediction, batch)      # kernels only: dict of device tensors
    host = packer.to_host(packed)                # pinned buffers, one async copy each, one event
    packer.check()                               # the one host read of the counters

Keys of `pack` (the reference's directory names; H, W = the full resolution, see below):
  scannet_semantic/pred_path_semantic           uint8 (N,H,W)    map[semantic_segmentation_idx + 1]   :284-293
  scannet_semantic/pred_path_panoptic_semantic  uint8 (N,H,W)    map[panoptic semantic idx]           :298-306
  scannet_semantic/gt_path                      uint8            map[batch semantic], depth masked    :264-279
  scannet_panoptic/pred_path                    uint8 (N,H,W,3)  B, G = instance id, R = map[class]   :139-154,223-237
  scannet_panoptic/gt_path                      uint8 (.,.,.,3)  from batch panoptic // and % max_instances_per_category,
                                                                 depth masked                          :196-218
  scannet_instance/gt_path                      shift 1000: uint16 map[sem] * 1000 + inst (wrapping as the
                                                reference's uint16 arithmetic); shift 65536: uint8 x3 as the
                                                panoptic encoding; depth masked                        :352-399
  mapping/pred_semantic                         float32 (N,1,H,W) map[idx + 1] + clamp(score, 0, 0.999)  :467-482
  mapping/pred_panoptic_semantic                float32 (N,1,H,W) map[panoptic semantic idx] + clamp(score) :486-502
  mapping/pred_panoptic_instance                float32 (N,H,W)   float(instance id) + clamp(score)    :505-524
  mapping/pred_scene                            float32 (N,)      float(scene idx) + clamp(score), no + 1 :546-552
  mapping/pred_panoptic_instance_meta           the prediction's instance meta, passed through untouched
                                                (a `Deferred`: it copies to the host when it is read)
Ground-truth entries only with `write_ground_truth` and only when the batch carries the labels (its
`<key>_fullres` entry or the plain one); they keep the labels' own size.  With `max_depth` the raw depth
is read from batch['_no_preprocessing']['depth'] as ONE device tensor (N, H, W), uint16 or float32
(the reference holds a list of host arrays there); where depth > max_depth class and instance are 0.

`pack` reads the `<key>_fullres` entry of a prediction key when there is one, else the plain key (the
reference's `get_fullres`).  Every prediction output has the size of `semantic_segmentation_idx` so
read; a map of another size is sampled with nearest neighbour inside the packing kernel (the rule of
`add_fullres_predictions`, so that packing a network-resolution label map gives the bytes of packing its
`_fullres` twin).  It launches kernels only -- no host copy, no synchronisation, and after the first
call for a shape no allocation; outputs rotate over `ring` sets of buffers, so the set of call k may be
copied out while call k + 1 packs.  It can therefore follow the forward inside a captured graph:
`GraphedInference(model, batch, do_postprocessing=True, after=packer.pack)`.  (The first `ring` calls create
the class table and the buffers; the captured call must find its ring set's buffers, so `ring <= warmup + 1`
of the GraphedInference, or run pack() `ring` times beforehand.)

Values a format cannot hold are counted on the device, one int64 counter per cause (`CAUSES`), and
packed as documented in include/emsanet_hip.h; `check()` raises ValueError naming the causes.

`instance_outputs` serves the `scannet-instance` prediction (:405-442): mask planes and text lines.  It
has to know the number of instances on the host to size the stack: it is the ONE call here that
synchronises.

The arrays have exactly the layout `cv2.imwrite` is given in the reference.  The `scannet_*` outputs and
the mask planes become PNG files on the device with `emsanet_amd/png.py` (`PngEncoder.encode_packed`,
`write_scannet_output`); no image codec is a dependency.
"""
import json
import os

import numpy as np
import torch

from . import _lib
from . import functional as Fn
from ._lib import EmsaExportJob, check
from .metrics import _LABEL_DTYPES

FORMATS = ('scannet-semantic', 'scannet-instance', 'scannet-panoptic', 'mapping')
SCORE_MAX = 0.999                                   # /root/reference/inference_dataset.py:43

# EMSA_EXPORT_* of include/emsanet_hip.h
LABEL_U8, PANOPTIC_BGR, SEM_INST_U16, CLASS_SCORE_F32 = 0, 1, 2, 3
_DEPTH_U16, _DEPTH_F32 = 4, 5
MAX_JOBS = 16
CAUSES = ('a label (+ 1 where the map has no void) outside the class mapping table',
          'a semantic class above 255 in a three-channel (BGR) output',
          'an instance id above 65535 in a three-channel (BGR) output',
          'map[semantic] * 1000 + instance does not fit uint16 (use shift=65536)')

_PAN_SEM = 'panoptic_segmentation_deeplab_semantic_idx'
_PAN_INST = 'panoptic_segmentation_deeplab_instance_idx'
_PAN_META = 'panoptic_segmentation_deeplab_instance_meta'
_OUT_DTYPE = {LABEL_U8: torch.uint8, PANOPTIC_BGR: torch.uint8, SEM_INST_U16: torch.uint16,
              CLASS_SCORE_F32: torch.float32}


def get_fullres(d, key):
    """d[key + '_fullres'] when the dictionary has it, else d[key] (KeyError naming `key`)"""
    t = d.get(key + '_fullres')
    if t is None:
        t = d.get(key)
    if t is None:
        raise KeyError(f"'{key}' (nor '{key}_fullres') is not in the dictionary")
    return t


def _has(d, key):
    return d is not None and (torch.is_tensor(d.get(key + '_fullres')) or torch.is_tensor(d.get(key)))


def _map3(t, name, what, dtypes):
    """(N, h, w) device map of one of `dtypes` ((N, 1, h, w) is squeezed)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} must be a tensor")
    if not t.is_cuda:
        raise NotImplementedError(f"{name}: {what} is a CPU tensor; the outputs are packed on the GPU only")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"{name}: {what} has shape {tuple(t.shape)}; (N, h, w) maps only")
    if t.dtype not in dtypes:
        raise TypeError(f"{name}: {what} has dtype {t.dtype}; one of {', '.join(str(d) for d in dtypes)}")
    return t.contiguous()


class PackJob:
    """one job of `export_pack`: see emsa_export_pack in include/emsanet_hip.h.  src0 / src1 (N, h, w)
    device maps, dst the dense output, lut a uint8 device table or None (then lut_size > 0: identity
    with that bound; 0: no table), depth (N, H, W) uint16 / float32 with max_depth"""

    def __init__(self, kind, src0, dst, src1=None, lut=None, lut_size=0, add=0, divisor=0, depth=None,
                 max_depth=0.0):
        self.kind, self.src0, self.src1, self.dst = kind, src0, src1, dst
        self.lut, self.lut_size, self.add, self.divisor = lut, int(lut_size), int(add), int(divisor)
        self.depth, self.max_depth = depth, float(max_depth)


def _depth_code(depth, name):
    if depth.dtype in (torch.uint16, torch.int16):       # int16 storage of raw uint16 depth, as normalize_depth
        return _DEPTH_U16
    if depth.dtype == torch.float32:
        return _DEPTH_F32
    raise TypeError(f"{name}: the raw depth has dtype {depth.dtype}; uint16 or float32")


def export_pack(jobs, counters):
    """ONE launch of emsa_export_pack over `jobs` (<= 16 PackJob of equal output size); counters: int64
    (4,) device tensor, added to.  Nothing is copied, allocated or synchronised."""
    name = 'export_pack'
    if not 1 <= len(jobs) <= MAX_JOBS:
        raise ValueError(f"{name}: {len(jobs)} jobs; 1 ... {MAX_JOBS} per launch")
    if not torch.is_tensor(counters) or not counters.is_cuda or counters.dtype != torch.int64 or \
            counters.numel() != len(CAUSES) or not counters.is_contiguous():
        raise TypeError(f"{name}: counters must be a contiguous int64 ({len(CAUSES)},) tensor on the GPU")
    table = (EmsaExportJob * len(jobs))()
    shape = None
    for e, j in zip(table, jobs):
        src0 = _map3(j.src0, name, 'src0', tuple(_LABEL_DTYPES))
        n, h, w = src0.shape
        if j.kind not in _OUT_DTYPE:
            raise ValueError(f"{name}: unknown job kind {j.kind}")
        want = _OUT_DTYPE[j.kind]
        dst = j.dst
        if not torch.is_tensor(dst) or not dst.is_cuda or dst.dtype != want or not dst.is_contiguous():
            raise TypeError(f"{name}: dst must be a contiguous {want} tensor on the GPU")
        dims = tuple(dst.shape)
        if j.kind == PANOPTIC_BGR:
            if len(dims) != 4 or dims[3] != 3:
                raise ValueError(f"{name}: a BGR output is (N, H, W, 3), got {dims}")
            dims = dims[:3]
        if len(dims) != 3 or dims[0] != n or (shape is not None and dims != shape):
            raise ValueError(f"{name}: output {tuple(dst.shape)} against {shape or (n, 'H', 'W')}: the jobs of "
                             "one launch write (N, H, W) outputs of one size")
        shape = dims
        src1 = None
        if j.kind == CLASS_SCORE_F32:
            src1 = _map3(j.src1, name, 'src1 (score)', (torch.float32,))
        elif j.kind == SEM_INST_U16 or (j.kind == PANOPTIC_BGR and j.divisor == 0):
            src1 = _map3(j.src1, name, 'src1 (instance)', tuple(_LABEL_DTYPES))
        if src1 is not None and src1.shape != src0.shape:
            raise ValueError(f"{name}: src1 {tuple(src1.shape)} against src0 {tuple(src0.shape)}")
        if j.lut is not None:
            if not torch.is_tensor(j.lut) or not j.lut.is_cuda or j.lut.dtype != torch.uint8 or \
                    j.lut.dim() != 1 or not j.lut.is_contiguous():
                raise TypeError(f"{name}: lut must be a contiguous 1-D uint8 tensor on the GPU")
            if j.lut_size != j.lut.numel():
                raise ValueError(f"{name}: lut_size {j.lut_size} against a table of {j.lut.numel()}")
        depth = None
        if j.depth is not None:
            depth = _map3(j.depth, name, 'the raw depth', (torch.uint16, torch.int16, torch.float32))
            if tuple(depth.shape) != shape:
                raise ValueError(f"{name}: raw depth {tuple(depth.shape)} against the output {shape}")
            e.depth, e.depth_dtype, e.max_depth = depth.data_ptr(), _depth_code(depth, name), j.max_depth
        e.src0, e.src0_dtype = src0.data_ptr(), _LABEL_DTYPES[src0.dtype]
        if src1 is not None:
            e.src1 = src1.data_ptr()
            e.src1_dtype = _LABEL_DTYPES.get(src1.dtype, 0)
        e.lut = None if j.lut is None else j.lut.data_ptr()
        e.dst, e.divisor, e.kind = dst.data_ptr(), j.divisor, j.kind
        e.lut_size, e.add, e.h, e.w = j.lut_size, j.add, h, w
        j._keep = (src0, src1, depth)                     # contiguous copies live until the launch is queued
    check(_lib.lib().emsa_export_pack(table, len(jobs), shape[0], shape[1], shape[2], counters.data_ptr(),
                                      Fn._stream()), 'emsa_export_pack')


def _check_mapping(mapping):
    """the class table WITH void as a host uint8 array, or None"""
    if mapping is None:
        return None
    if torch.is_tensor(mapping):
        if mapping.dtype != torch.uint8:
            raise TypeError(f"semantic_class_mapping has dtype {mapping.dtype}; a uint8 table")
        mapping = mapping.detach().cpu().numpy()
    mapping = np.asarray(mapping)
    if mapping.dtype != np.uint8:
        raise TypeError(f"semantic_class_mapping has dtype {mapping.dtype}; a uint8 table")
    if mapping.ndim != 1 or mapping.size < 1:
        raise ValueError("semantic_class_mapping must be a 1-D table")
    return np.ascontiguousarray(mapping)


class PackedOutputs(dict):
    """what `pack` returns: key -> device tensor, and `turn`, the ring set the tensors belong to"""
    turn = 0


class HostOutputs(dict):
    """what `to_host` returns: key -> pinned host tensor (other entries passed through).  The copies are
    in flight until `event` has passed: `synchronize()` waits for it and returns the NumPy views."""
    event = None
    semantic_class_mapping = None

    def synchronize(self):
        if self.event is not None:
            self.event.synchronize()
        return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in self.items()}


class InstanceOutputs:
    """masks uint8 (total, H, W) on the device; lines[i]: the text lines of sample i; the planes of sample
    i are masks[start[i]:start[i + 1]], in the order of its lines"""

    def __init__(self, masks, lines, start):
        self.masks, self.lines, self.start = masks, lines, start

    def __iter__(self):
        return iter((self.masks, self.lines))


class InferenceOutputPacker:
    """see the module docstring.  semantic_class_mapping: uint8 table indexed by the class WITH void
    (ScanNet 20 -> benchmark ids, /root/reference/inference_dataset.py:647-650), None = identity;
    n_semantic_classes (with void; the packer is handed no label list, so it cannot know it otherwise), when
    given, is the length the table must at least have and a shorter table is refused here.  Without it a
    label beyond the table is found on the device: it packs as 0, is counted, and `check()` names it.
    shift: 1000 or 65536, the ground-truth encoding of `scannet-instance` (:340-346)."""

    def __init__(self, formats=FORMATS, max_instances_per_category=1000, semantic_class_mapping=None,
                 shift=1000, max_depth=None, write_ground_truth=False, instance_use_panoptic_score=True,
                 ring=2, n_semantic_classes=None):
        formats = (formats,) if isinstance(formats, str) else tuple(formats)
        for f in formats:
            if f not in FORMATS:
                raise ValueError(f"InferenceOutputPacker: unknown output format '{f}'; one of {FORMATS}")
        if shift not in (1000, 1 << 16):
            raise ValueError(f"InferenceOutputPacker: shift={shift}; 1000 or 65536 "
                             "(/root/reference/inference_dataset.py:346)")
        if int(max_instances_per_category) < 1 or int(ring) < 1:
            raise ValueError("InferenceOutputPacker: max_instances_per_category and ring must be >= 1")
        if max_depth is not None and not float(max_depth) == float(max_depth):
            raise ValueError("InferenceOutputPacker: max_depth is NaN")
        self.mapping = _check_mapping(semantic_class_mapping)
        if self.mapping is not None and n_semantic_classes is not None and \
                self.mapping.size < int(n_semantic_classes):
            raise ValueError(f"InferenceOutputPacker: semantic_class_mapping has {self.mapping.size} entries, "
                             f"the label list with void has {int(n_semantic_classes)}")
        self.formats = formats
        self.divisor = int(max_instances_per_category)
        self.shift = int(shift)
        self.max_depth = None if max_depth is None else float(max_depth)
        self.write_ground_truth = bool(write_ground_truth)
        self.instance_use_panoptic_score = bool(instance_use_panoptic_score)
        self.ring = int(ring)
        self._turn = -1
        self._buf = {}
        self._pinned = {}
        self._dev = {}

    # ---- device state --------------------------------------------------------------------------------
    def _state(self, device):
        """(counters, class table or None) on `device`, created in the first call"""
        key = str(device)
        st = self._dev.get(key)
        if st is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EmsaError("InferenceOutputPacker: first call for this device inside a stream "
                                     "capture: run pack() once before capturing")
            lut = None if self.mapping is None else torch.from_numpy(self.mapping).to(device)
            st = self._dev[key] = (Fn._zeros((len(CAUSES),), device, torch.int64), lut)
        return st

    def _out(self, turn, key, shape, dtype, device):
        k = (turn, key, tuple(shape), dtype, str(device))
        t = self._buf.get(k)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EmsaError(f"InferenceOutputPacker: no buffer for '{key}' {tuple(shape)} yet and "
                                     "the stream is capturing: run pack() `ring` times before capturing")
            t = self._buf[k] = Fn._empty(tuple(shape), device, dtype)
        return t

    def _lut(self, lut, bound):
        """(table, lut_size): the mapping, or the identity with `bound` (0 = no bound)"""
        return (lut, lut.numel()) if lut is not None else (None, bound)

    # ---- pack ----------------------------------------------------------------------------------------
    def _jobs(self, prediction, batch):
        """[(key, kind, {job arguments}, output (N, H, W) or None = the prediction's size)]"""
        name = 'InferenceOutputPacker.pack'
        label = tuple(_LABEL_DTYPES)

        def pred(key, dtypes=label):
            return _map3(get_fullres(prediction, key), name, f"prediction['{key}']", dtypes)

        def gt(key):
            return _map3(get_fullres(batch, key), name, f"batch['{key}']", label)

        depth = {}
        if self.max_depth is not None and self.write_ground_truth:
            raw = (batch.get('_no_preprocessing') or {}).get('depth') if batch is not None else None
            if raw is None:
                raise KeyError(f"{name}: max_depth is set but batch['_no_preprocessing']['depth'] is missing")
            depth = {'depth': raw, 'max_depth': self.max_depth}
        with_gt = self.write_ground_truth and batch is not None
        jobs = []
        if 'scannet-semantic' in self.formats:
            jobs.append(('scannet_semantic/pred_path_semantic', LABEL_U8,
                         dict(src0=pred('semantic_segmentation_idx'), add=1, bound=256), None))
            if _has(prediction, _PAN_SEM):
                jobs.append(('scannet_semantic/pred_path_panoptic_semantic', LABEL_U8,
                             dict(src0=pred(_PAN_SEM), bound=256), None))
            if with_gt and _has(batch, 'semantic'):
                s = gt('semantic')
                jobs.append(('scannet_semantic/gt_path', LABEL_U8, dict(src0=s, bound=256, **depth), s.shape))
        if 'scannet-panoptic' in self.formats:
            jobs.append(('scannet_panoptic/pred_path', PANOPTIC_BGR,
                         dict(src0=pred(_PAN_SEM), src1=pred(_PAN_INST), bound=0), None))
            if with_gt and _has(batch, 'panoptic'):
                p = gt('panoptic')
                jobs.append(('scannet_panoptic/gt_path', PANOPTIC_BGR,
                             dict(src0=p, divisor=self.divisor, bound=0, **depth), p.shape))
        if 'scannet-instance' in self.formats and with_gt and _has(batch, 'semantic') and \
                _has(batch, 'instance'):
            s, i = gt('semantic'), gt('instance')
            if self.shift == 1000:
                jobs.append(('scannet_instance/gt_path', SEM_INST_U16, dict(src0=s, src1=i, bound=256, **depth),
                             s.shape))
            else:
                jobs.append(('scannet_instance/gt_path', PANOPTIC_BGR, dict(src0=s, src1=i, bound=0, **depth),
                             s.shape))
        if 'mapping' in self.formats:
            f32 = (torch.float32,)
            score = self._score_key()
            jobs.append(('mapping/pred_semantic', CLASS_SCORE_F32,
                         dict(src0=pred('semantic_segmentation_idx'), add=1, bound=256,
                              src1=pred('semantic_segmentation_score', f32)), None))
            jobs.append(('mapping/pred_panoptic_semantic', CLASS_SCORE_F32,
                         dict(src0=pred(_PAN_SEM), bound=256,
                              src1=pred('panoptic_segmentation_deeplab_semantic_score', f32)), None))
            jobs.append(('mapping/pred_panoptic_instance', CLASS_SCORE_F32,
                         dict(src0=pred(_PAN_INST), src1=pred(score, f32), bound=0, no_lut=True), None))
        return jobs

    def _score_key(self):
        return 'panoptic_segmentation_deeplab_' + \
            ('panoptic_score' if self.instance_use_panoptic_score else 'instance_score')

    def _require(self, prediction, name):
        """the keys the formats read, checked before anything is launched"""
        need = [('scannet-semantic', 'semantic_segmentation_idx')]
        for f in ('scannet-panoptic', 'scannet-instance', 'mapping'):
            need += [(f, _PAN_SEM), (f, _PAN_INST)]
        need += [('mapping', k) for k in ('semantic_segmentation_idx', 'semantic_segmentation_score',
                                          'panoptic_segmentation_deeplab_semantic_score', self._score_key(),
                                          'scene_class_idx', 'scene_class_score')]
        for f, k in need:
            if f in self.formats and not _has(prediction, k):
                raise KeyError(f"{name}: format '{f}' needs prediction['{k}'] (an eval forward with "
                               "do_postprocessing=True; the panoptic keys need enable_panoptic)")

    def _build(self, prediction, batch, turn):
        """(outputs of ring set `turn`, job groups: one list of PackJob per output size, counters)"""
        name = 'InferenceOutputPacker.pack'
        self._require(prediction, name)
        full = _map3(get_fullres(prediction, 'semantic_segmentation_idx'), name,
                     "prediction['semantic_segmentation_idx']", tuple(_LABEL_DTYPES))
        dev = full.device
        counters, lut = self._state(dev)
        out, groups = PackedOutputs(), {}
        out.turn = turn
        for key, kind, a, shape in self._jobs(prediction, batch):
            shape = tuple(full.shape if shape is None else shape)
            dims = shape + (3,) if kind == PANOPTIC_BGR else shape
            dst = self._out(turn, key, dims, _OUT_DTYPE[kind], dev)
            table, size = (None, 0) if a.pop('no_lut', False) else self._lut(lut, a['bound'])
            a.pop('bound')
            groups.setdefault(shape, []).append(PackJob(kind, dst=dst, lut=table, lut_size=size, **a))
            out[key] = dst
        return out, list(groups.values()), counters

    def job_groups(self, prediction, batch=None):
        """the map jobs `pack` would launch next, as lists of `PackJob` (one list per output size, each at
        most one `export_pack` launch per 16 jobs) writing into the buffers of the ring set used last --
        for timing `emsa_export_pack` alone (tools/export_bench.py); the ring does not advance"""
        return self._build(prediction, batch, max(self._turn, 0))[1]

    def pack(self, prediction, batch=None):
        name = 'InferenceOutputPacker.pack'
        turn = (self._turn + 1) % self.ring
        out, groups, counters = self._build(prediction, batch, turn)
        self._turn = turn
        dev = counters.device
        for jobs in groups:
            for i in range(0, len(jobs), MAX_JOBS):
                export_pack(jobs[i:i + MAX_JOBS], counters)
        if 'mapping' in self.formats:
            for k in ('mapping/pred_semantic', 'mapping/pred_panoptic_semantic'):
                out[k] = out[k].unsqueeze(1)                   # "topk format (topk, h, w) with topk=1"
            idx, sc = prediction['scene_class_idx'], prediction['scene_class_score']
            if not (torch.is_tensor(idx) and idx.is_cuda and torch.is_tensor(sc) and sc.is_cuda):
                raise NotImplementedError(f"{name}: the scene prediction is not on the GPU")
            n = idx.numel()
            dst = self._out(turn, 'mapping/pred_scene', (1, 1, n), torch.float32, dev)
            export_pack([PackJob(CLASS_SCORE_F32, idx.reshape(1, 1, n), dst,
                                 src1=sc.reshape(1, 1, n) if sc.dtype == torch.float32
                                 else sc.float().reshape(1, 1, n))], counters)
            out['mapping/pred_scene'] = dst.view(n)
            if _PAN_META in prediction:
                out['mapping/pred_panoptic_instance_meta'] = prediction[_PAN_META]
        return out

    # ---- host side -----------------------------------------------------------------------------------
    def to_host(self, packed):
        """every tensor of `packed` into a pinned host buffer of this object (one per key and ring set: the
        set `packed` came from, so the host copy of call k stays valid until call k + ring is copied out)
        with one asynchronous copy each, and ONE event behind them: -> HostOutputs.
        Device and pinned buffers are kept per shape seen; `release()` drops them."""
        host = HostOutputs()
        host.semantic_class_mapping = self.mapping
        turn = getattr(packed, 'turn', max(self._turn, 0))
        for k, v in packed.items():
            if not torch.is_tensor(v):
                host[k] = v
                continue
            key = (turn, k, tuple(v.shape), v.dtype)
            p = self._pinned.get(key)
            if p is None:
                p = self._pinned[key] = torch.empty(tuple(v.shape), dtype=v.dtype, pin_memory=True)
            p.copy_(v, non_blocking=True)
            host[k] = p
        host.event = torch.cuda.Event()
        host.event.record()
        return host

    def release(self):
        """drop every device and pinned buffer (after a change of shapes; earlier results become invalid)"""
        self._buf.clear()
        self._pinned.clear()

    def check(self):
        """the one host read of the counters (it waits for the packing queued so far); raises ValueError
        naming every cause that fired, and starts counting afresh"""
        bad = []
        for counters, _ in self._dev.values():
            c = counters.cpu().tolist()
            if any(c):
                counters.zero_()
                bad += [f"{n} x {CAUSES[i]}" for i, n in enumerate(c) if n]
        if bad:
            raise ValueError("InferenceOutputPacker: values the output formats cannot hold: " + '; '.join(bad))

    # ---- scannet-instance prediction -----------------------------------------------------------------
    def instance_outputs(self, prediction, batch, basenames, output_size=None):
        """the `scannet-instance` prediction (/root/reference/inference_dataset.py:405-442) ->
        InstanceOutputs(masks, lines, start): one 0 / 255 plane (H, W) per instance that owns pixels, in
        ascending id order per sample, and per sample the lines
        'predicted_masks/<basename>_<rank:03d>.png <mapped class> <panoptic score:0.4f>\\n'.
        Class and score are those of the instance meta.  SYNCHRONISES: the instance count is read on the
        host to size the stack (the one such call of this module); `batch` is not read."""
        name = 'InferenceOutputPacker.instance_outputs'
        for k in (_PAN_INST, _PAN_META):
            if (k == _PAN_META and k not in prediction) or (k != _PAN_META and not _has(prediction, k)):
                raise KeyError(f"{name}: format 'scannet-instance' needs prediction['{k}']")
        inst = _map3(get_fullres(prediction, _PAN_INST), name, f"prediction['{_PAN_INST}']",
                     tuple(_LABEL_DTYPES))
        n, h, w = inst.shape
        if len(basenames) != n:
            raise ValueError(f"{name}: {len(basenames)} basenames for {n} samples")
        H, W = (h, w) if output_size is None else (int(output_size[0]), int(output_size[1]))
        dev = inst.device
        counters, lut = self._state(dev)
        meta = prediction[_PAN_META]
        tables = getattr(meta, 'device_tables', None)
        L = _lib.lib()
        if tables is not None:
            if tables.get('panoptic_score') is None:
                raise ValueError(f"{name}: the instance meta carries no panoptic score (compute_scores=False)")
            area, cls, score = (tables.get(k) for k in ('area', 'instance_class', 'panoptic_score'))
            for k, t, dt in (('area', area, torch.int32), ('instance_class', cls, torch.int32),
                             ('panoptic_score', score, torch.float32)):
                if not torch.is_tensor(t) or t.device != dev or t.dtype != dt or t.dim() != 2 or \
                        t.shape[0] != n or t.shape[1] < 2 or tuple(t.shape) != tuple(area.shape):
                    raise TypeError(f"{name}: device_tables['{k}'] must be a {dt} (N = {n}, slots >= 2) tensor "
                                    f"on {dev}, all three of one shape")
            area, cls = area.contiguous(), cls.contiguous()
            slots = area.shape[1]
            rank, by_rank, cls_by_rank = (Fn._empty((n, slots), dev, torch.int32) for _ in range(3))
            count, start = Fn._empty((n,), dev, torch.int32), Fn._empty((n + 1,), dev, torch.int32)
            table, size = self._lut(lut, 256)
            check(L.emsa_export_instance_ranks(area.data_ptr(), cls.data_ptr(), Fn._p(table), size, n, slots,
                                               rank.data_ptr(), by_rank.data_ptr(), cls_by_rank.data_ptr(),
                                               count.data_ptr(), start.data_ptr(), counters.data_ptr(),
                                               Fn._stream()), 'emsa_export_instance_ranks')
            start_h = start.cpu().numpy()                                   # <- the synchronisation
            ids_h, cls_h = by_rank.cpu().numpy(), cls_by_rank.cpu().numpy()
            score_h = tables['panoptic_score'].cpu().numpy()
            entries = [[(int(ids_h[i, r]), int(cls_h[i, r]), float(score_h[i, ids_h[i, r]]))
                        for r in range(int(start_h[i + 1] - start_h[i]))] for i in range(n)]
        else:
            # a plain list of dictionaries: the rank table is built here and uploaded
            entries = [instance_entries(m, self.mapping) for m in meta]
            if len(entries) != n:
                raise ValueError(f"{name}: {len(entries)} meta dictionaries for {n} samples")
            slots = max([2] + [e[-1][0] + 1 for e in entries if e])
            rank_h = np.full((n, slots), -1, np.int32)
            for i, e in enumerate(entries):
                for r, (j, _, _) in enumerate(e):
                    rank_h[i, j] = r
            count_h = np.array([len(e) for e in entries], np.int32)
            start_h = np.concatenate([[0], np.cumsum(count_h)]).astype(np.int32)
            rank, count, start = (torch.from_numpy(a).to(dev) for a in (rank_h, count_h, start_h))
        total = int(start_h[-1])
        masks = Fn._empty((total, H, W), dev, torch.uint8)
        check(L.emsa_export_instance_masks(inst.data_ptr(), _LABEL_DTYPES[inst.dtype], n, h, w, H, W,
                                           rank.data_ptr(), slots, count.data_ptr(), start.data_ptr(), total,
                                           Fn._p(masks) if total else None, Fn._stream()),
              'emsa_export_instance_masks')
        lines = [[instance_line(basenames[i], r, c, s) for r, (_, c, s) in enumerate(e)]
                 for i, e in enumerate(entries)]
        return InstanceOutputs(masks, lines, [int(v) for v in start_h])


def instance_entries(meta, mapping=None):
    """[(instance id, mapped class, panoptic score)] of one sample's meta dictionary, ascending ids,
    instances without pixels left out (/root/reference/inference_dataset.py:420-436)"""
    out = []
    for j in sorted(meta):
        m = meta[j]
        if m['area'] == 0:
            continue
        c = int(m['semantic_idx'])
        out.append((int(j), c if mapping is None else int(mapping[c]), float(m['panoptic_score'])))
    return out


def instance_line(basename, rank, semantic_idx, panoptic_score):
    """/root/reference/inference_dataset.py:429-439"""
    return f"predicted_masks/{basename}_{rank:03d}.png {semantic_idx} {panoptic_score:0.4f}\n"


def write_mapping_output(host, identifiers, output_path, compressed=True, semantic_class_mapping=None):
    """the `.npz` / `.json` tree of the `mapping` format (/root/reference/inference_dataset.py:456-552) from
    the `mapping/...` entries of `to_host(...)` (waited for here) or of a plain dict of arrays.
    identifiers[i]: the tuple of strings of sample i; its last element names the file, the others the
    directories.  The meta's 'semantic_idx' goes through the class mapping (that of the packer, when
    `host` came from one)."""
    mapping = _check_mapping(semantic_class_mapping)
    if mapping is None:
        mapping = getattr(host, 'semantic_class_mapping', None)
    arrays = host.synchronize() if hasattr(host, 'synchronize') else dict(host)
    save = np.savez_compressed if compressed else np.savez
    written = []
    for key in ('pred_semantic', 'pred_panoptic_semantic', 'pred_panoptic_instance', 'pred_scene'):
        a = arrays.get('mapping/' + key)
        if a is None:
            continue
        a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
        if len(identifiers) != a.shape[0]:
            raise ValueError(f"write_mapping_output: {len(identifiers)} identifiers for {a.shape[0]} samples")
        for i, ident in enumerate(identifiers):
            d = os.path.join(output_path, key, *ident[:-1])
            os.makedirs(d, exist_ok=True)
            fn = os.path.join(d, ident[-1] + '.npz')
            save(fn, a[i])
            written.append(fn)
    meta = arrays.get('mapping/pred_panoptic_instance_meta')
    if meta is not None:
        for i, ident in enumerate(identifiers):
            m = {int(k): dict(v) for k, v in meta[i].items()}
            for v in m.values():
                if 'semantic_idx' in v:                                   # instances with pixels
                    c = int(v['semantic_idx'])
                    v['semantic_idx'] = c if mapping is None else int(mapping[c])
            d = os.path.join(output_path, 'pred_panoptic_instance_meta', *ident[:-1])
            os.makedirs(d, exist_ok=True)
            fn = os.path.join(d, ident[-1] + '.json')
            with open(fn, 'w') as f:
                json.dump(m, f, sort_keys=True, indent=4)
            written.append(fn)
    return written
