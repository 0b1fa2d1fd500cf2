# -*- coding: utf-8 -*-
"""
Training targets on device: the `targets` dictionary of `emsanet_amd.loss.TrainingLosses` from the
raw label maps of a batch.

The reference builds these targets on the CPU inside its data-loader workers with four transforms of
the un-vendored `nicr_mt_scene_analysis` library (/root/reference/emsanet/preprocessing.py:89-104,
156-213): `InstanceClearStuffIDs`, `MultiscaleSupervisionGenerator`, `InstanceTargetGenerator` and
`OrientationTargetGenerator`.  `TrainingTargetGenerator.generate` replaces them with three kernel
launches for all scales (csrc/targets.hip), so a loader ships two small integer label maps instead of
five float / boolean maps at four scales.

Rules, per scale s (H_s = H / s, W_s = W / s); [U] = the un-vendored library is the only source and the
rule is restated here:
  down-scaling   the label at (y, x) of scale s is the label at (y * s, x * s): nearest neighbour as
                 `cv2.INTER_NEAREST` and torch 'nearest' agree on for integer factors.  [U]
  stuff clearing the instance id is 0 where `is_thing[semantic]` is false and on void
                 (preprocessing.py:89-104; `is_thing` is indexed by the label WITH void, 0 = void, as in
                 `metrics.panoptic_targets`); foreground = cleared id != 0.
  centres        per image, scale and remaining id: the mean of the instance's pixel coordinates AT
                 THAT SCALE, rounded half to even, exactly, in integers from count / sum_y / sum_x
                 (`int(round(mean))` of the Panoptic-DeepLab target generator).  [U]  An id without a
                 sampled pixel at a coarse scale has no centre there.
  center         (N,1,H_s,W_s) float32: max over the image's centres of exp(-d2 / (2 sigma_s^2)), d2 =
                 (y-cy)^2 + (x-cx)^2, 0 outside the window |y-cy|, |x-cx| <= 3 sigma_s + 1 ("a gauss up
                 to 3*sigma", /root/reference/emsanet/args.py:462-466; the + 1 is Panoptic-DeepLab's
                 6 sigma + 3 patch [U]).  sigma_1 = args.instance_center_sigma, sigma_s = (4 sigma) // s
                 (preprocessing.py:187-191).  d2 is an integer: the value comes from a table computed
                 in float64 and rounded to fp32 once, so the map is bit-exact and exactly 1.0 at a centre.
  offset         (N,2,H_s,W_s) float32 (dy, dx), channels-last strides: on the foreground (cy - y) / H_s,
                 (cx - x) / W_s for the 'tanh' and 'relative' encodings (normalized_offset,
                 preprocessing.py:193-197; the inverse of `postprocessing.instance_assign`), cy - y, cx - x
                 in pixels for 'deeplab'; 0 elsewhere.  One fp32 division of an exact integer.
  orientation    (N,H_s,W_s) float32: `orientations[image, id]` of the pixel's instance, 0 where it has
                 none (no instance, or NaN); orientation_foreground = foreground &
                 use_orientation[semantic] & the angle is not NaN (preprocessing.py:206-213).  [U]
  semantic       (N,H_s,W_s) int64, the down-scaled label, unchanged by the stuff clearing.
  scene          passed through as int64.
  normal         (N,3,H_s,W_s) float32 over (N,H_s,W_s,3) memory, from batch['normal'] -- float32
                 (N,H,W,3) or (N,3,H,W), channel 0 the image-x component, (0,0,0) = invalid: the vector at
                 (y, x) of scale s is the full-resolution vector at (y * s, x * s), copied bit for bit (the
                 nearest rule of the label maps), so its validity is that of the sampled vector.  Nothing is
                 interpolated or re-normalised.  One more launch (csrc/normal.hip).  [U]
`center_mask` is not produced (the loss takes None).
"""
import numpy as np
import torch

from . import _lib
from ._lib import EmsaNormalScale, EmsaTargetScale, check
from . import functional as Fn
from .functional import _stream
from .postprocessing import normal_map, thing_table

_LABEL_DTYPES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2, torch.int16: 3, torch.uint16: 4}   # EMSA_LABEL_*
MAX_INSTANCES = 1024
MAX_SIGMA = 16
DEFAULT_SCALES = (1, 32, 16, 8)      # the order TrainingLosses documents: full, then /32, /16, /8
N_LAUNCHES = 3
N_NORMAL_LAUNCHES = 1                # on top, with the normal task


def scale_sigma(sigma, scale):
    """sigma of the heat map at `scale` (/root/reference/emsanet/preprocessing.py:187-191)"""
    return int(sigma) if scale == 1 else (4 * int(sigma)) // scale


def gauss_table(sigma):
    """float32 [2 (3 sigma + 1)^2 + 1]: exp(-d2 / (2 sigma^2)) in float64, rounded once"""
    r = 3 * sigma + 1
    d2 = np.arange(2 * r * r + 1, dtype=np.float64)
    return np.exp(-d2 / (2.0 * sigma * sigma)).astype(np.float32)


def orientation_table(list_of_dicts, max_instances=256):
    """the reference's per-sample {instance id: angle in rad} dictionaries -> float32
    (N, max_instances) table indexed by the id, NaN = this instance has no orientation; in pinned host
    memory where a GPU is present, so `BatchStager` can copy it asynchronously"""
    table = torch.full((len(list_of_dicts), int(max_instances)), float('nan'), dtype=torch.float32)
    for i, d in enumerate(list_of_dicts):
        for k, v in d.items():
            k = int(k)
            if not 0 < k < max_instances:
                raise ValueError(f"orientation_table: instance id {k} outside (0, {max_instances})")
            table[i, k] = float(v)
    return table.pin_memory() if torch.cuda.is_available() else table


class TrainingTargetGenerator:
    """`generate(batch)` -> the `targets` dictionary of `TrainingLosses.forward(outputs, targets)`.

    args: `tasks`, `instance_center_sigma`, `instance_offset_encoding`,
    `semantic_no_multiscale_supervision`, `instance_no_multiscale_supervision`,
    `normal_no_multiscale_supervision` (with a switch set that task gets its full-scale entry only).
    With the 'normal' task and a batch that carries 'normal', `targets['normal']` is the list of the
    down-scaled maps.  is_thing / use_orientation: per class, indexed by the label
    WITH void.  scales: the first is the full resolution, then the side outputs in the decoder's order.
    max_instances bounds the instance ids: [0, max_instances), at most 1024.  ring: the outputs and the
    workspace rotate over that many sets, so the targets of the previous ring - 1 calls stay valid.

    `generate` only launches kernels on the current stream: no host copy, no synchronisation, and no
    allocation after the first call for a shape, so it can be captured into a graph (call it once
    before capturing).  An id outside [0, max_instances), a negative label or a label outside the
    is_thing table counts as "no instance" and makes `check()` -- the one host read -- raise."""

    def __init__(self, args, is_thing, use_orientation=None, scales=DEFAULT_SCALES, max_instances=256,
                 ring=2):
        tasks = tuple(args.tasks)
        self.with_semantic = 'semantic' in tasks
        self.with_instance = 'instance' in tasks or 'orientation' in tasks
        self.with_orientation = 'orientation' in tasks
        self.with_scene = 'scene' in tasks
        self.with_normal = 'normal' in tasks
        self.is_thing = tuple(bool(t) for t in is_thing)
        if use_orientation is None:
            use_orientation = [False] * len(self.is_thing)
        self.use_orientation = tuple(bool(t) for t in use_orientation)
        if len(self.use_orientation) != len(self.is_thing) or not self.is_thing:
            raise ValueError("TrainingTargetGenerator: is_thing and use_orientation must name every class, "
                             "void included")
        self.scales = tuple(int(s) for s in scales)
        if not self.scales or self.scales[0] != 1 or any(s < 1 for s in self.scales) or \
                len(self.scales) > 8:
            raise ValueError(f"TrainingTargetGenerator: scales={scales}; 1 to 8 scales, the full resolution "
                             "(1) first")
        if not 2 <= int(max_instances) <= MAX_INSTANCES:
            raise ValueError(f"TrainingTargetGenerator: max_instances={max_instances} outside "
                             f"[2, {MAX_INSTANCES}]")
        if ring < 1:
            raise ValueError("TrainingTargetGenerator: ring must be >= 1")
        self.max_instances = int(max_instances)
        self.ring = int(ring)
        self.sigma = int(args.instance_center_sigma)
        self.normalized_offset = args.instance_offset_encoding in ('relative', 'tanh')
        sem_ms = not args.semantic_no_multiscale_supervision
        inst_ms = not args.instance_no_multiscale_supervision
        # (scale, sigma or 0, semantic wanted, instance wanted) of every scale with an output
        self.plan = []
        for i, s in enumerate(self.scales):
            sem = self.with_semantic and (i == 0 or sem_ms)
            inst = self.with_instance and (i == 0 or inst_ms)
            if not (sem or inst):
                continue
            sg = scale_sigma(self.sigma, s) if inst else 0
            if inst and not 1 <= sg <= MAX_SIGMA:
                raise ValueError(f"TrainingTargetGenerator: sigma_{s} = {sg} (instance_center_sigma = "
                                 f"{self.sigma}) outside [1, {MAX_SIGMA}]")
            self.plan.append((s, sg, sem, inst))
        normal_ms = not getattr(args, 'normal_no_multiscale_supervision', False)
        self.normal_scales = tuple(s for i, s in enumerate(self.scales) if i == 0 or normal_ms) \
            if self.with_normal else ()
        self._tables = {}            # device -> (is_thing, use_orientation, gauss tables, flags)
        self._rings = {}             # (device, N, H, W) -> [next slot, slots]
        self._last = None

    # -- per-device constants, uploaded once (not inside a stream capture) ---------------------------
    def _constants(self, device):
        c = self._tables.get(device)
        if c is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EmsaError("TrainingTargetGenerator: first call inside a stream capture; call "
                                     "generate once before capturing")
            tabs = [gauss_table(sg) for _s, sg, _sem, inst in self.plan if inst]
            gauss = torch.from_numpy(np.concatenate(tabs)).to(device) if tabs else None
            c = self._tables[device] = (thing_table(self.is_thing, device),
                                        thing_table(self.use_orientation, device), gauss,
                                        Fn._zeros((2,), device, torch.int32))
        return c

    def _slots(self, device, n, h, w):
        key = (device, n, h, w)
        r = self._rings.get(key)
        if r is not None:
            return r
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EmsaError("TrainingTargetGenerator: first call for this shape inside a stream "
                                 "capture; call generate once before capturing")
        L = _lib.lib()
        slots = []
        for _ in range(self.ring):
            desc = (EmsaTargetScale * len(self.plan))()
            sem_out, inst_out = [], []
            for e, (s, sg, sem, inst) in zip(desc, self.plan):
                hs, ws = h // s, w // s
                e.scale, e.sigma = s, sg
                if sem:
                    t = Fn._empty((n, hs, ws), device, torch.int64)
                    e.semantic = t.data_ptr()
                    sem_out.append(t)
                if inst:
                    d = {'center': Fn._empty((n, 1, hs, ws), device, torch.float32),
                         # (N,2,H_s,W_s) with channels-last strides: the loss's permute is a view
                         'offset': Fn._empty((n, hs, ws, 2), device, torch.float32).permute(0, 3, 1, 2),
                         'foreground': Fn._empty((n, hs, ws), device, torch.bool)}
                    e.center, e.offset = d['center'].data_ptr(), d['offset'].data_ptr()
                    e.foreground = d['foreground'].data_ptr()
                    if self.with_orientation:
                        d['orientation'] = Fn._empty((n, hs, ws), device, torch.float32)
                        d['orientation_foreground'] = Fn._empty((n, hs, ws), device, torch.bool)
                        e.orientation = d['orientation'].data_ptr()
                        e.orientation_foreground = d['orientation_foreground'].data_ptr()
                    inst_out.append(d)
            nbytes = L.emsa_targets_workspace_bytes(n, len(self.plan), self.max_instances) if self.plan else 0
            slots.append({'desc': desc, 'semantic': sem_out, 'instance': inst_out,
                          'ws': Fn._zeros((nbytes,), device, torch.uint8),
                          'scene': Fn._empty((n,), device, torch.int64)})
            if self.with_normal:
                ndesc = (EmsaNormalScale * len(self.normal_scales))()
                normal_out = []
                for e, s in zip(ndesc, self.normal_scales):
                    # (N,3,H_s,W_s) with channels-last strides, like 'offset'
                    t = Fn._empty((n, h // s, w // s, 3), device, torch.float32)
                    e.scale, e.out = s, t.data_ptr()
                    normal_out.append(t.permute(0, 3, 1, 2))
                slots[-1].update(normal_desc=ndesc, normal=normal_out)
        r = self._rings[key] = [0, slots]
        return r

    @staticmethod
    def _label_map(batch, key):
        t = batch.get(key)
        if not torch.is_tensor(t):
            raise TypeError(f"TrainingTargetGenerator.generate: batch['{key}'] must be a tensor")
        if not t.is_cuda:
            raise NotImplementedError(f"TrainingTargetGenerator.generate: batch['{key}'] is a CPU tensor; "
                                      "the targets are generated on the GPU only")
        if t.dtype not in _LABEL_DTYPES:
            raise TypeError(f"TrainingTargetGenerator.generate: batch['{key}'] has dtype {t.dtype}; "
                            "int64, int32, int16, uint16 or uint8 label maps only")
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError(f"TrainingTargetGenerator.generate: batch['{key}'] must be a contiguous "
                             f"(N, H, W) map, got {tuple(t.shape)}")
        return t

    def check_size(self, h, w):
        """ValueError unless every scale divides the map size"""
        for s in self.scales:
            if h % s or w % s:
                raise ValueError(f"TrainingTargetGenerator: {h}x{w} is not divisible by the scale {s}")

    def generate(self, batch):
        sem = batch.get('semantic')
        if torch.is_tensor(sem) and sem.dim() == 3:
            self.check_size(*sem.shape[1:])
        sem = self._label_map(batch, 'semantic')
        n, h, w = sem.shape
        device = sem.device
        inst = orient = None
        if self.with_instance:
            inst = self._label_map(batch, 'instance')
            if inst.shape != sem.shape or inst.device != device:
                raise ValueError(f"TrainingTargetGenerator.generate: semantic {tuple(sem.shape)} vs "
                                 f"instance {tuple(inst.shape)}")
        if self.with_orientation:
            orient = batch.get('orientations')
            if not torch.is_tensor(orient) or not orient.is_cuda:
                raise NotImplementedError("TrainingTargetGenerator.generate: batch['orientations'] must "
                                          "be a tensor on the GPU (see orientation_table)")
            if orient.dtype != torch.float32 or tuple(orient.shape) != (n, self.max_instances) or \
                    not orient.is_contiguous():
                raise ValueError("TrainingTargetGenerator.generate: batch['orientations'] must be a "
                                 f"contiguous float32 ({n}, {self.max_instances}) table")
        scene = batch.get('scene')
        if self.with_scene and (not torch.is_tensor(scene) or not scene.is_cuda or
                                tuple(scene.shape) != (n,)):
            raise NotImplementedError("TrainingTargetGenerator.generate: batch['scene'] must be an (N,) "
                                      "tensor on the GPU")
        normal = None
        if self.with_normal and batch.get('normal') is not None:
            normal, normal_chw, shape = normal_map(batch['normal'], 'TrainingTargetGenerator.generate',
                                                   "batch['normal']")
            if shape != (n, h, w) or normal.device != device:
                raise ValueError(f"TrainingTargetGenerator.generate: semantic {tuple(sem.shape)} vs "
                                 f"normal {tuple(batch['normal'].shape)}")
        is_thing, use_orientation, gauss, flags = self._constants(device)
        ring = self._slots(device, n, h, w)
        slot = ring[1][ring[0]]
        ring[0] = (ring[0] + 1) % self.ring
        self._last = (slot, n)

        out = {}
        if self.plan:
            L, st = _lib.lib(), _stream()
            desc, k, m = slot['desc'], len(self.plan), self.max_instances
            sd = _LABEL_DTYPES[sem.dtype]
            ip, idt = (inst.data_ptr(), _LABEL_DTYPES[inst.dtype]) if inst is not None else (None, 0)
            ws = slot['ws'].data_ptr()
            if self.with_instance:
                check(L.emsa_targets_stats(sem.data_ptr(), sd, ip, idt, is_thing.data_ptr(),
                                           len(self.is_thing), n, h, w, desc, k, m, ws, st),
                      'emsa_targets_stats')
                check(L.emsa_targets_finalize(n, h, w, desc, k, m, ws, st), 'emsa_targets_finalize')
            check(L.emsa_targets_render(sem.data_ptr(), sd, ip, idt,
                                        orient.data_ptr() if orient is not None else None,
                                        is_thing.data_ptr(), use_orientation.data_ptr(),
                                        len(self.is_thing), n, h, w, desc, k, m,
                                        1 if self.normalized_offset else 0,
                                        gauss.data_ptr() if gauss is not None else None, ws,
                                        flags.data_ptr(), st), 'emsa_targets_render')
        if self.with_semantic:
            out['semantic'] = list(slot['semantic'])
        if self.with_instance:
            out['instance'] = [dict(d) for d in slot['instance']]
        if normal is not None:
            check(_lib.lib().emsa_normal_targets(normal.data_ptr(), 1 if normal_chw else 0, n, h, w,
                                                 slot['normal_desc'], len(self.normal_scales), _stream()),
                  'emsa_normal_targets')
            out['normal'] = list(slot['normal'])
        if self.with_scene:
            out['scene'] = slot['scene']
            out['scene'].copy_(scene)         # (a copy: the caller may refill its buffer)
        return out

    def last_centers(self):
        """the centres behind the targets of the last `generate`: per scale with instance targets an
        int32 (N, max_instances, 2) device tensor (cy, cx) indexed by the instance id, -1 = the id has
        no centre at that scale (torch operators on the workspace: not for the training loop)"""
        slot, n = self._last
        k, m = len(self.plan), self.max_instances
        first = (k * n * 3 * m * 8 + k * n * m * 4) // 4          # csrc/targets.hip: acc | list | centre_of
        packed = slot['ws'].view(torch.int32)[first:first + k * n * m].view(k, n, m)
        out = []
        for z, (_s, _sg, _sem, inst) in enumerate(self.plan):
            if inst:
                p = packed[z]
                out.append(torch.where(p.unsqueeze(-1) < 0, p.unsqueeze(-1).expand(n, m, 2),
                                       torch.stack([p >> 16, p & 0xFFFF], -1)))
        return out

    def check(self):
        """the one host read: raises ValueError if any call since the last check saw an instance id
        outside [0, max_instances) or a semantic label outside the is_thing table (such pixels were
        treated as carrying no instance)"""
        for flags in [c[3] for c in self._tables.values()]:
            bad_id, bad_label = (int(v) for v in flags.cpu())
            if bad_id or bad_label:
                flags.zero_()
                what = []
                if bad_id:
                    what.append(f"an instance id outside [0, {self.max_instances})")
                if bad_label:
                    what.append(f"a semantic label outside [0, {len(self.is_thing)})")
                raise ValueError("TrainingTargetGenerator: " + " and ".join(what) + " since the last check")
