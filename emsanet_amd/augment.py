# -*- coding: utf-8 -*-
"""
Training augmentation on device: the random part of the reference's training preprocessor
(/root/reference/emsanet/preprocessing.py:106-123) -- `RandomResize(aug_scale_min, aug_scale_max)`,
`RandomCrop(input_height, input_width)`, `RandomHSVJitter(10/180, 20/255, 50/255)`,
`RandomHorizontalFlip(0.5)` -- fused with `NormalizeRGB` / `NormalizeDepth` + HWC->CHW
(preprocessing.py:216-226).  `TrainingAugmenter.apply` replaces them with two kernel launches for the
whole batch and all of its maps (one more with an orientation table, one more with a normal map;
csrc/augment.hip, csrc/normal.hip), so a loader ships un-augmented raw frames.  `resize_normalize` is
the deterministic validation twin (`Resize(validation_input_height, validation_input_width)`,
preprocessing.py:147-154).

Rules; [U] = the un-vendored `nicr_mt_scene_analysis` library / cv2 is the only source and the rule is
restated here (tests/augment_reference.py is the NumPy restatement):

One output pixel (y, x) of the H x W crop of sample i comes from the source frame Hs x Ws through the
sample's parameter row (Hr, Wr, cy, cx, flip, dh, ds, dv).

  composed index  xr = cx + (W-1-x if flip else x), yr = cy + y: coordinates in the virtually resized
                  frame Hr x Wr, which is never materialised.
  RGB             bilinear with half-pixel centres, in integers only.  Per axis, for the coordinate X of
                  n_out mapped onto n_in: t = (2 X + 1) n_in - n_out, d = 2 n_out, i0 = floor(t / d),
                  r = t - i0 d; the weight of i0 + 1 is a = (r * 2048 + n_out) // d in 0 ... 2048, that of
                  i0 is 2048 - a; both indices are clamped to [0, n_in - 1].  value = (sum of the four
                  u8 * wy * wx + 2^21) >> 22, a uint8.  No float appears: bit-exact by construction, the
                  identity at Hr = Hs, Wr = Ws.  Against Pillow's Image.resize(BILINEAR): equal at scale
                  1, within 1 grey level elsewhere (Pillow rounds between its two passes).  [U] relative
                  to cv2.INTER_LINEAR.
  depth, labels   nearest: i = (X * n_in) // n_out per axis; values are copied unchanged, so invalid
                  depth zeros stay zero and no label is invented.  [U] relative to cv2.INTER_NEAREST.
  HSV jitter      on the resized uint8 RGB, in fp32: r, g, b = u8 / 255; v = max, c = v - min, s = c / v
                  (0 where v = 0); h in [0, 6): 0 where c = 0, else ((g - b) / c) mod 6 where v = r,
                  (b - r) / c + 2 where v = g, (r - g) / c + 4 otherwise.  h' = (h + 6 dh) mod 6,
                  s' = clip(s + ds, 0, 1), v' = clip(v + dv, 0, 1); back to RGB as
                  channel_n = v' - v' s' clip(min(k, 4 - k), 0, 1), k = (n + h') mod 6, n = 5, 3, 1 for
                  r, g, b.  dh is a fraction of the full hue circle, ds and dv fractions of the unit range
                  [U].  The result is NOT re-quantised to 8 bits (a stated deviation from the reference's
                  uint8 round trip: finer, loses nothing).  With all three amplitudes 0 the stage is
                  compiled out and the output is bit-equal to `normalize_rgb` of the resized uint8 values.
  normalisation   the expressions of `postprocessing.normalize_rgb` / `normalize_depth`: float32
                  (N,3,H,W) and (N,1,H,W), what the model takes.
  orientations    for a flipped sample theta -> (2 pi - theta) mod 2 pi in [0, 2 pi), in fp32 with
                  2 pi = 6.2831855: a = 2pi - theta; a -= 2pi * floor(a / 2pi); a += 2pi if a < 0;
                  a -= 2pi if a >= 2pi.  NaN stays NaN.  [U]
  normals         with `with_normal=True`: float32 (N,Hs,Ws,3) or (N,3,Hs,Ws), channel 0 the image-x
                  component, (0,0,0) = invalid.  The composed index and the nearest rule of depth and the
                  labels; values are copied, and channel 0 is negated on a flipped sample.  Nothing is
                  interpolated or re-normalised, so an invalid pixel stays (+-0, 0, 0): still invalid.
                  One more launch (csrc/normal.hip).  [U]
  scene           passes through.  Without `with_normal=True` the 'normal' task is refused (a flip has to
                  negate a component: the caller opts in to the rule above).

Parameters are counter-based and integer, so the NumPy restatement reproduces them bit for bit:
  hash            lowbias32(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
                  (all mod 2^32; the mixer of the dropout masks).  hash(seed, step, sample, draw) =
                  L(L(L(L(seed + 0x9E3779B9) + step) + sample) + draw).
  uniform [0, n)  (hash * n) >> 32 with a 64-bit product.
  draws           0: q, the scale numerator (scale = q / 1024), uniform in [round(min * 1024),
                  round(max * 1024)]; Hr = (Hs q + 512) >> 10, Wr = (Ws q + 512) >> 10.  1: cy uniform in
                  [0, Hr - H].  2: cx uniform in [0, Wr - W].  3: flip = hash < round(p * 2^32).
                  4, 5, 6: dh, ds, dv = float(int(2 u - 2^24)) * float32(amplitude / 2^24), u = hash >> 8.
  refused         ValueError: Hr < H or Wr < W at the smallest scale (the reference's behaviour there is
                  unknown: no padding rule is guessed); H, W, Hs, Ws above 4096 or a resized side above
                  16384 (the integer products above stay below 2^31).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check
from . import functional as Fn
from .functional import _stream
from .postprocessing import RGB_MEAN, RGB_STD, normal_map

_LABEL_DTYPES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2, torch.int16: 3, torch.uint16: 4}   # EMSA_LABEL_*
MAX_SIDE = 4096
MAX_RESIZED = 16384
DEFAULT_HSV_JITTER = (10 / 180, 20 / 255, 50 / 255)      # preprocessing.py:117-121
_WHO = 'TrainingAugmenter'


def scale_numerators(scale_min, scale_max):
    """(q_min, q_max): the scale range in 1/1024 steps"""
    q_min, q_max = int(round(float(scale_min) * 1024)), int(round(float(scale_max) * 1024))
    if q_min < 1 or q_max < q_min:
        raise ValueError(f"{_WHO}: scale range [{scale_min}, {scale_max}]")
    return q_min, q_max


def resized_size(hs, ws, q):
    return (hs * q + 512) >> 10, (ws * q + 512) >> 10


class TrainingAugmenter:
    """`apply(batch)`: raw device tensors in, an augmented and normalised batch out.

    args: `input_height`, `input_width`, `aug_scale_min`, `aug_scale_max`, `input_modalities`, `tasks`.
    depth_stats = (mean, std) of the depth normalisation.  hsv_jitter: the amplitudes of (dh, ds, dv);
    all three 0 removes the stage.  flip_p: the probability of a flip.  ring: the outputs rotate over
    that many sets, so the results of the previous ring - 1 calls stay valid.  with_normal: augment
    batch['normal'] too when 'normal' is in `tasks` (refused otherwise).

    batch: 'rgb' uint8 (N,Hs,Ws,3) and / or 'depth' uint16 (N,Hs,Ws) as `input_modalities` says,
    'semantic' (with the semantic task) and 'instance' (instance / orientation) label maps (N,Hs,Ws) of
    int64, int32, int16, uint16 or uint8, 'orientations' float32 (N, max_instances) (orientation),
    'scene' (N,), 'normal' float32 (N,Hs,Ws,3) or (N,3,Hs,Ws) (with_normal) -- all on the GPU.
    Returned: 'rgb' float32 (N,3,H,W), 'depth' float32 (N,1,H,W), the label maps (N,H,W) in their own
    type, the orientation table, 'scene' and 'normal' float32 (N,3,H,W) over (N,H,W,3) memory, ready for
    `EMSANet.forward` and `TrainingTargetGenerator.generate`.

    `apply` only launches kernels on the current stream: no host copy, no synchronisation and no
    allocation after the first call for a shape, so it can be captured into a graph (call it once
    before capturing); the step counter lives on the device and the draw kernel advances it, so every
    replay draws fresh parameters."""

    def __init__(self, args, depth_stats=(0.0, 1.0), seed=0, hsv_jitter=DEFAULT_HSV_JITTER, flip_p=0.5,
                 ring=2, with_normal=False):
        tasks = tuple(args.tasks)
        if 'normal' in tasks and not with_normal:
            raise NotImplementedError(f"{_WHO}: the 'normal' task is not augmented (a horizontal flip "
                                      "would have to negate a component of the normals)")
        self.height, self.width = int(args.input_height), int(args.input_width)
        self.q_min, self.q_max = scale_numerators(args.aug_scale_min, args.aug_scale_max)
        self.modalities = tuple(args.input_modalities)
        self.with_semantic = 'semantic' in tasks
        self.with_instance = 'instance' in tasks or 'orientation' in tasks
        self.with_orientation = 'orientation' in tasks
        self.with_scene = 'scene' in tasks
        self.with_normal = 'normal' in tasks and bool(with_normal)
        self.depth_stats = (float(depth_stats[0]), float(depth_stats[1]))
        self.hsv_jitter = tuple(float(a) for a in hsv_jitter)
        if len(self.hsv_jitter) != 3 or any(not 0.0 <= a <= 1.0 for a in self.hsv_jitter):
            raise ValueError(f"{_WHO}: hsv_jitter={hsv_jitter}; three amplitudes in [0, 1]")
        if not 0.0 <= float(flip_p) <= 1.0:
            raise ValueError(f"{_WHO}: flip_p={flip_p}")
        self.flip_threshold = int(round(float(flip_p) * 2 ** 32))
        if ring < 1:
            raise ValueError(f"{_WHO}: ring must be >= 1")
        self.ring = int(ring)
        if self.height < 1 or self.width < 1 or self.height > MAX_SIDE or self.width > MAX_SIDE:
            raise ValueError(f"{_WHO}: crop {self.height}x{self.width}; sides in [1, {MAX_SIDE}]")
        self._seed, self._step = int(seed) & 0xFFFFFFFF, 0
        self._state = {}             # device -> int32[2] {seed, step}
        self._rings = {}             # key -> [next slot, slots]
        self._identity = {}          # (device, n, h, w) -> the table of resize_normalize
        self._last = None
        self._mean = (ctypes.c_float * 3)(*RGB_MEAN)
        self._std = (ctypes.c_float * 3)(*RGB_STD)

    # -- host checks ---------------------------------------------------------------------------------
    def check_size(self, hs, ws):
        """ValueError unless source frames of hs x ws can be augmented to the crop"""
        if not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE):
            raise ValueError(f"{_WHO}: source frames of {hs}x{ws}; sides in [1, {MAX_SIDE}]")
        hr, wr = resized_size(hs, ws, self.q_min)
        if hr < self.height or wr < self.width:
            raise ValueError(f"{_WHO}: at the smallest scale {self.q_min}/1024 a {hs}x{ws} frame is resized "
                             f"to {hr}x{wr}, smaller than the {self.height}x{self.width} crop")
        hr, wr = resized_size(hs, ws, self.q_max)
        if hr > MAX_RESIZED or wr > MAX_RESIZED:
            raise ValueError(f"{_WHO}: at the largest scale {self.q_max}/1024 a {hs}x{ws} frame is resized "
                             f"to {hr}x{wr}; sides up to {MAX_RESIZED}")

    def _inputs(self, batch, who):
        """the tensors the configuration asks for, checked: (rgb, depth, [labels], orientations, scene,
        n, hs, ws, maps, normal); normal = (tensor, chw flag) or None"""
        def tensor(key):
            t = batch.get(key)
            if not torch.is_tensor(t):
                raise TypeError(f"{who}: batch['{key}'] must be a tensor")
            return t

        rgb = depth = orient = scene = normal = None
        shape = None
        maps = []

        def same(key, t):
            nonlocal shape
            s = tuple(t.shape[:3])
            if t.dim() < 3 or (shape is not None and s != shape):
                raise ValueError(f"{who}: batch['{key}'] has shape {tuple(t.shape)}, the other maps {shape}")
            shape = s

        if 'rgb' in self.modalities:
            rgb = tensor('rgb')
            if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3:
                raise TypeError(f"{who}: batch['rgb'] must be a uint8 (N, H, W, 3) tensor")
            same('rgb', rgb)
            maps.append(('rgb', rgb))
        if 'depth' in self.modalities:
            depth = tensor('depth')
            if depth.dtype not in (torch.uint16, torch.int16) or depth.dim() != 3:
                raise TypeError(f"{who}: batch['depth'] must be a uint16 (N, H, W) tensor")
            same('depth', depth)
            maps.append(('depth', depth))
        labels = []
        for key, wanted in (('semantic', self.with_semantic), ('instance', self.with_instance)):
            if not wanted:
                continue
            t = tensor(key)
            if t.dtype not in _LABEL_DTYPES or t.dim() != 3:
                raise TypeError(f"{who}: batch['{key}'] has dtype {t.dtype} and shape {tuple(t.shape)}; "
                                "int64, int32, int16, uint16 or uint8 (N, H, W) label maps only")
            same(key, t)
            labels.append((key, t))
            maps.append((key, t))
        if self.with_normal:
            t, chw, s = normal_map(batch.get('normal'), who, "batch['normal']",
                                   hw=None if shape is None else shape[1:])
            if shape is not None and s != shape:
                raise ValueError(f"{who}: batch['normal'] has shape {tuple(t.shape)}, the other maps {shape}")
            shape = s
            normal = (t, chw)
            # (contiguous itself, or a channels-last view of contiguous (N,H,W,3) memory)
            maps.append(('normal', t if t.is_contiguous() else t.permute(0, 2, 3, 1)))
        if shape is None:
            raise ValueError(f"{who}: neither an input modality nor a label map to work on")
        n, hs, ws = shape
        if self.with_orientation:
            orient = tensor('orientations')
            if orient.dtype != torch.float32 or orient.dim() != 2 or orient.shape[0] != n:
                raise ValueError(f"{who}: batch['orientations'] must be a float32 ({n}, max_instances) table")
            maps.append(('orientations', orient))
        if self.with_scene:
            scene = tensor('scene')
            if tuple(scene.shape) != (n,):
                raise ValueError(f"{who}: batch['scene'] must be an ({n},) tensor")
            maps.append(('scene', scene))
        return rgb, depth, labels, orient, scene, n, hs, ws, maps, normal

    @staticmethod
    def _on_device(maps, who):
        device = None
        for key, t in maps:
            if not t.is_cuda:
                raise NotImplementedError(f"{who}: batch['{key}'] is a CPU tensor; the augmentation runs "
                                          "on the GPU only")
            if not t.is_contiguous():
                raise ValueError(f"{who}: batch['{key}'] must be contiguous")
            if device is not None and t.device != device:
                raise ValueError(f"{who}: batch['{key}'] is on {t.device}, other entries on {device}")
            device = t.device
        return device

    # -- device state and outputs, created once (not inside a stream capture) --------------------------
    @staticmethod
    def _no_capture(what):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EmsaError(f"{_WHO}: first call {what} inside a stream capture; call it once before "
                                 "capturing")

    def _device_state(self, device):
        s = self._state.get(device)
        if s is None:
            self._no_capture('on this device')
            host = np.array([self._seed, self._step], dtype=np.uint32).view(np.int32)
            s = self._state[device] = torch.from_numpy(host).to(device)
        return s

    def _slots(self, device, n, hs, ws, h, w, labels, orient, scene):
        key = (device, n, hs, ws, h, w, tuple(t.dtype for _k, t in labels),
               None if orient is None else orient.shape[1], None if scene is None else scene.dtype)
        r = self._rings.get(key)
        if r is not None:
            return r
        self._no_capture('for this shape')
        slots = []
        for _ in range(self.ring):
            s = {'params': Fn._zeros((n, 8), device, torch.int32)}
            if 'rgb' in self.modalities:
                s['rgb'] = Fn._empty((n, 3, h, w), device, torch.float32)
            if 'depth' in self.modalities:
                s['depth'] = Fn._empty((n, 1, h, w), device, torch.float32)
            for k, t in labels:
                s[k] = Fn._empty((n, h, w), device, t.dtype)
            if orient is not None:
                s['orientations'] = Fn._empty(orient.shape, device, orient.dtype)      # (dense: _on_device)
            if scene is not None:
                s['scene'] = Fn._empty(scene.shape, device, scene.dtype)
            if self.with_normal:
                s['normal'] = Fn._empty((n, h, w, 3), device, torch.float32).permute(0, 3, 1, 2)
            slots.append(s)
        r = self._rings[key] = [0, slots]
        return r

    def _run(self, batch, h, w, table, draw, hsv, who):
        rgb, depth, labels, orient, scene, n, hs, ws, maps, normal = self._inputs(batch, who)
        if draw:
            self.check_size(hs, ws)
        elif not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"{who}: {hs}x{ws} -> {h}x{w}; sides in [1, {MAX_SIDE}]")
        device = self._on_device(maps + ([('params', table)] if table is not None else []), who)
        if table is not None and (table.dtype != torch.int32 or tuple(table.shape) != (n, 8)):
            raise ValueError(f"{who}: params must be an int32 ({n}, 8) table")
        ring = self._slots(device, n, hs, ws, h, w, labels, orient, scene)
        slot = ring[1][ring[0]]
        ring[0] = (ring[0] + 1) % self.ring
        L, st = _lib.lib(), _stream()
        if draw:
            state = self._device_state(device)
            check(L.emsa_augment_params(state.data_ptr(), slot['params'].data_ptr(), n, hs, ws, h, w,
                                        self.q_min, self.q_max, self.flip_threshold, *self.hsv_jitter, st),
                  'emsa_augment_params')
        else:
            slot['params'].copy_(table)
        self._last = slot
        lab = [(t.data_ptr(), _LABEL_DTYPES[t.dtype], slot[k].data_ptr()) for k, t in labels]
        lab += [(None, 0, None)] * (2 - len(lab))
        check(L.emsa_augment_apply(rgb.data_ptr() if rgb is not None else None,
                                   depth.data_ptr() if depth is not None else None,
                                   lab[0][0], lab[0][1], lab[1][0], lab[1][1], slot['params'].data_ptr(),
                                   n, hs, ws, h, w,
                                   slot['rgb'].data_ptr() if rgb is not None else None,
                                   slot['depth'].data_ptr() if depth is not None else None,
                                   lab[0][2], lab[1][2], 1.0 / 255.0, self._mean, self._std,
                                   self.depth_stats[0], self.depth_stats[1], 1, 1 if hsv else 0, st),
              'emsa_augment_apply')
        out = {k: slot[k] for k in ('rgb', 'depth') if k in slot}
        for k, _t in labels:
            out[k] = slot[k]
        if orient is not None:
            check(L.emsa_augment_orientations(orient.data_ptr(), slot['orientations'].data_ptr(),
                                              slot['params'].data_ptr(), n, orient.shape[1], st),
                  'emsa_augment_orientations')
            out['orientations'] = slot['orientations']
        if normal is not None:
            check(L.emsa_augment_normal(normal[0].data_ptr(), 1 if normal[1] else 0,
                                        slot['params'].data_ptr(), n, hs, ws, h, w,
                                        slot['normal'].data_ptr(), st), 'emsa_augment_normal')
            out['normal'] = slot['normal']
        if scene is not None:
            out['scene'] = slot['scene']
            out['scene'].copy_(scene)         # (a copy: the caller may refill its buffer)
        return out

    # -- public ------------------------------------------------------------------------------------------
    def apply(self, batch, params=None):
        """the augmented batch.  params: an int32 (N, 8) device table (Hr, Wr, cy, cx, flip and the bits
        of dh, ds, dv) used instead of a draw (the step does not advance) -- for tests and for
        reproducing a sample; its rows are the caller's responsibility (source indices are clamped)"""
        if params is not None and not torch.is_tensor(params):
            raise TypeError(f"{_WHO}.apply: params must be a tensor")
        return self._run(batch, self.height, self.width, params, params is None,
                         any(a != 0.0 for a in self.hsv_jitter), f'{_WHO}.apply')

    def resize_normalize(self, batch, height, width):
        """the deterministic validation twin: every map resized to height x width (RGB bilinear, depth and
        labels nearest) and normalised, no crop, jitter or flip -- the apply kernel with the table
        (height, width, 0, 0, 0, 0, 0, 0)"""
        who = f'{_WHO}.resize_normalize'
        height, width = int(height), int(width)
        if not (1 <= height <= MAX_SIDE and 1 <= width <= MAX_SIDE):
            raise ValueError(f"{who}: {height}x{width}; sides in [1, {MAX_SIDE}]")
        *_x, n, _hs, _ws, maps, _normal = self._inputs(batch, who)
        device = self._on_device(maps, who)
        key = (device, n, height, width)
        table = self._identity.get(key)
        if table is None:
            self._no_capture('for this shape')
            table = self._identity[key] = torch.tensor([[height, width, 0, 0, 0, 0, 0, 0]] * n,
                                                       dtype=torch.int32).to(device)
        return self._run(batch, height, width, table, False, False, who)

    def last_params(self):
        """the int32 (N, 8) table of the last call, on the host (a host read: not for the loop)"""
        if self._last is None:
            raise RuntimeError(f"{_WHO}.last_params: no call yet")
        return self._last['params'].cpu()

    def state_dict(self):
        """{seed, step}: with it a resumed run continues the sequence (a host read)"""
        for s in self._state.values():
            seed, step = (int(v) for v in s.cpu().numpy().view(np.uint32))
            return {'seed': seed, 'step': step}
        return {'seed': self._seed, 'step': self._step}

    def load_state_dict(self, state):
        self._seed, self._step = int(state['seed']) & 0xFFFFFFFF, int(state['step']) & 0xFFFFFFFF
        host = torch.from_numpy(np.array([self._seed, self._step], dtype=np.uint32).view(np.int32))
        for s in self._state.values():
            s.copy_(host)
