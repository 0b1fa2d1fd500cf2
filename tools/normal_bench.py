#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time the kernels of the surface-normal task (csrc/normal.hip) at the training batch of the flagship
workload, 32 x 480 x 640: the L1 loss forward and backward at full resolution, the multi-scale targets,
the augmentation (source 480 x 640, drawn scales 1.0 ... 1.4), the unit-length post-processing and the
angular-error metric.

Protocol: device events around the call, warm-up first, median of --reps (20); the calls rotate over
--sets (4) copies of the inputs.  Reported per kernel beside
  (a) the algorithmic bytes (every operand once) and the fraction of the HBM rate (--peak-tbs, 8 TB/s)
      they reach: all six are bandwidth bound
  (b) the yardstick: the same mathematics written in plain torch on the device, timed the same way

    python tools/normal_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + i)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


# ---- the yardsticks: plain torch on the device ---------------------------------------------------------
def torch_l1(pred, target_hwc):
    t = target_hwc.permute(0, 3, 1, 2)
    m = (target_hwc != 0).any(-1, keepdim=True).permute(0, 3, 1, 2)
    return ((pred - t).abs() * m).sum() / (3 * m.sum()).clamp(min=1)


def torch_targets(normal_hwc, scales):
    """(a copy at every scale, the full resolution included: the generator hands out buffers of its own)"""
    return [normal_hwc[:, ::s, ::s].clone(memory_format=torch.contiguous_format) for s in scales]


def torch_augment(normal_hwc, table, h, w):
    """gather with the index maps of the composed resize / crop / flip, built on the device"""
    n, hs, ws, _ = normal_hwc.shape
    t = table.long()
    hr, wr, cy, cx, flip = (t[:, k, None] for k in range(5))
    y = torch.arange(h, device=table.device)[None]
    x = torch.arange(w, device=table.device)[None]
    yn = (((cy + y) * hs) // hr).clamp(max=hs - 1)
    xn = (((cx + torch.where(flip != 0, w - 1 - x, x)) * ws) // wr).clamp(max=ws - 1)
    out = normal_hwc[torch.arange(n, device=table.device)[:, None, None], yn[:, :, None], xn[:, None, :]]
    sign = torch.where(flip != 0, -1.0, 1.0).view(n, 1, 1)
    return torch.cat([out[..., :1] * sign[..., None], out[..., 1:]], -1)


def torch_angular_error(pred, target_hwc):
    p = pred.permute(0, 2, 3, 1)
    m = (target_hwc != 0).any(-1)
    angle = torch.atan2(torch.linalg.cross(p, target_hwc, dim=-1).norm(dim=-1), (p * target_hwc).sum(-1))
    return (angle * m).sum(), m.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import (MeanAbsoluteNormalError, NormalPostprocessing, TrainingAugmenter,
                             TrainingTargetGenerator, default_args)
    from emsanet_amd.loss import NormalLoss
    from emsanet_amd.targets import DEFAULT_SCALES, N_NORMAL_LAUNCHES

    assert torch.cuda.is_available(), "normal_bench.py times kernels: it needs the GPU"
    dev = torch.device('cuda:0')
    n, h, w, k = a.batch_size, a.height, a.width, a.sets
    pixels = n * h * w
    g = torch.Generator(device='cpu').manual_seed(0)

    def normals():
        v = torch.nn.functional.normalize(torch.randn(n, h, w, 3, generator=g), dim=-1)
        v[torch.rand(n, h, w, generator=g) < 0.3] = 0.0
        return v.to(dev)

    targets = [normals() for _ in range(k)]
    # predictions as the head returns them: the first 3 channels of rows of 8 floats
    preds = [torch.randn(n, h, w, 8, generator=g).to(dev).permute(0, 3, 1, 2)[:, :3] for _ in range(k)]
    args = default_args(tasks=('semantic', 'normal'), input_height=h, input_width=w)
    res = {'batch_size': n, 'height': h, 'width': w, 'reps': a.reps, 'peak_tbs': a.peak_tbs,
           'scales': list(DEFAULT_SCALES), 'target_launches': N_NORMAL_LAUNCHES, 'kernels': {}}

    def report(name, fn, ref_fn, nbytes):
        med, lo, hi = event_ms(fn, a.reps, a.warmup)
        rmed, rlo, rhi = event_ms(ref_fn, a.reps, a.warmup)
        res['kernels'][name] = {
            'ms': {'median': med, 'min': lo, 'max': hi}, 'algorithmic_bytes': nbytes,
            'floor_us_at_peak': nbytes / (a.peak_tbs * 1e12) * 1e6,
            'fraction_of_peak': nbytes / (med * 1e-3) / (a.peak_tbs * 1e12),
            'torch_ms': {'median': rmed, 'min': rlo, 'max': rhi}, 'speedup_over_torch': rmed / med}

    # loss: forward reads 16 B of the prediction row + 12 B of the target per pixel; backward reads the
    # same and writes rows of 16 B
    crit = NormalLoss()
    leaves = [p.detach().requires_grad_(True) for p in preds]
    report('l1_fwd', lambda i: crit([preds[i % k]], [targets[i % k]]),
           lambda i: torch_l1(preds[i % k], targets[i % k]), pixels * (16 + 12))

    def fwd_bwd(i):
        crit([leaves[i % k]], [targets[i % k]])[0][0].backward()
        leaves[i % k].grad = None

    def torch_fwd_bwd(i):
        torch_l1(leaves[i % k], targets[i % k]).backward()
        leaves[i % k].grad = None
    report('l1_fwd_bwd', fwd_bwd, torch_fwd_bwd, pixels * (16 + 12) + pixels * (16 + 12 + 16))

    # targets: every scale reads and writes 12 B per output pixel
    gen = TrainingTargetGenerator(default_args(tasks=('normal',)), [False, True])
    sem = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    out_pixels = sum(n * (h // s) * (w // s) for s in DEFAULT_SCALES)

    def generate(i):
        check = gen.generate({'semantic': sem, 'normal': targets[i % k]})
        return check['normal']
    report('targets', generate, lambda i: torch_targets(targets[i % k], DEFAULT_SCALES), out_pixels * 24)

    # augmentation: 12 B read and written per output pixel (the whole apply() is timed on both sides of
    # the normal launch: its own time is the difference)
    aug = TrainingAugmenter(args, with_normal=True)
    plain = TrainingAugmenter(default_args(tasks=('semantic',), input_height=h, input_width=w))
    rgb = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev)
    depth = torch.zeros(n, h, w, dtype=torch.int16, device=dev).view(torch.uint16)
    base = {'rgb': rgb, 'depth': depth, 'semantic': sem}
    with_ms = event_ms(lambda i: aug.apply(dict(base, normal=targets[i % k])), a.reps, a.warmup)
    without_ms = event_ms(lambda i: plain.apply(base), a.reps, a.warmup)
    table = aug._last['params'].clone()
    torch_ms = event_ms(lambda i: torch_augment(targets[i % k], table, h, w), a.reps, a.warmup)
    own = with_ms[0] - without_ms[0]
    res['kernels']['augment'] = {
        'apply_with_normal_ms': {'median': with_ms[0], 'min': with_ms[1], 'max': with_ms[2]},
        'apply_without_normal_ms': {'median': without_ms[0], 'min': without_ms[1], 'max': without_ms[2]},
        'ms': {'median': own}, 'algorithmic_bytes': pixels * 24,
        'floor_us_at_peak': pixels * 24 / (a.peak_tbs * 1e12) * 1e6,
        'fraction_of_peak': pixels * 24 / (own * 1e-3) / (a.peak_tbs * 1e12) if own > 0 else None,
        'torch_ms': {'median': torch_ms[0], 'min': torch_ms[1], 'max': torch_ms[2]},
        'speedup_over_torch': torch_ms[0] / own if own > 0 else None}

    # unit vectors: 16 B read, 12 B written
    post = NormalPostprocessing()
    report('unit', lambda i: post({'normal_output': preds[i % k]}),
           lambda i: torch.nn.functional.normalize(preds[i % k], dim=1), pixels * (16 + 12))

    # metric: 16 B + 12 B read
    metric = MeanAbsoluteNormalError()
    report('angular_error', lambda i: metric.update(preds[i % k], targets[i % k]),
           lambda i: torch_angular_error(preds[i % k], targets[i % k]), pixels * (16 + 12))
    metric.reset()
    metric.update(preds[0], targets[0])
    s, c = torch_angular_error(preds[0].double(), targets[0].double())
    res['angular_error_check'] = {'kernel_mae_rad': metric.compute()['mae_rad'],
                                  'torch_fp64_mae_rad': float(s) / int(c), 'pixels': int(c)}
    res['l1_check'] = {'kernel': float(crit([preds[0]], [targets[0]])[0][0]),
                       'torch_fp64': float(torch_l1(preds[0].double(), targets[0].double()))}
    got = aug.apply(dict(base, normal=targets[0]))['normal'].permute(0, 2, 3, 1)
    res['augment_equals_torch'] = bool(torch.equal(got, torch_augment(targets[0], aug._last['params'], h, w)))
    res['targets_equal_torch'] = all(
        torch.equal(x.permute(0, 2, 3, 1), y)
        for x, y in zip(generate(0), torch_targets(targets[0], DEFAULT_SCALES)))
    assert np.isfinite(res['l1_check']['kernel'])

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
