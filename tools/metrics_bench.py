#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time the device-side validation metrics (emsanet_amd/metrics.py) at the validation batch of the
flagship workload: `update()` of MeanIntersectionOverUnion (41 classes) and PanopticQuality on
32 x 480 x 640 int64 maps.

Protocol: device events around the calls, warm-up first, median of --reps (20); inputs are COLD --
the calls rotate over --sets (4) copies of the maps, ~630 MB, more than the 256 MB memory-side cache.
Reported beside
  (a) the NumPy reference (tests/test_metrics.py) on the same maps, including their D2H copy
  (b) the eval forward + post-processing of a batch of the same size (--no-forward skips it)
and as the fraction of the HBM rate (--peak-tbs, 8 TB/s) the map reads reach.

    python tools/metrics_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_CLASSES = 41
DIVISOR = 1 << 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--numpy-reps', type=int, default=1)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    ap.add_argument('--no-forward', action='store_true')
    ap.add_argument('--kernels-only', action='store_true',
                    help='only the timed update() calls: the target of a kernel trace '
                         '(rocprofv3 --kernel-trace --stats -- python tools/metrics_bench.py --kernels-only)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import test_metrics as R
    from emsanet_amd import MeanIntersectionOverUnion, PanopticQuality

    dev = torch.device('cuda:0')
    n, h, w = a.batch_size, a.height, a.width
    pred, target = R.rectangle_batch(n, h, w, 56, DIVISOR, seed=3)
    # 41-class semantic maps with the same region structure (piecewise constant)
    sem = lambda ids: ((ids // DIVISOR) * 6 + (ids % DIVISOR) % 6) % N_CLASSES       # noqa: E731
    sem_pred, sem_target = sem(pred), sem(target)
    sets = [[torch.from_numpy(x).to(dev) for x in (pred, target, sem_pred, sem_target)]
            for _ in range(a.sets)]
    pixels = n * h * w

    miou = MeanIntersectionOverUnion(N_CLASSES, ignore_first_class=True)
    pq = PanopticQuality(num_categories=R.SCENE_CATEGORIES, ignored_label=0,
                         max_instances_per_category=DIVISOR, offset=256 ** 3, is_thing=R.SCENE_IS_THING)

    def both(i):
        p, t, sp, st = sets[i % a.sets]
        miou.update(sp, st)
        pq.update(p, t)

    def only_miou(i):
        miou.update(*sets[i % a.sets][2:])

    def only_pq(i):
        pq.update(*sets[i % a.sets][:2])

    res = {'batch': [n, h, w], 'n_classes': N_CLASSES, 'reps': a.reps, 'cold_sets': a.sets,
           'segments_per_image': int(len(np.unique(target[0])))}
    for key, fn in (('update_both', both), ('update_miou', only_miou), ('update_pq', only_pq)):
        med, lo, hi = event_ms(fn, a.reps, a.warmup)
        res[key + '_ms'] = {'median': med, 'min': lo, 'max': hi}
    if a.kernels_only:
        print(json.dumps(res))
        return
    # results are those of the reference (the benchmark times what the tests check)
    miou.reset()
    pq.reset()
    both(0)
    got_pq, got_miou = pq.compute(), miou.compute()

    times = []
    for _ in range(a.numpy_reps):
        t0 = time.perf_counter()
        p, t, sp, st = (x.cpu().numpy() for x in sets[0])
        cm, _ = R.confusion_reference(sp, st, N_CLASSES)
        ref = R.PanopticQualityReference(R.SCENE_CATEGORIES, 0, DIVISOR, R.SCENE_IS_THING)
        ref.update(p, t)
        want_pq, want_miou = ref.compute(), R.miou_reference(cm, True)
        times.append((time.perf_counter() - t0) * 1e3)
    res['numpy_reference_with_d2h_ms'] = statistics.median(times)
    res['max_abs_diff_vs_numpy'] = max([abs(got_miou - want_miou)] + [abs(got_pq[k] - want_pq[k]) for k in want_pq])
    res['all_pq'], res['miou'] = got_pq['all_pq'], got_miou

    peak = a.peak_tbs * 1e12
    for key, nbytes in (('update_both', 32 * pixels), ('update_miou', 16 * pixels), ('update_pq', 16 * pixels)):
        sec = res[key + '_ms']['median'] * 1e-3
        res[key + '_traffic'] = {'bytes': nbytes, 'floor_us_at_peak': nbytes / peak * 1e6,
                                 'fraction_of_peak': nbytes / sec / peak}

    if not a.no_forward:
        from emsanet_amd import full_args, nyuv2_config
        from emsanet_amd.model import EMSANet
        model = EMSANet(full_args(input_height=h, input_width=w, enable_panoptic=True), nyuv2_config())
        model.to(dev).eval()
        g = torch.Generator().manual_seed(0)
        batch = {'rgb': torch.randn(n, 3, h, w, generator=g).to(dev),
                 'depth': torch.randn(n, 1, h, w, generator=g).to(dev)}

        def forward(i):
            with torch.no_grad():
                model(batch, do_postprocessing=True)

        med, lo, hi = event_ms(forward, 5, 2)
        res['eval_forward_postprocessing_ms'] = {'median': med, 'min': lo, 'max': hi, 'dtype': 'f32'}
        res['metrics_share_of_eval_forward'] = res['update_both_ms']['median'] / med

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
