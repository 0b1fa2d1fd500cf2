#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time the device-side training-target generation (emsanet_amd/targets.py) at the training batch of the
flagship workload: `generate()` on 32 x 480 x 640 label maps (uint8 semantic, uint16 instance, about
20 instances per image, all four scales, all tasks), and the same at batch size 1.

Protocol: device events around the call, warm-up first, median of --reps (20); the calls rotate over
--sets (4) copies of the label maps.  Reported beside
  (a) the algorithmic bytes (labels read + targets written) and the fraction of the HBM rate
      (--peak-tbs, 8 TB/s) they reach
  (b) the launch count
  (c) the NumPy reference (tests/targets_reference.py) per image on the host, single process and with a
      pool of --workers (16) processes: the CPU side of the argument for a device path
  (d) the share of a bf16 training step (--step-ms, default 32.8 ms for bs 32: 976.7 images/s with hipGraph,
      profiles/INDEX.md)

    python tools/targets_bench.py [--out FILE.json]
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import targets_reference as R   # noqa: E402


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


def scene(n, h, w, instances, seed):
    sem, inst = R.rectangles_scene(n, h, w, instances, seed=seed, cell=40)
    ori = np.full((n, 256), np.nan, np.float32)
    ori[:, 1:instances + 1:2] = 0.5
    return sem.astype(np.uint8), inst.astype(np.uint16), ori, np.arange(n, dtype=np.int64) % 10


def _reference_one(job):
    sem, inst, ori = job
    t0 = time.perf_counter()
    R.reference_targets(sem[None], inst[None], R.IS_THING, R.USE_ORIENTATION, ori[None])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-sizes', type=int, nargs='+', default=[32, 1])
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--instances', type=int, default=20)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--numpy-images', type=int, default=32)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    ap.add_argument('--step-ms', type=float, default=32.8,
                    help='bf16 training step of bs 32 to compare with (profiles/INDEX.md)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import TrainingTargetGenerator, full_args
    from emsanet_amd.targets import N_LAUNCHES

    dev = torch.device('cuda:0')
    h, w = a.height, a.width
    res = {'height': h, 'width': w, 'instances_per_image': a.instances, 'reps': a.reps,
           'launches_per_batch': N_LAUNCHES, 'scales': [1, 32, 16, 8]}
    for n in a.batch_sizes:
        sem, inst, ori, scn = scene(n, h, w, a.instances, seed=3)
        sets = [{'semantic': torch.from_numpy(sem).to(dev), 'instance': torch.from_numpy(inst).to(dev),
                 'orientations': torch.from_numpy(ori).to(dev), 'scene': torch.from_numpy(scn).to(dev)}
                for _ in range(a.sets)]
        gen = TrainingTargetGenerator(full_args(), R.IS_THING, R.USE_ORIENTATION)
        med, lo, hi = event_ms(lambda i: gen.generate(sets[i % a.sets]), a.reps, a.warmup)
        gen.check()
        # results are those of the reference (the benchmark times what the tests check)
        got = gen.generate(sets[0])
        ref = R.reference_targets(sem[:1], inst[:1], R.IS_THING, R.USE_ORIENTATION, ori[:1])
        same = all(np.array_equal(g['center'][:1].cpu().numpy(), r['center'])
                   for g, r in zip(got['instance'], ref['instance']))
        pixels = sum(n * (h // s) * (w // s) for s in (1, 32, 16, 8))
        # per output pixel: semantic 8, center 4, offset 8, foreground 1, orientation 4, its mask 1;
        # per sampled input pixel of every scale: 1 (uint8) + 2 (uint16), read by stats and by render
        nbytes = pixels * (8 + 4 + 8 + 1 + 4 + 1) + 2 * pixels * 3
        key = f'bs{n}'
        res[key] = {'generate_ms': {'median': med, 'min': lo, 'max': hi}, 'algorithmic_bytes': nbytes,
                    'floor_us_at_peak': nbytes / (a.peak_tbs * 1e12) * 1e6,
                    'fraction_of_peak': nbytes / (med * 1e-3) / (a.peak_tbs * 1e12),
                    'center_equals_reference': bool(same)}
        if n == 32:
            res[key]['share_of_bf16_step'] = med / a.step_ms
            res[key]['bf16_step_ms'] = a.step_ms

    # the NumPy reference on the host
    k = a.numpy_images
    sem, inst, ori, _ = scene(k, h, w, a.instances, seed=5)
    jobs = [(sem[i], inst[i], ori[i]) for i in range(k)]
    single = [_reference_one(j) for j in jobs[:4]]
    res['numpy_reference_ms_per_image_one_process'] = statistics.median(single) * 1e3
    workers = max(1, min(a.workers, os.cpu_count() or a.workers))
    with multiprocessing.get_context('spawn').Pool(workers) as pool:
        pool.map(_reference_one, jobs[:workers])                 # start-up and imports
        t0 = time.perf_counter()
        pool.map(_reference_one, jobs, chunksize=1)
        wall = time.perf_counter() - t0
    res['numpy_reference_workers'] = workers
    res['numpy_reference_ms_per_image_with_workers'] = wall / k * 1e3
    res['numpy_reference_images_per_s_with_workers'] = k / wall

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
