#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time the device-side training augmentation (emsanet_amd/augment.py) at the training batch of the
flagship workload: `apply()` -- the parameter draw and the one fused resize / crop / HSV jitter / flip /
normalise launch, plus the orientation table -- on 32 x 480 x 640 raw RGB-D frames with a uint8
semantic and a uint16 instance map, scales 1.0 ... 1.4, crop 480 x 640.

Protocol: device events around the call, warm-up first, median of --reps (20); the calls rotate over
--sets (4) copies of the raw inputs (4 x 79 MB read, 2 x 255 MB written: more than the Infinity Cache
holds).  Reported beside
  (a) the algorithmic bytes (26 B written per output pixel; every source byte read once) and the
      fraction of the HBM rate (--peak-tbs, 8 TB/s) they reach
  (b) the yardstick: `normalize_rgb` + `normalize_depth` on the same raw frames in the same run -- the
      two launches `apply` replaces
  (c) the same with the HSV stage compiled out (amplitudes 0)
  (d) the host side per image, single process and with a pool of --workers (16) processes: the NumPy
      reference (tests/augment_reference.py, float32 HSV) and a Pillow pipeline (Image.resize BILINEAR /
      NEAREST + crop + flip, then the same NumPy HSV and normalisation)
  (e) the share of a bf16 training step (--step-ms, default 32.8 ms for bs 32, profiles/INDEX.md)

    python tools/augment_bench.py [--out FILE.json]
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

import augment_reference as R   # noqa: E402

STATS = (2000.0, 900.0)


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
    return {'median': statistics.median(times), 'min': min(times), 'max': max(times)}


def _numpy_one(job):
    b, row, h, w = job
    t0 = time.perf_counter()
    R.reference_apply(b, row, h, w, STATS, hsv=True, dtype=np.float32)
    return time.perf_counter() - t0


def _pillow_one(job):
    from PIL import Image
    b, row, h, w = job
    t0 = time.perf_counter()
    hr, wr, cy, cx, flip, dh, ds, dv = R.unpack_row(row[0])

    def geom(a, mode):
        im = Image.fromarray(a[0]).resize((wr, hr), mode).crop((cx, cy, cx + w, cy + h))
        a = np.asarray(im)
        return a[:, ::-1] if flip else a

    rgb = geom(b['rgb'], Image.BILINEAR)
    R.normalize_rgb_unit(R.hsv_jitter(rgb, dh, ds, dv, np.float32), np.float32).transpose(2, 0, 1).copy()
    R.normalize_depth(geom(b['depth'], Image.NEAREST), *STATS)
    np.ascontiguousarray(geom(b['semantic'], Image.NEAREST))
    np.ascontiguousarray(geom(b['instance'], Image.NEAREST))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--host-images', type=int, default=32)
    ap.add_argument('--peak-tbs', type=float, default=8.0)
    ap.add_argument('--step-ms', type=float, default=32.8,
                    help='bf16 training step of bs 32 to compare with (profiles/INDEX.md)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import TrainingAugmenter, full_args
    from emsanet_amd.postprocessing import normalize_depth, normalize_rgb

    dev = torch.device('cuda:0')
    n, h, w = a.batch_size, a.height, a.width
    raw = R.random_batch(n, h, w, seed=3, max_instances=256)
    sets = [{k: torch.from_numpy(v).to(dev) for k, v in raw.items()} for _ in range(a.sets)]
    args = full_args(input_height=h, input_width=w)
    res = {'batch_size': n, 'height': h, 'width': w, 'reps': a.reps, 'sets': a.sets,
           'scales': [args.aug_scale_min, args.aug_scale_max], 'launches_per_batch': 3}

    aug = TrainingAugmenter(args, STATS, seed=1)
    res['apply_ms'] = event_ms(lambda i: aug.apply(sets[i % a.sets]), a.reps, a.warmup)
    plain = TrainingAugmenter(args, STATS, seed=1, hsv_jitter=(0.0, 0.0, 0.0))
    res['apply_without_hsv_ms'] = event_ms(lambda i: plain.apply(sets[i % a.sets]), a.reps, a.warmup)

    def yardstick(i):
        s = sets[i % a.sets]
        normalize_rgb(s['rgb'])
        normalize_depth(s['depth'], *STATS)

    res['normalize_pair_ms'] = event_ms(yardstick, a.reps, a.warmup)
    res['apply_over_normalize_pair'] = res['apply_ms']['median'] / res['normalize_pair_ms']['median']

    # the benchmark times what the tests check: sample 0 against the reference under the drawn table
    got = aug.apply(sets[0])
    table = aug.last_params().numpy()
    ref = R.reference_apply({k: v[:1] for k, v in raw.items()}, table[:1], h, w, STATS, hsv=True)
    res['max_abs_diff_vs_reference'] = float(np.abs(got['rgb'][:1].cpu().numpy() - ref['rgb']).max())
    res['labels_equal_reference'] = bool(np.array_equal(got['instance'][:1].cpu().numpy(), ref['instance']))

    pixels = n * h * w
    # written per output pixel: rgb 12, depth 4, semantic 1, instance 2 (+ 3 + 2 + 1 + 2 source bytes read)
    written, read = pixels * (12 + 4 + 1 + 2), pixels * (3 + 2 + 1 + 2)
    res['algorithmic_bytes'] = {'written': written, 'read': read}
    res['floor_us_at_peak'] = (written + read) / (a.peak_tbs * 1e12) * 1e6
    res['fraction_of_peak'] = (written + read) / (res['apply_ms']['median'] * 1e-3) / (a.peak_tbs * 1e12)
    pair_bytes = pixels * (12 + 4 + 3 + 2)
    res['normalize_pair_fraction_of_peak'] = pair_bytes / (res['normalize_pair_ms']['median'] * 1e-3) / \
        (a.peak_tbs * 1e12)
    res['share_of_bf16_step'] = res['apply_ms']['median'] / a.step_ms
    res['bf16_step_ms'] = a.step_ms

    # the host side
    k = a.host_images
    host = R.random_batch(k, h, w, seed=5, max_instances=256)
    tab = R.draw_table(1, 0, k, h, w, h, w)
    jobs = [({key: v[i:i + 1] for key, v in host.items() if key in ('rgb', 'depth', 'semantic', 'instance')},
             tab[i:i + 1], h, w) for i in range(k)]
    workers = max(1, min(a.workers, os.cpu_count() or a.workers))
    res['host_workers'] = workers
    with multiprocessing.get_context('spawn').Pool(workers) as pool:
        for name, fn in (('numpy_reference', _numpy_one), ('pillow_pipeline', _pillow_one)):
            single = [fn(j) for j in jobs[:4]]
            res[f'{name}_ms_per_image_one_process'] = statistics.median(single) * 1e3
            pool.map(fn, jobs[:workers])                             # start-up and imports
            t0 = time.perf_counter()
            pool.map(fn, jobs, chunksize=1)
            wall = time.perf_counter() - t0
            res[f'{name}_ms_per_image_with_workers'] = wall / k * 1e3
            res[f'{name}_images_per_s_with_workers'] = k / wall

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
