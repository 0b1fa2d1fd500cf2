#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time `InferenceOutputPacker.pack()` + `to_host()` (emsanet_amd/export.py) for the four inference output
formats at full resolution 480 x 640 and 968 x 1296 (ScanNet's frame size), batch 8 and 32, beside what a
user does without it (`host_way` below): the reference's sequence of torch and NumPy operations, in its
order and dtypes -- class maps cast to uint8 and scores clamped on the device, `.cpu()`, then `+ 1`, the
table look-up, the casts, the three-channel stack and the float32 add in NumPy, image by image where the
reference loops.

The prediction is synthetic (blocky label maps, random scores) in the dtypes the post-processing yields:
packing depends on the shapes and dtypes only, and a 32 x 968 x 1296 eval forward is not what is timed.

Protocol: warm-up first.  `pack_ms`: device events around pack(), median of --reps.  `pack_to_host_ms`:
host clock around pack() + to_host() + waiting for its event.  `kernel`: device events around the ONE
emsa_export_pack launch of the (n, h, w) job group; its bytes are counted from the shapes (sources read
once, outputs written once) and set against the 8.0 TB/s HBM3E peak of the MI355X's data sheet.
`host_way_ms`: host clock around the device casts, the .cpu() copies and the NumPy packing (--numpy-reps,
default 2).  The host way's result must equal the packed outputs, bit for bit.
No target is set.

    python tools/export_bench.py [--out FILE.json]
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

HBM_PEAK = 8.0e12
SCORE_MAX = 0.999


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {'median': statistics.median(times), 'min': min(times), 'max': max(times)}


def host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {'median': statistics.median(times), 'min': min(times), 'max': max(times)}


def synthetic_prediction(n, h, w, dev, seed=0):
    """the `_fullres` entries the formats read, (n, h, w): 16 x 16 blocks of classes / instance ids"""
    g = torch.Generator().manual_seed(seed)

    def blocks(high, dtype):
        t = torch.randint(0, high, (n, (h + 15) // 16, (w + 15) // 16), generator=g)
        return t.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w].to(dtype).contiguous().to(dev)

    def score():
        return torch.rand(n, h, w, generator=g).to(dev)
    p = {'semantic_segmentation_idx': blocks(40, torch.int64), 'semantic_segmentation_score': score(),
         'panoptic_segmentation_deeplab_semantic_idx': blocks(41, torch.int64),
         'panoptic_segmentation_deeplab_instance_idx': blocks(65, torch.int32),
         'panoptic_segmentation_deeplab_semantic_score': score(),
         'panoptic_segmentation_deeplab_panoptic_score': score(),
         'scene_class_idx': torch.randint(0, 10, (n,), generator=g).to(dev),
         'scene_class_score': torch.rand(n, generator=g).to(dev)}
    return {k + ('_fullres' if v.dim() == 3 else ''): v for k, v in p.items()}


def host_way(pred, table):
    """-> (outputs under the packer's keys, bytes copied to the host)"""
    copied = [0]

    def cpu(t):
        copied[0] += t.numel() * t.element_size()
        return t.cpu().numpy()

    def bgr(semantic, instance):
        s8, i16 = semantic.astype('uint8'), instance.astype('uint16')
        return np.stack([(i16 & 0xFF).astype('uint8'), (i16 >> 8).astype('uint8'), s8], axis=2)

    def class_plus_score(classes_u8, score):
        score = cpu(torch.clamp(score, min=0, max=SCORE_MAX))
        classes = table[cpu(classes_u8)]
        out = classes.astype('float32') + score
        assert (out.astype('uint8') == classes).all()
        return out

    sem, pan_sem = pred['semantic_segmentation_idx_fullres'], pred['panoptic_segmentation_deeplab_semantic_idx_fullres']
    pan_inst = pred['panoptic_segmentation_deeplab_instance_idx_fullres']
    out = {}
    out['scannet_semantic/pred_path_semantic'] = np.stack([table[p + 1] for p in cpu(sem.to(torch.uint8))])
    out['scannet_semantic/pred_path_panoptic_semantic'] = np.stack([table[p] for p in cpu(pan_sem.to(torch.uint8))])
    s, i = table[cpu(pan_sem)], cpu(pan_inst)
    out['scannet_panoptic/pred_path'] = np.stack([bgr(s[b], i[b]) for b in range(s.shape[0])])
    c = sem.to(torch.uint8)
    c += 1
    out['mapping/pred_semantic'] = class_plus_score(c, pred['semantic_segmentation_score_fullres'])[:, None]
    out['mapping/pred_panoptic_semantic'] = class_plus_score(
        pan_sem.to(torch.uint8), pred['panoptic_segmentation_deeplab_semantic_score_fullres'])[:, None]
    score = cpu(torch.clamp(pred['panoptic_segmentation_deeplab_panoptic_score_fullres'], min=0, max=SCORE_MAX))
    out['mapping/pred_panoptic_instance'] = cpu(pan_inst).astype('float32') + score
    score = cpu(torch.clamp(pred['scene_class_score'], min=0, max=SCORE_MAX))
    out['mapping/pred_scene'] = cpu(pred['scene_class_idx']).astype('float32') + score
    return out, copied[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='480x640,968x1296')
    ap.add_argument('--batches', default='8,32')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--numpy-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import InferenceOutputPacker
    from emsanet_amd import export as E

    dev = torch.device('cuda:0')
    table = ((np.arange(41) * 7 + 3) % 251).astype(np.uint8)
    res = {'reps': a.reps, 'formats': list(E.FORMATS), 'hbm_peak_bytes_per_s': HBM_PEAK, 'cases': []}
    for size in a.sizes.split(','):
        h, w = (int(v) for v in size.split('x'))
        for n in (int(v) for v in a.batches.split(',')):
            pred = synthetic_prediction(n, h, w, dev)
            packer = InferenceOutputPacker(E.FORMATS, 1000, table, ring=2)
            case = {'batch': [n, h, w]}
            packed = packer.pack(pred, {})
            tensors = {k: v for k, v in packed.items() if torch.is_tensor(v)}
            case['packed_d2h_bytes_per_image'] = sum(v.numel() * v.element_size() for v in tensors.values()) / n
            case['pack_ms'] = event_ms(lambda: packer.pack(pred, {}), a.reps, a.warmup)

            def pack_to_host():
                packer.to_host(packer.pack(pred, {})).event.synchronize()
            case['pack_to_host_ms'] = host_ms(pack_to_host, a.reps, a.warmup)

            # the one emsa_export_pack launch over the (n, h, w) group: the jobs pack() launches
            counters = torch.zeros(4, dtype=torch.int64, device=dev)
            groups = packer.job_groups(pred, {})
            assert len(groups) == 1 and len(groups[0]) <= E.MAX_JOBS
            jobs = groups[0]
            nbytes = sum(t.numel() * t.element_size() for j in jobs for t in (j.dst, j.src0, j.src1)
                         if t is not None)
            k = event_ms(lambda: E.export_pack(jobs, counters), a.reps, a.warmup)
            case['kernel'] = {'jobs': len(jobs), 'ms': k, 'bytes': nbytes,
                              'bytes_per_s': nbytes / (k['median'] * 1e-3),
                              'fraction_of_hbm_peak': nbytes / (k['median'] * 1e-3) / HBM_PEAK}
            packer.check()

            if a.numpy_reps > 0:
                case['host_way_ms'] = host_ms(lambda: host_way(pred, table), a.numpy_reps, 1)
                want, copied = host_way(pred, table)
                case['host_way_d2h_bytes_per_image'] = copied / n
                got = packer.to_host(packer.pack(pred, {})).synchronize()
                assert set(want) == set(k for k, v in got.items() if isinstance(v, np.ndarray))
                case['equal_to_host_way'] = all(np.array_equal(got[k], want[k]) for k in want)
                case['host_way_over_pack_to_host'] = case['host_way_ms']['median'] / \
                    case['pack_to_host_ms']['median']
            res['cases'].append(case)
            print(json.dumps(case), flush=True)
            del pred, packer, packed, tensors, jobs, groups
            torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
