#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time `PngDecoder.decode()` (emsanet_amd/png.py, csrc/png_decode.hip) on one training batch as the reference's
datasets store it: per sample an RGB frame, a 16-bit depth frame, a semantic and an instance map, each a PNG
file -- 4 x batch files made here with Pillow (default compress_level 6, Pillow's filter choice).  RGB and
depth are noise over a gradient (they hardly compress: the decoder's worst case), the label maps are the
16 x 16 blocks of tools/export_bench.py.  Beside it the host way in the same process: Pillow decodes the
same files on a 16-thread pool into pinned arrays, which are then copied to the device.

Protocol: warm-up first.  `decode_ms`: device events around the four decode calls on device-resident files,
median of --reps.  `bytes_to_stack_ms`: host clock around PngFiles.from_bytes + copy + decode + check().
`host_way_ms`: host clock around the pool's decode + the H2D copies and their wait (--host-reps).
`pcie_bytes`: what crosses either way.  With --step: the bf16 graphed training step (the one of
tools/fp16_train_bench.py) timed alone and with one batch decode enqueued on a second stream per step.
No target is set: the yardstick is the host way in the same run.

    python tools/png_decode_bench.py [--step] [--out FILE.json]
"""
import argparse
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from export_bench import event_ms, host_ms   # noqa: E402

from PIL import Image   # noqa: E402


def make_batch(n, h, w, seed=0):
    """-> {key: (n, h, w[, 3]) array}: noisy rgb / depth, blocky label maps"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    ramp = (yy * 3 + xx * 5) % 256
    rgb = np.stack([np.stack([ramp, ramp // 2 + 40, 255 - ramp], 2)] * n)
    rgb = np.clip(rgb + g.integers(-24, 25, rgb.shape), 0, 255).astype(np.uint8)
    depth = (np.stack([ramp * 20 + 500] * n) + g.integers(0, 64, (n, h, w))).astype(np.uint16)

    def blocks(high, dtype):
        t = g.integers(0, high, (n, (h + 15) // 16, (w + 15) // 16))
        return np.ascontiguousarray(np.repeat(np.repeat(t, 16, 1), 16, 2)[:, :h, :w].astype(dtype))
    return {'rgb': rgb, 'depth': depth, 'semantic': blocks(41, np.uint8), 'instance': blocks(65, np.uint16)}


def to_png(img):
    f = io.BytesIO()
    Image.fromarray(img).save(f, format='PNG')
    return f.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--step', action='store_true', help='also time the bf16 graphed step with the decode beside it')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import PngDecoder, PngFiles

    dev = torch.device('cuda:0')
    n, h, w = a.batch_size, a.height, a.width
    arrays = make_batch(n, h, w)
    with ThreadPoolExecutor(a.threads) as pool:
        files = {k: list(pool.map(to_png, v)) for k, v in arrays.items()}
    res = {'batch': [n, h, w], 'files': 4 * n, 'reps': a.reps, 'producer': 'PIL save, compress_level 6',
           'decoder': 'one wave per file: chunk walk + inflate + Adler-32, then unfilter + layout; 2 launches per call',
           'file_bytes': {k: sum(len(f) for f in v) for k, v in files.items()},
           'raw_bytes': {k: int(v.nbytes) for k, v in arrays.items()}}
    res['pcie_bytes'] = {'files_h2d': sum(res['file_bytes'].values()), 'raw_h2d': sum(res['raw_bytes'].values()),
                         'status_d2h': 4 * 4 * n}

    dec = PngDecoder(ring=2)
    resident = {k: PngFiles.from_bytes(v).to(dev) for k, v in files.items()}
    torch.cuda.synchronize()
    res['decode_ms'] = event_ms(lambda: dec.decode_batch(resident), a.reps, a.warmup)
    for k, f in resident.items():
        res.setdefault('decode_ms_by_key', {})[k] = event_ms(lambda: dec.decode(f, tag=k), a.reps, 1)['median']
    stacks = dec.decode_batch(resident)
    dec.check()
    res['decoded_equals_source'] = bool(all(np.array_equal(stacks[k].cpu().numpy(), arrays[k]) for k in arrays))

    def bytes_to_stack():
        out = dec.decode_batch({k: PngFiles.from_bytes(v).to(dev) for k, v in files.items()})
        dec.check()
        return out
    res['bytes_to_stack_ms'] = host_ms(bytes_to_stack, a.reps, a.warmup)

    pinned = {k: torch.from_numpy(np.empty_like(v)).pin_memory() for k, v in arrays.items()}
    jobs = [(k, i) for k in files for i in range(n)]

    def one(job):
        k, i = job
        pinned[k][i].numpy()[...] = np.asarray(Image.open(io.BytesIO(files[k][i])))

    with ThreadPoolExecutor(a.threads) as pool:
        def host_way():
            list(pool.map(one, jobs))
            out = {k: v.to(dev, non_blocking=True) for k, v in pinned.items()}
            torch.cuda.synchronize()
            return out
        res['host_way_ms'] = host_ms(host_way, a.host_reps, 1)
        res['host_way_threads'] = a.threads
        theirs = host_way()
    res['host_way_equals_source'] = bool(all(np.array_equal(theirs[k].cpu().numpy(), arrays[k]) for k in arrays))
    res['host_way_over_bytes_to_stack'] = res['host_way_ms']['median'] / res['bytes_to_stack_ms']['median']
    res['device_path_beats_host_threads'] = bool(res['host_way_over_bytes_to_stack'] > 1.0)
    print(json.dumps(res), flush=True)

    if a.step:
        from fp16_train_bench import build, time_replays
        from oracle.emsanet_oracle import synthetic_batch
        batch = {k: v.to(dev) for k, v in synthetic_batch(n, h, w, seed=1).items()}
        ns = argparse.Namespace(height=h, width=w, batch_size=n, losses=False, init_scale=1024.0)
        step, _, _ = build(torch.bfloat16, False, ns, batch, dev)
        alone = [time_replays(step, a.steps) for _ in range(3)]
        side = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        both = []
        for _ in range(3):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                with torch.cuda.stream(side):
                    dec.decode_batch(resident)
                step.replay()
            e1.record()
            torch.cuda.synchronize()                   # (also waits for the side stream's last decode)
            both.append(e0.elapsed_time(e1) / a.steps)
        dec.check()
        res['bf16_graph_step_ms'] = {'alone': min(alone), 'with_decode_on_second_stream': min(both),
                                     'all_alone': alone, 'all_with_decode': both}

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
