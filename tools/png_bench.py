#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Time `PngEncoder.encode_packed()` + `to_host()` (emsanet_amd/png.py) on the `scannet-semantic` and
`scannet-panoptic` prediction outputs of `InferenceOutputPacker.pack()` -- two uint8 label maps and one
three-channel panoptic image per sample -- at 480 x 640 and 968 x 1296, batch 8 and 32, beside the host
way: the packed arrays copied to the host (`packer.to_host`) and every image written as PNG by
`PIL.Image.save(format='PNG', compress_level=1)` into memory (`zlib.compress(level=1)` of the filter-0
scanlines when Pillow is missing).  The prediction is the synthetic one of tools/export_bench.py (16 x 16
blocks of classes / instance ids).

Protocol: warm-up first.  `encode_ms`: device events around encode_packed(), median of --reps.
`encode_to_host_ms`: host clock around encode_packed() + to_host() of every key (to_host synchronises).
`host_way_ms`: host clock around packer.to_host(), its wait, and the PNG writes (--host-reps, default 2).
Bytes to the host per image: the packed maps against the files.  One file per key is read back with
Pillow and must equal the packed array.  No target is set: the yardstick is the host way in the same run.

    python tools/png_bench.py [--out FILE.json]
"""
import argparse
import io
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from export_bench import event_ms, host_ms, synthetic_prediction   # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None

FORMATS = ('scannet-semantic', 'scannet-panoptic')


def host_png(a):
    """one image (H, W) uint8 / uint16 or (H, W, 3) B,G,R -> PNG bytes made on the host"""
    if a.ndim == 3:
        a = a[:, :, ::-1]
    if Image is not None:
        f = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(f, format='PNG', compress_level=1)
        return f.getvalue()
    body = a.astype('>u2').view(np.uint8) if a.dtype == np.uint16 else a
    body = np.ascontiguousarray(body).reshape(a.shape[0], -1)
    return zlib.compress(np.concatenate([np.zeros((a.shape[0], 1), np.uint8), body], 1).tobytes(), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='480x640,968x1296')
    ap.add_argument('--batches', default='8,32')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from emsanet_amd import InferenceOutputPacker, PngEncoder

    dev = torch.device('cuda:0')
    table = ((np.arange(41) * 7 + 3) % 251).astype(np.uint8)
    res = {'reps': a.reps, 'formats': list(FORMATS), 'encoder': 'one wave per strip of 4 rows, 64-byte tiles',
           'host_codec': 'PIL compress_level=1' if Image is not None else 'zlib level 1, no framing',
           'cases': []}
    for size in a.sizes.split(','):
        h, w = (int(v) for v in size.split('x'))
        for n in (int(v) for v in a.batches.split(',')):
            pred = synthetic_prediction(n, h, w, dev)
            packer = InferenceOutputPacker(FORMATS, 1000, table, ring=2)
            enc = PngEncoder(ring=2)
            packed = packer.pack(pred, {})
            case = {'batch': [n, h, w], 'keys': sorted(packed)}
            case['packed_d2h_bytes_per_image'] = sum(v.numel() * v.element_size() for v in packed.values()) / n
            case['encode_ms'] = event_ms(lambda: enc.encode_packed(packed), a.reps, a.warmup)

            def encode_to_host():
                return {k: enc.to_host(e) for k, e in enc.encode_packed(packed).items()}
            case['encode_to_host_ms'] = host_ms(encode_to_host, a.reps, a.warmup)
            files = encode_to_host()
            case['encoded_d2h_bytes_per_image'] = sum(len(f) for fs in files.values() for f in fs) / n

            def host_way():
                arrays = packer.to_host(packed).synchronize()
                return {k: [host_png(img) for img in arrays[k]] for k in packed}
            if a.host_reps > 0:
                case['host_way_ms'] = host_ms(host_way, a.host_reps, 1)
                theirs = host_way()
                case['host_way_bytes_per_image'] = sum(len(f) for fs in theirs.values() for f in fs) / n
                case['encoded_over_host_way_bytes'] = case['encoded_d2h_bytes_per_image'] / \
                    case['host_way_bytes_per_image']
                case['host_way_over_encode_to_host'] = case['host_way_ms']['median'] / \
                    case['encode_to_host_ms']['median']
            case['packed_over_encoded_d2h_bytes'] = case['packed_d2h_bytes_per_image'] / \
                case['encoded_d2h_bytes_per_image']
            if Image is not None:
                arrays = packer.to_host(packed).synchronize()
                ok = True
                for k, fs in files.items():
                    got = np.asarray(Image.open(io.BytesIO(bytes(fs[-1]))))
                    want = arrays[k][-1][:, :, ::-1] if arrays[k].ndim == 4 else arrays[k][-1]
                    ok = ok and np.array_equal(got, want)
                case['files_decode_to_packed_arrays'] = bool(ok)
            res['cases'].append(case)
            print(json.dumps(case), flush=True)
            del pred, packer, enc, packed, files
            torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
