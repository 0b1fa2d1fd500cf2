"""PNG files encoded on the device (emsanet_amd/png.py, csrc/png.hip), judged by decoding them with the
independent decoder of tests/png_cases.py (hand-parsed chunks, zlib.crc32, zlib.decompress, and PIL when
it imports): every comparison is exact.  Every output and scratch buffer is poisoned and guard-banded
(tests/guard.py); the guards are checked after each case."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as C   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAYOUTS = (C.GRAY8, C.BGR8, C.GRAY16)
SIZES = [(1, 1), (1, 7), (5, 1), (7, 5), (33, 130), (64, 64), (65, 259)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _round_trip(enc, stack, layout, arena=None, pil=True):
    """encode `stack` (NumPy), check the offsets table, the poison behind the files, every file against
    its source; -> the files as bytes"""
    from emsanet_amd import png as P
    m, h, w = stack.shape[:3]
    enc.release()                                  # fresh, poisoned buffers: no file of an earlier case
    e = enc.encode(_dev(stack))
    files = [bytes(f) for f in enc.to_host(e)]
    if arena is not None:
        arena.check()
    bound = P.png_bound(layout, h, w)
    off = e.offsets.cpu().tolist()
    assert e.m == m and len(off) == m + 1 and off[0] == 0
    assert all(b > a for a, b in zip(off, off[1:])), off
    assert off[m] <= m * bound and all(b - a <= bound for a, b in zip(off, off[1:])), (off, bound)
    assert e.data.numel() == m * bound
    assert bool((e.data[off[m]:] == 0xFF).all()), "bytes behind the last file were written"
    raw = e.data[:off[m]].cpu().numpy().tobytes()
    assert [raw[a:b] for a, b in zip(off, off[1:])] == files
    for i, f in enumerate(files):
        got = (C.decode_checked if pil else C.decode)(f)
        assert got.dtype == stack.dtype and got.shape == stack[i].shape, (i, got.dtype, got.shape)
        assert np.array_equal(got, stack[i]), (i, int((got != stack[i]).sum()))
    return files


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('h,w', SIZES)
def test_exact_round_trip_small_sizes(h, w, layout, guard_allocations):
    """sizes below one tile, one strip, one row; odd sizes; more than one strip and tile; M = 1 and 3;
    all zero (one run through filter bytes and strips), all 255 (9-bit literals, 258-chunks), and three
    different images in one stack (the offsets table)"""
    from emsanet_amd import png as P
    enc = P.PngEncoder(ring=1)
    for m in (1, 3):
        for name, stack in C.size_cases(layout, h, w, m).items():
            _round_trip(enc, stack, layout, guard_allocations)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_exact_round_trip_run_edges_and_blobs(layout, guard_allocations):
    """the run-edge rows (runs of 1 ... 519 at offsets 62 ... 66, literals around 144, a run over a row
    end, constant rows over strip borders) at 27 x 1100, M = 1 and 3; the blob maps at 96 x 128"""
    from emsanet_amd import png as P
    enc = P.PngEncoder(ring=1)
    for m in (1, 3):
        _round_trip(enc, C.run_edge_stack(layout, m), layout, guard_allocations)
    blob = C.blob_maps(96, 128)[layout]
    _round_trip(enc, np.stack([blob, blob[::-1].copy(), np.roll(blob, 5, 1)]), layout, guard_allocations)


@pytest.mark.parametrize('layout,h,w', [(C.BGR8, 64, 4096), (C.GRAY8, 33, 130)])
def test_worst_case_input_stays_inside_the_bound(layout, h, w, guard_allocations):
    """random bytes in [144, 255]: every literal costs 9 bits, no run of three; the widest legal row"""
    from emsanet_amd import png as P
    rng = np.random.default_rng(7)
    shape = (1, h, w, 3) if layout == C.BGR8 else (1, h, w)
    stack = rng.integers(144, 256, shape).astype(np.uint8)
    files = _round_trip(P.PngEncoder(ring=1), stack, layout, guard_allocations, pil=False)
    bound = P.png_bound(layout, h, w)
    print(f"worst case {h}x{w} layout {layout}: file {len(files[0])} bytes, bound {bound}")
    assert len(files[0]) <= bound
    assert len(files[0]) > 1.1 * stack.size                     # (it is the worst case: nothing compressed)


def test_adler_sums_do_not_wrap(guard_allocations):
    """2 x 4096 BGR8 of all 255: scanlines of a zero and 12,288 bytes of 0xFF"""
    from emsanet_amd import png as P
    stack = np.full((1, 2, 4096, 3), 255, np.uint8)
    _round_trip(P.PngEncoder(ring=1), stack, C.BGR8, guard_allocations)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_label_maps_compress(layout, guard_allocations):
    """the 480 x 640 blob map: at most 3 x the size of zlib level 1 on the same filter-0 scanlines (a
    stored-block encoder is 30 - 60 x, a distance-1-only encoder fails on the colour layout).
    Measured on an MI355X: 12,937 / 21,740 / 18,646 bytes against 9,737 / 15,709 / 13,335 of zlib level 1
    (1.33 / 1.38 / 1.40)"""
    from emsanet_amd import png as P
    img = C.blob_maps(480, 640)[layout]
    files = _round_trip(P.PngEncoder(ring=1), img[None], layout, guard_allocations, pil=False)
    ref = len(zlib.compress(C.scanlines(img, layout), 1))
    print(f"blob 480x640 layout {layout}: file {len(files[0])} bytes, zlib level 1 {ref} bytes, "
          f"ratio {len(files[0]) / ref:.3f}, raw {img.nbytes}")
    assert len(files[0]) <= 3 * ref


def test_two_encodes_are_byte_equal_and_the_ring_keeps_the_first(guard_allocations):
    from emsanet_amd import png as P
    enc = P.PngEncoder(ring=2)
    for layout in LAYOUTS:
        stack = _dev(C.run_edge_stack(layout, 3))
        other = _dev(C.run_edge_stack(layout, 3)[::-1].copy())
        e1 = enc.encode(stack)
        e2 = enc.encode(stack)
        assert e1.turn != e2.turn and e1.data.data_ptr() != e2.data.data_ptr()
        f1 = [bytes(f) for f in enc.to_host(e1)]                 # read after call k + 1 was queued
        f2 = [bytes(f) for f in enc.to_host(e2)]
        assert f1 == f2
        assert torch.equal(e1.offsets, e2.offsets)
        e3 = enc.encode(other)                                   # call k + 2 reuses the set of call k ...
        assert e3.data.data_ptr() == e1.data.data_ptr()
        assert [bytes(f) for f in enc.to_host(e2)] == f1         # ... and leaves the set of call k + 1 alone
        f3 = [bytes(f) for f in enc.to_host(e3)]
        assert f3 == f1[::-1]                                    # a file depends on its own image only
        guard_allocations.check()


class _Meta(list):
    device_tables = None


def _synthetic(n=2, h=96, w=128, seed=11):
    """a post-processed prediction and a labelled batch, blocky, in the dtypes the post-processing yields"""
    g = torch.Generator().manual_seed(seed)

    def blocks(high, dtype, size=16):
        t = torch.randint(0, high, (n, h // size, w // size), generator=g)
        return t.repeat_interleave(size, 1).repeat_interleave(size, 2).to(dtype).contiguous().to(DEV)
    inst = blocks(5, torch.int32, 32)
    pred = {'semantic_segmentation_idx': blocks(40, torch.int64),
            'panoptic_segmentation_deeplab_semantic_idx': blocks(41, torch.int64),
            'panoptic_segmentation_deeplab_instance_idx': inst}
    counts = [torch.bincount(inst[i].flatten().cpu().long(), minlength=6) for i in range(n)]
    pred['panoptic_segmentation_deeplab_instance_meta'] = _Meta(
        [{j: ({'area': int(counts[i][j]), 'semantic_idx': 3 + j, 'panoptic_score': 0.5 + 0.01 * j + 0.1 * i}
              if counts[i][j] else {'area': 0}) for j in range(1, 6)} for i in range(n)])
    sem_gt, inst_gt = blocks(41, torch.uint8), blocks(7, torch.int32, 32)
    batch = {'semantic': sem_gt, 'instance': inst_gt, 'panoptic': sem_gt.long() * 1000 + inst_gt.long()}
    return pred, batch


def test_packer_to_files_end_to_end(tmp_path, guard_allocations):
    from emsanet_amd import InferenceOutputPacker
    from emsanet_amd import png as P
    pred, batch = _synthetic()
    packer = InferenceOutputPacker(('scannet-semantic', 'scannet-instance', 'scannet-panoptic'), 1000,
                                   write_ground_truth=True)
    packed = packer.pack(pred, batch)
    want = packer.to_host(packed).synchronize()
    packer.check()
    keys = {'scannet_semantic/pred_path_semantic', 'scannet_semantic/pred_path_panoptic_semantic',
            'scannet_semantic/gt_path', 'scannet_panoptic/pred_path', 'scannet_panoptic/gt_path',
            'scannet_instance/gt_path'}
    assert set(packed) == keys
    enc = P.PngEncoder(ring=2)
    encoded = enc.encode_packed(packed)
    assert set(encoded) == keys and len({e.turn for e in encoded.values()}) == 1
    files = {k: [bytes(f) for f in enc.to_host(e)] for k, e in encoded.items()}
    for k in keys:
        assert len(files[k]) == 2
        for i, f in enumerate(files[k]):
            got = C.decode_checked(f)
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k][i]), (k, i)
    assert want['scannet_instance/gt_path'].dtype == np.uint16 and want['scannet_panoptic/pred_path'].shape[-1] == 3

    names = ['scene0707_00_000000', 'scene0707_00_000200']
    out = packer.instance_outputs(pred, batch, names)
    assert out.masks.shape[0] == out.start[-1] >= 2
    mask_files = [bytes(f) for f in enc.to_host(enc.encode(out.masks))]
    masks = out.masks.cpu().numpy()
    for i, f in enumerate(mask_files):
        assert np.array_equal(C.decode_checked(f), masks[i])
    guard_allocations.check()

    root = str(tmp_path / 'run')
    P.write_scannet_output(files, [b + '.png' for b in names], root, instance=out, instance_files=mask_files)
    for k in keys:
        for i, b in enumerate(names):
            with open(os.path.join(root, *k.split('/'), b + '.png'), 'rb') as fh:
                assert np.array_equal(C.decode(fh.read()), want[k][i]), (k, i)
    d = os.path.join(root, 'scannet_instance', 'pred_path_panoptic_instance')
    for i, b in enumerate(names):
        with open(os.path.join(d, b + '.txt')) as fh:
            lines = fh.readlines()
        assert lines == out.lines[i] and len(lines) == out.start[i + 1] - out.start[i]
        for r, line in enumerate(lines):
            rel = line.split(' ')[0]
            assert rel == f"predicted_masks/{b}_{r:03d}.png"
            with open(os.path.join(d, rel), 'rb') as fh:
                assert np.array_equal(C.decode(fh.read()), masks[out.start[i] + r])


def test_encode_replayed_from_a_graph(guard_allocations, monkeypatch):
    """`ring` eager calls create the buffers; then encode() alone is captured on a side stream (a linear
    graph) and replayed after the source stack was overwritten in place"""
    from emsanet_amd import _lib
    from emsanet_amd import png as P
    first = C.run_edge_stack(C.BGR8, 2)
    second = np.ascontiguousarray(first[::-1, ::-1])
    stack = _dev(first)
    enc = P.PngEncoder(ring=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    # a first call while the stream captures is refused before anything is allocated or launched
    # (the capture state is stubbed: a real capture is not broken off to show it)
    fresh = P.PngEncoder(ring=2)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(_lib.EmsaError, match='capturing'):
            fresh.encode(stack)
    assert not fresh._buf
    with torch.cuda.stream(side):
        for _ in range(enc.ring):
            enc.encode(stack)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            e = enc.encode(stack)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for i, f in enumerate(enc.to_host(e)):
        assert np.array_equal(C.decode(bytes(f)), first[i])
    stack.copy_(_dev(second))
    graph.replay()
    torch.cuda.synchronize()
    for i, f in enumerate(enc.to_host(e)):
        assert np.array_equal(C.decode(bytes(f)), second[i])
