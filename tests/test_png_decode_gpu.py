"""PNG files decoded on the device (emsanet_amd/png.py PngDecoder, csrc/png_decode.hip) against NumPy images
that zlib, the independent decoder of png_cases.py and Pillow agree on (png_decode_cases.py): every comparison
is exact.  Every output, status and scratch buffer is poisoned and guard-banded (tests/guard.py), the file
bytes lie flush between guard bands too.  Malformed files are the vectors the sanitized host build of the
same decode core has passed (test_png_decode.py); each is decoded once."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_decode_cases as D   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401

C = D.C
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAYOUTS = D.LAYOUTS


def _by_name():
    return {(e['name'], e['layout']): e for e in D.corpus()}


def _entry(img, layout, **kw):
    return dict(file=D.checked(D.frame_filtered(img, layout, **kw), img, layout), layout=layout,
                h=img.shape[0], w=img.shape[1], image=img, status=D.OK)


def _files(entries, arena=None):
    """the entries' files on the device; with an arena the bytes lie flush between guard bands"""
    from emsanet_amd import PngFiles
    f = PngFiles.from_bytes([e['file'] for e in entries]).to(DEV)
    if arena is not None:
        f = PngFiles(arena.put(f.data), f.offsets, f.m, f.layout, f.h, f.w, f.file_bytes)
    return f


def _want(e, order='rgb'):
    if e['image'] is None:
        shape = (e['h'], e['w'], 3) if e['layout'] == D.BGR8 else (e['h'], e['w'])
        return np.zeros(shape, np.uint16 if e['layout'] == D.GRAY16 else np.uint8)
    return e['image'][:, :, ::-1] if (order == 'bgr' and e['layout'] == D.BGR8) else e['image']


def _exact(entries, arena, order='rgb', dec=None):
    """one decode call over `entries`; every image must equal its source; -> the stack"""
    from emsanet_amd import PngDecoder
    dec = dec or PngDecoder(ring=1, order=order)
    stack = dec.decode(_files(entries, arena))
    dec.check()
    got = stack.cpu().numpy()
    assert got.shape[0] == len(entries)
    for i, e in enumerate(entries):
        want = _want(e, order)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape, (i, got.dtype, got.shape)
        assert np.array_equal(got[i], want), (i, e.get('name'), int((got[i] != want).sum()))
    if arena is not None:
        arena.check()
    return stack


@pytest.mark.parametrize('layout', LAYOUTS)
def test_sizes(layout, guard_allocations):
    """below one tile, one band, one row; odd sizes; more rows than one band of 64; M = 1 and 3 with three
    different images (smooth, noise, flat) and the five filter types cycling from three different starts;
    67 x 129 with M = 5; the widest and the tallest image"""
    names = _by_name()
    for h, w in D.SIZES:
        three = [names[(f'size_{h}x{w}_{i}', layout)] for i in range(3)]
        _exact(three[:1], guard_allocations)
        _exact(three, guard_allocations, order='bgr')
    _exact([_entry(D.make_image(layout, 67, 129, 20 + i, ('smooth', 'noise')[i % 2]), layout,
                   filters=D.ALL_FILTERS[i:] + D.ALL_FILTERS[:i]) for i in range(5)], guard_allocations)
    for h, w in ((3, 4096), (4096, 3)):
        _exact([_entry(D.make_image(layout, h, w, 30), layout, filters=D.ALL_FILTERS)], guard_allocations)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_training_size(layout, guard_allocations):
    """480 x 640: noise over a gradient, the five filters cycling, 8 KiB IDAT chunks as libpng writes them"""
    img = D.make_image(layout, 480, 640, 40)
    e = _entry(img, layout, filters=D.ALL_FILTERS, idat_split=8192)
    assert e['file'].count(b'IDAT') >= 8
    _exact([e], guard_allocations)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_filters(layout, guard_allocations):
    """each type on every row, all five cycling, types 2, 3, 4 on row 0 (the row above is zero), at 9 x 70 and
    at 130 x 67 (more rows than one band, odd stride): one call of nine files per size"""
    names = _by_name()
    for h, w in ((9, 70), (130, 67)):
        _exact([names[(f'filters_{h}x{w}_{k}', layout)] for k in range(len(D.FILTER_PLANS))], guard_allocations)


def test_deflate_forms(guard_allocations):
    """zlib levels 0 (stored), 1, 6, 9; Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE; windows of 512 bytes and 32 KiB: one
    call.  Then 256 x 256 x 3 of noise over a gradient, long enough for several dynamic blocks"""
    names = _by_name()
    forms = ['level_0', 'level_1', 'level_6', 'level_9', 'strategy_fixed', 'strategy_huffman_only', 'strategy_rle',
             'wbits_9', 'wbits_15']
    _exact([names[(n, D.BGR8)] for n in forms], guard_allocations)
    img = D.make_image(D.BGR8, 256, 256, 41)
    e = _entry(img, D.BGR8, filters=0, level=6)
    z = b''.join(b for k, b in C.parse_chunks(e['file']) if k == b'IDAT')
    assert len(z) > 100000                         # zlib closes a block every 16383 symbols at this level
    _exact([e], guard_allocations)


@pytest.mark.parametrize('name', [n for n, *_ in D.hand_made()])
def test_hand_made_streams(name, guard_allocations):
    """empty stored block and a stored block of 65535; length 258 at distance 1 over scanline ends; distance <
    length with a non-dividing length; distance 32768; a distance tree of one code and 15-bit codes; 16 / 17 /
    18 repeats over the literal/distance border"""
    _exact([_by_name()[(name, D.GRAY8)]], guard_allocations)


def test_chunking(guard_allocations):
    """the IDAT split at each of the first 40 byte positions of the stream (40 files, one call): in the zlib
    header, in the dynamic block header, in the middle of codes; 1-byte IDATs; ancillary chunks in front of,
    and behind, IDATs split at 3 and 11"""
    img = D.make_image(D.BGR8, 33, 40, 50)
    z = D.deflate(D.filter_scanlines(img, D.BGR8, D.ALL_FILTERS))
    assert (z[2] >> 1) & 3 == 2 and len(z) > 80
    entries = [dict(file=D.checked(D.frame_stream(z, D.BGR8, 33, 40, idat_split=(p,)), img, D.BGR8),
                    layout=D.BGR8, h=33, w=40, image=img) for p in range(1, 41)]
    _exact(entries, guard_allocations)
    names = _by_name()
    _exact([names[('one_byte_idats', D.GRAY16)], names[('ancillary_chunks', D.GRAY16)]], guard_allocations)


def test_other_producers(guard_allocations):
    """Pillow's encoder (its own filter choice per row), optimize=True and compress_level 1 / 6 / 9, over the
    blob maps and a noisy RGB image"""
    from PIL import Image

    def pil(img, **kw):
        f = io.BytesIO()
        Image.fromarray(img).save(f, format='PNG', **kw)
        return f.getvalue()
    blobs = C.blob_maps(120, 160)
    rng = np.random.default_rng(60)
    noisy = (np.clip(D.make_image(D.BGR8, 120, 160, 61).astype(np.int64) + rng.integers(-20, 21, (120, 160, 3)),
                     0, 255)).astype(np.uint8)
    for layout, img in ((D.GRAY8, blobs[D.GRAY8]), (D.BGR8, blobs[D.BGR8]), (D.GRAY16, blobs[D.GRAY16]),
                        (D.BGR8, noisy)):
        kws = [dict(optimize=True), dict(compress_level=1), dict(compress_level=6), dict(compress_level=9)]
        _exact([dict(file=D.checked(pil(img, **kw), img, layout), layout=layout, h=120, w=160, image=img)
                for kw in kws], guard_allocations)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_round_trip_through_the_encoder(layout, guard_allocations):
    """PngEncoder.encode -> PngFiles.from_encoded -> decode(order='bgr') gives the stack back; the files never
    leave the device"""
    from emsanet_amd import PngDecoder, PngEncoder, PngFiles
    stack = torch.from_numpy(np.ascontiguousarray(C.run_edge_stack(layout, 3)[:, :, :300])).to(DEV)
    enc, dec = PngEncoder(ring=1), PngDecoder(ring=1, order='bgr')
    files = PngFiles.from_encoded(enc.encode(stack))
    assert files.data.is_cuda and (files.layout, files.m, files.h, files.w) == (layout, 3, 27, 300)
    back = dec.decode(files)
    dec.check()
    assert back.dtype == stack.dtype and torch.equal(back, stack)
    guard_allocations.check()


_MALFORMED = {n: (f, layout, h, w, status) for n, f, layout, h, w, status in D.malformed()}


@pytest.mark.parametrize('name', list(_MALFORMED))
def test_malformed(name, guard_allocations):
    """the bad file between two good ones, one call, run once: its status, its all-zero image, the exact
    neighbours, intact guard bands, and check() names index 1"""
    from emsanet_amd import PngDecodeError, PngDecoder
    f, layout, h, w, status = _MALFORMED[name]
    good = [_entry(D.make_image(layout, h, w, 70 + i, 'noise'), layout, filters=D.ALL_FILTERS) for i in range(2)]
    bad = dict(file=f, layout=layout, h=h, w=w, image=None)
    entries = [good[0], bad, good[1]]
    from emsanet_amd import PngFiles
    host = b''.join(e['file'] for e in entries)
    offsets = torch.tensor(np.cumsum([0] + [len(e['file']) for e in entries]), dtype=torch.int64)
    data = guard_allocations.put(torch.frombuffer(bytearray(host), dtype=torch.uint8).to(DEV))
    files = PngFiles(data, offsets.to(DEV), 3, layout, h, w, max(len(e['file']) for e in entries))
    dec = PngDecoder(ring=1)
    stack = dec.decode(files)
    assert dec.status.cpu().tolist() == [0, status, 0]
    got = stack.cpu().numpy()
    for i, e in enumerate(entries):
        assert np.array_equal(got[i], _want(e)), i
    guard_allocations.check()
    with pytest.raises(PngDecodeError, match='file 1') as info:
        dec.check()
    assert (info.value.index, info.value.status) == (1, status) and len(info.value.failures) == 1
    dec.check()                                    # checked statuses are not reported twice


def test_offsets_outside_the_buffer_are_refused_per_file(guard_allocations):
    """an offsets table that points outside the data: nothing is read, the files get EMSA_PNGD_CHUNK"""
    from emsanet_amd import PngDecoder, PngFiles
    e = _by_name()[('size_7x5_0', D.GRAY8)]
    f = _files([e, e, e], guard_allocations)
    n = len(e['file'])
    f.offsets.copy_(torch.tensor([0, n, 5 * n, 3 * n], dtype=torch.int64))
    dec = PngDecoder(ring=1)
    stack = dec.decode(f)
    assert dec.status.cpu().tolist() == [0, D.CHUNK, D.CHUNK]
    assert np.array_equal(stack[0].cpu().numpy(), e['image']) and not bool(stack[1:].any())


def test_two_decodes_are_bit_equal_and_the_ring_keeps_the_first(guard_allocations):
    from emsanet_amd import PngDecoder
    names = _by_name()
    for layout in LAYOUTS:
        entries = [names[(f'size_65x259_{i}', layout)] for i in range(3)]
        dec = PngDecoder(ring=2)
        files = _files(entries, guard_allocations)
        a = dec.decode(files)
        b = dec.decode(files)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
        c = dec.decode(_files(entries[::-1], guard_allocations))
        assert c.data_ptr() == a.data_ptr() and torch.equal(c, b.flip(0))
        dec.check()
        guard_allocations.check()


def test_decode_replayed_from_a_graph(guard_allocations, monkeypatch):
    """`ring` eager calls create the buffers; then decode() alone is captured on a side stream and replayed
    after other files were copied into the same byte buffer and offsets table"""
    from emsanet_amd import PngDecoder, PngFiles, _lib
    names = _by_name()
    first = [names[(f'size_33x130_{i}', D.BGR8)] for i in (0, 1)]
    second = [names[(f'size_33x130_{i}', D.BGR8)] for i in (2, 0)]
    a, b = (PngFiles.from_bytes([e['file'] for e in es]) for es in (first, second))
    room = max(a.data.numel(), b.data.numel())
    data = torch.zeros(room, dtype=torch.uint8, device=DEV)
    offsets = torch.zeros(3, dtype=torch.int64, device=DEV)
    files = PngFiles(data, offsets, 2, D.BGR8, 33, 130, max(a.file_bytes, b.file_bytes))

    def load(src):
        data[:src.data.numel()].copy_(src.data)
        offsets.copy_(src.offsets)
    load(a)
    dec = PngDecoder(ring=2)
    fresh = PngDecoder(ring=2)
    with monkeypatch.context() as mp:              # (the capture state is stubbed: no real capture is broken off)
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(_lib.EmsaError, match='capturing'):
            fresh.decode(files)
    assert not fresh._buf
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(dec.ring):
            dec.decode(files)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            stack = dec.decode(files)
    torch.cuda.current_stream().wait_stream(side)
    for src, entries in ((a, first), (b, second)):
        load(src)
        graph.replay()
        torch.cuda.synchronize()
        dec.check()
        got = stack.cpu().numpy()
        for i, e in enumerate(entries):
            assert np.array_equal(got[i], e['image']), i


def _png_batches(raw):
    from emsanet_amd import PngFiles

    def files(a, layout):
        return PngFiles.from_bytes([D.frame_filtered(img, layout, filters=D.ALL_FILTERS, idat_split=8192)
                                    for img in a])
    for j, b in enumerate(raw):
        hb = {'rgb': files(b['rgb'], D.BGR8), 'depth': files(b['depth'], D.GRAY16),
              'semantic': files(b['semantic'], D.GRAY8), 'instance': files(b['instance'], D.GRAY16),
              'orientations': torch.from_numpy(b['orientations']).pin_memory(),
              'scene': torch.from_numpy(b['scene']).pin_memory(), 'name': f'batch{j}'}
        yield hb


def _array_batches(raw):
    for j, b in enumerate(raw):
        hb = {k: torch.from_numpy(v).pin_memory() for k, v in b.items()}
        hb['name'] = f'batch{j}'
        yield hb


def test_batch_stager_decodes_png_batches():
    """two batches of rgb / depth / semantic / instance files at 64 x 96: what the stager hands out equals what
    it hands out for the decoded arrays, bit for bit -- plain, and with an augmenter and a target generator"""
    import augment_reference as R
    from test_augment_gpu import STATS, _args, _aug, _generator, _same, _same_targets
    from emsanet_amd import PngDecoder
    from emsanet_amd.staging import BatchStager
    n, h, w = 2, 64, 96
    raw = [R.random_batch(n, h, w, seed=80 + j) for j in range(2)]
    assert raw[0]['semantic'].dtype == np.uint8 and raw[0]['instance'].dtype == np.uint16

    dec = PngDecoder(ring=2)
    stager = BatchStager(_png_batches(raw), DEV, depth_stats=STATS, decoder=dec)
    got = list(stager)
    dec.check()
    want = list(BatchStager(_array_batches(raw), DEV, depth_stats=STATS))
    assert len(got) == len(want) == 2
    file_bytes = sum(v.data.numel() for hb in _png_batches(raw) for v in hb.values() if hasattr(v, 'file_bytes'))
    small = sum(raw[0][k].nbytes + raw[1][k].nbytes for k in ('orientations', 'scene'))
    assert stager.bytes_staged == file_bytes + small
    for g, x in zip(got, want):
        assert sorted(g) == sorted(x) and g['name'] == x['name']
        for k in x:
            if torch.is_tensor(x[k]):
                assert _same(g[k], x[k]), k

    args = _args(h, w)
    dec = PngDecoder(ring=2)
    got = list(BatchStager(_png_batches(raw), DEV, decoder=dec, augmenter=_aug(h, w, seed=6, ring=2),
                           target_generator=_generator(args, ring=2)))
    dec.check()
    want = list(BatchStager(_array_batches(raw), DEV, augmenter=_aug(h, w, seed=6, ring=2),
                            target_generator=_generator(args, ring=2)))
    torch.cuda.synchronize()
    for g, x in zip(got, want):
        assert sorted(g) == sorted(x)
        for k in x:
            if torch.is_tensor(x[k]):
                assert _same(g[k], x[k]), k
        _same_targets(g['targets'], x['targets'])

    with pytest.raises(Exception, match='no decoder'):
        next(iter(BatchStager(_png_batches(raw), DEV)))
