"""CPU: the host side of the PNG encoder (emsanet_amd/png.py, the argument checks of csrc/png.hip) and
the decoder the GPU tests judge the device's files with (tests/png_cases.py)."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as C   # noqa: E402

E_SHAPE = -1


def _closed_form(layout, h, w):
    """the bound from the format, strip by strip: bits -> bytes, then the framing"""
    n_row = 1 + w * C.BPP[layout]
    total = 8 + 25 + 12 + 2 + 4                                   # signature, IHDR, IEND, zlib header, Adler
    for first in range(0, h, 4):
        n = min(4, h - first) * n_row
        bits = 3 + 9 * n + 7 + 3                                 # block header, literals >= 144, EOB, stored header
        total += 12 + (bits + 7) // 8 + 4                        # chunk framing, padding, LEN / NLEN
    return total + 5                                             # the final empty stored block


def test_png_bound_closed_form_and_monotonic():
    from emsanet_amd import png as P
    from emsanet_amd import _lib
    L = _lib.lib()
    sizes = [(1, 1), (1, 7), (5, 1), (7, 5), (33, 130), (64, 64), (65, 259), (480, 640), (968, 1296),
             (4096, 4096), (4095, 4096), (3, 4096), (4096, 1)]
    for layout in (P.GRAY8, P.BGR8, P.GRAY16):
        for h, w in sizes:
            b = P.png_bound(layout, h, w)
            assert b == _closed_form(layout, h, w), (layout, h, w)
            assert b == L.emsa_png_bound(layout, h, w), (layout, h, w)
            raw = h * (1 + w * C.BPP[layout])
            assert b >= 1.125 * raw + 8 + 25 + 12 + 2 + 4
        for h in range(1, 40):
            assert P.png_bound(layout, h + 1, 33) > P.png_bound(layout, h, 33)
            assert P.png_bound(layout, 33, h + 1) > P.png_bound(layout, 33, h)
    assert (P.GRAY8, P.BGR8, P.GRAY16) == (C.GRAY8, C.BGR8, C.GRAY16) == (0, 1, 2)
    for bad in ((3, 4, 4), (-1, 4, 4)):
        with pytest.raises(ValueError):
            P.png_bound(*bad)
    for h, w in ((0, 4), (4, 0), (4097, 4), (4, 4097)):
        with pytest.raises(ValueError):
            P.png_bound(P.GRAY8, h, w)
        assert L.emsa_png_bound(P.GRAY8, h, w) == E_SHAPE
        assert L.emsa_png_ws_bytes(P.GRAY8, 1, h, w) == E_SHAPE


def test_workspace_holds_a_worst_case_slot_per_strip():
    from emsanet_amd import png as P
    from emsanet_amd import _lib
    L = _lib.lib()
    for layout in (P.GRAY8, P.BGR8, P.GRAY16):
        for m, h, w in ((1, 1, 1), (3, 65, 259), (32, 480, 640)):
            strips = (h + 3) // 4
            slot = (9 * 4 * (1 + w * C.BPP[layout]) + 20) // 8 + 9
            assert L.emsa_png_ws_bytes(layout, m, h, w) >= m * strips * (slot + 16 + 8)
    assert L.emsa_png_ws_bytes(P.GRAY8, 0, 4, 4) == E_SHAPE and L.emsa_png_ws_bytes(3, 1, 4, 4) == E_SHAPE


def test_layout_inference_and_refusals():
    from emsanet_amd import png as P
    z = lambda dt, *s: torch.zeros(s, dtype=dt)   # noqa: E731
    assert P.infer_layout(z(torch.uint8, 2, 4, 5)) == P.GRAY8
    assert P.infer_layout(z(torch.uint8, 2, 4, 5, 3)) == P.BGR8
    assert P.infer_layout(z(torch.uint16, 2, 4, 5)) == P.GRAY16
    enc = P.PngEncoder()
    with pytest.raises(NotImplementedError):
        enc.encode(z(torch.uint8, 2, 4, 5))                           # a CPU tensor
    with pytest.raises(TypeError):
        enc.encode(z(torch.int32, 2, 4, 5))
    with pytest.raises(TypeError):
        enc.encode(np.zeros((2, 4, 5), np.uint8))
    for shape in ((2, 4, 5, 4), (4, 5), (2, 4, 5, 3, 1)):
        with pytest.raises(ValueError):
            enc.encode(z(torch.uint8, *shape))
    with pytest.raises(ValueError):
        enc.encode(z(torch.uint16, 2, 4, 5, 3))
    for shape in ((2, 0, 5), (2, 5, 0), (0, 4, 5), (1, 4097, 2), (1, 2, 4097)):
        with pytest.raises(ValueError):
            enc.encode(z(torch.uint8, *shape))
    with pytest.raises(ValueError):
        enc.encode(z(torch.uint8, 2, 4, 5), layout=P.BGR8)            # the layout against the stack
    with pytest.raises(ValueError):
        P.PngEncoder(ring=0)
    assert enc._turn == -1 and not enc._buf                           # nothing advanced, nothing allocated


def test_c_call_refuses_before_any_launch():
    """geometry first (EMSA_E_SHAPE with null pointers, as test_capi_symbols.test_geometry_rejected_cleanly),
    then the pointers"""
    from emsanet_amd import png as P
    from emsanet_amd import _lib
    L = _lib.lib()
    b = P.png_bound(P.BGR8, 7, 5)
    enc = lambda layout, m, h, w, nbytes: L.emsa_png_encode(None, layout, m, h, w, None, nbytes, None, None, None)   # noqa: E731
    assert enc(P.BGR8, 3, 7, 5, 3 * b - 1) == E_SHAPE                 # data_bytes too small
    assert enc(P.BGR8, 3, 7, 5, 0) == E_SHAPE
    for h, w in ((0, 5), (7, 0), (4097, 5), (7, 4097)):
        assert enc(P.GRAY8, 1, h, w, 1 << 40) == E_SHAPE
    assert enc(3, 1, 7, 5, 1 << 40) == E_SHAPE and enc(-1, 1, 7, 5, 1 << 40) == E_SHAPE
    assert enc(P.GRAY8, 0, 7, 5, 1 << 40) == E_SHAPE
    assert enc(P.BGR8, 3, 7, 5, 3 * b) == -2                          # EMSA_E_ARG: null pointers


def test_write_scannet_output_tree(tmp_path):
    from emsanet_amd import png as P
    from emsanet_amd.export import InstanceOutputs, instance_line
    names = ['scene0707_00_000000.png', 'scene0707_00_000200.png']
    files = {'scannet_semantic/pred_path_semantic': [b'a0', memoryview(b'a1')],
             'scannet_semantic/pred_path_panoptic_semantic': [b'b0', b'b1'],
             'scannet_semantic/gt_path': [b'c0', b'c1'],
             'scannet_panoptic/pred_path': [b'd0', b'd1'],
             'scannet_instance/gt_path': [b'e0', b'e1']}
    lines = [[instance_line('scene0707_00_000000', 0, 33, 0.72341), instance_line('scene0707_00_000000', 1, 5, 0.9038)],
             []]
    inst = InstanceOutputs(None, lines, [0, 2, 2])
    out = str(tmp_path / 'out')
    written = P.write_scannet_output(files, names, out, instance=inst, instance_files=[b'm0', b'm1'])
    tree = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    want = sorted([f"{k}/{n}" for k in files for n in names] +
                  ['scannet_instance/pred_path_panoptic_instance/predicted_masks/scene0707_00_000000_000.png',
                   'scannet_instance/pred_path_panoptic_instance/predicted_masks/scene0707_00_000000_001.png',
                   'scannet_instance/pred_path_panoptic_instance/scene0707_00_000000.txt',
                   'scannet_instance/pred_path_panoptic_instance/scene0707_00_000200.txt'])
    assert tree == [w.replace('/', os.sep) for w in want]
    assert sorted(os.path.relpath(w, out) for w in written) == tree
    assert open(os.path.join(out, 'scannet_semantic', 'pred_path_semantic', names[1]), 'rb').read() == b'a1'
    assert open(os.path.join(out, 'scannet_panoptic', 'pred_path', names[0]), 'rb').read() == b'd0'
    d = os.path.join(out, 'scannet_instance', 'pred_path_panoptic_instance')
    assert open(os.path.join(d, 'predicted_masks', 'scene0707_00_000000_001.png'), 'rb').read() == b'm1'
    assert open(os.path.join(d, 'scene0707_00_000000.txt')).read() == \
        'predicted_masks/scene0707_00_000000_000.png 33 0.7234\npredicted_masks/scene0707_00_000000_001.png 5 0.9038\n'
    assert open(os.path.join(d, 'scene0707_00_000200.txt')).read() == ''
    with pytest.raises(ValueError):
        P.write_scannet_output({'mapping/pred_scene': [b'', b'']}, names, out)
    with pytest.raises(ValueError):
        P.write_scannet_output({'scannet_panoptic/pred_path': [b'x']}, names, out)
    with pytest.raises(ValueError):
        P.write_scannet_output({}, names, out, instance=inst, instance_files=[b'm0'])


@pytest.mark.parametrize('layout', [C.GRAY8, C.BGR8, C.GRAY16])
def test_the_decoder_accepts_zlib_files_and_rejects_damage(layout):
    img = C.blob_maps(96, 128)[layout]
    for level, split in ((1, 0), (6, 100), (0, 0)):
        f = C.frame(img, layout, level, split)
        got = C.decode_checked(f)
        assert got.dtype == img.dtype and np.array_equal(got, img)
    f = bytearray(C.frame(img, layout))
    assert np.array_equal(C.decode(bytes(f)), img)
    bad = bytearray(f)
    bad[29] ^= 0x10                                                  # a bit of the IHDR CRC
    with pytest.raises(C.PngError, match='CRC'):
        C.decode(bytes(bad))
    bad = bytearray(f)
    bad[60] ^= 0x01                                                  # a data bit: the chunk's CRC catches it
    with pytest.raises(C.PngError, match='CRC'):
        C.decode(bytes(bad))
    # a wrong Adler-32 under a right CRC
    chunks = C.parse_chunks(bytes(f))
    z = bytearray(chunks[1][1])
    z[-1] ^= 0x01
    body = bytes(z)
    broken = bytes(f[:33]) + struct.pack('>I', len(body)) + b'IDAT' + body + \
        struct.pack('>I', zlib.crc32(b'IDAT' + body) & 0xFFFFFFFF) + bytes(f[-12:])
    C.parse_chunks(broken)
    with pytest.raises(C.PngError, match='zlib'):
        C.decode(broken)
    with pytest.raises(C.PngError):
        C.decode(bytes(f) + b'\0')
    with pytest.raises(C.PngError):
        C.decode(bytes(f[:-1]))


def test_the_decoder_undoes_every_filter_type():
    """a file whose rows use filters 0 ... 4 (the encoder under test writes 0 only; the decoder must not
    depend on that)"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 9, 3)).astype(np.uint8)
    rgb = img[:, :, ::-1].reshape(5, -1).astype(np.int64)
    rows = []
    for y in range(5):
        up = rgb[y - 1] if y else np.zeros(27, np.int64)
        line = []
        for x in range(27):
            a = rgb[y, x - 3] if x >= 3 else 0
            b = up[x]
            c = up[x - 3] if x >= 3 and y else 0
            pred = (0, a, b, (a + b) // 2, C._paeth(int(a), int(b), int(c)))[y]
            line.append((rgb[y, x] - pred) & 255)
        rows.append(bytes([y]) + bytes(line))
    z = zlib.compress(b''.join(rows))
    chunk = lambda k, b: struct.pack('>I', len(b)) + k + b + struct.pack('>I', zlib.crc32(k + b) & 0xFFFFFFFF)   # noqa: E731
    f = C.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', 9, 5, 8, 2, 0, 0, 0)) + chunk(b'IDAT', z) + chunk(b'IEND', b'')
    assert np.array_equal(C.decode_checked(f), img)


def test_shared_inputs_hold_what_they_promise():
    ids = C.run_edge_pixels()
    assert ids.shape == (27, C.EDGE_WIDTH)
    runs = set()
    for row in ids:
        cut = np.flatnonzero(np.diff(row)) + 1
        for a, b in zip(np.r_[0, cut], np.r_[cut, row.size]):
            if row[a] in (9, 10, 11):
                runs.add((int(a) if a in range(62, 67) else -1, int(b - a)))
    assert {L for _, L in runs} == set(C.RUN_LENGTHS)
    assert {o for o, _ in runs} >= {62, 63, 64, 65, 66}
    g = C.pixels_to_image(ids, C.GRAY8)
    assert {0, 143, 144, 255} <= set(np.unique(g).tolist())
    assert (g[3, -300:] == g[4, 0]).all() and (g[4, :300] == g[3, -1]).all()      # the run over the row end
    maps = C.blob_maps(96, 128)
    assert maps[C.GRAY8].max() <= 40 and maps[C.BGR8].shape == (96, 128, 3) and maps[C.GRAY16].dtype == np.uint16
    for layout, img in maps.items():
        assert len(C.scanlines(img, layout)) == 96 * (1 + 128 * C.BPP[layout])
