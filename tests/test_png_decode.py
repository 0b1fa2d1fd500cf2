"""CPU side of the PNG decoder (emsanet_amd/png.py, csrc/png_decode.hip): what is refused on the host, and the
decode core itself -- csrc/png_inflate_core.h built as plain C++ into tools/png_decode_host.cpp with
AddressSanitizer and UBSan, a stand-alone program, run over the whole corpus of png_decode_cases.py, valid and
malformed.  The GPU tests send only these vectors."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_decode_cases as D   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(depth, color, interlace=0, h=5, w=7, comp=0, filt=0):
    return D.C.SIGNATURE + D.chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, color, comp, filt, interlace))


def test_png_info_supported_and_refused():
    from emsanet_amd import png_info
    from emsanet_amd import png as P
    assert png_info(_head(8, 0)) == (P.GRAY8, 5, 7)
    assert png_info(_head(8, 2)) == (P.BGR8, 5, 7)
    assert png_info(_head(16, 0)) == (P.GRAY16, 5, 7)
    assert png_info(memoryview(_head(8, 0, h=4096, w=1) + b'rest')) == (P.GRAY8, 4096, 1)
    for e in D.corpus()[:5]:
        assert png_info(e['file']) == (e['layout'], e['h'], e['w'])
    refused = [(_head(8, 3), 'palette'), (_head(8, 4), 'alpha'), (_head(8, 6), 'alpha'), (_head(16, 6), 'alpha'),
               (_head(16, 2), '16-bit RGB'), (_head(1, 0), 'below 8'), (_head(2, 0), 'below 8'),
               (_head(4, 0), 'below 8'), (_head(4, 3), 'palette'), (_head(8, 0, interlace=1), 'interlaced'),
               (_head(8, 2, interlace=1), 'interlaced'), (_head(8, 0, h=4097), 'EMSA_PNG_MAX_SIDE'),
               (_head(8, 0, w=4097), 'EMSA_PNG_MAX_SIDE'), (_head(8, 0, h=0), 'EMSA_PNG_MAX_SIDE'),
               (_head(8, 5), 'colour type 5'), (_head(12, 0), 'bit depth 12'), (_head(8, 0, comp=1), 'compression'),
               (_head(8, 0, filt=1), 'filter method'), (b'\x88' + _head(8, 0)[1:], 'not a PNG'),
               (_head(8, 0)[:32], 'not a PNG'), (b'', 'not a PNG'),
               (D.C.SIGNATURE + D.chunk(b'IDAT', b'\0' * 13), 'not a PNG')]
    for data, word in refused:
        with pytest.raises(ValueError, match=word):
            png_info(data)


def test_png_files_refusals():
    import torch
    from emsanet_amd import PngFiles, PngDecoder
    from emsanet_amd import png as P
    small = [e for e in D.corpus() if e['status'] == D.OK and (e['h'], e['w']) == (7, 5)]
    gray = [e['file'] for e in small if e['layout'] == D.GRAY8]
    wide = [e['file'] for e in small if e['layout'] == D.GRAY16]
    f = PngFiles.from_bytes(gray)
    assert (f.m, f.layout, f.h, f.w) == (len(gray), D.GRAY8, 7, 5) and f.file_bytes == max(len(g) for g in gray)
    assert f.offsets.tolist() == [0] + list(np.cumsum([len(g) for g in gray]))
    assert bytes(f.data.numpy().tobytes()) == b''.join(gray)
    with pytest.raises(ValueError, match='no files'):
        PngFiles.from_bytes([])
    with pytest.raises(ValueError, match='file 2 has layout 2'):
        PngFiles.from_bytes(gray[:2] + wide[:1])
    other = D.frame_filtered(D.make_image(D.GRAY8, 7, 6), D.GRAY8)
    with pytest.raises(ValueError, match=r'file 1 has layout 0, size 7 x 6'):
        PngFiles.from_bytes([gray[0], other])
    with pytest.raises(ValueError, match='file 1: png_info: palette'):
        PngFiles.from_bytes([gray[0], _head(8, 3)])
    with pytest.raises(ValueError, match='uint8'):
        PngFiles(f.data.to(torch.int8), f.offsets, f.m, f.layout, f.h, f.w, f.file_bytes)
    with pytest.raises(ValueError, match='layout'):
        PngFiles(f.data, f.offsets, f.m, 3, f.h, f.w, f.file_bytes)
    with pytest.raises(ValueError, match='sides'):
        PngFiles(f.data, f.offsets, f.m, 0, 4097, f.w, f.file_bytes)
    with pytest.raises(ValueError, match='bytes'):
        PngFiles(f.data, f.offsets, f.m, 0, f.h, f.w, (1 << 30) + 1)
    with pytest.raises(ValueError, match='no key'):
        PngFiles.from_encoded(P.EncodedStack(f.data, f.offsets, f.m, 0))
    with pytest.raises(NotImplementedError, match='host memory'):
        PngDecoder().decode(f)
    with pytest.raises(TypeError):
        PngDecoder().decode(gray)
    with pytest.raises(ValueError, match='order'):
        PngDecoder(order='gbr')
    with pytest.raises(ValueError, match='ring'):
        PngDecoder(ring=0)


def test_workspace_geometry_refusals():
    from emsanet_amd import _lib
    L = _lib.lib()
    ws = L.emsa_png_decode_ws_bytes
    assert ws(D.BGR8, 2, 480, 640, 1000) >= 2 * (1000 + 480 * (1 + 1920))
    assert ws(D.GRAY16, 1, 4096, 4096, 1 << 30) >= (1 << 30) + 4096 * (1 + 8192)
    assert ws(D.GRAY8, 1, 1, 1, 1) > 0
    bad = [(3, 1, 8, 8, 100), (-1, 1, 8, 8, 100), (0, 0, 8, 8, 100), (0, 65536, 8, 8, 100), (0, 1, 0, 8, 100),
           (0, 1, 8, 0, 100), (0, 1, 4097, 8, 100), (0, 1, 8, 4097, 100), (0, 1, 8, 8, 0), (0, 1, 8, 8, -5),
           (0, 1, 8, 8, (1 << 30) + 1)]
    for args in bad:
        assert ws(*args) == -1, args
    # emsa_png_decode checks geometry, order and the workspace size before any pointer or launch
    dec = L.emsa_png_decode
    assert dec(None, None, 0, 1, 3, 0, 8, 8, None, None, None, 1 << 20, None) == -1
    assert dec(None, None, 0, 1, 0, 2, 8, 8, None, None, None, 1 << 20, None) == -1
    assert dec(None, None, 0, 1, 0, 0, 8, 8, None, None, None, 8 * 9, None) == -1
    assert dec(None, None, 0, 1, 0, 0, 8, 8, None, None, None, ws(0, 1, 8, 8, 16), None) == -2


def _compiler():
    """the sanitized build needs a host compiler with the sanitizer runtimes: g++ / clang++, else hipcc with
    the flags passed to its host side"""
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if shutil.which('g++'):
        return ['g++'], san + ['-static-libasan', '-static-libubsan']       # (clang links them statically)
    if shutil.which('clang++'):
        return ['clang++'], san
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    return [hipcc, '-x', 'c++'], ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                                  '-fno-sanitize-recover=undefined']


def test_host_build_of_the_core_under_sanitizers(tmp_path):
    """every corpus entry in both channel orders: a valid one must come out to the byte, a malformed one with
    the expected status and an all-zero image, and ASan / UBSan must have nothing to report (either ends the
    program with a non-zero exit code)"""
    cxx, san = _compiler()
    exe = str(tmp_path / 'png_decode_host')
    r = subprocess.run(cxx + ['-std=c++17', '-O1', '-g'] + san +
                       ['-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tools', 'png_decode_host.cpp'),
                        '-o', exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    entries = [(e, order) for e in D.corpus() for order in ((0, 1) if e['layout'] == D.BGR8 else (0,))]
    corpus = str(tmp_path / 'corpus.bin')
    with open(corpus, 'wb') as f:
        f.write(b'PNGDCORP' + struct.pack('<i', len(entries)))
        for e, order in entries:
            f.write(struct.pack('<iiiiq', e['layout'], order, e['h'], e['w'], len(e['file'])) + e['file'])
    images = str(tmp_path / 'images.bin')
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([exe, corpus, images], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(entries)
    blob = open(images, 'rb').read()
    pos, seen = 0, set()
    for (e, order), line in zip(entries, lines):
        _, status, _ = line.split()
        n = e['h'] * e['w'] * D.BPP[e['layout']]
        got, pos = blob[pos:pos + n], pos + n
        assert int(status) == e['status'], (e['name'], order, status)
        want = bytes(n) if e['image'] is None else D.expected_bytes(e['image'], e['layout'], ('rgb', 'bgr')[order])
        assert got == want, (e['name'], order)
        seen.add(e['status'])
    assert pos == len(blob)
    assert seen == set(range(14))                 # every status code of the header has a vector
