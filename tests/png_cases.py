"""Shared inputs of the PNG tests (NumPy, seeded, no reference data) and a decoder that shares nothing
with the code under test: chunks parsed by hand, every CRC checked with zlib.crc32, the IDAT payloads
joined and inflated with zlib, the filters undone here."""
import io
import struct
import zlib

import numpy as np

GRAY8, BGR8, GRAY16 = 0, 1, 2
BPP = {GRAY8: 1, BGR8: 3, GRAY16: 2}
SIGNATURE = b'\x89PNG\r\n\x1a\n'


# ---- inputs ---------------------------------------------------------------------------------------
def blob_maps(H, W):
    """-> {layout: image}: 40 discs drawn in order over a zero map; class in 1 ... 40, instance 0 or
    (k + 1) * 37.  GRAY8: the class map; BGR8: B = inst & 255, G = inst >> 8, R = class; GRAY16:
    class * 1000 + inst % 1000"""
    rng = np.random.default_rng(0)
    cls = np.zeros((H, W), np.int64)
    inst = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    for k in range(40):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(20, 120)
        c = rng.integers(1, 41)
        i = rng.integers(0, 2) * (k + 1) * 37
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        cls[disc] = c
        inst[disc] = i
    return {GRAY8: cls.astype(np.uint8),
            BGR8: np.stack([inst & 255, inst >> 8, cls], 2).astype(np.uint8),
            GRAY16: (cls * 1000 + inst % 1000).astype(np.uint16)}


RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519)
EDGE_VALUES = (0, 143, 144, 255, 7, 200)
EDGE_WIDTH = 1100


_ROW_PLAN = ((1, 2, 3, 4, 257, 258, 259), (260, 516), (261, 517), (519,))     # each fits 1100 - 66


def run_edge_pixels():
    """(27, 1100) int64 'pixel ids' (pixels_to_image turns an id into a layout's sample bytes).
    20 rows: for every start offset 62 ... 66, four rows that lay out runs of exactly 1, 2, 3, 4, 257,
    258, 259, 260, 261, 516, 517, 519 equal pixels, each followed by one separator, over a ground without
    equal neighbours -- the offsets and the odd scanline length put the runs across the 64-byte tile
    borders at every phase.  Run ids 9, 10, 11 and the separator map to bytes on both sides of the 8- /
    9-bit literal border (143, 144, 255, 0).  Then a run that ends one row and goes on in the next (it
    may only be joined over the filter byte if that byte is kept), and five constant rows, which cross
    a strip border and every tile border inside them."""
    W = EDGE_WIDTH
    rows, k = [], 0
    for off in (62, 63, 64, 65, 66):
        for plan in _ROW_PLAN:
            row = np.arange(W) % 5 + 1
            x = off
            for L in plan:
                row[x:x + L] = 9 + k % 3
                row[x + L] = 20
                x += L + 1
                k += 1
            assert x <= W
            rows.append(row)
    head, nxt = np.arange(W) % 7 + 1, np.arange(W) % 7 + 1
    head[-300:] = 41
    nxt[:300] = 41
    return np.stack(rows[:3] + [head, nxt] + [np.full(W, 40)] * 5 + rows[3:]).astype(np.int64)


def pixels_to_image(ids, layout):
    """ids -> image of `layout`: sample bytes on both sides of 144, 255 and 143 / 144 included"""
    table = np.array([(i * 53 + 11) % 256 for i in range(64)], np.int64)
    table[9], table[10], table[11], table[20], table[30], table[40], table[41] = 143, 144, 255, 0, 145, 255, 143
    v = table[ids % 64]
    if layout == GRAY8:
        return v.astype(np.uint8)
    if layout == BGR8:
        return np.stack([v, (v + 1) % 256, 255 - v], 2).astype(np.uint8)
    return (v * 256 + (255 - v)).astype(np.uint16)


def run_edge_stack(layout, m):
    """(m, 27, 1100[, 3]): the run-edge rows; image i is rolled by i rows and 7 i columns"""
    ids = run_edge_pixels()
    return np.stack([pixels_to_image(np.roll(ids, (i, 7 * i), (0, 1)), layout) for i in range(m)])


def size_cases(layout, h, w, m):
    """{name: (m, h, w[, 3]) stack} for one size: all zero, all 255 (all 65535), and m different images
    (a crop of the run-edge rows around column 62, random samples, stripes of 5 equal pixels)"""
    shape = (m, h, w, 3) if layout == BGR8 else (m, h, w)
    dt = np.uint16 if layout == GRAY16 else np.uint8
    ids = np.tile(run_edge_pixels()[:, 55:], (3, 1))
    rng = np.random.default_rng(h * 131 + w)
    mixed = [pixels_to_image(ids[:h, :w], layout),
             rng.integers(0, 256 if dt == np.uint8 else 65536, shape[1:]).astype(dt),
             pixels_to_image((np.arange(h * w).reshape(h, w) // 5) % 64, layout)]
    return {'zeros': np.zeros(shape, dt),
            'ones': np.full(shape, 255 if dt == np.uint8 else 65535, dt),
            'mixed': np.stack(mixed[:m])}


def scanlines(image, layout):
    """the filter-0 stream of one image as PNG stores it: per row a 0, then R,G,B / big-endian samples"""
    h = image.shape[0]
    if layout == BGR8:
        body = image[:, :, ::-1].reshape(h, -1)
    elif layout == GRAY16:
        body = image.astype('>u2').view(np.uint8).reshape(h, -1)
    else:
        body = image
    return np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(body)], 1).tobytes()


# ---- decoder --------------------------------------------------------------------------------------
class PngError(ValueError):
    pass


def parse_chunks(data):
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("bad signature")
    pos, chunks = 8, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk")
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise PngError("chunk runs past the file")
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise PngError(f"CRC of chunk {kind!r} at {pos}")
        chunks.append((kind, body))
        pos += 12 + n
        if kind == b'IEND':
            break
    if pos != len(data):
        raise PngError("bytes behind IEND")
    return chunks


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def decode(data):
    """-> image as the encoder was given it: uint8 (H, W), uint8 (H, W, 3) in B,G,R order, uint16 (H, W)"""
    chunks = parse_chunks(data)
    kinds = [k for k, _ in chunks]
    if kinds[0] != b'IHDR' or kinds[-1] != b'IEND' or len(chunks[0][1]) != 13 or chunks[-1][1] != b'':
        raise PngError(f"chunk order {kinds[:3]} ... {kinds[-1]}")
    idat = [i for i, k in enumerate(kinds) if k == b'IDAT']
    if not idat or idat != list(range(idat[0], idat[0] + len(idat))):
        raise PngError("IDAT chunks missing or not consecutive")
    W, H, depth, color, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    if (depth, color) not in ((8, 0), (8, 2), (16, 0)) or comp or filt or lace:
        raise PngError(f"IHDR depth {depth} colour {color} compression {comp} filter {filt} interlace {lace}")
    bpp = {(8, 0): 1, (8, 2): 3, (16, 0): 2}[(depth, color)]
    try:
        raw = zlib.decompress(b''.join(chunks[i][1] for i in idat))       # checks the Adler-32
    except zlib.error as e:
        raise PngError(f"zlib: {e}")
    stride = W * bpp
    if len(raw) != H * (1 + stride):
        raise PngError(f"{len(raw)} scanline bytes for {H} x (1 + {stride})")
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + stride)
    if rows[:, 0].max() > 4:
        raise PngError("illegal filter type")
    out = np.zeros((H, stride), np.uint8)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:]
        if f == 0:
            out[y] = line
            continue
        up = out[y - 1] if y else np.zeros(stride, np.uint8)
        cur = out[y]
        for x in range(stride):
            a = int(cur[x - bpp]) if x >= bpp else 0
            b = int(up[x])
            c = int(up[x - bpp]) if x >= bpp and y else 0
            pred = (a, b, (a + b) // 2, _paeth(a, b, c))[f - 1]
            cur[x] = (int(line[x]) + pred) & 255
    if bpp == 1:
        return out
    if bpp == 3:
        return np.ascontiguousarray(out.reshape(H, W, 3)[:, :, ::-1])
    return out.view('>u2').astype(np.uint16).reshape(H, W)


def decode_checked(data):
    """decode(), and PIL (when it imports) must read the same pixels"""
    img = decode(data)
    try:
        from PIL import Image
    except ImportError:
        return img
    pil = np.asarray(Image.open(io.BytesIO(bytes(data))))
    if img.ndim == 3:
        pil = pil[:, :, ::-1]
    if not (pil.shape == img.shape and np.array_equal(pil.astype(np.int64), img.astype(np.int64))):
        raise PngError("PIL reads other pixels")
    return img


def frame(image, layout, level=1, idat_split=0):
    """a PNG file made with zlib and hand framing (the decoder's own test vector)"""
    def chunk(kind, body):
        return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)
    h, w = image.shape[:2]
    depth, color = {GRAY8: (8, 0), BGR8: (8, 2), GRAY16: (16, 0)}[layout]
    z = zlib.compress(scanlines(image, layout), level)
    parts = [z] if not idat_split else [z[:idat_split], z[idat_split:]]
    return SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, color, 0, 0, 0)) + \
        b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b'')
