"""Test vectors of the PNG decoder (emsanet_amd/png.py PngDecoder, csrc/png_decode.hip), made with NumPy, zlib
and a deflate bit-writer for hand-made streams.  Colour images are (H, W, 3) in R, G, B order -- the file's
own order, what `PngDecoder(order='rgb')` returns.  Every valid file is checked here with the independent
decoder of png_cases.py and with Pillow before any code under test sees it (`checked`).

`corpus()` is the list both test modules share: test_png_decode.py runs all of it through the sanitized host
build of the decode core; test_png_decode_gpu.py sends the same vectors to the device."""
import functools
import io
import struct
import zlib

import numpy as np

import png_cases as C

GRAY8, BGR8, GRAY16 = C.GRAY8, C.BGR8, C.GRAY16
LAYOUTS = (GRAY8, BGR8, GRAY16)
BPP = C.BPP
# EMSA_PNGD_* of include/emsanet_hip.h
OK, CHUNK, IHDR, TRUNCATED, ZLIB_HEADER, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, SYMBOL, DISTANCE, TOO_MANY, \
    TOO_FEW, FILTER, ADLER = range(14)


# ---- images -----------------------------------------------------------------------------------------
def make_image(layout, h, w, seed=0, kind='smooth'):
    """'noise': uniform samples; 'smooth': a gradient plus a little noise (filters and matches pay off)"""
    rng = np.random.default_rng(seed * 1000003 + h * 131 + w)
    shape = (h, w, 3) if layout == BGR8 else (h, w)
    top = 65536 if layout == GRAY16 else 256
    if kind == 'noise':
        v = rng.integers(0, top, shape)
    else:
        yy, xx = np.mgrid[:h, :w]
        base = (yy * 3 + xx * 5) * (top // 256)
        if layout == BGR8:
            base = np.stack([base, base // 2 + 40, 255 - base % 256], 2)
        v = (base + rng.integers(0, 4 if kind == 'smooth' else 1, shape)) % top
    return v.astype(np.uint16 if layout == GRAY16 else np.uint8)


def file_rows(image, layout):
    """(H, stride) uint8: the samples in the file's byte order"""
    h = image.shape[0]
    if layout == GRAY16:
        return image.astype('>u2').view(np.uint8).reshape(h, -1)
    return np.ascontiguousarray(image).reshape(h, -1)


def filter_scanlines(image, layout, filters=0):
    """the filtered scanline stream: row y gets filter type filters[y % len] (an int: every row)"""
    body = file_rows(image, layout).astype(np.int32)
    h, stride = body.shape
    bpp = BPP[layout]
    filters = [filters] if isinstance(filters, int) else list(filters)
    f = np.array([filters[y % len(filters)] for y in range(h)], np.int32)
    a = np.zeros_like(body)
    a[:, bpp:] = body[:, :-bpp]
    b = np.zeros_like(body)
    b[1:] = body[:-1]
    c = np.zeros_like(body)
    c[1:, bpp:] = body[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(body), a, b, (a + b) // 2, paeth])[f, np.arange(h)]
    rows = np.concatenate([f[:, None], (body - pred) & 255], 1).astype(np.uint8)
    return rows.tobytes()


# ---- framing ----------------------------------------------------------------------------------------
def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)


def ihdr(layout, h, w, depth=None, color=None, interlace=0):
    d, c = {GRAY8: (8, 0), BGR8: (8, 2), GRAY16: (16, 0)}[layout]
    return chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, d if depth is None else depth,
                                      c if color is None else color, 0, 0, interlace))


PHYS = chunk(b'pHYs', struct.pack('>IIB', 2835, 2835, 1))
TEXT = chunk(b'tEXt', b'Comment\0made by the decoder tests')


def frame_stream(z, layout, h, w, idat_split=(), extra_chunks=False):
    """a PNG file around the zlib stream `z`.  idat_split: an int = IDAT chunks of that many bytes, or the
    split positions.  extra_chunks: pHYs and tEXt in front of the IDATs, tEXt behind them"""
    if isinstance(idat_split, int):
        cuts = list(range(idat_split, len(z), idat_split))
    else:
        cuts = sorted(p for p in idat_split if 0 < p < len(z))
    edges = [0] + cuts + [len(z)]
    idats = b''.join(chunk(b'IDAT', z[a:b]) for a, b in zip(edges, edges[1:]))
    return C.SIGNATURE + ihdr(layout, h, w) + (PHYS + TEXT if extra_chunks else b'') + idats + \
        (TEXT if extra_chunks else b'') + chunk(b'IEND', b'')


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(raw) + co.flush()


def frame_filtered(image, layout, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15,
                   idat_split=(), extra_chunks=False):
    h, w = image.shape[:2]
    z = deflate(filter_scanlines(image, layout, filters), level, strategy, wbits)
    return frame_stream(z, layout, h, w, idat_split, extra_chunks)


def checked(data, image, layout):
    """`data` decodes to `image` for the independent decoder (small files, or filter 0 only: its filter loop
    is per byte) and for Pillow; -> data"""
    data = bytes(data)
    small = image.size * image.itemsize <= 60000
    if small or all(r[0] == 0 for r in _rows_of(data, image, layout)):
        got = C.decode(data)
        if layout == BGR8:
            got = got[:, :, ::-1]
        assert got.dtype == image.dtype and np.array_equal(got, image), "png_cases.decode reads other pixels"
    from PIL import Image
    pil = np.asarray(Image.open(io.BytesIO(data)))
    assert pil.shape == image.shape and np.array_equal(pil.astype(np.int64), image.astype(np.int64)), \
        "Pillow reads other pixels"
    return data


def _rows_of(data, image, layout):
    raw = zlib.decompress(b''.join(b for k, b in C.parse_chunks(data) if k == b'IDAT'))
    rowlen = 1 + image.shape[1] * BPP[layout]
    return [raw[i:i + 1] for i in range(0, len(raw), rowlen)]


# ---- a deflate bit-writer ---------------------------------------------------------------------------
class BitWriter:
    """deflate's packing: values LSB first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n

    def code(self, code, length):
        self.bits(int(format(code, f'0{length}b')[::-1], 2), length)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def raw(self, data):
        assert self.n % 8 == 0
        for v in data:
            self.bits(v, 8)

    def getvalue(self):
        return self.acc.to_bytes((self.n + 7) // 8, 'little')


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131,
             163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
              3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def length_symbol(length):
    k = 28 if length == 258 else max(i for i in range(28) if _LEN_BASE[i] <= length)
    return 257 + k, length - _LEN_BASE[k], _LEN_EXTRA[k]


def distance_symbol(dist):
    k = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return k, dist - _DIST_BASE[k], _DIST_EXTRA[k]


def canonical(lengths):
    """{symbol: (code, length)} of the canonical Huffman code (RFC 1951, 3.2.2)"""
    code, out = 0, {}
    for L in range(1, 16):
        for s, l in enumerate(lengths):
            if l == L:
                out[s] = (code, L)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def put_tokens(bw, tokens, lit, dist):
    """tokens: ints (literals), (length, distance) matches, ('sym', s) a raw literal/length symbol,
    ('dsym', length, d) a match with the raw distance symbol d; then the end of block"""
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lit[t])
        elif t[0] == 'sym':
            bw.code(*lit[t[1]])
        else:
            length, d = (t[1], t[2]) if t[0] == 'dsym' else t
            s, x, e = length_symbol(length)
            bw.code(*lit[s])
            bw.bits(x, e)
            if t[0] == 'dsym':
                bw.code(*dist[d])
            else:
                s, x, e = distance_symbol(d)
                bw.code(*dist[s])
                bw.bits(x, e)
    bw.code(*lit[256])


def fixed_block(bw, tokens, final=True):
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, final=False, nlen=None):
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    bw.bits(len(data), 16)
    bw.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    bw.raw(data)


_CL_LENGTHS = [4] * 13 + [5] * 6          # a complete code over the 19 code-length symbols
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def run_length_ops(seq):
    """the code-length sequence as (symbol, extra value, extra bits): zeros in runs of 11 ... 138 (18) and
    3 ... 10 (17), a repeated length as itself and 16s of 3 ... 6; runs go over the whole sequence, so over
    the border between the literal/length and the distance lengths"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r - 11, 7, i, r))
                i, run = i + r, run - r
            if run >= 3:
                ops.append((17, run - 3, 3, i, run))
                i, run = i + run, 0
            ops += [(0, 0, 0, i + k, 1) for k in range(run)]
            i += run
        else:
            ops.append((v, 0, 0, i, 1))
            i, run = i + 1, run - 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r - 3, 2, i, r))
                i, run = i + r, run - r
            ops += [(v, 0, 0, i + k, 1) for k in range(run)]
            i += run
    return ops


def dynamic_header(bw, lit_lengths, dist_lengths, final=True):
    """-> the ops written (symbol, extra, bits, first index, count)"""
    assert 257 <= len(lit_lengths) <= 286 and 1 <= len(dist_lengths) <= 30
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(len(lit_lengths) - 257, 5)
    bw.bits(len(dist_lengths) - 1, 5)
    bw.bits(19 - 4, 4)
    for s in _CL_ORDER:
        bw.bits(_CL_LENGTHS[s], 3)
    cl = canonical(_CL_LENGTHS)
    ops = run_length_ops(list(lit_lengths) + list(dist_lengths))
    for s, x, e, _, _ in ops:
        bw.code(*cl[s])
        bw.bits(x, e)
    return ops


def dynamic_block(bw, tokens, lit_lengths, dist_lengths, final=True):
    ops = dynamic_header(bw, lit_lengths, dist_lengths, final)
    put_tokens(bw, tokens, canonical(lit_lengths), canonical(dist_lengths))
    return ops


def zlib_wrap(deflate_bytes, raw, header=b'\x78\x01'):
    return header + deflate_bytes + struct.pack('>I', zlib.adler32(raw) & 0xFFFFFFFF)


def inflate_tokens(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, d = t
            for _ in range(length):
                out.append(out[-d])
    return bytes(out)


def gray_image_of(raw, h, w):
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w)
    assert not rows[:, 0].any()
    return np.ascontiguousarray(rows[:, 1:])


# ---- hand-made valid streams ------------------------------------------------------------------------
@functools.lru_cache(None)
def hand_made():
    """-> [(name, file, GRAY8, image)]: all GRAY8 with filter 0, so the scanline stream is the image with a
    zero in front of every row"""
    out = []

    def add(name, deflate_bytes, raw, h, w, **kw):
        z = zlib_wrap(deflate_bytes, raw)
        assert zlib.decompress(z) == raw, name
        img = gray_image_of(raw, h, w)
        out.append((name, checked(frame_stream(z, GRAY8, h, w, **kw), img, GRAY8), GRAY8, img))

    rng = np.random.default_rng(5)
    # an empty stored block, then a stored block of 65535 bytes, then one of 1: 256 rows of 1 + 255
    img = rng.integers(0, 256, (256, 255)).astype(np.uint8)
    raw = C.scanlines(img, GRAY8)
    bw = BitWriter()
    stored_block(bw, b'')
    stored_block(bw, raw[:65535])
    stored_block(bw, raw[65535:], final=True)
    add('stored_empty_and_65535', bw.getvalue(), raw, 256, 255)

    # length 258 at distance 1, matches over scanline ends: 5 zero rows of 1 + 300
    tokens = [0] + [(258, 1)] * 5 + [(214, 1)]
    raw = inflate_tokens(tokens)
    bw = BitWriter()
    fixed_block(bw, tokens)
    add('len258_dist1_over_row_ends', bw.getvalue(), raw, 5, 300)

    # distance < length, the length no multiple of the distance: 5 over 2 and 10 over 3 inside row 0 (1 + 20
    # bytes), then the other 21 rows as 258 and 183 over 21
    tokens = [0, 9, 8, (5, 2), 7, 6, 5, (10, 3), (258, 21), (183, 21)]
    raw = inflate_tokens(tokens)
    assert len(raw) == 21 * 22
    bw = BitWriter()
    fixed_block(bw, tokens)
    add('dist_below_length', bw.getvalue(), raw, 22, 20)

    # distance 32768: 128 stored rows of 1 + 255, row 128 = row 0 by one match of 256
    img = rng.integers(0, 256, (129, 255)).astype(np.uint8)
    img[128] = img[0]
    raw = C.scanlines(img, GRAY8)
    bw = BitWriter()
    stored_block(bw, raw[:32768])
    fixed_block(bw, [(256, 32768)])
    add('distance_32768', bw.getvalue(), raw, 129, 255, idat_split=8192)

    # dynamic block, distance tree of one code (distance 1, length 1), a 15-bit code (256 and 257), the
    # zero run 14 ... 255 as 18s
    lit = [0] * 258
    for s in range(14):
        lit[s] = s + 1
    lit[256] = lit[257] = 15
    tokens = []
    for y in range(5):
        tokens += [0] + [1 + (y + x) % 13 for x in range(4)] + [(3, 1)]
    raw = inflate_tokens(tokens)
    bw = BitWriter()
    dynamic_block(bw, tokens, lit, [1])
    add('dynamic_single_distance_15_bit_code', bw.getvalue(), raw, 5, 7)

    # code-length repeats over the literal/distance border: a 16 (lengths 256, 257 and sixteen distance
    # codes, all 4), a 17 (258, 259 and two distance lengths zero), an 18 (258 ... 285 and four)
    # (rows of 1 + 8 over the literals 0, 1, 2, the rest as matches of 3 at the one distance the tree has)
    for name, lit_tail, dist, head, d in (('16', [4, 4], [4] * 16, [0, 1, 2, 1, 0, 0, 1, 1, 0], 9),
                                          ('17', [4, 4, 0, 0], [0, 0, 1], [0, 1, 2], 3),
                                          ('18', [4, 4] + [0] * 28, [0] * 4 + [1], [0, 1, 2, 0, 1, 2], 6)):
        lit = [1, 2, 3] + [0] * 253 + lit_tail
        tokens = head + [(3, d)] * ((54 - len(head)) // 3)
        raw = inflate_tokens(tokens)
        bw = BitWriter()
        ops = dynamic_block(bw, tokens, lit, dist)
        n_lit = len(lit)
        assert any(o[0] == int(name) and o[3] < n_lit < o[3] + o[4] for o in ops), (name, ops)
        add(f'repeat_{name}_over_the_border', bw.getvalue(), raw, 6, 8)
    return out


# ---- malformed files --------------------------------------------------------------------------------
@functools.lru_cache(None)
def malformed():
    """-> [(name, file, layout, h, w, expected status)], GRAY8 7 x 5 unless the name says otherwise"""
    h, w = 5, 7
    img = make_image(GRAY8, h, w, 3, 'noise')
    raw = C.scanlines(img, GRAY8)
    good = frame_stream(deflate(raw), GRAY8, h, w)
    out = []

    def add(name, status, z=None, data=None):
        out.append((name, frame_stream(z, GRAY8, h, w) if data is None else data, GRAY8, h, w, status))

    add('bad_signature', CHUNK, data=b'\x88' + good[1:])
    add('chunk_runs_past_the_file', CHUNK, data=good[:-16] + good[-12:])
    add('idat_not_consecutive', CHUNK,
        data=C.SIGNATURE + ihdr(GRAY8, h, w) + chunk(b'IDAT', deflate(raw)[:9]) + TEXT +
        chunk(b'IDAT', deflate(raw)[9:]) + chunk(b'IEND', b''))
    add('ihdr_other_width', IHDR, data=frame_stream(deflate(raw), GRAY8, h, w + 1))
    add('ihdr_other_depth', IHDR, data=C.SIGNATURE + ihdr(GRAY8, h, w, depth=16) + good[33:])
    add('truncated_at_zlib_header', TRUNCATED, z=b'\x78')
    big = make_image(GRAY8, 64, 64, 4, 'smooth')
    zbig = deflate(filter_scanlines(big, GRAY8, 1), 6)
    assert (zbig[2] >> 1) & 3 == 2                                  # a dynamic block
    out.append(('truncated_in_dynamic_header', frame_stream(zbig[:12], GRAY8, 64, 64), GRAY8, 64, 64, TRUNCATED))
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(1, 2)
    put = [0, 5]
    for t in put:
        bw.code(*FIXED_LIT[t])
    start = bw.n
    fixed_rest = BitWriter()
    fixed_block(fixed_rest, [0, 5, (33, 1), (5, 2)])
    cut = (start + 12) // 8                                          # the match takes bits start ... start + 12
    assert cut * 8 > start
    add('truncated_in_match', TRUNCATED, z=b'\x78\x01' + fixed_rest.getvalue()[:cut])
    add('truncated_before_adler', TRUNCATED, z=deflate(raw)[:-4])
    add('zlib_header_check', ZLIB_HEADER, z=b'\x78\x02' + deflate(raw)[2:])
    add('zlib_header_method', ZLIB_HEADER, z=b'\x79\x1c' + deflate(raw)[2:])
    add('zlib_header_dictionary', ZLIB_HEADER, z=b'\x78\x20' + deflate(raw)[2:])
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(3, 2)
    add('block_type_3', BLOCK_TYPE, z=zlib_wrap(bw.getvalue() + b'\0' * 8, raw))
    bw = BitWriter()
    stored_block(bw, raw, final=True, nlen=len(raw))
    add('stored_nlen', STORED_LEN, z=zlib_wrap(bw.getvalue(), raw))
    bw = BitWriter()
    dynamic_header(bw, [1, 1, 1] + [0] * 253 + [2, 2], [1])
    add('code_lengths_oversubscribed', CODE_LENGTHS, z=zlib_wrap(bw.getvalue() + b'\0' * 8, raw))
    bw = BitWriter()
    dynamic_header(bw, [1] + [0] * 255 + [2], [1])
    add('code_lengths_incomplete', CODE_LENGTHS, z=zlib_wrap(bw.getvalue() + b'\0' * 8, raw))
    bw = BitWriter()
    dynamic_header(bw, [1, 2] + [0] * 254 + [3, 3], [2, 2])
    add('distance_code_lengths_incomplete', CODE_LENGTHS, z=zlib_wrap(bw.getvalue() + b'\0' * 8, raw))
    bw = BitWriter()
    fixed_block(bw, [0, 1, 2, ('dsym', 4, 30)])
    add('distance_symbol_30', SYMBOL, z=zlib_wrap(bw.getvalue() + b'\0' * 4, raw))
    bw = BitWriter()
    fixed_block(bw, [0, 1, 2, ('sym', 286)])
    add('length_symbol_286', SYMBOL, z=zlib_wrap(bw.getvalue() + b'\0' * 4, raw))
    bw = BitWriter()
    fixed_block(bw, [0, (39, 4)])
    add('distance_before_the_start', DISTANCE, z=zlib_wrap(bw.getvalue(), raw))
    add('too_many_bytes', TOO_MANY, z=deflate(raw + b'\0'))
    bw = BitWriter()
    fixed_block(bw, [0, (258, 1)])
    add('too_many_bytes_in_a_match', TOO_MANY, z=zlib_wrap(bw.getvalue(), raw))
    add('too_few_bytes', TOO_FEW, z=deflate(raw[:-1]))
    bad = bytearray(raw)
    bad[2 * (1 + w)] = 5
    add('filter_type_5', FILTER, z=deflate(bytes(bad)))
    z = bytearray(deflate(raw))
    z[-1] ^= 1
    add('adler_mismatch', ADLER, z=bytes(z))
    return out


# ---- the corpus -------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (5, 1), (7, 5), (33, 130), (64, 64), (65, 259)]
ALL_FILTERS = (0, 1, 2, 3, 4)
FILTER_PLANS = [0, 1, 2, 3, 4, ALL_FILTERS, (2, 0, 1), (3, 4, 0), (4, 1, 3, 2)]     # the last three: 2, 3, 4 on row 0


@functools.lru_cache(None)
def valid_small():
    """-> [(name, file, layout, image)]: the sizes list with the five filters cycling, every filter plan at
    9 x 70 and 130 x 67, the deflate forms, chunkings"""
    out = []

    def add(name, layout, img, **kw):
        out.append((name, checked(frame_filtered(img, layout, **kw), img, layout), layout, img))

    for layout in LAYOUTS:
        for h, w in SIZES:
            for i in range(3):
                add(f'size_{h}x{w}_{i}', layout, make_image(layout, h, w, i, ('smooth', 'noise', 'flat')[i]),
                    filters=ALL_FILTERS[i:] + ALL_FILTERS[:i], level=(6, 1, 9)[i])
        for h, w in ((9, 70), (130, 67)):
            img = make_image(layout, h, w, 7)
            for k, plan in enumerate(FILTER_PLANS):
                add(f'filters_{h}x{w}_{k}', layout, img, filters=plan)
    img = make_image(BGR8, 40, 50, 8)
    for level in (0, 1, 6, 9):
        add(f'level_{level}', BGR8, img, filters=ALL_FILTERS, level=level)
    for name, s in (('fixed', zlib.Z_FIXED), ('huffman_only', zlib.Z_HUFFMAN_ONLY), ('rle', zlib.Z_RLE)):
        add(f'strategy_{name}', BGR8, img, filters=ALL_FILTERS, strategy=s)
    for wbits in (9, 15):
        add(f'wbits_{wbits}', BGR8, img, filters=ALL_FILTERS, wbits=wbits)
    tiny = make_image(GRAY16, 7, 5, 9)
    add('one_byte_idats', GRAY16, tiny, filters=ALL_FILTERS, idat_split=1)
    add('ancillary_chunks', GRAY16, tiny, filters=ALL_FILTERS, idat_split=(3, 11), extra_chunks=True)
    return out


@functools.lru_cache(None)
def corpus():
    """-> list of dicts: name, file, layout, h, w, status, image (None for a malformed file)"""
    out = []
    for name, f, layout, img in valid_small() + hand_made():
        out.append(dict(name=name, file=f, layout=layout, h=img.shape[0], w=img.shape[1], status=OK, image=img))
    for name, f, layout, h, w, status in malformed():
        out.append(dict(name=name, file=f, layout=layout, h=h, w=w, status=status, image=None))
    return out


def expected_bytes(image, layout, order='rgb'):
    """the bytes emsa_png_decode leaves for one image"""
    if layout == BGR8 and order == 'bgr':
        image = image[:, :, ::-1]
    return np.ascontiguousarray(image).tobytes()
