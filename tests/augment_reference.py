"""NumPy restatement of the augmentation rules of emsanet_amd/augment.py (the docstring there states
them once): the counter-based parameter draw, the integer bilinear / nearest resize composed with crop
and flip, the HSV jitter (float64 here; float32 on request, the twin of the device arithmetic), the
normalisation and the orientation flip.  Plain loops over vectors, nothing shared with the engine."""
import numpy as np

RGB_MEAN, RGB_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
M32 = 0xFFFFFFFF


# ---- parameters ------------------------------------------------------------------------------------
def lowbias32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def aug_hash(seed, step, sample, draw):
    h = lowbias32((seed + 0x9E3779B9) & M32)
    h = lowbias32((h + step) & M32)
    h = lowbias32((h + sample) & M32)
    return lowbias32((h + draw) & M32)


def uniform_below(h, n):
    return (h * n) >> 32


def draw_row(seed, step, sample, hs, ws, h, w, q_min, q_max, flip_p, amplitudes):
    """(Hr, Wr, cy, cx, flip, dh, ds, dv) with the three deltas as np.float32"""
    q = q_min + uniform_below(aug_hash(seed, step, sample, 0), q_max - q_min + 1)
    hr, wr = (hs * q + 512) >> 10, (ws * q + 512) >> 10
    cy = uniform_below(aug_hash(seed, step, sample, 1), hr - h + 1)
    cx = uniform_below(aug_hash(seed, step, sample, 2), wr - w + 1)
    flip = int(aug_hash(seed, step, sample, 3) < int(round(flip_p * 2 ** 32)))
    deltas = []
    for k, amp in enumerate(amplitudes):
        u = aug_hash(seed, step, sample, 4 + k) >> 8
        deltas.append(np.float32(2 * u - 2 ** 24) * np.float32(amp / 2 ** 24))
    return (hr, wr, cy, cx, flip) + tuple(deltas)


def pack_rows(rows):
    """rows of draw_row -> the int32 (N, 8) table the engine uses"""
    t = np.zeros((len(rows), 8), np.int32)
    for i, r in enumerate(rows):
        t[i, :5] = r[:5]
        t[i, 5:] = np.array(r[5:], np.float32).view(np.int32)
    return t


def draw_table(seed, step, n, hs, ws, h, w, q_min=1024, q_max=1434, flip_p=0.5,
               amplitudes=(10 / 180, 20 / 255, 50 / 255)):
    return pack_rows([draw_row(seed, step, i, hs, ws, h, w, q_min, q_max, flip_p, amplitudes)
                      for i in range(n)])


def unpack_row(row):
    row = np.asarray(row, np.int32)
    return tuple(int(v) for v in row[:5]) + tuple(row[5:].view(np.float32))


# ---- geometry --------------------------------------------------------------------------------------
def bilinear_axis(X, n_in, n_out):
    """X: int array of coordinates in n_out -> (i0, i1, a): clamped indices and the weight of i1"""
    X = np.asarray(X, np.int64)
    t = (2 * X + 1) * n_in - n_out
    d = 2 * n_out
    i0 = t // d                            # floor
    r = t - i0 * d
    a = (r * 2048 + n_out) // d
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), a


def nearest_axis(X, n_in, n_out):
    return (np.asarray(X, np.int64) * n_in) // n_out


def source_coords(h, w, cy, cx, flip):
    x = np.arange(w)
    return cy + np.arange(h), cx + (w - 1 - x if flip else x)


def bilinear_u8(img, hr, wr, Y, X):
    """img (Hs, Ws, C) uint8; the pixels (Y, X) of its hr x wr resize, uint8 (len(Y), len(X), C)"""
    y0, y1, ay = bilinear_axis(Y, img.shape[0], hr)
    x0, x1, ax = bilinear_axis(X, img.shape[1], wr)
    p = img.astype(np.int64)
    ay, ax = ay[:, None, None], ax[None, :, None]
    top = (2048 - ax) * p[y0][:, x0] + ax * p[y0][:, x1]
    bot = (2048 - ax) * p[y1][:, x0] + ax * p[y1][:, x1]
    return (((2048 - ay) * top + ay * bot + (1 << 21)) >> 22).astype(np.uint8)


def nearest(img, hr, wr, Y, X):
    return img[nearest_axis(Y, img.shape[0], hr)][:, nearest_axis(X, img.shape[1], wr)]


def resize_bilinear_u8(img, hr, wr):
    """the whole hr x wr resize (for the comparison with Pillow)"""
    return bilinear_u8(img, hr, wr, np.arange(hr), np.arange(wr))


# ---- colour ----------------------------------------------------------------------------------------
def hsv_jitter(rgb_u8, dh, ds, dv, dtype=np.float64):
    """(..., 3) uint8 -> (..., 3) `dtype` in [0, 1] after the jitter; every operation in `dtype`"""
    f = dtype
    c6, c4, c2, c0, c1 = f(6), f(4), f(2), f(0), f(1)
    rgb = rgb_u8.astype(f) / f(255)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    c = v - np.minimum(r, np.minimum(g, b))
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(v > 0, c / v, c0).astype(f)
        hr_ = (g - b) / c
        hr_ = np.where(hr_ < 0, hr_ + c6, hr_)
        hg = (b - r) / c + c2
        hb = (r - g) / c + c4
    hue = np.where(c > 0, np.where(v == r, hr_, np.where(v == g, hg, hb)), c0).astype(f)
    hue = hue + c6 * f(dh)
    hue = hue - c6 * np.floor(hue / c6)
    s2 = np.clip(s + f(ds), c0, c1)
    v2 = np.clip(v + f(dv), c0, c1)
    vs = v2 * s2
    out = np.empty(rgb.shape, f)
    for ch, n in enumerate((5, 3, 1)):
        k = f(n) + hue
        k = k - c6 * np.floor(k / c6)
        m = np.clip(np.minimum(k, c4 - k), c0, c1)
        out[..., ch] = v2 - vs * m
    return out


def normalize_rgb_u8(rgb_u8):
    """(..., 3) uint8 -> float32: the engine's normalize_rgb, ((v * scale - mean) rounded once) * (1 / std)
    (the product v * scale and the difference are exact in float64: one rounding, as the device's fma)"""
    scale = np.float32(1.0 / 255.0)
    out = np.empty(rgb_u8.shape, np.float32)
    for ch in range(3):
        d = (rgb_u8[..., ch].astype(np.float64) * np.float64(scale) - np.float64(np.float32(RGB_MEAN[ch])))
        out[..., ch] = d.astype(np.float32) * (np.float32(1) / np.float32(RGB_STD[ch]))
    return out


def normalize_rgb_unit(rgb, dtype=np.float64):
    """(..., 3) in [0, 1] -> (v - mean) * (1 / std), in `dtype` with the engine's float32 constants"""
    f = dtype
    out = np.empty(rgb.shape, f)
    for ch in range(3):
        inv = f(np.float32(1) / np.float32(RGB_STD[ch]))
        out[..., ch] = (rgb[..., ch].astype(f) - f(np.float32(RGB_MEAN[ch]))) * inv
    return out


def normalize_depth(depth_u16, mean, std):
    v = depth_u16.astype(np.float32)
    out = (v - np.float32(mean)) * (np.float32(1) / np.float32(std))
    return np.where(depth_u16 == 0, np.float32(0), out).astype(np.float32)


# ---- orientations ----------------------------------------------------------------------------------
def flip_orientations(table, flips):
    """float32 (N, M), flips (N,) -> theta -> (2 pi - theta) mod 2 pi on the flipped rows, in float32"""
    two_pi = np.float32(6.2831855)
    out = table.astype(np.float32).copy()
    with np.errstate(invalid='ignore'):
        for i, fl in enumerate(flips):
            if not fl:
                continue
            a = two_pi - out[i]
            a = a - two_pi * np.floor(a / two_pi)
            a = np.where(a < 0, a + two_pi, a)
            a = np.where(a >= two_pi, a - two_pi, a)
            out[i] = a.astype(np.float32)
    return out


# ---- a whole batch -----------------------------------------------------------------------------------
def reference_apply(batch, table, h, w, depth_stats=(0.0, 1.0), hsv=True, dtype=np.float64):
    """batch: NumPy arrays 'rgb' (N,Hs,Ws,3) uint8, 'depth' (N,Hs,Ws) uint16, label maps, 'orientations'
    (any may be missing); table: int32 (N, 8).  Returns 'rgb_u8' (N,H,W,3), the resized, cropped and
    flipped uint8 frame; 'rgb' (N,3,H,W) in `dtype` (with hsv) or float32 (without: the engine's
    normalize_rgb of 'rgb_u8'); 'depth' (N,1,H,W) float32; the label maps; 'orientations'"""
    out = {}
    n = len(table)
    rows = [unpack_row(table[i]) for i in range(n)]
    for i, (hr, wr, cy, cx, flip, dh, ds, dv) in enumerate(rows):
        Y, X = source_coords(h, w, cy, cx, flip)
        if 'rgb' in batch:
            u8 = bilinear_u8(batch['rgb'][i], hr, wr, Y, X)
            out.setdefault('rgb_u8', np.empty((n, h, w, 3), np.uint8))[i] = u8
            if hsv:
                val = normalize_rgb_unit(hsv_jitter(u8, dh, ds, dv, dtype), dtype)
            else:
                val = normalize_rgb_u8(u8)
            out.setdefault('rgb', np.empty((n, 3, h, w), val.dtype))[i] = val.transpose(2, 0, 1)
        if 'depth' in batch:
            d = nearest(batch['depth'][i], hr, wr, Y, X)
            out.setdefault('depth_u16', np.empty((n, h, w), np.uint16))[i] = d
            out.setdefault('depth',np.empty((n, 1, h, w), np.float32))[i, 0] = normalize_depth(d, *depth_stats)
        for key in ('semantic', 'instance'):
            if key in batch:
                out.setdefault(key, np.empty((n, h, w), batch[key].dtype))[i] = nearest(batch[key][i], hr, wr, Y, X)
    if 'orientations' in batch:
        out['orientations'] = flip_orientations(batch['orientations'], [r[4] for r in rows])
    if 'scene' in batch:
        out['scene'] = batch['scene'].copy()
    return out


def random_batch(n, hs, ws, seed=0, sem_dtype=np.uint8, inst_dtype=np.uint16, max_instances=16):
    """random raw frames: noise RGB (every bilinear tap differs), depth with ~5 % invalid zeros, blocky
    label maps (8 x 8 cells, so nearest neighbours differ at cell edges), orientations with NaNs"""
    g = np.random.default_rng(seed)
    rgb = g.integers(0, 256, (n, hs, ws, 3), dtype=np.uint8)
    depth = g.integers(300, 8000, (n, hs, ws)).astype(np.uint16)
    depth[g.random((n, hs, ws)) < 0.05] = 0
    cells = (n, (hs + 7) // 8, (ws + 7) // 8)
    up = lambda a: np.repeat(np.repeat(a, 8, 1), 8, 2)[:, :hs, :ws]          # noqa: E731
    sem = up(g.integers(0, 41, cells)).astype(sem_dtype)
    inst = up(g.integers(0, max_instances, cells)).astype(inst_dtype)
    ori = (g.random((n, max_instances)) * 2 * np.pi).astype(np.float32)
    ori[g.random((n, max_instances)) < 0.3] = np.nan
    ori[:, 1] = 0.0
    return {'rgb': rgb, 'depth': depth, 'semantic': np.ascontiguousarray(sem),
            'instance': np.ascontiguousarray(inst), 'orientations': ori,
            'scene': g.integers(0, 10, n).astype(np.int64)}
