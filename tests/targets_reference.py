"""Brute-force NumPy restatement of the training-target rules of emsanet_amd/targets.py (a helper, not
a test): one Python loop per instance, float64 `exp` rounded to fp32, Python `round` on exact
fractions.  Plus the label scenes the CPU and GPU tests share."""
from fractions import Fraction

import numpy as np

DEFAULT_SCALES = (1, 32, 16, 8)

# the test label list WITH void: 0 void, 1 thing + orientation, 2 thing, 3 stuff, 4 thing + orientation,
# 5 thing
IS_THING = (False, True, True, False, True, True)
USE_ORIENTATION = (False, True, False, False, True, False)


def scale_sigma(sigma, s):
    return sigma if s == 1 else (4 * sigma) // s


def reference_targets(semantic, instance, is_thing, use_orientation=None, orientations=None, scene=None,
                      scales=DEFAULT_SCALES, sigma=8, normalized_offset=True, max_instances=256):
    """semantic / instance (N,H,W) integer arrays, orientations (N, max_instances) float32 with NaN or
    None -> dict(semantic=[...], instance=[{...}], scene, centers=[per scale: per image {id: (cy, cx)}],
    bad_id, bad_label).  A pixel whose id or label is out of range carries no instance."""
    semantic = np.asarray(semantic).astype(np.int64)
    instance = np.asarray(instance).astype(np.int64)
    n, h, w = semantic.shape
    is_thing = np.asarray(is_thing, dtype=bool)
    use_o = np.zeros(len(is_thing), bool) if use_orientation is None else np.asarray(use_orientation, bool)
    out = {'semantic': [], 'instance': [], 'centers': [], 'bad_id': False, 'bad_label': False,
           'scene': None if scene is None else np.asarray(scene).astype(np.int64)}
    for s in scales:
        assert h % s == 0 and w % s == 0
        sem = semantic[:, ::s, ::s]
        ids = instance[:, ::s, ::s]
        hs, ws = sem.shape[1:]
        bad_id = (ids < 0) | (ids >= max_instances)
        bad_label = (sem < 0) | (sem >= len(is_thing))
        out['bad_id'] |= bool(bad_id.any())
        out['bad_label'] |= bool(bad_label.any())
        thing = is_thing[np.where(bad_label, 0, sem)] & (sem != 0)
        ids = np.where(bad_id | bad_label | ~thing, 0, ids)
        sg = scale_sigma(sigma, s)
        assert sg >= 1
        radius = 3 * sg + 1
        center = np.zeros((n, 1, hs, ws), np.float32)
        offset = np.zeros((n, 2, hs, ws), np.float32)
        orient = np.zeros((n, hs, ws), np.float32)
        ofg = np.zeros((n, hs, ws), bool)
        centers = []
        for i in range(n):
            per_image = {}
            for k in np.unique(ids[i]):
                if k == 0:
                    continue
                ys, xs = np.nonzero(ids[i] == k)
                cy = int(round(Fraction(int(ys.sum()), len(ys))))       # half to even, exact
                cx = int(round(Fraction(int(xs.sum()), len(xs))))
                per_image[int(k)] = (cy, cx)
                y0, y1 = max(0, cy - radius), min(hs, cy + radius + 1)
                x0, x1 = max(0, cx - radius), min(ws, cx + radius + 1)
                yy, xx = np.mgrid[y0:y1, x0:x1]
                d2 = (yy - cy) ** 2 + (xx - cx) ** 2
                g = np.exp(-d2.astype(np.float64) / (2.0 * sg * sg)).astype(np.float32)
                center[i, 0, y0:y1, x0:x1] = np.maximum(center[i, 0, y0:y1, x0:x1], g)
                dy, dx = (cy - ys).astype(np.float32), (cx - xs).astype(np.float32)
                if normalized_offset:
                    dy, dx = dy / np.float32(hs), dx / np.float32(ws)
                offset[i, 0, ys, xs] = dy
                offset[i, 1, ys, xs] = dx
                if orientations is not None and not np.isnan(orientations[i, k]):
                    orient[i, ys, xs] = orientations[i, k]
                    ofg[i, ys, xs] = use_o[sem[i, ys, xs]]
            centers.append(per_image)
        out['semantic'].append(np.ascontiguousarray(sem))
        d = {'center': center, 'offset': offset, 'foreground': ids != 0}
        if orientations is not None:
            d['orientation'], d['orientation_foreground'] = orient, ofg
        out['instance'].append(d)
        out['centers'].append(centers)
    return out


def rect(a, y0, y1, x0, x1, v):
    """rows y0..y1, columns x0..x1, both inclusive"""
    a[y0:y1 + 1, x0:x1 + 1] = v


def edge_scene(max_instances=256):
    """(semantic, instance, orientations, scene) at 96x128, N = 3, labels of IS_THING: every case the
    kernels can get wrong at the side scales 12x16, 6x8 and 3x4 (see the list in test_targets_gpu.py)"""
    n, h, w = 3, 96, 128
    rng = np.random.RandomState(5)
    sem = np.zeros((n, h, w), np.int64)
    inst = np.zeros((n, h, w), np.int64)
    ori = np.full((n, max_instances), np.nan, np.float32)
    # image 0: labels of every kind, no instance at all
    sem[0] = np.repeat(np.repeat(rng.randint(0, 6, (12, 16)), 8, 0), 8, 1)
    # image 1: the hand-placed cases, on a stuff background with a void band
    s, i = sem[1], inst[1]
    s[:] = 3
    s[88:] = 0
    top = max_instances - 1
    # rows y0..y1, columns x0..x1, class (None = leave the background), id, angle (None = NaN)
    for y0, y1, x0, x1, cls, k, angle in (
            (10, 29, 10, 39, 1, top, 0.5),        # non-contiguous id, the largest one allowed
            (50, 50, 70, 70, 2, 7, 1.25),         # one pixel; on no coarse grid: gone at /8, /16, /32
            (0, 11, 100, 127, 4, 3, None),        # touches two borders (clipped window); no angle
            (40, 55, 10, 25, 1, 20, -2.0),        # two instances whose windows overlap ...
            (44, 59, 30, 45, 2, 21, 1.0),         # ... this one of a class that uses no orientation
            (70, 79, 10, 29, None, 30, 0.7),      # on the stuff background: cleared
            (89, 95, 40, 59, None, 31, 0.7),      # on void: cleared
            (76, 86, 108, 120, 5, 40, None),      # holds (80, 112) but no multiple of 32: gone at /32
            (64, 65, 64, 65, 1, 50, 3.0),         # mean (64.5, 64.5) -> (64, 64): half to even
            (67, 68, 81, 82, 4, 51, -3.0)):       # mean (67.5, 81.5) -> (68, 82)
        if cls is not None:
            rect(s, y0, y1, x0, x1, cls)
        rect(i, y0, y1, x0, x1, k)
        if angle is not None:
            ori[1, k] = angle
    # image 2: random rectangles that overwrite each other (ragged instances), random classes
    s, i = sem[2], inst[2]
    s[:] = 3
    for k in range(1, 25):
        y0, x0 = rng.randint(0, h - 4), rng.randint(0, w - 4)
        y1, x1 = min(h - 1, y0 + rng.randint(1, 30)), min(w - 1, x0 + rng.randint(1, 40))
        rect(s, y0, y1, x0, x1, rng.randint(0, 6))
        rect(i, y0, y1, x0, x1, k * 9)
        if k % 3:
            ori[2, k * 9] = rng.uniform(-np.pi, np.pi)
    scene = np.array([0, 4, 9], np.int64)
    return sem, inst, ori, scene


def rectangles_scene(n, h, w, count, seed, cell=20, max_instances=256, big_first=False):
    """`count` disjoint thing rectangles per image on a stuff background, one per `cell` x `cell` cell
    and centred within a pixel of the cell's middle: the centres (of rectangles: their means) are
    pairwise >= cell - 3 apart in the Chebyshev sense and the rectangles never touch.  Every second
    side length is even (a mean of x.5).  With big_first, image 0 is one instance covering the whole
    image instead."""
    rng = np.random.RandomState(seed)
    sem = np.full((n, h, w), 3, np.int64)
    inst = np.zeros((n, h, w), np.int64)
    cells = [(cy, cx) for cy in range(h // cell) for cx in range(w // cell)]
    assert cell >= 12 and count <= len(cells) and count < max_instances
    for i in range(n):
        if big_first and i == 0:
            sem[i], inst[i] = 1, max_instances - 1
            continue
        for k, j in enumerate(rng.permutation(len(cells))[:count]):
            cy = cells[j][0] * cell + cell // 2 + rng.randint(-1, 2)
            cx = cells[j][1] * cell + cell // 2 + rng.randint(-1, 2)
            hy, hx = rng.randint(0, cell // 2 - 2), rng.randint(0, cell // 2 - 2)
            ey, ex = rng.randint(0, 2), rng.randint(0, 2)
            rect(sem[i], cy - hy, cy + hy + ey, cx - hx, cx + hx + ex, (1, 2, 4, 5)[k % 4])
            rect(inst[i], cy - hy, cy + hy + ey, cx - hx, cx + hx + ex, k + 1)
    return sem, inst


def corner_scene(max_instances=256):
    """(semantic, instance, orientations, scene) at 32x32, N = 2: the side scales are 1x1, 2x2 and 4x4
    maps (1, 4 and 16 pixels: none a multiple of 64), and the full-scale window (radius 25) of every
    instance is clipped on two sides.  Image 0: a 3x3 thing at each of the four image corners, the
    bottom-right one with the last id of the table, max_instances - 1; only the top-left one is
    sampled by the side scales.  Image 1: one instance, again the last id, over the whole image: its
    centre is (0, 0) at 1x1 and at 2x2 (mean 0.5, half to even) and (2, 2) at 4x4 (mean 1.5)."""
    n, h, w = 2, 32, 32
    sem = np.full((n, h, w), 3, np.int64)
    inst = np.zeros((n, h, w), np.int64)
    ori = np.full((n, max_instances), np.nan, np.float32)
    top = max_instances - 1
    for y0, x0, cls, k, angle in ((0, 0, 1, 1, 0.25), (0, 29, 2, 2, None), (29, 0, 4, top - 1, -1.5),
                                  (29, 29, 1, top, 2.5)):
        rect(sem[0], y0, y0 + 2, x0, x0 + 2, cls)
        rect(inst[0], y0, y0 + 2, x0, x0 + 2, k)
        if angle is not None:
            ori[0, k] = angle
    sem[1], inst[1] = 4, top
    ori[1, top] = -0.75
    return sem, inst, ori, np.array([2, 7], np.int64)
