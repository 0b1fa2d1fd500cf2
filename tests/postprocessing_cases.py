"""Constructed inputs of the eval post-processing edge tests, shared by the CPU module (which checks
that the inputs have the properties the cases are about) and the GPU module (which runs the HIP
kernels of emsanet_amd/csrc/postproc.hip on them against oracle/postprocessing_oracle.py).
Everything here is host-side torch; nothing touches the device."""
import functools
import math

import torch

from oracle import postprocessing_oracle as O

CHUNK = 1024            # pixels per workgroup of the NMS pass == sort width of the merge pass
PIXELS_1D = 4096 * 256  # threads of a capped 1-D launch: more pixels than this make the kernels stride
ASSIGN_THREADS = 1024 * 256   # threads per image of the assignment kernel
U = 2.0 ** -24          # unit round-off of fp32 (round to nearest)


# ---- centres ---------------------------------------------------------------------------------
def distinct_heat(n=2, h=64, w=80, seed=21):
    """distinct random fp32 values in [0.1, 1): with an NMS window of 1 every pixel survives and the
    order (score desc) has no ties.  Spacing 0.9 / (n h w) >= 8e-5 >> 2^-24: distinct after rounding"""
    g = torch.Generator().manual_seed(seed)
    total = n * h * w
    perm = torch.randperm(total, generator=g).double()
    return (0.1 + 0.9 * (perm + 0.5) / total).float().reshape(n, 1, h, w)


def default_heat(case, n=2, h=136, w=128, seed=5):
    """the saturated constructions of tests/test_postprocessing.py at 136 x 128 (17 chunks: with
    top_k = 64 a plateau hands 17 * 64 = 1088 candidates to the merge pass)"""
    heat = torch.full((n, 1, h, w), 0.75)
    if case == 'late_peaks':
        # isolated higher pixels in the lower rows, i.e. in the last chunks of the scan order
        g = torch.Generator().manual_seed(seed)
        for i in range(n):
            for _ in range(9):
                y = int(torch.randint(80, h, (1,), generator=g))
                x = int(torch.randint(0, w, (1,), generator=g))
                heat[i, 0, y, x] = 0.8 + 0.01 * float(torch.rand(1, generator=g))
    elif case == 'two_levels':
        heat[:, :, h // 2:] = 0.875            # the better plateau comes second in position order
        heat[1, 0, :, : w // 3] = 0.05         # below the threshold
    elif case != 'plateau':
        raise ValueError(case)
    return heat


def merge_candidates(heat, threshold, kernel, top_k, foreground=None):
    """per image: sum over 1024-pixel chunks of min(survivors in the chunk, top_k) -- what the NMS pass
    hands to the merge pass; above 1024 the merge runs in rounds"""
    _, keep = O.center_keep_mask(heat, threshold, kernel, foreground)
    n = heat.shape[0]
    flat = keep.reshape(n, -1)
    pad = (-flat.shape[1]) % CHUNK
    flat = torch.cat([flat, flat.new_zeros(n, pad)], 1).reshape(n, -1, CHUNK)
    return flat.sum(-1).clamp(max=top_k).sum(-1)


CAP_TOP_K = 8


def cap_heat(seed=23):
    """33 x 64 = 2112 pixels: two whole chunks and one of 64 pixels, so with top_k = 8 the candidate lists
    hold cap = 3 * 8 = 24 entries per image.  Window 1, threshold 0.1: a pixel survives iff it is set.
    Distinct scores in [0.2, 1), everything else 0.  Survivors per chunk:
      image 0: 8, 8, 8   the candidate count equals cap, nothing is cut
      image 1: 9, 8, 8   cap + 1: the ninth of the first chunk (its lowest score) is cut
      image 2: 5, 3, 0   top_k survivors exactly: every centre slot is used, none padded
    the last pixel of the map (the last of the partial chunk) is set in images 0 and 1"""
    g = torch.Generator().manual_seed(seed)
    h, w = 33, 64
    counts = ((8, 8, 8), (9, 8, 8), (5, 3, 0))
    heat = torch.zeros(len(counts), 1, h, w)
    total = sum(sum(c) for c in counts)
    scores = (0.2 + 0.8 * (torch.randperm(total, generator=g).double() + 0.5) / total).float()
    k = 0
    for i, per_chunk in enumerate(counts):
        flat = heat[i, 0].view(-1)
        for c, m in enumerate(per_chunk):
            size = min(CHUNK, h * w - c * CHUNK)
            pos = torch.randperm(size, generator=g)[:m] + c * CHUNK
            if m and c == 2:
                pos[0] = h * w - 1
            flat[pos.unique()[:m]] = scores[k:k + m]
            assert int((flat[c * CHUNK:c * CHUNK + size] > 0).sum()) == m
            k += m
    return heat


def blob_heat(n, h, w, seed, n_blobs=12):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
    heat = torch.zeros(n, 1, h, w)
    for i in range(n):
        for _ in range(n_blobs):
            cy, cx = float(torch.rand(1, generator=g) * h), float(torch.rand(1, generator=g) * w)
            a = float(torch.rand(1, generator=g)) * 0.9 + 0.05
            heat[i, 0] = torch.maximum(heat[i, 0], a * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 32.0))
    return heat + torch.rand(n, 1, h, w, generator=g) * 0.02


# ---- assignment ------------------------------------------------------------------------------
NEAR_TIES, NEAR_RIM, RIM = 24, 200, 6.0      # 24 / 307,200 < 1e-4 and 224 / 307,200 < 1e-3: within the caps


def random_centers(n, k, h, w, seed):
    """n x k distinct integer pixel positions (y, x) as float32, like the centre kernel writes them"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        p = torch.randperm(h * w, generator=g)[:k]
        out.append(torch.stack([p // w, p % w], 1).float())
    return torch.stack(out)


def assign_case(n=1, h=480, w=640, k=64, seed=31, normalized=True, near=False):
    """offsets that mostly point at a centre (what a trained head produces: whole regions vote for
    one centre) plus noise, so that the borders between two centres' regions cross many pixels;
    rows [0, 8) carry zero offsets: integer coordinates, every distance exact in fp32, and the first
    two centres are placed so that column 15 of those rows is an EXACT tie between them.
    near: add the constructed near-ties below (only where the image is large enough for the caps)"""
    g = torch.Generator().manual_seed(seed)
    centers = random_centers(n, k, h, w, seed + 1)
    centers[:, 0] = torch.tensor([4.0, 10.0])
    centers[:, 1] = torch.tensor([4.0, 20.0])
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
    off = torch.empty(n, 2, h, w)
    for i in range(n):
        bh, bw = max(h // 16, 1), max(w // 16, 1)
        pick = torch.randint(0, k, (bh, bw), generator=g)
        pick = pick.repeat_interleave(-(-h // bh), 0).repeat_interleave(-(-w // bw), 1)[:h, :w]
        ty, tx = centers[i, pick, 0], centers[i, pick, 1]
        mix = torch.rand(h, w, generator=g)          # 0: stay where the pixel is, 1: point at the centre
        off[i, 0] = (ty - yy) * mix + torch.randn(h, w, generator=g) * 3.0
        off[i, 1] = (tx - xx) * mix + torch.randn(h, w, generator=g) * 3.0
    off[:, :, :8] = 0.0
    sy, sx = (float(h), float(w)) if normalized else (1.0, 1.0)
    off[:, 0] /= sy
    off[:, 1] /= sx
    fg = torch.rand(n, h, w, generator=g) > 0.3
    # constructed near-ties, where an fp32 evaluation MAY decide differently from fp64 (the second part
    # of the rule is about these): NEAR_TIES pixels of row h/2 point at the bisector of a centre and
    # its nearest neighbour, NEAR_RIM pixels of row h/2 + 1 at the rim of the distance threshold 6
    # around a centre -- up to the fp32 rounding of the offset itself
    ya, yb = h // 2, h // 2 + 1
    for i in range(n if near else 0):
        c = centers[i].double()
        dd = ((c[:, None] - c[None]) ** 2).sum(-1) + torch.eye(k, dtype=torch.float64) * 1e18
        for x in range(min(NEAR_TIES, w)):
            a = int(torch.randint(0, k, (1,), generator=g))
            b = int(dd[a].argmin())
            along = torch.stack([-(c[b] - c[a])[1], (c[b] - c[a])[0]]) / float(dd[a, b]) ** 0.5
            t = (c[a] + c[b]) / 2 + along * float(torch.rand(1, generator=g, dtype=torch.float64)) * 2.0
            off[i, 0, ya, x], off[i, 1, ya, x] = (t[0] - ya) / sy, (t[1] - x) / sx
        for x in range(min(NEAR_RIM, w)):
            a = int(torch.randint(0, k, (1,), generator=g))
            th = float(torch.rand(1, generator=g, dtype=torch.float64)) * 6.283185307179586
            t = c[a] + RIM * torch.tensor([math.sin(th), math.cos(th)], dtype=torch.float64)
            off[i, 0, yb, x], off[i, 1, yb, x] = (t[0] - yb) / sy, (t[1] - x) / sx
        fg[i, ya:yb + 1] = True
    return off, centers, fg


def assign_bound(off, sqdist, h, w, normalized):
    """E (H,W,K) fp64: bound on |d_fp32 - d| for the squared distance d of a pixel to a centre as an
    fp32 evaluation of the kernel's expression computes it, u = 2^-24:

      cy' = fl(y + fl(o_y * s_y))   or, contracted, fl(y + o_y * s_y)      (y, s_y, centres: exact)
          |cy' - cy| <= u |o_y s_y| + u |cy| (1 + u)  =: e_y            (one rounding less when fused)
      dy' = fl(cy' - k_y) = (dy + (cy' - cy)) (1 + t1),             |t| <= u throughout
      d'  = fl(fl(dy'^2) + fl(dx'^2))  or  fl(fma(dy', dy', fl(dx'^2)))
          = [(dy + .)^2 (1 + t1)^2 (1 + t2) + (dx + .)^2 (1 + t3)^2 (1 + t4)] (1 + t5)
      with D = (dy + e_y)^2 + (dx + e_x)^2 <= d + 2 sqrt(d) e + e^2,  e = sqrt(e_y^2 + e_x^2)
      (Cauchy-Schwarz):  |d' - d| <= ((1 + u)^4 - 1) D + (D - d)  <=  4.01 u D + 2 sqrt(d) e + e^2
    so  E = 4.01 u (d + 2 sqrt(d) e + e^2) + 2 sqrt(d) e + e^2.
    Consequences the tests check, d = the fp64 value, j = its arg-min, k = the fp32 choice:
      k != j                -> d_k - d_j <= E_k + E_j
      threshold T^2 crossed -> |d_chosen - T^2| <= E_chosen       (T^2 exact in fp32 for T = 6)"""
    sy, sx = (float(h), float(w)) if normalized else (1.0, 1.0)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64),
                            indexing='ij')
    oy, ox = off[0].double() * sy, off[1].double() * sx
    ey = U * oy.abs() + U * (yy + oy).abs() * (1 + U)
    ex = U * ox.abs() + U * (xx + ox).abs() * (1 + U)
    e = torch.sqrt(ey * ey + ex * ex)[..., None]
    cross = 2.0 * torch.sqrt(sqdist) * e + e * e
    return 4.01 * U * (sqdist + cross) + cross


def assign_check(ids, off, centers, n_centers, fg, normalized, max_distance, cap):
    """two-part rule for the ids (N,H,W) an fp32 evaluation assigned: (1) the share of pixels that differ
    from the fp64 arg-min stays within `cap`; (2) every differing pixel is a near-tie in fp64 (see
    assign_bound).  Returns (share, largest gap / bound ratio, largest gap, its bound)."""
    n, _, h, w = off.shape
    ids = ids.long()
    differ, worst, worst_gap, worst_bound = 0, 0.0, 0.0, 0.0
    for i in range(n):
        k = int(n_centers[i])
        if k == 0:
            assert int(ids[i].abs().max()) == 0
            continue
        d = O.instance_assign_sqdist(off[i:i + 1], [(centers[i, :k],)], normalized)[0]
        E = assign_bound(off[i], d, h, w, normalized)
        best, arg = d.min(-1)
        ref = arg + 1
        T2 = None if not max_distance else float(max_distance) ** 2
        if T2 is not None:
            ref = torch.where(best > T2, torch.zeros_like(ref), ref)
        if fg is not None:
            ref = torch.where(fg[i].bool(), ref, torch.zeros_like(ref))
            assert int(ids[i][~fg[i].bool()].abs().max()) == 0          # exact: no arithmetic involved
        assert int(ids[i].min()) >= 0 and int(ids[i].max()) <= k
        bad = ids[i] != ref
        differ += int(bad.sum())
        if not bad.any():
            continue
        got, want = ids[i][bad], ref[bad]
        db, Eb = d[bad], E[bad]
        rows = torch.arange(len(got))
        dj, Ej = best[bad], Eb[rows, arg[bad]]
        # where the kernel chose a centre: its fp64 distance and bound
        dk = db[rows, (got - 1).clamp(min=0)]
        Ek = Eb[rows, (got - 1).clamp(min=0)]
        gap = torch.zeros_like(dj)
        bound = torch.ones_like(dj)
        both = (got > 0) & (want > 0)
        gap[both], bound[both] = (dk - dj)[both], (Ek + Ej)[both]
        if T2 is not None:
            lost = (got == 0) & (want > 0)           # kernel: beyond the threshold, fp64: within
            gap[lost], bound[lost] = (T2 - dj)[lost], Ej[lost]
            extra = (got > 0) & (want == 0)          # kernel: within, fp64: beyond
            gap[extra], bound[extra] = (dk - T2)[extra], Ek[extra]
            # (want == 0 & got > 0 can only come from the threshold: foreground was checked above)
        else:
            assert bool(both.all()), "an id of 0 that the fp64 reference does not have"
        assert bool((gap >= 0).all())
        ratio = gap / bound
        j = int(ratio.argmax())
        if float(ratio[j]) >= worst:
            worst, worst_gap, worst_bound = float(ratio[j]), float(gap[j]), float(bound[j])
        assert float(ratio.max()) <= 1.0, (
            f"a differing pixel is no near-tie: gap {float(gap[j]):.3e} > bound {float(bound[j]):.3e}")
    share = differ / float(n * h * w)
    assert share <= cap, f"share of differing pixels {share:.3e} > {cap}"
    return share, worst, worst_gap, worst_bound


# ---- panoptic ---------------------------------------------------------------------------------
NC, TOP_K = 40, 64
IS_THING = [bool(i % 3) for i in range(NC)]


@functools.lru_cache(maxsize=None)
def big_panoptic(n=4, h=480, w=640, seed=41):
    """blocky semantic / instance maps at (4, 480, 640) = 1,228,800 pixels with all 64 instance ids,
    scores, centre scores, and the oracle's merge + score maps (computed once, shared, read-only)"""
    g = torch.Generator().manual_seed(seed)
    sem = torch.randint(0, NC, (n, h // 8, w // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    ids = torch.randint(0, TOP_K + 1, (n, h // 16, w // 16), generator=g)
    ids = ids.repeat_interleave(16, 1).repeat_interleave(16, 2).to(torch.int32)
    score = torch.rand(n, h, w, generator=g)
    cscore = torch.rand(n, TOP_K, generator=g)
    ref_m = O.panoptic_merge(sem, ids, IS_THING, top_k=TOP_K)
    ref_s = O.panoptic_scores(score, ref_m['instance'], ref_m['semantic'], list(cscore))
    return sem, ids, score, cscore, ref_m, ref_s


def small_merge_case():
    """one 8 x 16 map, 6 classes (0, 2, 5 stuff; 1, 3, 4 thing), top_k = 4:
      id 1: 8 pixels of class 4 first in scan order, then 8 of class 3 -> a vote tie, class 3 wins
      id 2: wholly on stuff pixels (class 2)              -> no votes: class -1, pixels stay stuff
      id 4 (= top_k): thing class 1                       -> a regular instance
      id 5 (= top_k + 1): thing class 1                   -> ignored: void
      id 3: its pixels carry the labels -1 and 255 (void, no votes) and two pixels of class 4
      row 7: labels -1 / 255 without an instance           -> void"""
    is_thing = [False, True, False, True, True, False]
    top_k = 4
    sem = torch.zeros(1, 8, 16, dtype=torch.int64)
    ids = torch.zeros(1, 8, 16, dtype=torch.int32)
    sem[0, 0, :8], sem[0, 0, 8:] = 4, 3
    ids[0, 0] = 1
    sem[0, 1], ids[0, 1] = 2, 2
    sem[0, 2], ids[0, 2] = 1, 4
    sem[0, 3], ids[0, 3] = 1, 5
    sem[0, 4, :7], sem[0, 4, 7:14], sem[0, 4, 14:] = -1, 255, 4
    ids[0, 4] = 3
    sem[0, 5] = 5                                                       # plain stuff
    sem[0, 6] = 3                                                       # thing pixels without an id
    sem[0, 7, :8], sem[0, 7, 8:] = -1, 255
    return sem, ids, is_thing, top_k


# ---- per-instance sums ------------------------------------------------------------------------
def stats_case(slots, n=2, h=48, w=64, seed=51):
    """ids drawn from a few values around the LDS / global switch (<= 1024 slots: LDS histogram),
    including 0, a negative id and ids at and beyond `slots`; scores with 0, 1, > 1, negative and NaN;
    orientation components with +-2e4 (beyond the +-2^14 clamp) and NaN"""
    g = torch.Generator().manual_seed(seed + slots)
    values = torch.tensor([-1, 0, 1, 2, 3, 17, 255, 256, 511, 1022, 1023, 1024, 1025, 1030, 5000])
    ids = values[torch.randint(0, len(values), (n, h, w), generator=g)].to(torch.int32)
    score = torch.rand(n, h, w, generator=g)
    special = torch.tensor([0.0, 1.0, 1.5, -0.25, float('nan'), 1e-10, 0.999999])
    sel = torch.rand(n, h, w, generator=g) < 0.3
    score[sel] = special[torch.randint(0, len(special), (int(sel.sum()),), generator=g)]
    ori = torch.randn(n, 2, h, w, generator=g)
    spec_o = torch.tensor([2e4, -2e4, float('nan'), 16384.0, -16384.0, 0.0])
    sel = torch.rand(n, 2, h, w, generator=g) < 0.3
    ori[sel] = spec_o[torch.randint(0, len(spec_o), (int(sel.sum()),), generator=g)]
    mask = torch.rand(n, h, w, generator=g) > 0.4
    return ids, score, ori, mask


# ---- normalisation ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_frames(n=4, h=480, w=640, seed=61):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    rgb[0, 0, 0] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    rgb[-1, -1, -1] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    depth = torch.randint(0, 65536, (n, h, w), generator=g, dtype=torch.int32)
    depth[0, :5] = 0
    edge = torch.tensor([0, 1, 32767, 32768, 65535], dtype=torch.int32)
    depth[1, 0, :5] = edge
    depth[-1, -1, -5:] = edge
    return rgb, depth


def norm_tol(ref):
    """the suite's 2e-6 on normalised values, scaled by the magnitude where that exceeds 1"""
    return 2e-6 * ref.abs().clamp(min=1.0)
