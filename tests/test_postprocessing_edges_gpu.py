"""The eval post-processing kernels (emsanet_amd/csrc/postproc.hip) at real frame sizes and at the
edges tests/test_postprocessing.py does not reach: the merge of the centre top-k in rounds, top_k up to
512, other NMS windows, every softmax / arg-max template and its class-count boundaries, the
grid-stride loops of every capped launch, the LDS / global switch of the per-instance sums, the
constructed panoptic-merge cases, the full input range of the normalisation, and the dtype contract of
the Python wrappers.  References: oracle/postprocessing_oracle.py (fp64 where arithmetic matters) or
torch itself; the inputs are built in tests/postprocessing_cases.py, whose claimed properties
tests/test_postprocessing_edges.py checks without a device.

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (index maps, ids, areas,
integer sums and the -1 padding of the centre lists are compared exactly, and -1 is what 0xFF reads
as): outputs and the integer work buffers -- candidate lists of n * cap entries, votes of
(top_k + 1) * nc, per-slot sums -- lie between two bands of 0xFF; inputs are placed with `_d`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocessing_cases as C   # noqa: E402
import guard   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)
from oracle import postprocessing_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _d(t):
    """`t` on the device, flush between two bands of 0xFF"""
    return guard.put(t.to(DEV))


def _err():
    from emsanet_amd._lib import EmsaError
    return EmsaError


# ---- 1. centres --------------------------------------------------------------------------------
def _check_centers(heat, threshold, kernel, top_k, fg=None, twice=True):
    from emsanet_amd.postprocessing import instance_centers
    dfg = None if fg is None else _d(fg)
    c1, s1, n1, surv = instance_centers(_d(heat), threshold, kernel, top_k, dfg, return_survivors=True)
    if twice:
        c2, s2, n2 = instance_centers(_d(heat), threshold, kernel, top_k, dfg)
        assert torch.equal(c1, c2) and torch.equal(s1, s2) and torch.equal(n1, n2)   # reproducible
    guard.check()
    ref = O.instance_centers(heat, threshold, kernel, top_k, fg)
    _, keep = O.center_keep_mask(heat, threshold, kernel, fg)
    assert surv.cpu().tolist() == keep.reshape(keep.shape[0], -1).sum(1).tolist()
    assert c1.shape == (heat.shape[0], top_k, 2) and s1.shape == (heat.shape[0], top_k)
    for i in range(heat.shape[0]):
        k = int(n1[i])
        assert k == len(ref[i][0]), (i, k, len(ref[i][0]))
        assert torch.equal(c1[i, :k].cpu(), ref[i][0]), i
        assert torch.equal(s1[i, :k].cpu(), ref[i][1]), i                # bit-equal scores
        assert bool((c1[i, k:] == -1).all()) and bool((s1[i, k:] == 0).all())
    return c1, s1, n1, ref


def test_center_sort_widths_are_what_the_cases_assume():
    from emsanet_amd import _lib
    L = _lib.lib()
    assert L.emsa_center_candidates_max() == C.CHUNK == 1024
    assert L.emsa_center_ws_entries(64, 80, 1) == 5                       # chunks of 1024 pixels
    assert L.emsa_center_ws_entries(136, 128, 1) == 17
    assert L.emsa_center_ws_entries(64, 80, 512) == 5 * 512


@pytest.mark.parametrize('top_k', [512, 257, 1])
def test_center_topk_merge_in_rounds_small(top_k):
    """64 x 80, window 1, distinct heat: every pixel survives; 5 chunks x top_k candidates -- 2560 for
    top_k = 512 (a four-round merge, write-back of the NMS pass in two strides), 1285 for 257"""
    heat = C.distinct_heat()
    _, _, n1, _ = _check_centers(heat, 0.1, 1, top_k)
    assert n1.cpu().tolist() == [top_k] * 2


@pytest.mark.parametrize('case', ['plateau', 'two_levels', 'late_peaks'])
def test_center_topk_merge_in_rounds_default_parameters(case):
    """136 x 128, window 17, top_k 64: 17 chunks x 64 = 1088 candidates, two rounds"""
    heat = C.default_heat(case)
    _, _, n1, _ = _check_centers(heat, 0.1, 17, 64)
    assert n1.cpu().tolist() == [64] * 2


def test_center_candidate_lists_exactly_full_and_one_over():
    """33 x 64, top_k 8: cap = 24 candidates per image.  Image 0 hands in exactly 24, image 1 has a ninth
    survivor in its first chunk, which is cut, image 2 has exactly top_k survivors: all eight centre
    slots used, none padded (tests/test_postprocessing_edges.py: the heat map's claims)"""
    from emsanet_amd import _lib
    heat, k = C.cap_heat(), C.CAP_TOP_K
    assert _lib.lib().emsa_center_ws_entries(33, 64, k) == 3 * k
    c1, s1, n1, _ = _check_centers(heat, 0.1, 1, k)
    assert n1.cpu().tolist() == [k] * 3
    assert bool((c1 >= 0).all()) and bool((s1 >= 0.2).all())


@pytest.mark.parametrize('kernel', [3, 31])
def test_center_nms_windows(kernel):
    heat = C.blob_heat(2, 20, 24, seed=7)
    _, _, n1, _ = _check_centers(heat, 0.1, kernel, 64)
    assert int(n1.min()) > 0
    if kernel == 31:                                                     # larger than the image
        assert n1.cpu().tolist() == [1, 1]


def test_center_refusals():
    from emsanet_amd.postprocessing import instance_centers
    heat = C.blob_heat(1, 20, 24, seed=7).to(DEV)
    for kw in ({'nms_kernel_size': 16}, {'nms_kernel_size': 0}, {'top_k': 513}, {'top_k': 0}):
        with pytest.raises(_err()):
            instance_centers(heat, **kw)
    torch.cuda.synchronize()
    assert int(instance_centers(heat, top_k=512)[2][0]) > 0               # 512 itself is served


def test_center_score_edges():
    # heat exactly at the threshold is kept
    at = torch.full((1, 1, 4, 4), 0.1)
    _, _, n1, _ = _check_centers(at, 0.1, 3, 64)
    assert int(n1[0]) == 16
    # an image entirely below the threshold beside a full one
    heat = C.blob_heat(3, 40, 56, seed=8)
    heat[1] = 0.0999
    c, s, n1, ref = _check_centers(heat, 0.1, 17, 64)
    assert int(n1[1]) == 0 and int(n1[0]) > 0 and int(n1[2]) > 0
    assert bool((c[1] == -1).all()) and bool((s[1] == 0).all())
    alone = _check_centers(heat[2:], 0.1, 17, 64)
    assert torch.equal(alone[0][0], c[2]) and torch.equal(alone[1][0], s[2])   # unaffected by the neighbour
    # a foreground mask that removes the global maximum (and its surroundings)
    fg = torch.ones(3, 40, 56, dtype=torch.bool)
    for i in (0, 2):
        y, x = [int(v) for v in ref[i][0][0]]
        fg[i, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = False
    c2, s2, n2, ref2 = _check_centers(heat, 0.1, 17, 64, fg)
    for i in (0, 2):
        assert float(s2[i, 0]) < float(s[i, 0])
        assert not bool((c2[i, :int(n2[i])] == c[i, 0]).all(1).any())


# ---- 2. assignment -----------------------------------------------------------------------------
def _assign(off, centers, nc, fg, normalized, dist):
    from emsanet_amd.postprocessing import instance_assign
    return instance_assign(_d(off), _d(centers), _d(nc), None if fg is None else _d(fg),
                           normalized, dist).cpu()


@pytest.mark.parametrize('with_fg,dist', [(False, None), (True, None), (False, 6.0), (True, 6.0)])
def test_assignment_real_frame_64_centres(with_fg, dist):
    """one 480 x 640 image: 307,200 pixels on 262,144 threads, so the per-image grid strides.  Two-part
    rule (tests/postprocessing_cases.py: assign_bound / assign_check): the share of pixels differing
    from the fp64 arg-min stays within 1e-4 (1e-3 with the distance threshold), and every differing
    pixel is a near-tie within the fp32 rounding bound of the kernel's own expression"""
    off, centers, mask = C.assign_case(near=True)
    nc = torch.tensor([64], dtype=torch.int32)
    fg = mask if with_fg else None
    ids = _assign(off, centers, nc, fg, True, dist)
    share, worst, gap, bound = C.assign_check(ids, off, centers, nc, fg, True, dist, 1e-3 if dist else 1e-4)
    print(f"assignment 480x640 fg={with_fg} dist={dist}: share of differing pixels {share:.3e}, "
          f"largest near-tie gap {gap:.3e} (bound there {bound:.3e}, ratio {worst:.3f})")
    # zero offsets in rows [0, 8): exact arithmetic, exact ties included -> equal to the fp64 arg-min
    d = O.instance_assign_sqdist(off[:, :, :8], [(centers[0],)], True)[0]
    best, arg = d.min(-1)
    ref = arg + 1
    if dist:
        ref[best > dist * dist] = 0
    if with_fg:
        ref[~mask[0, :8]] = 0
    assert torch.equal(ids[0, :8].long(), ref)
    # and the share against the existing fp32 oracle, as in tests/test_postprocessing.py
    rid = O.instance_assign(off, [(centers[0], None)], fg, True, max_distance=dist)
    assert (ids != rid).float().mean().item() <= (1e-3 if dist else 1e-4)


@pytest.mark.parametrize('normalized', [True, False])
def test_assignment_small_edges(normalized):
    """512 centres (the maximum), an image without centres beside one with, un-normalised offsets"""
    off, centers, mask = C.assign_case(n=2, h=60, w=80, k=512, seed=35, normalized=normalized)
    nc = torch.tensor([512, 0], dtype=torch.int32)
    for fg, dist in ((None, None), (mask, 6.0)):
        ids = _assign(off, centers, nc, fg, normalized, dist)
        guard.check()
        assert int(ids[1].abs().max()) == 0                               # no centres: no instance
        assert int(ids[0].max()) > 256
        C.assign_check(ids, off, centers, nc, fg, normalized, dist, 1e-3 if dist else 1e-4)
    nc = torch.tensor([0, 37], dtype=torch.int32)
    ids = _assign(off, centers, nc, None, normalized, None)
    assert int(ids[0].abs().max()) == 0 and int(ids[1].max()) == 37
    C.assign_check(ids, off, centers, nc, None, normalized, None, 1e-4)


# ---- 3. softmax / arg-max ----------------------------------------------------------------------
def _check_softmax(x, dev_x=None):
    from emsanet_amd.postprocessing import softmax_argmax
    score, idx = softmax_argmax(_d(x) if dev_x is None else dev_x)
    guard.check()
    rs, ri = O.softmax_argmax(x)
    assert idx.dtype == torch.int64 and score.dtype == torch.float32
    assert torch.equal(idx.cpu(), ri)
    err = (score.cpu().double() - rs).abs().max().item()
    assert err <= 1e-6, err
    return score, idx


@pytest.mark.parametrize('c', [1, 2, 16, 17, 19, 37, 40, 41, 64])
def test_softmax_argmax_class_counts(c):
    """every template (<= 16, <= 40, <= 64 classes) on both sides of its boundaries; pixel counts around
    the 256-pixel workgroup; 41 and 64 classes ask for 69,632 bytes of dynamic LDS"""
    g = torch.Generator().manual_seed(100 + c)
    for shape in ((1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (2, 30, 41)):
        n, h, w = shape
        x = torch.randn(n, c, h, w, generator=g) * 4
        if c >= 6:
            x[0, 3, 0, 0] = x[0, 5, 0, 0] = 17.0                         # a tie: first maximum wins
        _check_softmax(x)
        _check_softmax(x, _d(x).contiguous(memory_format=torch.channels_last))


def test_softmax_argmax_refuses_65_classes():
    from emsanet_amd.postprocessing import softmax_argmax
    with pytest.raises(_err()):
        softmax_argmax(torch.zeros(1, 65, 2, 2, device=DEV))
    with pytest.raises(_err()):
        softmax_argmax(torch.zeros(3, 65, device=DEV))


def test_softmax_argmax_padded_view_ignores_the_pad_channels():
    from emsanet_amd.postprocessing import softmax_argmax
    g = torch.Generator().manual_seed(7)
    n, c, h, w = 2, 37, 30, 41
    x = torch.randn(n, c, h, w, generator=g) * 4
    buf = torch.empty(n, h, w, 40)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    buf[..., 37], buf[..., 38], buf[..., 39] = float('inf'), float('nan'), 1e30
    view = _d(buf)[..., :c].permute(0, 3, 1, 2)
    assert view.stride(3) == 40
    s1, i1 = _check_softmax(x, view)
    s2, i2 = softmax_argmax(_d(x))
    assert torch.equal(s1, s2) and torch.equal(i1, i2)


@pytest.mark.parametrize('c', [3, 19, 40, 64])
def test_softmax_argmax_logit_edges(c):
    g = torch.Generator().manual_seed(200 + c)
    p = 300
    base = torch.randn(1, c, 1, p, generator=g) * 3
    # all logits equal: score 1 / C, index 0
    s, i = _check_softmax(torch.full((1, c, 1, p), -2.5))
    assert int(i.abs().max()) == 0 and float((s - 1.0 / c).abs().max()) <= 1e-6
    # one logit 80 above the rest
    x = base.clone()
    x[0, c - 2] = base.max() + 80.0
    s, i = _check_softmax(x)
    assert bool((i == c - 2).all()) and float(s.min()) == 1.0
    # all logits shifted by +-1e4
    _check_softmax(base + 1e4)
    _check_softmax(base - 1e4)
    # -inf in non-maximal classes
    x = base.clone()
    top = base.argmax(1, keepdim=True)
    x[:, 0::2] = float('-inf')
    x.scatter_(1, top, base.gather(1, top))
    _, i = _check_softmax(x)
    assert torch.equal(i.cpu(), top[:, 0])
    # a tie between the first and the last class
    x = base.clone()
    x[0, 0] = x[0, c - 1] = base.max() + 1.0
    _, i = _check_softmax(x)
    assert int(i.abs().max()) == 0


@pytest.mark.parametrize('n', [1, 257])
@pytest.mark.parametrize('c', [10, 64])
def test_softmax_argmax_rows(n, c):
    """the (N, C) form of the scene head"""
    from emsanet_amd.postprocessing import softmax_argmax
    g = torch.Generator().manual_seed(300 + n + c)
    x = torch.randn(n, c, generator=g) * 4
    score, idx = softmax_argmax(_d(x))
    rs, ri = O.softmax_argmax(x)
    assert score.shape == idx.shape == (n,)
    assert torch.equal(idx.cpu(), ri) and (score.cpu().double() - rs).abs().max() <= 1e-6


# ---- 4. panoptic merge, scores, per-instance sums ----------------------------------------------
def test_panoptic_merge_and_scores_on_a_batch_of_real_frames():
    """(4, 480, 640) = 1,228,800 pixels > 4096 x 256 threads: the votes / merge / pixel-score kernels
    stride (and the per-image stats grid does).  Bit-equal to the oracle, twice in a row"""
    from emsanet_amd.postprocessing import panoptic_merge, panoptic_scores
    sem, ids, score, cscore, ref_m, (rs, ri, rp, per) = C.big_panoptic()
    dsem, dids, dscore, dcs = _d(sem), _d(ids), _d(score), _d(cscore)
    for _ in range(2):
        m = panoptic_merge(dsem, dids, C.IS_THING, top_k=C.TOP_K)
        for key in ('semantic', 'instance', 'panoptic', 'instance_class'):
            assert torch.equal(m[key].cpu(), ref_m[key].to(m[key].dtype)), key
        got = panoptic_scores(dscore, m['instance'], m['semantic'], dcs)
        guard.check()
        assert torch.equal(got['semantic_score'].cpu(), rs)
        assert torch.equal(got['instance_score'].cpu(), ri)
        assert torch.equal(got['panoptic_score'].cpu(), rp)
    area, isem, ipan = (got[k].cpu() for k in ('area', 'instance_semantic_score', 'instance_panoptic_score'))
    for i, d in enumerate(per):
        assert len(d) > 50
        for k, (a, mean, pan) in d.items():
            assert (int(area[i, k]), float(isem[i, k]), float(ipan[i, k])) == (a, mean, pan)


def test_panoptic_merge_constructed_cases():
    from emsanet_amd.postprocessing import panoptic_merge
    sem, ids, is_thing, top_k = C.small_merge_case()
    ref = O.panoptic_merge(sem, ids, is_thing, top_k=top_k)
    for s in (sem, sem.flip(2)):            # the tie must not depend on which class is met first
        i = ids if s is sem else ids.flip(2)
        r = ref if s is sem else {k: (v.flip(2) if v.dim() == 3 else v) for k, v in ref.items()}
        got = panoptic_merge(_d(s), _d(i), is_thing, top_k=top_k)
        for key in ('semantic', 'instance', 'panoptic', 'instance_class'):
            assert torch.equal(got[key].cpu(), r[key].to(got[key].dtype)), key
    assert got['instance_class'][0].cpu().tolist() == [-1, 3, -1, 4, 1]   # tie -> lower class; stuff -> -1
    # label_divisor <= top_k is refused
    with pytest.raises(_err()):
        panoptic_merge(_d(sem), _d(ids), is_thing, top_k=top_k, label_divisor=top_k)
    torch.cuda.synchronize()
    got = panoptic_merge(_d(sem), _d(ids), is_thing, top_k=top_k, label_divisor=top_k + 1)
    ref = O.panoptic_merge(sem, ids, is_thing, label_divisor=top_k + 1, top_k=top_k)
    assert torch.equal(got['panoptic'].cpu(), ref['panoptic'])


@pytest.mark.parametrize('slots', [1024, 1025])
def test_instance_sums_at_the_lds_switch(slots):
    """<= 1024 id slots: per-workgroup LDS histogram; above: global atomics.  Integer-equal sums"""
    from emsanet_amd.postprocessing import instance_orientation_sums, instance_stats
    ids, score, ori, mask = C.stats_case(slots)
    for mk in (None, mask):
        dmk = None if mk is None else _d(mk)
        ra, rsum = O.instance_sums(ids, slots, score, mk)
        rvec, rcnt = O.instance_orientation_sums(ori, ids, slots, mk)
        for _ in range(2):
            area, ssum = instance_stats(_d(ids), slots, _d(score), dmk)
            assert torch.equal(area.cpu().long(), ra) and torch.equal(ssum.cpu(), rsum)
            assert torch.equal(instance_stats(_d(ids), slots, None, dmk).cpu().long(), ra)
            vec, cnt = instance_orientation_sums(_d(ori), _d(ids), slots, dmk)
            guard.check()
            assert torch.equal(vec.cpu(), rvec) and torch.equal(cnt.cpu().long(), rcnt)
    assert int(ra[:, slots - 1].min()) > 0


# ---- 5. normalisation --------------------------------------------------------------------------
def test_normalize_rgb_full_range_batch_of_real_frames():
    from emsanet_amd.postprocessing import RGB_MEAN, RGB_STD, normalize_rgb
    rgb, _ = C.big_frames()
    drgb = _d(rgb)
    for mean, std, scale in ((RGB_MEAN, RGB_STD, 1.0 / 255.0), ((100.0, 110.0, 120.0), (50.0, 60.0, 70.0), 1.0)):
        out = normalize_rgb(drgb, mean, std, scale).cpu()
        ref = ((rgb.double() * scale - torch.tensor(mean, dtype=torch.float64)) /
               torch.tensor(std, dtype=torch.float64)).permute(0, 3, 1, 2)
        assert out.shape == (4, 3, 480, 640)
        assert bool(((out.double() - ref).abs() <= C.norm_tol(ref)).all())
        assert float(ref.abs().max()) > 2.0
    for std in ((0.0, 1.0, 1.0), (1.0, 1.0, 0.0)):
        with pytest.raises(_err()):
            normalize_rgb(drgb[:1, :8, :8], RGB_MEAN, std)
    with pytest.raises(_err()):
        normalize_rgb(rgb)                                                # a host tensor
    torch.cuda.synchronize()


@pytest.mark.parametrize('keep_zero', [True, False])
def test_normalize_depth_full_range_batch_of_real_frames(keep_zero):
    """values at and above 32768 are negative in the int16 view the wrapper accepts"""
    from emsanet_amd.postprocessing import normalize_depth
    _, depth = C.big_frames()
    d16 = torch.from_numpy(depth.numpy().astype(np.uint16).view(np.int16))
    assert int(d16.min()) < 0
    for mean, std in ((2841.9, 1417.3), (1000.0, -250.5)):
        out = normalize_depth(_d(d16), mean, std, keep_zero).cpu()
        ref = (depth.double() - mean) / std
        if keep_zero:
            ref[depth == 0] = 0.0
        ref = ref[:, None]
        assert out.shape == (4, 1, 480, 640)
        assert bool(((out.double() - ref).abs() <= C.norm_tol(ref)).all())
        zero = out[:, 0][depth == 0]
        assert bool((zero == 0).all()) if keep_zero else bool((zero != 0).all())
        u16 = torch.from_numpy(depth.numpy().astype(np.uint16)).to(DEV)  # the unsigned view of the same bits
        assert torch.equal(normalize_depth(u16, mean, std, keep_zero).cpu(), out)
    with pytest.raises(_err()):
        normalize_depth(d16[:1, :8, :8].to(DEV), 1.0, 0.0)
    with pytest.raises(_err()):
        normalize_depth(d16, 1.0, 1.0)                                    # a host tensor
    with pytest.raises(_err()):
        normalize_depth(depth[:1, :8, :8].to(DEV), 1.0, 1.0)              # int32: not a 16-bit frame
    torch.cuda.synchronize()


# ---- 6. dtype contract of the wrappers ---------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_16bit_activations_are_read_as_their_fp32_images(dtype):
    from emsanet_amd.postprocessing import instance_assign, instance_centers, softmax_argmax
    g = torch.Generator().manual_seed(71)
    n, h, w = 2, 40, 56
    logits = (torch.randn(n, 19, h, w, generator=g) * 4).to(dtype).to(DEV)
    heat = C.blob_heat(n, h, w, seed=9).to(dtype).to(DEV)
    off = ((torch.rand(n, 2, h, w, generator=g) * 2 - 1) * 0.2).to(dtype).to(DEV)
    s16, i16 = softmax_argmax(logits)
    s32, i32 = softmax_argmax(logits.float())
    assert torch.equal(s16, s32) and torch.equal(i16, i32)
    rs, ri = O.softmax_argmax(logits.float().cpu())
    assert torch.equal(i16.cpu(), ri) and (s16.cpu().double() - rs).abs().max() <= 1e-6
    r16 = softmax_argmax(logits[:, :, 0, 0])
    r32 = softmax_argmax(logits[:, :, 0, 0].float())
    assert torch.equal(r16[0], r32[0]) and torch.equal(r16[1], r32[1])
    c16 = instance_centers(heat)
    c32 = instance_centers(heat.float())
    assert all(torch.equal(a, b) for a, b in zip(c16, c32)) and int(c32[2].min()) > 0
    ref = O.instance_centers(heat.float().cpu())
    assert torch.equal(c16[0][0, :int(c16[2][0])].cpu(), ref[0][0])
    a16 = instance_assign(off, c32[0].to(dtype), c32[2])                  # (centres < 256: exact in bf16)
    a32 = instance_assign(off.float(), c32[0], c32[2])
    assert torch.equal(a16, a32) and int(a32.max()) > 1


def test_integer_inputs_are_converted_to_the_width_the_kernels_read():
    from emsanet_amd.postprocessing import (instance_assign, instance_orientation_sums, instance_stats,
                                            panoptic_merge, panoptic_scores)
    g = torch.Generator().manual_seed(72)
    n, h, w, nc, k = 2, 40, 56, 40, 16
    is_thing = [bool(i % 3) for i in range(nc)]
    sem = torch.randint(0, nc, (n, h // 4, w // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    ids = torch.randint(0, 9, (n, h // 8, w // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    score = torch.rand(n, h, w, generator=g)
    cscore = torch.rand(n, k, generator=g)
    ori = torch.randn(n, 2, h, w, generator=g)
    dsem, dids = _d(sem), _d(ids)                                 # both int64
    good = panoptic_merge(dsem, dids.int(), is_thing, top_k=k)
    ref = O.panoptic_merge(sem, ids.int(), is_thing, top_k=k)
    assert torch.equal(good['panoptic'].cpu(), ref['panoptic'])
    for s, i in ((dsem, dids), (dsem.int(), dids.int()), (dsem.int(), dids), (dsem.to(torch.uint8), dids.short())):
        got = panoptic_merge(s, i, is_thing, top_k=k)
        for key in good:
            assert torch.equal(got[key], good[key]), (s.dtype, i.dtype, key)
    a, ss = instance_stats(dids.int(), k + 1, _d(score))
    ra, rsum = O.instance_sums(ids, k + 1, score)
    assert torch.equal(a.cpu().long(), ra) and torch.equal(ss.cpu(), rsum)
    for i, v in ((dids, _d(score)), (dids.int(), score.double().to(DEV)), (dids.short(), _d(score))):
        a2, s2 = instance_stats(i, k + 1, v)
        assert torch.equal(a2, a) and torch.equal(s2, ss)
    v1 = instance_orientation_sums(_d(ori), dids.int(), k + 1)
    v2 = instance_orientation_sums(_d(ori), dids, k + 1)
    assert torch.equal(v1[0], v2[0]) and torch.equal(v1[1], v2[1])
    p1 = panoptic_scores(_d(score), good['instance'], good['semantic'], _d(cscore))
    p2 = panoptic_scores(score.double().to(DEV), good['instance'].long(), good['semantic'].int(),
                         cscore.half().to(DEV))
    p3 = panoptic_scores(_d(score), good['instance'], good['semantic'], cscore.half().float().to(DEV))
    assert torch.equal(p1['semantic_score'], p2['semantic_score']) and torch.equal(p1['area'], p2['area'])
    for key in p3:
        assert torch.equal(p2[key], p3[key]), key
    # int64 centre counts
    cen = C.random_centers(n, k, h, w, 3).to(DEV)
    off = ((torch.rand(n, 2, h, w, generator=g) * 2 - 1) * 0.2).to(DEV)
    cnt = torch.tensor([k, 5], dtype=torch.int32, device=DEV)
    assert torch.equal(instance_assign(off, cen, cnt), instance_assign(off, cen, cnt.long()))
    # what cannot be converted is refused by name, never reinterpreted
    E = _err()
    with pytest.raises(E, match='semantic_idx'):
        panoptic_merge(dsem.float(), dids.int(), is_thing, top_k=k)
    with pytest.raises(E, match='instance_ids'):
        panoptic_merge(dsem, dids.float(), is_thing, top_k=k)
    with pytest.raises(E, match='ids'):
        instance_stats(dids.float(), k + 1)
    with pytest.raises(E, match='logits'):
        from emsanet_amd.postprocessing import softmax_argmax
        softmax_argmax(dsem[:, None].expand(n, 4, h, w))
    torch.cuda.synchronize()


def test_host_tensors_are_refused():
    from emsanet_amd import postprocessing as P
    E = _err()
    x = torch.zeros(1, 4, 8, 8)
    ids = torch.zeros(1, 8, 8, dtype=torch.int32)
    sem = torch.zeros(1, 8, 8, dtype=torch.int64)
    cen, sc, nc = P.instance_centers(torch.rand(1, 1, 8, 8, device=DEV), top_k=4)
    dev_off = torch.zeros(1, 2, 8, 8, device=DEV)
    calls = [lambda: P.softmax_argmax(x), lambda: P.softmax_argmax(x[:, :, 0, 0]),
             lambda: P.instance_centers(x[:, :1]),
             lambda: P.instance_centers(x[:, :1].to(DEV), foreground=torch.ones(1, 8, 8, dtype=torch.bool)),
             lambda: P.instance_assign(x[:, :2], cen, nc),
             lambda: P.instance_assign(dev_off, cen.cpu(), nc),
             lambda: P.instance_assign(dev_off, cen, nc.cpu()),
             lambda: P.panoptic_merge(sem, _d(ids), [True, False]),
             lambda: P.panoptic_merge(_d(sem), ids, [True, False]),
             lambda: P.instance_stats(ids, 5),
             lambda: P.instance_stats(_d(ids), 5, x[:, 0]),
             lambda: P.instance_stats(_d(ids), 5, None, sem),
             lambda: P.panoptic_scores(x[:, 0], _d(ids), _d(sem), sc),
             lambda: P.panoptic_scores(x[:, 0].to(DEV), ids, _d(sem), sc),
             lambda: P.panoptic_scores(x[:, 0].to(DEV), _d(ids), sem, sc),
             lambda: P.panoptic_scores(x[:, 0].to(DEV), _d(ids), _d(sem), sc.cpu()),
             lambda: P.instance_orientation_sums(x[:, :2], _d(ids), 5),
             lambda: P.instance_orientation_sums(x[:, :2].to(DEV), ids, 5)]
    for j, call in enumerate(calls):
        with pytest.raises(E):
            call()
            pytest.fail(f"call {j} accepted a host tensor")
    torch.cuda.synchronize()


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
