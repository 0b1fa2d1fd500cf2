"""CPU side of tests/test_postprocessing_edges_gpu.py: the constructed inputs (tests/postprocessing_cases.py)
have the properties the GPU cases are about, and the oracle extensions agree with the oracle they
extend.  No device is touched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocessing_cases as C   # noqa: E402
from oracle import postprocessing_oracle as O   # noqa: E402


@pytest.mark.parametrize('top_k,rounds', [(512, True), (257, True), (1, False)])
def test_distinct_heat_needs_a_merge_in_rounds(top_k, rounds):
    heat = C.distinct_heat()
    assert heat.dtype == torch.float32 and heat.shape == (2, 1, 64, 80)
    assert float(heat.min()) >= 0.1 and float(heat.max()) < 1.0
    for i in range(2):
        assert len(torch.unique(heat[i])) == 64 * 80                      # no ties
    _, keep = O.center_keep_mask(heat, 0.1, 1)
    assert bool(keep.all())                                              # window 1: every pixel survives
    cand = C.merge_candidates(heat, 0.1, 1, top_k)
    assert cand.tolist() == [5 * top_k] * 2                              # 5 chunks x top_k
    assert bool((cand > C.CHUNK).all()) == rounds
    if top_k == 512:
        assert -(-(5 * 512 - 1024) // (1024 - 512)) + 1 == 4             # a four-round merge


@pytest.mark.parametrize('case', ['plateau', 'two_levels', 'late_peaks'])
def test_default_parameter_heat_needs_a_merge_in_rounds(case):
    heat = C.default_heat(case)
    assert heat.shape[-2] * heat.shape[-1] == 17 * C.CHUNK
    cand = C.merge_candidates(heat, 0.1, 17, 64)
    assert bool((cand > C.CHUNK).all()), cand
    ref = O.instance_centers(heat, 0.1, 17, 64)
    for i in range(2):
        assert len(ref[i][0]) == 64
        pos = ref[i][0][:, 0] * heat.shape[-1] + ref[i][0][:, 1]
        if case == 'two_levels':
            assert int(pos.min()) >= 8 * C.CHUNK        # the whole top-k lies beyond the first 8 chunks
        if case == 'late_peaks':
            assert int(pos[ref[i][1] > 0.75].min()) >= 10 * C.CHUNK      # the peaks: in the last chunks
    if case == 'late_peaks':
        assert float(ref[0][1][0]) > 0.75 and float(ref[0][1][-1]) == 0.75  # peaks first, then plateau


def test_keep_mask_is_what_instance_centers_uses():
    heat = C.blob_heat(2, 20, 24, seed=7)
    for kernel in (3, 17, 31):                                           # 31: larger than the image
        x, keep = O.center_keep_mask(heat, 0.1, kernel)
        ref = O.instance_centers(heat, 0.1, kernel, 512)
        for i in range(2):
            assert len(ref[i][0]) == int(keep[i].sum()) > 0
    assert int(O.center_keep_mask(heat, 0.1, 31)[1][0].sum()) == 1       # one global maximum survives
    # heat exactly at the threshold is kept (the comparison runs in fp32 on both sides)
    at = torch.full((1, 1, 4, 4), 0.1)
    assert len(O.instance_centers(at, 0.1, 3, 8)[0][0]) == 8


def test_big_inputs_exceed_the_capped_grids():
    sem, ids, score, cscore, ref_m, _ = C.big_panoptic()
    assert sem.numel() == 4 * 480 * 640 > C.PIXELS_1D
    for i in range(4):
        assert sorted(ids[i].unique().tolist()) == list(range(C.TOP_K + 1))   # all 64 ids and 0
    assert (ref_m['semantic'] == 0).any() and (ref_m['instance'] > 0).any()
    rgb, depth = C.big_frames()
    assert rgb.shape[:3].numel() > C.PIXELS_1D and depth.numel() > C.PIXELS_1D
    assert int(rgb.min()) == 0 and int(rgb.max()) == 255
    for v in (0, 1, 32767, 32768, 65535):
        assert bool((depth == v).any())
    # (..., and both halves of the stride carry them)
    assert int(depth.reshape(-1)[C.PIXELS_1D:].max()) == 65535
    assert 480 * 640 > C.ASSIGN_THREADS                                   # one image makes 2a stride


@pytest.mark.parametrize('fg,dist', [(False, None), (True, None), (False, 6.0)])
def test_assignment_bound_holds_for_an_fp32_evaluation_of_the_oracle(fg, dist):
    """the near-tie rule and the share cap of the GPU test, applied to the oracle's own fp32 evaluation
    (torch, no contraction): the bound is derived, not fitted"""
    off, centers, mask = C.assign_case(near=True)
    assert off.shape == (1, 2, 480, 640) and centers.shape == (1, 64, 2)
    ref = [(centers[0], None)]
    d = O.instance_assign_sqdist(off[:, :, :8], [(centers[0],)], True)[0]
    assert torch.equal(d[:, 15, 0], d[:, 15, 1])                          # the exact ties are there
    # ... and so are the near-ties: pixels whose two best centres (or whose best centre and the rim of
    # the distance threshold) lie closer in fp64 than the bound, i.e. pixels part two is about
    dall = O.instance_assign_sqdist(off, [(centers[0],)], True)[0]
    E = C.assign_bound(off[0], dall, 480, 640, True)
    two, idx = dall.topk(2, dim=-1, largest=False)
    Etwo = E.gather(-1, idx)
    assert int((two[..., 1] - two[..., 0] <= Etwo.sum(-1))[240].sum()) >= 20
    assert int(((two[..., 0] - 36.0).abs() <= Etwo[..., 0])[241].sum()) >= 150
    assert C.NEAR_TIES / (480 * 640) <= 1e-4 and (C.NEAR_TIES + C.NEAR_RIM) / (480 * 640) <= 1e-3
    assert bool(mask[0, 240:242].all())
    del dall, E, two, idx, Etwo
    ids32 = O.instance_assign(off, ref, mask if fg else None, True, max_distance=dist)
    nc = torch.tensor([64])
    share, worst, gap, bound = C.assign_check(ids32, off, centers, nc, mask if fg else None, True, dist,
                                              1e-3 if dist else 1e-4)
    print(f"fp32 oracle vs fp64: share {share:.3e}, worst gap {gap:.3e} (bound {bound:.3e})")
    assert worst <= 1.0
    # a clearly wrong centre on ONE pixel is caught by part two although the share stays far below the cap
    x = 300 if not fg else int(torch.nonzero(mask[0, 200])[0])
    far = int(O.instance_assign_sqdist(off, [(centers[0],)], True)[0][200, x].argmax()) + 1
    wrong = ids32.clone()
    wrong[0, 200, x] = far
    with pytest.raises(AssertionError, match='near-tie'):
        C.assign_check(wrong, off, centers, nc, mask if fg else None, True, dist, 1e-3 if dist else 1e-4)


def test_small_assignment_inputs_obey_the_rule_in_fp32():
    """the inputs of the existing small test and the un-normalised case"""
    for normalized in (True, False):
        off, centers, mask = C.assign_case(n=2, h=60, w=80, k=64, seed=33, normalized=normalized)
        ids32 = O.instance_assign(off, [(centers[0], None), (centers[1], None)], None, normalized)
        C.assign_check(ids32, off, centers, torch.tensor([64, 64]), None, normalized, None, 1e-4)


def test_merge_oracle_extensions_keep_the_old_behaviour():
    g = torch.Generator().manual_seed(11)
    nc = 40
    is_thing = [bool(i % 3) for i in range(nc)]
    sem = torch.randint(0, nc, (2, 10, 14), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    ids = torch.randint(0, 9, (2, 5, 7), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.int32)
    a = O.panoptic_merge(sem, ids, is_thing)
    b = O.panoptic_merge(sem, ids, is_thing, top_k=64)
    for key in ('semantic', 'instance', 'panoptic'):
        assert torch.equal(a[key], b[key])
    assert b['instance_class'].shape == (2, 65)
    # the constructed case says what its docstring says
    sem, ids, is_thing, top_k = C.small_merge_case()
    r = O.panoptic_merge(sem, ids, is_thing, top_k=top_k)
    assert r['instance_class'][0].tolist() == [-1, 3, -1, 4, 1]
    assert r['semantic'][0, 0].tolist() == [4] * 16 and r['instance'][0, 0].tolist() == [1] * 16
    assert r['semantic'][0, 1].tolist() == [3] * 16 and int(r['instance'][0, 1].max()) == 0
    assert int(r['panoptic'][0, 3].max()) == 0                           # id top_k + 1: ignored
    assert r['panoptic'][0, 2].tolist() == [2 * 1000 + 4] * 16           # id top_k: kept
    assert r['panoptic'][0, 4].tolist() == [0] * 14 + [5 * 1000 + 3] * 2
    assert int(r['panoptic'][0, 6:].max()) == 0 and r['panoptic'][0, 5].tolist() == [6000] * 16


@pytest.mark.parametrize('slots', [1024, 1025])
def test_sum_oracles_agree_with_the_dictionary_oracles(slots):
    import math
    ids, score, ori, mask = C.stats_case(slots)
    assert bool((ids == slots - 1).any()) and bool((ids == slots).any()) and bool((ids < 0).any())
    assert bool(score.isnan().any()) and bool((score > 1).any()) and bool((score < 0).any())
    assert bool((ori.abs() > 16384).any()) and bool(ori.isnan().any())
    for mk in (None, mask):
        area, ssum = O.instance_sums(ids, slots, score, mk)
        vec, cnt = O.instance_orientation_sums(ori, ids, slots, mk)
        assert torch.equal(area, cnt) and torch.equal(area, O.instance_sums(ids, slots, None, mk))
        assert int(area[:, 0].sum()) == 0
        for i in range(ids.shape[0]):
            for k in range(1, slots):
                m = ids[i] == k
                if mk is not None:
                    m = m & mk[i]
                assert int(area[i, k]) == int(m.sum())
        assert int(area.sum()) > 2000
        # the angle dictionaries of the existing oracle follow from the sums
        ref = O.instance_orientations(ori, ids.clamp(max=slots - 1) * (ids < slots), mk)
        for i, d in enumerate(ref):
            for k, a in d.items():
                assert a == math.atan2(float(vec[i, k, 0]), float(vec[i, k, 1])) % (2.0 * math.pi)
    # the score sums are the ones panoptic_scores' means are made of
    ids2 = (ids.clamp(min=0) * (ids < slots)).to(torch.int32)
    _, _, _, per = O.panoptic_scores(score, ids2, torch.ones_like(ids2, dtype=torch.int64),
                                     list(torch.ones(2, slots)))
    area, ssum = O.instance_sums(ids, slots, score)
    for i, d in enumerate(per):
        for k, (a, mean, _) in d.items():
            assert a == int(area[i, k])
            import numpy as np
            assert mean == float(np.float32(float(ssum[i, k]) / float(a) / 2.0 ** 30))


def test_cap_heat_fills_the_candidate_lists_exactly():
    heat = C.cap_heat()
    k = C.CAP_TOP_K
    assert heat.shape == (3, 1, 33, 64) and -(-33 * 64 // C.CHUNK) == 3           # cap = 3 * top_k
    _, keep = O.center_keep_mask(heat, 0.1, 1)
    assert keep.reshape(3, -1).sum(1).tolist() == [3 * k, 3 * k + 1, k]
    assert C.merge_candidates(heat, 0.1, 1, k).tolist() == [3 * k, 3 * k, k]
    ref = O.instance_centers(heat, 0.1, 1, k)
    assert [len(r[0]) for r in ref] == [k, k, k]
    vals = heat[heat > 0]
    assert vals.unique().numel() == vals.numel() == 7 * k + 1 and float(vals.min()) >= 0.2
    # the survivor that image 1 loses to the cap is the lowest of its first chunk: not among the top k
    first = heat[1, 0].view(-1)[:C.CHUNK]
    assert float(first[first > 0].min()) < float(ref[1][1].min())
