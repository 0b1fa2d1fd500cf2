"""The SE channel reductions, the excitation MLP, the adaptive average pool and the 3x3/2 max pool at
the edges of their launch rules, on poisoned, guard-banded buffers.

Every reference is fp64 (or int64) on the CPU, computed from the same rounded inputs the kernel reads
(tests/reduce_pool_reference.py).  Two kinds of input:

* integer-valued (-3 .. 3, exact in fp32 / bf16 / fp16): every product and partial sum is an integer
  below 2^24, so fp32 summation is exact in ANY order and the comparison is equality -- a dropped,
  repeated or misassigned pixel, split or lane cannot pass at any map size;
* Gaussian with a non-zero mean, through `close()` at the tolerances stated in tests/test_ops16_gpu.py:
  1e-4 of the tensor's largest magnitude for fp32, 2e-4 for fp32 results from 16-bit inputs and for the
  parameter gradients, 6e-3 (bf16) / 1e-3 (fp16) for results stored in 16 bits.  `tight()` applies the
  same factor WITHOUT close()'s floor of 1 on the magnitude: the fp32 kernels sum at most 2,048 products
  per output (rounding error ~ sqrt(2048) * 6e-8 of the terms' magnitude), two orders below 1e-4.

The launch rules are restated in Python and asserted per case (`emsa_channel_ws_floats` for the
reductions), so the case lists show by themselves which branch each case takes.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import reduce_pool_reference as R
from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, close, rnd

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
TOL_STORE = {F32: 1e-4, BF16: 6e-3, F16: 1e-3}       # a result stored in the activation type
TOL_F32 = {F32: 1e-4, BF16: 2e-4, F16: 2e-4}         # an fp32 result computed from such inputs
NAME = {F32: 'fp32', BF16: 'bf16', F16: 'fp16'}


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _lib():
    from emsanet_amd import _lib
    return _lib.lib()


def act(t_nchw, dtype=F32):
    """CPU NCHW tensor -> GPU activation in `dtype` (logical NCHW, NHWC memory) between NaN bands"""
    t = t_nchw.to(dtype).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return guard.put(t)


def dev(t):
    return guard.put(t.float().contiguous().to(DEV))


def tight(got, ref, tol, what):
    """close(), and the same factor without its floor of 1: max |got-ref| <= tol * max|ref|"""
    err = close(got, ref, tol=tol, what=what)
    lim = tol * ref.detach().double().abs().max().item()
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e} (= {tol:g} of the largest magnitude)"


def same(got, ref, what):
    """equality of every element (no NaN on either side; -inf equals -inf)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert not torch.isnan(got).any(), f"{what}: NaN (an element the kernel did not write)"
    bad = got != ref
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                           f"{tuple(bad.nonzero()[0].tolist())}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}")


def gauss(*shape, seed, dtype, mean=1.0, scale=1.0):
    """Gaussian values around `mean`, rounded to `dtype`, as fp64"""
    return (rnd(*shape, seed=seed, scale=scale) + mean).to(dtype).double()


# =================================================================================================
# 1. channel reductions
# =================================================================================================
# (n, h, w, c, splits, chunk, dtypes): splits / chunk computed by hand from channel_splits
SPLIT_CASES = [
    (3, 6, 10, 8, 1, 60, DTYPES),                 # baseline: one workgroup per image
    (1, 3, 43, 8, 3, 43, DTYPES),                 # 64-pixel rule, 129 = 3 x 43 (ragged against 64)
    (1, 15, 20, 8, 5, 60, DTYPES),                # the /32 map at batch 1 ...
    (32, 15, 20, 8, 5, 60, DTYPES),               # ... and at batch 32 (32 x 1 <= 64 -> 64-pixel rule)
    (32, 19, 27, 8, 9, 57, DTYPES),               # n * splits = 64: the 64-pixel rule still
    (33, 19, 27, 8, 2, 257, DTYPES),              # n * splits = 66: the 512-pixel rule stays, last chunk 256
    (1, 113, 145, 8, 256, 65, DTYPES),            # cap of 256: splits 253 .. 255 are empty
    (2, 165, 200, 8, 64, 516, DTYPES),            # cap of 64 of the 512-pixel rule, last chunk 492
    # fp32 C = 64: 16 row lanes, four pixels per lane and iteration
    (1, 1, 7, 64, 1, 7, [F32]),                   # fewer pixels than lanes
    (1, 7, 9, 64, 1, 63, [F32]),                  # 4 * lanes - 1: remainder loop only
    (1, 8, 8, 64, 1, 64, [F32]),                  # 4 * lanes: one unrolled iteration, no remainder
    (1, 5, 13, 64, 2, 33, [F32]),                 # 4 * lanes + 1 -> two splits of 33 and 32
]
# (dtype, c, route): each at 15 x 20 with n = 1 and n = 3 (five splits of 60 pixels)
WIDTH_CASES = [
    (F32, 4, ('narrow', 256, 0)),                 # one channel vector, 256 row lanes
    (F32, 40, ('narrow', 25, 6)),                 # 10 vectors x 25 lanes: 6 idle threads
    (F32, 512, ('narrow', 2, 0)),
    (F32, 1024, ('narrow', 1, 0)),
    (F32, 1028, ('wide', 2, 1)),                  # channel_dot_wide_kernel: second group has one live thread
    (F32, 2048, ('wide', 2, 256)),
    (BF16, 8, ('narrow', 256, 0)), (F16, 8, ('narrow', 256, 0)),
    (BF16, 72, ('narrow', 28, 4)), (F16, 72, ('narrow', 28, 4)),        # 9 vectors x 28 lanes
    (BF16, 2048, ('narrow', 1, 0)), (F16, 2048, ('narrow', 1, 0)),
]
REDUCE_CASES = [(n, h, w, c, s, k, dt) for n, h, w, c, s, k, dts in SPLIT_CASES for dt in dts] + \
               [(n, 15, 20, c, 5, 60, dt) for dt, c, _ in WIDTH_CASES for n in (1, 3)]


def _reduce_id(case):
    n, h, w, c, s, _, dt = case
    return f"n{n}-{h}x{w}-c{c}-s{s}-{NAME[dt]}"


def test_reduction_case_lists_reach_their_branches():
    """the restated rules give the (splits, chunk) and the kernel route written beside each case, and
    the library sizes its workspace by the same partition"""
    L = _lib()
    for n, h, w, c, splits, chunk, _ in SPLIT_CASES:
        assert R.channel_splits(h * w, n) == (splits, chunk), (n, h, w)
        assert L.emsa_channel_ws_floats(n, h * w, c) == n * splits * c, (n, h, w)
    for dt, c, route in WIDTH_CASES:
        assert R.reduction_route(dt, c) == route, (dt, c)
    # both rules, both caps, trailing empty splits, a chunk that does not divide the map
    assert sum(sp * 65 >= 113 * 145 for sp in range(256)) == 3
    assert R.channel_splits(300, 1, invariant=True) == (1, 300)
    assert R.channel_splits(1200, 3, invariant=True) == (3, 400)
    assert R.channel_splits(1200, 33) == (3, 400) and R.channel_splits(1200, 1) == (19, 64)
    guard.check()


@pytest.mark.parametrize('kind', ['int', 'gauss'])
@pytest.mark.parametrize('case', REDUCE_CASES, ids=_reduce_id)
def test_channel_reductions(case, kind):
    Fn = _fn()
    n, h, w, c, splits, chunk, dtype = case
    hw = h * w
    assert R.channel_splits(hw, n) == (splits, chunk)
    assert _lib().emsa_channel_ws_floats(n, hw, c) == n * splits * c
    if kind == 'int':
        x = R.int_map(n, c, h, w, 1, chunk)
        d = R.int_map(n, c, h, w, 2, max(chunk // 2, 1))
        assert int((x * d).abs().sum((2, 3)).max()) < 2 ** 24      # every partial sum is exact in fp32
        gap = Fn.channel_mean(act(x, dtype))
        ds = Fn.se_scale_bwd_reduce(act(d, dtype), act(x, dtype))
        same(ds, (d * x).sum((2, 3)), 'se_scale_bwd_reduce == int64 sum')
        assert torch.equal(gap.cpu(), R.mean_bits(x.sum((2, 3)), hw)), \
            'channel_mean != float32(sum) * float32(1 / hw)'
    else:
        x = gauss(n, c, h, w, seed=3, dtype=dtype)
        d = gauss(n, c, h, w, seed=4, dtype=dtype)
        gap = Fn.channel_mean(act(x, dtype))
        ds = Fn.se_scale_bwd_reduce(act(d, dtype), act(x, dtype))
        tight(gap, x.mean((2, 3)), TOL_F32[dtype], 'channel_mean')
        tight(ds, (d * x).sum((2, 3)), TOL_F32[dtype], 'se_scale_bwd_reduce')
    guard.check()


def _mlp_weights(c, cr, seed):
    """(w1 [cr][c], b1, w2 [c][cr], b2), weights at scale 0.2"""
    return [rnd(cr, c, seed=seed, scale=0.2), rnd(cr, seed=seed + 1, scale=0.5),
            rnd(c, cr, seed=seed + 2, scale=0.2), rnd(c, seed=seed + 3, scale=0.5)]


# (dtype, n, h, w, c, cr, splits, route of the reduction)
PAIR_CASES = [
    (F32, 1, 15, 20, 64, 4, 5, 'narrow'),
    (BF16, 3, 15, 20, 72, 9, 5, 'narrow'),
    (F32, 1, 113, 145, 8, 2, 256, 'narrow'),      # 256 splits, three of them empty
    (F16, 1, 113, 145, 8, 2, 256, 'narrow'),
    (F32, 1, 15, 20, 2048, 128, 5, 'wide'),       # wide kernel, five splits
    (F32, 3, 15, 20, 1028, 64, 5, 'wide'),        # wide kernel, ragged second channel group
]


@pytest.mark.parametrize('case', PAIR_CASES, ids=lambda k: f"{NAME[k[0]]}-n{k[1]}-{k[2]}x{k[3]}-c{k[4]}")
def test_se_pair_launch_is_bit_identical(case):
    """se_pair_fwd == channel_mean + se_mlp_fwd per input, bit for bit, and right against fp64"""
    Fn = _fn()
    dtype, n, h, w, c, cr, splits, route = case
    assert R.channel_splits(h * w, n)[0] == splits and R.reduction_route(dtype, c)[0] == route
    xa = gauss(n, c, h, w, seed=5, dtype=dtype)
    xb = gauss(n, c, h, w, seed=6, dtype=dtype, mean=-0.5)
    wa = [t * (1.0 if i else 4.0 / c ** 0.5) for i, t in enumerate(_mlp_weights(c, cr, 11))]
    wb = [t * (1.0 if i else 4.0 / c ** 0.5) for i, t in enumerate(_mlp_weights(c, cr, 21))]
    da, db = [dev(t) for t in wa], [dev(t) for t in wb]
    ga, gb, ha, hb, sa, sb = Fn.se_pair_fwd(act(xa, dtype), act(xb, dtype), da, db)
    for xin, wts, dw, g_, h_, s_ in ((xa, wa, da, ga, ha, sa), (xb, wb, db, gb, hb, sb)):
        g1 = Fn.channel_mean(act(xin, dtype))
        h1, s1 = Fn.se_mlp_fwd(g1, *dw)
        assert torch.equal(g_, g1) and torch.equal(h_, h1) and torch.equal(s_, s1)
        gap = xin.mean((2, 3))
        hid, s = R.se_mlp_reference(gap, *wts, torch.zeros(n, c))[:2]
        tight(g_, gap, TOL_F32[dtype], 'pair gap')
        tight(h_, hid, TOL_F32[dtype], 'pair hidden')
        tight(s_, s, TOL_F32[dtype], 'pair scale')
    guard.check()


@pytest.mark.parametrize('dtype', [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('n', [3, 33])
@pytest.mark.parametrize('h,w', [(15, 20), (30, 40)])
def test_batch_invariant_reductions(h, w, n, dtype):
    """emsa_set_batch_invariant(1): sample i of a batch has the bits of the same sample run alone.
    At 30 x 40 a batch of 33 is partitioned differently from a single sample without the switch
    (3 splits against 19), a batch of 3 is not (19 both): with the switch off only the tolerance holds"""
    Fn, L = _fn(), _lib()
    c, hw = 8, h * w
    x = gauss(n, c, h, w, seed=7, dtype=dtype)
    d = gauss(n, c, h, w, seed=8, dtype=dtype)
    wts = [dev(t) for t in _mlp_weights(c, 2, 31)]
    picks = sorted({0, 1, n - 1})

    def run(xs, ds_):
        a, b = act(xs, dtype), act(ds_, dtype)
        return (Fn.channel_mean(a), Fn.se_scale_bwd_reduce(b, a), Fn.se_pair_fwd(a, b, wts, wts)[1])

    prev = L.emsa_set_batch_invariant(1)
    try:
        inv = R.channel_splits(hw, n, invariant=True)[0]
        assert inv == R.channel_splits(hw, 1, invariant=True)[0] == (hw + 511) // 512
        assert L.emsa_channel_ws_floats(n, hw, c) == n * inv * c
        assert L.emsa_channel_ws_floats(1, hw, c) == inv * c
        whole = run(x, d)
        for i in picks:
            for got, alone, what in zip(whole, run(x[i:i + 1], d[i:i + 1]), ('mean', 'dot', 'pair mean')):
                assert torch.equal(got[i:i + 1], alone), f"{what}: sample {i} of {n} differs from the sample alone"
        tight(whole[0], x.mean((2, 3)), TOL_F32[dtype], 'channel_mean (batch invariant)')
        tight(whole[1], (d * x).sum((2, 3)), TOL_F32[dtype], 'se_scale_bwd_reduce (batch invariant)')
    finally:
        L.emsa_set_batch_invariant(prev)
    assert L.emsa_channel_ws_floats(n, hw, c) == n * R.channel_splits(hw, n)[0] * c
    whole = run(x, d)
    tight(whole[0], x.mean((2, 3)), TOL_F32[dtype], 'channel_mean')
    tight(whole[1], (d * x).sum((2, 3)), TOL_F32[dtype], 'se_scale_bwd_reduce')
    for i in picks:
        alone = run(x[i:i + 1], d[i:i + 1])
        tight(whole[0][i:i + 1], alone[0].cpu(), TOL_F32[dtype], 'mean: batch against single')
        tight(whole[1][i:i + 1], alone[1].cpu(), TOL_F32[dtype], 'dot: batch against single')
    guard.check()


# =================================================================================================
# 2. excitation MLP
# =================================================================================================
# (n, c, cr, backward form): 'abc' = se_mlp_bwd_a_kernel + two se_mlp_bwd_w_kernel launches
# (n <= c and cr <= 32), 'one' = the fallback se_mlp_bwd_kernel
MLP_CASES = [(n, c, cr, 'abc' if cr <= 32 else 'one')
             for c, cr in ((64, 4), (128, 8), (256, 16), (512, 32), (1024, 64), (2048, 128))   # model widths:
             for n in (1, 32)] + [                # 64 / 32 / 16 / 8 / 4 / 2 lanes per hidden unit
    (3, 40, 5, 'abc'),                            # cr does not divide 256: 51 groups, one idle thread
    (3, 72, 9, 'abc'),                            # 28 groups, four idle threads; 16 lanes per unit
    (3, 528, 33, 'one'),                          # just past cr <= 32
    (32, 528, 33, 'one'),
    (8, 8, 2, 'abc'),                             # n == c: dz1 [n][cr] fills the dw2 buffer exactly
    (16, 8, 2, 'one'),                            # n > c: dz1 would not fit the dw2 buffer
]


@pytest.mark.parametrize('case', MLP_CASES, ids=lambda k: f"n{k[0]}-c{k[1]}-cr{k[2]}-{k[3]}")
def test_se_mlp(case):
    Fn = _fn()
    n, c, cr, form = case
    assert form == ('abc' if n <= c and cr <= 32 else 'one')
    # weights at scale 0.2; the squeeze vector at 1 / (0.2 sqrt(c)), so that the pre-activations are O(1)
    gap = rnd(n, c, seed=1, scale=5.0 / c ** 0.5) + 0.1 / c ** 0.5
    w1, b1, w2, b2 = _mlp_weights(c, cr, 40)
    dead = list(range(0, cr, 3))[:max(1, cr // 4)] if cr > 1 else []
    b1[dead] = -100.0                             # hidden units that are exactly 0 (ReLU' = 0)
    b2[0], b2[1], b2[c - 1] = 30.0, -30.0, 30.0   # saturated sigmoid: s (1 - s) underflows towards 0
    ds = rnd(n, c, seed=2, scale=4.0)
    hid, s, dgap, dw1, db1, dw2, db2 = R.se_mlp_reference(gap, w1, b1, w2, b2, ds)
    assert dead and bool((hid[:, dead] == 0).all()) and bool((hid > 0).any())
    assert bool((dw1[dead] == 0).all()) and bool((db1[dead] == 0).all())     # the reference's ReLU' at 0
    assert float(s[:, 0].min()) > 1 - 1e-9 and float(s[:, 1].max()) < 1e-9

    g, dw = dev(gap), [dev(t) for t in (w1, b1, w2, b2)]
    hid_g, s_g = Fn.se_mlp_fwd(g, *dw)
    tight(hid_g, hid, 1e-4, 'hidden')
    tight(s_g, s, 1e-4, 'scale')
    same(hid_g[:, dead], hid[:, dead], 'dead hidden units')
    # the backward reads the stored forward results; the reference's, rounded to fp32, so that every
    # ReLU decision is the reference's own
    out = Fn.se_mlp_bwd(g, dw[0], dw[2], dev(hid), dev(s), dev(ds))
    tight(out[0], dgap, 1e-4, 'dgap')
    for got, ref, what in zip(out[1:], (dw1, db1, dw2, db2), ('dw1', 'db1', 'dw2', 'db2')):
        tight(got, ref, 2e-4, what)
    same(out[1][dead], dw1[dead], 'dw1 of dead units')
    same(out[2][dead], db1[dead], 'db1 of dead units')
    # ... and the kernel's own (what the model feeds it)
    out = Fn.se_mlp_bwd(g, dw[0], dw[2], hid_g, s_g, dev(ds))
    tight(out[0], dgap, 1e-4, 'dgap (own forward)')
    for got, ref, what in zip(out[1:], (dw1, db1, dw2, db2), ('dw1', 'db1', 'dw2', 'db2')):
        tight(got, ref, 2e-4, what + ' (own forward)')
    guard.check()


@pytest.mark.parametrize('dtype', [F32, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize('c', [8, 2048])
@pytest.mark.parametrize('extra', [False, True])
def test_se_scale_bwd_apply(extra, c, dtype):
    Fn = _fn()
    n, h, w = 2, 15, 20
    dout = gauss(n, c, h, w, seed=1, dtype=dtype, mean=0.5)
    s = torch.rand(n, c, generator=torch.Generator().manual_seed(2)) + 0.1
    dgap = rnd(n, c, seed=3, scale=100.0)         # / hw: comparable with dout * s
    e = gauss(n, c, h, w, seed=4, dtype=dtype, mean=-0.25) if extra else None
    ref = dout * s.double()[:, :, None, None] + dgap.double()[:, :, None, None] / (h * w)
    if extra:
        ref = ref + e
    dx = Fn.se_scale_bwd_apply(act(dout, dtype), dev(s), dev(dgap), act(e, dtype) if extra else None)
    assert dx.dtype == dtype
    tight(dx, ref, TOL_STORE[dtype], 'se_scale_bwd_apply')
    guard.check()


# =================================================================================================
# 3. adaptive average pool
# =================================================================================================
# (dtype, c, n, h, w, bins, route): 'wg256' / 'wg1024' = adaptive_avgpool_fwd_wg_kernel with that many
# threads, 'general' = adaptive_avgpool_fwd_kernel (one thread per output element)
POOL_CASES = []
for _bins in (1, 5):
    POOL_CASES += [
        (F32, 4, 2, 15, 20, _bins, 'wg256'),      # one channel vector, 256 pixel lanes
        (F32, 40, 2, 15, 20, _bins, 'wg256'),     # 25 lanes, 6 idle threads
        (F32, 252, 2, 15, 20, _bins, 'wg256'),    # 63 vectors: the last width with 256 threads
        (F32, 256, 2, 15, 20, _bins, 'wg1024'),   # 64 vectors: the first with 1024
        (F32, 512, 2, 15, 20, _bins, 'wg1024'),   # the context module's input
        (F32, 1000, 2, 15, 20, _bins, 'wg1024'),  # 250 vectors x 4 lanes: 24 idle threads
        (F32, 2048, 1, 15, 20, _bins, 'wg1024'),
        (F32, 4096, 1, 15, 20, _bins, 'wg1024'),  # 1024 vectors: one lane
        (F32, 4100, 1, 15, 20, _bins, 'general'),  # 1025 vectors
        (F32, 6, 2, 15, 20, _bins, 'general'),    # not a whole number of vectors
        (BF16, 4, 2, 15, 20, _bins, 'general'),   # half a vector
    ]
    for _dt in (BF16, F16):
        POOL_CASES += [(_dt, 8, 2, 15, 20, _bins, 'wg256'), (_dt, 512, 2, 15, 20, _bins, 'wg1024'),
                       (_dt, 2048, 1, 15, 20, _bins, 'wg1024')]
for _dt in (F32, BF16):
    POOL_CASES += [(_dt, 8, 2, 10, 10, 5, 'wg256'),        # h w = 4 bins^2: the workgroup kernel
                   (_dt, 8, 2, 9, 11, 5, 'general')]       # h w = 4 bins^2 - 1: the general one
for _dt in DTYPES:
    for _c in (8, 64):
        _wg = 'wg1024' if _c // R.VEC[_dt] >= 64 else 'wg256'
        POOL_CASES += [
            (_dt, _c, 2, 15, 20, 5, _wg),         # exact 3 x 4 bins
            (_dt, _c, 2, 16, 32, 5, _wg),         # overlapping bins: rows 4, 5, 4, 5, 4 of 16
            (_dt, _c, 2, 17, 23, 5, _wg),         # overlapping in both directions
            (_dt, _c, 2, 7, 9, 4, 'general'),     # 63 < 4 * 16
            (_dt, _c, 2, 3, 4, 5, 'general'),     # more bins than pixels: every window is one pixel
            (_dt, _c, 2, 1, 1, 1, 'general'),
            (_dt, _c, 2, 1, 1, 5, 'general'),
        ]
POOL_CASES = list(dict.fromkeys(POOL_CASES))


@pytest.mark.parametrize('case', POOL_CASES,
                         ids=lambda k: f"{NAME[k[0]]}-c{k[1]}-n{k[2]}-{k[3]}x{k[4]}-b{k[5]}-{k[6]}")
def test_adaptive_avgpool(case):
    Fn = _fn()
    dtype, c, n, h, w, bins, route = case
    assert R.pool_route(dtype, c, h, w, bins) == route
    # forward, integer-valued: the bin sum is exact; what is left is one fp32 division (correctly
    # rounded: hipcc's default) and one rounding to the storage type
    xi = R.int_map(n, c, h, w, 1, 7)
    sums, count = R.pool_sums(xi, bins)
    ref = F.adaptive_avg_pool2d(xi.double(), bins)
    assert (sums.double() / count.double() - ref).abs().max().item() < 1e-12      # torch's bins are these
    y = Fn.adaptive_avgpool_fwd(act(xi, dtype), bins)
    assert y.dtype == dtype and tuple(y.shape) == (n, c, bins, bins)
    same(y, R.pool_mean_bits(sums, count, dtype), 'pool of integers == float32(sum) / float32(pixels)')
    # forward, Gaussian
    x = gauss(n, c, h, w, seed=2, dtype=dtype)
    tight(Fn.adaptive_avgpool_fwd(act(x, dtype), bins), F.adaptive_avg_pool2d(x, bins),
          TOL_STORE[dtype], 'pool')
    # backward: accumulate = 0 writes every element of a poisoned dx, accumulate = 1 adds to known values
    # (the cotangent is scaled by the pixels per bin, so that both terms of the accumulating form are
    #  far above the tolerance: asserted below)
    per_bin = max(1, (h * w) // (bins * bins))
    dy = gauss(n, c, bins, bins, seed=3, dtype=dtype, mean=2.0 * per_bin, scale=4.0 * per_bin)
    a = R.pool_bwd_reference(dy, h, w)
    dx = Fn.adaptive_avgpool_bwd(act(dy, dtype), Fn.act_empty(n, c, h, w, DEV, dtype=dtype), bins, False)
    tight(dx, a, TOL_STORE[dtype], 'pool bwd')
    dx0 = gauss(n, c, h, w, seed=4, dtype=dtype, mean=-4.0, scale=2.0)
    ref = (dx0 + a).to(dtype).double()            # 16-bit: round_T(dx0 + a), one rounding of the sum
    lim = 10 * TOL_STORE[dtype] * ref.abs().max().item()
    assert a.abs().max().item() > lim and dx0.abs().max().item() > lim
    dx = Fn.adaptive_avgpool_bwd(act(dy, dtype), act(dx0, dtype), bins, True)
    tight(dx, ref, TOL_STORE[dtype], 'pool bwd, accumulate')
    guard.check()


# =================================================================================================
# 4. max pool 3x3 / 2
# =================================================================================================
MAPS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 6), (6, 5), (9, 11), (12, 20)]
POOL_TYPES = [(4, F32)] + [(c, dt) for c in (8, 64) for dt in DTYPES]


def _maxpool_inputs(n, c, h, w):
    rng = np.random.default_rng(5)
    return {
        'relu': torch.relu(rnd(n, c, h, w, seed=0) - 0.8),       # the stem's case: windows of exact zeros
        'levels': torch.from_numpy(rng.integers(0, 3, (n, c, h, w))).float(),
        'constant': torch.full((n, c, h, w), 1.5),
        '-inf': torch.full((n, c, h, w), float('-inf')),
        'gauss': rnd(n, c, h, w, seed=6),                        # control: no ties
    }


@pytest.mark.parametrize('c,dtype', POOL_TYPES, ids=lambda v: NAME.get(v, f"c{v}"))
@pytest.mark.parametrize('h,w', MAPS)
def test_maxpool_ties(h, w, c, dtype):
    """y, the stored tap and dx equal F.max_pool2d's on the CPU exactly: a tied maximum belongs to the
    first tap in row-major window order, an all -inf window to its first in-range tap"""
    Fn = _fn()
    n = 2
    dyi = R.int_map(n, c, (h + 1) // 2, (w + 1) // 2, 9, 3)      # integers: dx sums <= 4 exact terms
    for name, x32 in _maxpool_inputs(n, c, h, w).items():
        x = x32.to(dtype).double()
        y, ind, tap = R.maxpool_reference(x)
        if name == 'relu':                                       # a condition on the input, not the kernel
            assert (y == 0).double().mean().item() >= 0.10, 'too few windows with an exact-zero maximum'
        if name in ('constant', '-inf'):
            # first in-range tap: 4 in the interior, beside the top / left border the first valid one
            assert int(tap[0, 0, 0, 0]) == 4 and bool((tap[:, :, 1:, 1:] == 0).all())
        yg, idx = Fn.maxpool_fwd(act(x, dtype))
        assert yg.dtype == dtype and idx.dtype == torch.int8
        same(yg, y, f'maxpool {name}')
        same(idx, tap.permute(0, 2, 3, 1), f'maxpool tap {name}')
        dx = Fn.maxpool_bwd(act(dyi, dtype), idx, (h, w))
        same(dx, R.maxpool_bwd_reference(dyi, ind, h, w), f'maxpool dx {name}')
    guard.check()


def test_maxpool_16bit_vector_widths():
    """C = 12 in bf16: the forward reads 4 channels per thread and accepts it, the backward reads 16-byte
    vectors (8 channels) and refuses it before any launch"""
    Fn = _fn()
    from emsanet_amd._lib import EmsaError
    n, c, h, w = 2, 12, 5, 6
    x = _maxpool_inputs(n, c, h, w)['relu'].to(BF16).double()
    y, ind, tap = R.maxpool_reference(x)
    yg, idx = Fn.maxpool_fwd(act(x, BF16))
    same(yg, y, 'maxpool bf16 C=12')
    same(idx, tap.permute(0, 2, 3, 1), 'maxpool tap bf16 C=12')
    with pytest.raises(EmsaError):
        Fn.maxpool_bwd(act(R.int_map(n, c, 3, 3, 9, 3), BF16), idx, (h, w))
    guard.check()
