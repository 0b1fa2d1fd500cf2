"""GPU: the pieces that let the NBt1D block's masked skip gradient dres = dout * (out > 0) stay out
of memory, each against today's kernels, bit for bit:

* bn_act writing its ReLU bit mask in the Winograd epilogue's layout (one word per pixel and
  64-channel tile, bit comp * 16 + col4) against decisions recomputed from its own output;
* bn_bwd reading that layout against bn_bwd reading today's;
* the 3x1 data gradient that masks its residual by those bits (emsa_conv1d_wino_resmask) against the
  same data gradient with the residual dres written by today's bn_bwd.

Channel counts 64 / 128 run the fast forms of the BatchNorm passes, 192 (48 channel vectors: not a
power of two) the general forward / apply loops beside the fast reduction, 1088 (272 vectors: more than
a workgroup has threads) the general loops and the wide reduction."""
import functools

import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu
EPS = 1e-3


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def _bn_case(n, c, h, w, with_drop):
    """inputs of a block's bn2 (BatchNorm -> * drop -> + residual -> ReLU) and of its backward"""
    seed = 1000 * c + 10 * h + w
    y = rnd(n, c, h, w, seed=seed)
    idn = rnd(n, c, h, w, seed=seed + 1)
    gamma = rnd(c, seed=seed + 2)
    gamma[3] = 0.0
    beta = rnd(c, seed=seed + 3, scale=0.3)
    y64 = y.double()
    mean = y64.mean((0, 2, 3))
    invstd = (1.0 / torch.sqrt(y64.var((0, 2, 3), unbiased=False) + EPS)).float()
    scale = gamma * invstd
    shift = beta - mean.float() * scale
    idn[0, 7] = -10.0                                  # no bit set in image 0, channel 7
    drop = None
    keep = torch.tensor(1.0 / 0.7, dtype=torch.float32)
    if with_drop:
        drop = (torch.rand(n, c, generator=torch.Generator().manual_seed(seed)) > 0.3).float() * keep
        drop[:, 3] = keep
    # channel 3 (gamma = 0): the ReLU argument shift * drop + idn is exactly zero
    idn[:, 3] = -(shift[3] * keep) if with_drop else -shift[3]
    if with_drop:
        drop = drop.to(DEV)
    dout = rnd(n, c, h, w, seed=seed + 4)
    dev = lambda t: t.to(DEV)                          # noqa: E731
    return dict(y=to_act(y), idn=to_act(idn), gamma=dev(gamma), mean=dev(mean.float()), invstd=dev(invstd),
                scale=dev(scale), shift=dev(shift), drop=drop, dout=to_act(dout))


def _decode(bits, n, c, h, w):
    """the Winograd-layout words -> bool (n, c, h, w)"""
    tiles = c // 64
    words = bits[:n * h * w * tiles].cpu().view(n * h * w, tiles)
    out = torch.zeros(n * h * w, c, dtype=torch.bool)
    for nt in range(tiles):
        for comp in range(4):
            for col4 in range(16):
                out[:, nt * 64 + col4 * 4 + comp] = ((words[:, nt] >> (comp * 16 + col4)) & 1).bool()
    return out.view(n, h, w, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize('with_drop', [True, False])
@pytest.mark.parametrize('c', [64, 128, 192, 1088])
def test_bn_act_winograd_mask_layout(c, with_drop):
    Fn = _fn()
    n, h, w = 2, 5, 7                                  # 70 pixels: the last wave is partly idle
    d = _bn_case(n, c, h, w, with_drop)
    ref, _ = Fn.bn_act(d['y'], d['scale'], d['shift'], d['drop'], d['idn'], Fn.ACT_RELU, want_mask=True)
    out, bits = Fn.bn_act(d['y'], d['scale'], d['shift'], d['drop'], d['idn'], Fn.ACT_RELU,
                          want_mask=True, wino_bits=True)
    torch.cuda.synchronize()
    assert bits._emsa_wbits and torch.equal(out, ref) and torch.isfinite(out).all()
    dec = _decode(bits, n, c, h, w)
    assert torch.equal(dec, (out > 0).cpu())
    # the inputs do what _bn_case says
    assert float(out[:, 3].abs().max()) == 0.0 and not dec[:, 3].any() and not dec[0, 7].any()
    assert 0.2 < float(dec.float().mean()) < 0.8


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('with_drop', [True, False])
@pytest.mark.parametrize('c', [64, 128, 192, 1088])
def test_bn_bwd_winograd_mask_layout(c, with_drop, train):
    Fn = _fn()
    n, h, w = 2, 5, 7
    d = _bn_case(n, c, h, w, with_drop)
    args = (d['y'], d['scale'], d['shift'], d['drop'], d['idn'], Fn.ACT_RELU)
    _, bits_old = Fn.bn_act(*args, want_mask=True)
    _, bits_new = Fn.bn_act(*args, want_mask=True, wino_bits=True)
    run = lambda bits, want: Fn.bn_bwd(d['dout'], bits, d['y'], d['gamma'], d['mean'], d['invstd'],   # noqa: E731
                                       d['drop'], Fn.ACT_RELU, train, want_dres=want)
    ref = run(bits_old, True)
    got = run(bits_new, True)
    lean = run(bits_new, False)
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    assert lean[1] is None
    for a, b in zip((ref[0], ref[2], ref[3]), (lean[0], lean[2], lean[3])):
        assert torch.equal(a, b)
    assert float(ref[1].abs().max()) > 0


def _wide(t, extra):
    """the same activation as a slice of a buffer with `extra` more floats per pixel"""
    Fn = _fn()
    n, c, h, w = t.shape
    buf = Fn.act_empty(n, c, h, w, t.device, ld=c + extra)
    buf.copy_(t)
    return buf


@pytest.mark.parametrize('ld_extra', [0, 8])
@pytest.mark.parametrize('hw', [(7, 10), (9, 15)])
@pytest.mark.parametrize('c', [64, 128])
def test_dgrad_masked_residual_equals_stored_dres(c, hw, ld_extra):
    """conv3x1 data gradient + residual: the residual masked by bits in the epilogue == the residual
    masked and stored by bn_bwd.  Odd line lengths (7, 9): the last Winograd pair of a line has a
    virtual second pixel; 140 / 270 pixels: a ragged last 64-pixel tile; c = 128: two channel tiles
    (the word index per tile); ld_extra: a residual with a pixel stride larger than c"""
    Fn = _fn()
    n, (h, w) = 2, hw
    d = _bn_case(n, c, h, w, True)
    args = (d['y'], d['scale'], d['shift'], d['drop'], d['idn'], Fn.ACT_RELU)
    out, bits_old = Fn.bn_act(*args, want_mask=True)
    _, bits_new = Fn.bn_act(*args, want_mask=True, wino_bits=True)
    dres = Fn.bn_bwd(d['dout'], bits_old, d['y'], d['gamma'], d['mean'], d['invstd'], d['drop'],
                     Fn.ACT_RELU, True, want_dres=True)[1]
    assert torch.equal(dres, d['dout'] * (out > 0))
    spec = Fn.ConvSpec(c, c, (3, 1), (1, 1), (1, 0))
    wt = rnd(c, c, 3, 1, seed=c + h, scale=(1.0 / (3 * c)) ** 0.5).to(DEV)
    ud = Fn.pack_wino(wt, fwd=False, dgrad=True)[1]
    dz = to_act(rnd(n, c, h, w, seed=c + h + 1))
    dout = d['dout']
    if ld_extra:
        dres, dout = _wide(dres, ld_extra), _wide(dout, ld_extra)
        assert Fn.ld_of(dout) == c + ld_extra
    assert Fn.dgrad_takes_res_bits(spec, dz, (h, w), dout)
    ref = Fn.conv_dgrad(dz, None, spec, (h, w), residual=dres, wino_u=ud)
    got = Fn.conv_dgrad(dz, None, spec, (h, w), residual=dout, res_bits=bits_new, wino_u=ud)
    plain = Fn.conv_dgrad(dz, None, spec, (h, w), wino_u=ud)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, ref)
    assert not torch.equal(got, plain)


def test_host_side_refusals():
    """what the launchers do not take is refused on the host, before any launch"""
    from emsanet_amd import _lib
    Fn = _fn()
    L = _lib.lib()
    one = torch.zeros(16, device=DEV).data_ptr()
    # the Winograd layout: whole 64-channel tiles, a mask and ReLU
    assert L.emsa_bn_act_fwd_wbits(one, one, one, one, None, None, 2, 4, 32, Fn.ACT_RELU, one, None) == _lib.E_SHAPE
    assert L.emsa_bn_act_fwd_wbits(one, one, one, one, None, None, 2, 4, 64, Fn.ACT_RELU, None, None) == -2
    assert L.emsa_bn_act_fwd_wbits(one, one, one, one, None, None, 2, 4, 64, Fn.ACT_NONE, one, None) == -2
    assert L.emsa_bn_bwd_reduce_wbits(one, one, one, one, one, None, 2, 4, 96, one, None) == _lib.E_SHAPE
    assert L.emsa_bn_bwd_reduce_wbits(one, None, one, one, one, None, 2, 4, 64, one, None) == -2
    assert L.emsa_bn_bwd_apply_wbits(*([one] * 6), None, one, 17, 2, 4, 96, 1, one, None, one, one,
                                     None) == _lib.E_SHAPE
    # the masked-residual data gradient: 1-D stride-1 convs with whole 64-channel output tiles
    dz = to_act(torch.zeros(2, 32, 4, 6))
    res = to_act(torch.zeros(2, 32, 4, 6))
    assert not Fn.dgrad_takes_res_bits(Fn.ConvSpec(32, 32, (3, 1), (1, 1), (1, 0)), dz, (4, 6), res)
    dz = to_act(torch.zeros(2, 64, 4, 6))
    res = to_act(torch.zeros(2, 64, 4, 6))
    assert Fn.dgrad_takes_res_bits(Fn.ConvSpec(64, 64, (3, 1), (1, 1), (1, 0)), dz, (4, 6), res)
    assert not Fn.dgrad_takes_res_bits(Fn.ConvSpec(64, 64, (3, 3), (1, 1), (1, 1)), dz, (4, 6), res)
    assert not Fn.dgrad_takes_res_bits(Fn.ConvSpec(64, 64, (3, 1), (2, 1), (1, 0)), dz, (8, 6), res)
    spec = Fn.ConvSpec(64, 64, (3, 1), (1, 1), (1, 0))
    g = spec.geom_dgrad(2, 4, 6, 64, 64)
    assert L.emsa_conv1d_wino_resmask(g, one, one, one, None, 64, one, None) == -2
    assert L.emsa_conv1d_wino_resmask(g, one, one, one, one, 64, None, None) == -2
    assert L.emsa_conv1d_wino_resmask(g, one, one, one, one, 32, one, None) == _lib.E_SHAPE
