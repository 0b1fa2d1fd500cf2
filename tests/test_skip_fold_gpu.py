"""GPU: the learned x2 up-sampling with the skip path's BatchNorm + ReLU formed at its skip load
(emsa_up2x_dw3x3_fwd_skipbn) against the two launches it replaces, bn_act followed by the up-sampler
with a stored skip tensor: bit for bit.

Inputs: channel 3 has scale = shift = 0 and channel 5 maps the value 2.0 (a quarter of its pixels) to
0.5 * 2.0 - 1.0, so that ReLU arguments are exactly zero; channel 7 is negative everywhere."""
import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu


def _inputs(n, c, h, w, seed):
    x = rnd(n, c, h, w, seed=seed)
    y = rnd(n, c, 2 * h, 2 * w, seed=seed + 1)
    y[:, 5, ::2, ::2] = 2.0
    scale = rnd(c, seed=seed + 2)
    shift = rnd(c, seed=seed + 3, scale=0.5)
    scale[3], shift[3] = 0.0, 0.0
    scale[5], shift[5] = 0.5, -1.0
    scale[7], shift[7] = 0.0, -1.0
    wdw = rnd(c, 1, 3, 3, seed=seed + 4, scale=0.3)
    bias = rnd(c, seed=seed + 5, scale=0.1)
    return to_act(x), to_act(y), scale.to(DEV), shift.to(DEV), wdw.to(DEV), bias.to(DEV)


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('c', [64, 128])
def test_folded_skip_equals_bn_act_then_upsampler(c, with_bias):
    from emsanet_amd import functional as Fn
    n, h, w = 2, 5, 7
    x, y, scale, shift, wdw, bias = _inputs(n, c, h, w, seed=c)
    if not with_bias:
        bias = None
    a = Fn.bn_act(y, scale, shift, None, None, Fn.ACT_RELU)
    # the inputs do what the docstring says
    z = y * scale.view(1, c, 1, 1) + shift.view(1, c, 1, 1)
    assert int((z == 0).sum()) >= n * 2 * h * 2 * w + n * h * w and float(a[:, 7].max()) == 0.0
    ref = Fn.up2x_dw_fwd(x, wdw, bias, a)
    got = Fn.up2x_dw_fwd_skipbn(x, wdw, bias, y, scale, shift)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (n, c, 2 * h, 2 * w) and Fn.ld_of(got) == c
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref)
    # the skip term really arrived: without it the result differs
    assert not torch.equal(ref, Fn.up2x_dw_fwd(x, wdw, bias, None))


def test_bn_bwd_recomputed_mask_equals_bit_mask():
    """the backward half of the fold: bn_bwd_aff (decisions recomputed from the BatchNorm input) ==
    bn_bwd with the bit mask bn_act wrote, fp32"""
    from emsanet_amd import functional as Fn
    n, c, h, w = 2, 64, 10, 14
    _, y, _, _, _, _ = _inputs(n, c, h // 2, w // 2, seed=7)
    gamma = rnd(c, seed=70).to(DEV)
    beta = rnd(c, seed=71, scale=0.3).to(DEV)
    y64 = y.double()
    mean = y64.mean((0, 2, 3))
    invstd = (1.0 / torch.sqrt(y64.var((0, 2, 3), unbiased=False) + 1e-5)).float()
    scale = gamma * invstd
    shift = beta - mean.float() * scale
    mean = mean.float()
    dy = to_act(rnd(n, c, h, w, seed=72))
    _, bits = Fn.bn_act(y, scale, shift, None, None, Fn.ACT_RELU, want_mask=True)
    ref = Fn.bn_bwd(dy, bits, y, gamma, mean, invstd, None, Fn.ACT_RELU, True, want_dres=False)
    got = Fn.bn_bwd_aff(dy, y, gamma, mean, invstd, (scale, shift))
    torch.cuda.synchronize()
    for a, b in zip((ref[0], ref[2], ref[3]), got):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_host_side_refusals():
    """shapes the launcher does not take are refused on the host, before any launch"""
    from emsanet_amd import _lib
    L = _lib.lib()
    one = torch.zeros(16, device=DEV).data_ptr()
    assert L.emsa_up2x_dw3x3_fwd_skipbn(*([one] * 7), 2, 2, 2, 6, None) == _lib.E_SHAPE
    # scale / shift beside the weights: 11 * c floats must fit the 64 KiB of LDS
    assert L.emsa_up2x_dw3x3_fwd_skipbn(*([one] * 7), 2, 2, 2, 1536, None) == _lib.E_SHAPE
    assert L.emsa_up2x_dw3x3_fwd_skipbn(one, one, one, None, one, one, one, 2, 2, 2, 64, None) == -2
    assert L.emsa_up2x_dw3x3_fwd_skipbn(one, one, one, one, None, one, one, 2, 2, 2, 64, None) == -2
