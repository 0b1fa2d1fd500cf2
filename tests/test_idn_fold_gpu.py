"""GPU: the down-sampling shortcut's BatchNorm formed inside bn2's normalise pass
(emsa_bn_act_fwd_raff, Fn.IDN_FOLD) against the two passes it replaces, bit for bit: the kernel at the
channel counts that take the fast form (64, 128) and the general loop (192, 1088), with and without
Dropout2d, with the ReLU bit mask in either layout; and a down-sampling NBt1D block forward and
backward with the fold on and off."""
import copy

import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


@pytest.mark.parametrize('wino_bits', [True, False])
@pytest.mark.parametrize('with_drop', [True, False])
@pytest.mark.parametrize('c', [64, 128, 192, 1088])
def test_bn_act_affine_residual(c, with_drop, wino_bits):
    Fn = _fn()
    n, h, w = 2, 5, 7                                  # 70 pixels: the last wave is partly idle
    seed = 100 * c
    y, yd = to_act(rnd(n, c, h, w, seed=seed)), to_act(rnd(n, c, h, w, seed=seed + 1))
    scale, shift = rnd(c, seed=seed + 2).to(DEV), rnd(c, seed=seed + 3, scale=0.3).to(DEV)
    sd, td = rnd(c, seed=seed + 4), rnd(c, seed=seed + 5, scale=0.3)
    sd[3], td[3] = 0.0, 0.0                            # a shortcut channel that is exactly zero
    sd, td = sd.to(DEV), td.to(DEV)
    drop = None
    if with_drop:
        drop = ((torch.rand(n, c, generator=torch.Generator().manual_seed(seed)) > 0.3).float() / 0.7).to(DEV)
    idn = Fn.bn_act(yd, sd, td, None, None, Fn.ACT_NONE)
    ref, rbits = Fn.bn_act(y, scale, shift, drop, idn, Fn.ACT_RELU, want_mask=True, wino_bits=wino_bits)
    got, gbits = Fn.bn_act(y, scale, shift, drop, yd, Fn.ACT_RELU, want_mask=True, wino_bits=wino_bits,
                           res_affine=(sd, td))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, ref)
    assert torch.equal(gbits, rbits)                   # (words no pass writes hold the arena's poison)
    assert getattr(gbits, '_emsa_wbits', False) == wino_bits
    assert float(idn[:, 3].abs().max()) == 0.0 and float(got.max()) > 0
    # the shortcut really arrived
    assert not torch.equal(ref, Fn.bn_act(y, scale, shift, drop, None, Fn.ACT_RELU))


def test_downsampling_block_folded_vs_unfolded(monkeypatch):
    """NBt1D 64 -> 128, stride 2 (n = 2, 18 x 28 -> 9 x 14): output and every gradient but the 1x1
    shortcut conv's (fp32 atomics in the parent: the rule of test_stem_stage_gpu.py, the unfolded
    block run twice) bit-equal; the shortcut activation is not allocated"""
    from emsanet_amd.nn import NonBottleneck1D
    Fn = _fn()
    torch.manual_seed(5)
    m = NonBottleneck1D(64, 128, stride=2, dropout_p=0.3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if 'bn' in k or k.startswith('downsample.1'):
                p.copy_(rnd(*p.shape, seed=len(k), scale=0.5) + (1.0 if k.endswith('weight') else 0.0))
    m = m.to(DEV).train()

    def run(fold, count=None):
        monkeypatch.setattr(Fn, 'IDN_FOLD', fold)
        e = copy.deepcopy(m)
        x = to_act(rnd(2, 64, 18, 28, seed=21)).requires_grad_()
        real = Fn._empty
        if count is not None:
            def counting(shape, device, dtype=torch.float32):
                count.append((tuple(shape) if not isinstance(shape, int) else (shape,), dtype))
                return real(shape, device, dtype)
            monkeypatch.setattr(Fn, '_empty', counting)
        out = e(x)
        if count is not None:
            monkeypatch.setattr(Fn, '_empty', real)
        out.backward(to_act(rnd(*out.shape, seed=22, scale=0.1)))
        torch.cuda.synchronize()
        res = {'out': out.detach(), 'dx': x.grad}
        res.update({k: p.grad for k, p in e.named_parameters()})
        return res
    a_new, a_old = [], []
    new, old, old2 = run(True, a_new), run(False, a_old), run(False)
    big = lambda rec: sum(1 for s, d in rec if s == (2, 9, 14, 128) and d == torch.float32)   # noqa: E731
    assert big(a_new) == big(a_old) - 1 and len(a_new) == len(a_old) - 1
    for k in old:
        assert new[k] is not None and torch.isfinite(new[k]).all(), k
        if k == 'downsample.0.weight':
            d_new = float((new[k] - old[k]).abs().max())
            d_old = float((old2[k] - old[k]).abs().max())
            lim = max(2 * d_old, 1e-6 * float(old[k].abs().max()))
            print(f"{k}: folded-vs-unfolded {d_new:.3e}, unfolded twice {d_old:.3e}, bound {lim:.3e}")
            assert d_new <= lim, k
        else:
            assert torch.equal(new[k], old[k]), k
    assert float(new['downsample.1.weight'].abs().max()) > 0
