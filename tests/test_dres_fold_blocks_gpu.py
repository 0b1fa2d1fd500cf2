"""GPU: NBt1D blocks with the masked skip gradient dres = dout * (out > 0) formed where it is
consumed (Fn.DRES_FOLD) against the same blocks with dres stored: an identity block (dres is the
residual of conv3x1_1's data gradient) and a down-sampling block (dres is the gradient entering the
shortcut BatchNorm's backward).  Every kernel on either path is deterministic except the
implicit-GEMM weight gradient of the 1x1 shortcut conv (fp32 atomics): that one follows the rule of
test_stem_stage_gpu.py -- the stored path runs twice, and folded-vs-stored may be no larger than
max(2 x stored-vs-stored, 1e-6 x max |stored|); everything else must be bit-equal."""
import copy

import pytest
import torch

from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

ATOMIC = ('downsample.0.weight',)


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _block(cin, cout, stride):
    from emsanet_amd.nn import NonBottleneck1D
    torch.manual_seed(5)
    m = NonBottleneck1D(cin, cout, stride=stride, dropout_p=0.3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if 'bn' in k or k.startswith('downsample.1'):
                p.copy_(rnd(*p.shape, seed=len(k), scale=0.5) + (1.0 if k.endswith('weight') else 0.0))
    return m.to(DEV).train()


def _run(m, fold, monkeypatch, hw_in, count=None):
    Fn = _fn()
    monkeypatch.setattr(Fn, 'DRES_FOLD', fold)
    e = copy.deepcopy(m)
    cin = e.conv3x1_1.in_channels
    x = to_act(rnd(2, cin, *hw_in, seed=21)).requires_grad_()
    real = Fn._empty
    if count is not None:
        def counting(shape, device, dtype=torch.float32):
            count.append((tuple(shape) if not isinstance(shape, int) else (shape,), dtype))
            return real(shape, device, dtype)
        monkeypatch.setattr(Fn, '_empty', counting)
    out = e(x)
    fwd = len(count) if count is not None else 0
    out.backward(to_act(rnd(*out.shape, seed=22, scale=0.1)))
    if count is not None:
        monkeypatch.setattr(Fn, '_empty', real)
        del count[:fwd]                                # keep the backward pass's allocations
    torch.cuda.synchronize()
    res = {'out': out.detach(), 'dx': x.grad}
    for k, p in e.named_parameters():
        assert p.grad is not None, k
        res[k] = p.grad
    return res


@pytest.mark.parametrize('cin,cout,stride', [(64, 64, 1), (64, 128, 2)])
def test_block_folded_vs_stored(cin, cout, stride, monkeypatch):
    Fn = _fn()
    m = _block(cin, cout, stride)
    hw_in = (9, 14) if stride == 1 else (18, 28)       # the block's own maps are 9 x 14
    before = Fn.DRES_FALLBACKS
    a_new, a_old = [], []
    new = _run(m, True, monkeypatch, hw_in, a_new)
    old = _run(m, False, monkeypatch, hw_in, a_old)
    old2 = _run(m, False, monkeypatch, hw_in)
    assert Fn.DRES_FALLBACKS == before
    # dres (2, cout, 9, 14) is not allocated on the folded path: one map of that size less in the
    # backward pass, nothing else changes
    big = lambda rec: sum(1 for s, d in rec if s == (2, 9, 14, cout) and d == torch.float32)   # noqa: E731
    assert big(a_new) == big(a_old) - 1 and len(a_new) == len(a_old) - 1
    bad = []
    for k in old:
        assert torch.isfinite(new[k]).all(), k
        d_new = float((new[k] - old[k]).abs().max())
        if k in ATOMIC:
            d_old = float((old2[k] - old[k]).abs().max())
            lim = max(2 * d_old, 1e-6 * float(old[k].abs().max()))
            print(f"{k}: folded-vs-stored {d_new:.3e}, stored twice {d_old:.3e}, bound {lim:.3e}")
            if d_new > lim:
                bad.append(f"{k}: {d_new:.3e} > {lim:.3e}")
        elif not torch.equal(new[k], old[k]):
            bad.append(f"{k}: not bit-equal (max diff {d_new:.3e})")
    assert not bad, '\n'.join(bad)
    assert float(new['dx'].abs().max()) > 0


def test_refused_shape_falls_back_and_counts(monkeypatch):
    """a block whose channel count is no multiple of 64 keeps today's mask layout and the stored
    dres, and counts the fallback; so does a block whose conv3x1_1 data gradient the masked-residual
    launch refuses (decided on the host); switched off, nothing is counted"""
    Fn = _fn()
    before = Fn.DRES_FALLBACKS
    m32 = _block(32, 32, 1)
    new = _run(m32, True, monkeypatch, (9, 14))
    assert Fn.DRES_FALLBACKS == before + 1
    old = _run(m32, False, monkeypatch, (9, 14))
    assert Fn.DRES_FALLBACKS == before + 1
    for k in old:
        assert torch.equal(new[k], old[k]), k
    m64 = _block(64, 64, 1)
    monkeypatch.setattr(Fn, 'dgrad_takes_res_bits', lambda *a: False)
    new = _run(m64, True, monkeypatch, (9, 14))
    assert Fn.DRES_FALLBACKS == before + 2
    old = _run(m64, False, monkeypatch, (9, 14))
    for k in old:
        assert torch.equal(new[k], old[k]), k
