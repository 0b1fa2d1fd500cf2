"""GPU: a decoder module and a small full model with the skip path's BatchNorm + ReLU folded into
the up-sampler (Fn.SKIP_FOLD, ops.SkipUpsampleFunction) against the same modules without the fold.

Every output and every gradient a deterministic kernel forms must be bit-equal.  The gradients the
unfolded path itself forms with fp32 atomics (the 3x3 / 1x1 weight gradients of the implicit-GEMM
kernel, the depth-wise dw / db of the up-sampler) follow the rule of test_stem_stage_gpu.py: the
unfolded path runs twice, and folded-vs-unfolded may be no larger than
max(2 x unfolded-vs-unfolded, 1e-6 x max |unfolded|)."""
import copy

import pytest
import torch

from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

# parameters of a DecoderModule whose gradients the unfolded path forms with atomics
ATOMIC = ('conv3x3.conv.weight', 'skip_fusion.conv.weight', 'upsampling.conv.weight',
          'upsampling.conv.bias')


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _module(upsampling='learned-3x3-zeropad'):
    from emsanet_amd.decoder import DecoderModule
    torch.manual_seed(3)
    m = DecoderModule(128, 64, 1, 0.0, 32, upsampling=upsampling)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith('bn2.weight'):
                p.uniform_(0.2, 0.4)                   # (the decoders' zero-residual init hides the blocks)
            elif 'norm' in k or 'bn' in k:
                p.copy_(rnd(*p.shape, seed=len(k), scale=0.5) + (1.0 if k.endswith('weight') else 0.0))
            elif 'upsampling' in k:
                p.add_(rnd(*p.shape, seed=len(k), scale=0.02))
    return m.to(DEV).train()


def _run(m, fold, monkeypatch, count=None):
    Fn = _fn()
    monkeypatch.setattr(Fn, 'SKIP_FOLD', fold)
    e = copy.deepcopy(m)
    x = to_act(rnd(2, 128, 6, 8, seed=11)).requires_grad_()
    skip = to_act(rnd(2, 32, 12, 16, seed=12)).requires_grad_()
    if count is not None:
        real = Fn._empty

        def counting(shape, device, dtype=torch.float32):
            count.append((tuple(shape) if not isinstance(shape, int) else (shape,), dtype))
            return real(shape, device, dtype)
        monkeypatch.setattr(Fn, '_empty', counting)
    out, side = e(x, skip, lambda t: None)
    if count is not None:
        monkeypatch.setattr(Fn, '_empty', real)
    out.backward(to_act(rnd(*out.shape, seed=13, scale=0.1)))
    torch.cuda.synchronize()
    res = {'out': out.detach(), 'dx': x.grad, 'dskip': skip.grad}
    for k, p in e.named_parameters():
        assert p.grad is not None, k
        res[k] = p.grad
    return res


def test_decoder_module_folded_vs_unfolded(monkeypatch):
    Fn = _fn()
    m = _module()
    before = Fn.SKIP_FOLD_FALLBACKS
    a_new, a_old = [], []
    new = _run(m, True, monkeypatch, a_new)
    old = _run(m, False, monkeypatch, a_old)
    old2 = _run(m, False, monkeypatch)
    assert Fn.SKIP_FOLD_FALLBACKS == before
    # the activation (2, 64, 12, 16) and its ReLU bit mask are not allocated on the folded path:
    # fp32 maps of the skip's size = conv output + module output (+ the activation when unfolded)
    big = lambda rec: sum(1 for s, d in rec if s == (2, 12, 16, 64) and d == torch.float32)   # noqa: E731
    assert big(a_old) == 3 and big(a_new) == 2
    assert len(a_new) == len(a_old) - 2
    bad = []
    for k in old:
        assert torch.isfinite(new[k]).all(), k
        d_new = float((new[k] - old[k]).abs().max())
        if k in ATOMIC:
            d_old = float((old2[k] - old[k]).abs().max())
            lim = max(2 * d_old, 1e-6 * float(old[k].abs().max()))
            print(f"{k}: folded-vs-unfolded {d_new:.3e}, unfolded twice {d_old:.3e}, bound {lim:.3e}")
            if d_new > lim:
                bad.append(f"{k}: {d_new:.3e} > {lim:.3e}")
        elif not torch.equal(new[k], old[k]):
            bad.append(f"{k}: not bit-equal (max diff {d_new:.3e})")
    assert not bad, '\n'.join(bad)
    # the skip path matters to the result and got its gradient
    assert float(new['dskip'].abs().max()) > 0 and float(new['skip_fusion.norm.weight'].abs().max()) > 0


def test_forced_switch_falls_back_and_counts(monkeypatch):
    """SKIP_FOLD = True in a configuration the fold does not cover (up-sampling without weights)
    runs today's launches and counts the fallback; switched off or below the rule's floor nothing is
    counted and nothing folds"""
    Fn = _fn()
    calls = []
    real = Fn.up2x_dw_fwd_skipbn
    monkeypatch.setattr(Fn, 'up2x_dw_fwd_skipbn', lambda *a: (calls.append(1), real(*a))[1])
    before = Fn.SKIP_FOLD_FALLBACKS
    plain = _module('nearest')
    _run(plain, True, monkeypatch)
    assert Fn.SKIP_FOLD_FALLBACKS == before + 1 and not calls
    # 16-bit features: refused by the rule's own shape / type test
    assert Fn.skip_fold(torch.zeros(2, 64, 6, 8, dtype=torch.bfloat16), 32, 64, True) is False
    assert Fn.SKIP_FOLD_FALLBACKS == before + 2
    m = _module()
    _run(m, False, monkeypatch)
    monkeypatch.setattr(Fn, '_SKIP_FOLD_ENV', None)
    _run(m, None, monkeypatch)                         # below the size floor: neither
    assert Fn.SKIP_FOLD_FALLBACKS == before + 2 and not calls
    monkeypatch.setattr(Fn, '_SKIP_FOLD_MIN_BYTES', 2 * 64 * 12 * 16 * 4)
    _run(m, None, monkeypatch)                         # the rule says yes
    assert Fn.SKIP_FOLD_FALLBACKS == before + 2 and len(calls) == 1
    ev = copy.deepcopy(m).eval()
    monkeypatch.setattr(Fn, 'SKIP_FOLD', True)
    with torch.no_grad():                              # eval keeps its own path: not a fallback
        ev(to_act(rnd(2, 128, 6, 8, seed=11)), to_act(rnd(2, 32, 12, 16, seed=12)), lambda t: None)
    assert Fn.SKIP_FOLD_FALLBACKS == before + 2 and len(calls) == 1


def test_full_model_train_step_folds_everywhere(monkeypatch):
    """one eager fp32 training step of a small full model, the folds forced on (this one, Fn.DRES_FOLD
    and Fn.IDN_FOLD of the NBt1D blocks): all six decoder modules fold, neither fold falls back, and the
    outputs equal the unfolded model's bit for bit"""
    import test_model_gpu as T
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.model import EMSANet
    from oracle.emsanet_oracle import synthetic_batch
    Fn = _fn()
    calls = []
    real = Fn.up2x_dw_fwd_skipbn
    monkeypatch.setattr(Fn, 'up2x_dw_fwd_skipbn', lambda *a: (calls.append(1), real(*a))[1])
    args = full_args(input_height=96, input_width=128)
    torch.manual_seed(0)
    model = EMSANet(args, nyuv2_config()).to(DEV).train()
    model.dropout_seed = 99
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 96, 128, seed=1).items()}
    before = (Fn.SKIP_FOLD_FALLBACKS, Fn.DRES_FALLBACKS)
    runs = {}
    for fold in (True, False):
        monkeypatch.setattr(Fn, 'SKIP_FOLD', fold)
        monkeypatch.setattr(Fn, 'DRES_FOLD', fold)
        monkeypatch.setattr(Fn, 'IDN_FOLD', fold)
        m = copy.deepcopy(model)
        outs = T._flatten(m(batch))
        sum((t * t).mean() for t in outs).backward()
        torch.cuda.synchronize()
        runs[fold] = ([o.detach() for o in outs], {k: p.grad for k, p in m.named_parameters()})
    assert (Fn.SKIP_FOLD_FALLBACKS, Fn.DRES_FALLBACKS) == before and len(calls) == 6
    for a, b in zip(runs[True][0], runs[False][0]):
        assert torch.equal(a, b)
    gmax = max(float(g.abs().max()) for g in runs[False][1].values() if g is not None)
    for k, g in runs[False][1].items():
        if g is None:
            continue
        d = float((runs[True][1][k] - g).abs().max())
        assert d <= 1e-4 * gmax, f"grad {k}: {d:.3e} vs max {gmax:.3e}"      # (atomics jitter of other kernels)
