"""GPU: the fused half-resolution stage (csrc/stem_stage.hip, ops.StemStageFunction) against the
kernels it replaces -- bn_act, se_pair_fwd, se_scale_add, maxpool_fwd forward; maxpool_bwd, the SE
backward and bn_bwd backward -- and both against an fp64 torch restatement of the backward pass.

Inputs per shape: y from randn; gamma with negative entries and one exact zero (channel 3); in image 0
channel 7 of both streams far below the batch mean, so that z < 0 everywhere there (no mask bit set,
pooled value 0, argmax = the first in-range tap); channel 5 made of a few repeated values, so that
pooling windows hold exact ties."""
import copy
import functools
import math

import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

C, CR = 64, 4
EPS = 1e-5
# (n, H, W) of the /2 maps: one window with every tap clipped; odd height and width (the last quad
# row and column half outside); even sizes; odd x even; several workgroups and reduction splits
SHAPES = [(2, 2, 2), (2, 5, 7), (2, 6, 10), (3, 9, 4), (3, 34, 46)]
ULP = 2.0 ** -23


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _y(n, h, w, seed):
    y = rnd(n, C, h, w, seed=seed)
    y[:, 5] = torch.round(y[:, 5])                     # exact ties inside the windows
    y[0, 7] = -3.0 - y[0, 7].abs()                     # z < 0 in the whole image
    return y


@functools.lru_cache(maxsize=None)
def _case(n, h, w):
    """inputs, the unfused forward (the saved state both backward paths start from) and the fp64
    reference of the backward pass; computed once per shape and left unchanged"""
    Fn = _fn()
    seed = 1000 * n + 10 * h + w
    ys = [_y(n, h, w, seed), _y(n, h, w, seed + 1)]
    gam, bet = [], []
    for m in range(2):
        g = rnd(C, seed=seed + 10 + m)
        g[3], g[7] = 0.0, 1.0 + g[7].abs()
        b = rnd(C, seed=seed + 20 + m, scale=0.3)
        b[7] = 0.0
        gam.append(g)
        bet.append(b)
    # batch statistics as bn_finalize hands them on: scale = gamma * invstd, shift = beta - mean * scale
    aff, st = [], []
    for y, g, b in zip(ys, gam, bet):
        y64 = y.double()
        mean = y64.mean((0, 2, 3))
        var = y64.var((0, 2, 3), unbiased=False)
        invstd = (1.0 / torch.sqrt(var + EPS)).float()
        scale = g * invstd
        shift = b - mean.float() * scale
        aff.append((scale, shift))
        st.append((mean.float(), invstd))
    for y, (scale, shift) in zip(ys, aff):            # the inputs do what the docstring says
        assert (y[0, 7] * scale[7] + shift[7]).max() < 0
    se = []
    for m in range(2):
        # (hidden biases shifted up: most of the four hidden units alive, some dead in some image)
        se.append((rnd(CR, C, seed=seed + 30 + m, scale=0.3), rnd(CR, seed=seed + 40 + m, scale=0.3) + 0.5,
                   rnd(C, CR, seed=seed + 50 + m, scale=0.3), rnd(C, seed=seed + 60 + m, scale=0.3)))
    oh, ow = (h + 1) // 2, (w + 1) // 2
    gf, gd = rnd(n, C, oh, ow, seed=seed + 70), rnd(n, C, oh, ow, seed=seed + 71)

    dev = lambda t: t.to(DEV)                          # noqa: E731
    d = dict(n=n, h=h, w=w, ys=[to_act(y) for y in ys], gamma=[dev(g) for g in gam],
             aff=[tuple(dev(t) for t in a) for a in aff], st=[tuple(dev(t) for t in s) for s in st],
             se=[tuple(dev(t) for t in s) for s in se], gf=to_act(gf), gd=to_act(gd))
    # ---- unfused forward ----
    acts, masks = [], []
    for y, (scale, shift) in zip(d['ys'], d['aff']):
        a, bits = Fn.bn_act(y, scale, shift, None, None, Fn.ACT_RELU, want_mask=True)
        acts.append(a)
        masks.append(bits)
    gr, gdp, hr, hd, sr, sd = Fn.se_pair_fwd(acts[0], acts[1], d['se'][0], d['se'][1])
    fused_map = Fn.se_scale_add(acts[0], sr, acts[1], sd)
    pf, idx_f = Fn.maxpool_fwd(fused_map)
    pd, idx_d = Fn.maxpool_fwd(acts[1])
    d.update(acts=acts, masks=masks, gap=[gr, gdp], hid=[hr, hd], s=[sr, sd], pf=pf, idx_f=idx_f,
             pd=pd, idx_d=idx_d, gap_means=[Fn.channel_mean(a) for a in acts])
    torch.cuda.synchronize()
    assert float(acts[0][0, 7].max()) == 0.0 and float(acts[1][0, 7].max()) == 0.0
    # ---- fp64 reference of the backward pass from that saved state ----
    c64 = lambda t: t.detach().cpu().double()          # noqa: E731

    def unpool(g, idx):
        g, idx = c64(g), idx.cpu().permute(0, 3, 1, 2)           # idx is stored NHWC
        pad = torch.zeros(n, C, 2 * oh + 1, 2 * ow + 1, dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                pad[:, :, kh:kh + 2 * oh:2, kw:kw + 2 * ow:2] += g * (idx == kh * 3 + kw)
        return pad[:, :, 1:1 + h, 1:1 + w]
    dout, ddn = unpool(d['gf'], idx_f), unpool(d['gd'], idx_d)
    ref = {}
    for m, name in enumerate(('rgb', 'depth')):
        y = ys[m].double()
        scale, shift = (c64(t) for t in d['aff'][m])
        mean, invstd = (c64(t) for t in d['st'][m])
        v = lambda t: t.view(1, C, 1, 1)               # noqa: E731
        z = y * v(scale) + v(shift)
        a, mask = z.clamp(min=0), (z > 0).double()
        w1, _, w2, _ = (c64(t) for t in d['se'][m])
        gap, hid, s = c64(d['gap'][m]), c64(d['hid'][m]), c64(d['s'][m])
        ds = (dout * a).sum((2, 3))
        g = ds * s * (1 - s)
        dz1 = (hid > 0).double() * (g @ w2)
        dgap = dz1 @ w1
        ref[f'se_{name}'] = (dz1.t() @ gap, dz1.sum(0), g.t() @ hid, g.sum(0))
        da = dout * s.view(n, C, 1, 1) + dgap.view(n, C, 1, 1) / (h * w)
        if m == 1:
            da = da + ddn
        dz = mask * da
        xh = (y - v(mean)) * v(invstd)
        db, dg = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
        cnt = n * h * w
        ref[f'dy_{name}'] = v(c64(d['gamma'][m]) * invstd) * (dz - v(db) / cnt - xh * v(dg) / cnt)
        ref[f'dgamma_{name}'], ref[f'dbeta_{name}'] = dg, db
    d['ref'] = ref
    return d


def _unfused_bwd(d):
    Fn = _fn()
    n, h, w = d['n'], d['h'], d['w']
    dout = Fn.maxpool_bwd(d['gf'], d['idx_f'], (h, w))
    ddn = Fn.maxpool_bwd(d['gd'], d['idx_d'], (h, w))
    out = {}
    for m, name in enumerate(('rgb', 'depth')):
        w1, _, w2, _ = d['se'][m]
        ds = Fn.se_scale_bwd_reduce(dout, d['acts'][m])
        dgap, dw1, db1, dw2, db2 = Fn.se_mlp_bwd(d['gap'][m], w1, w2, d['hid'][m], d['s'][m], ds)
        da = Fn.se_scale_bwd_apply(dout, d['s'][m], dgap, ddn if m == 1 else None)
        dy, _, dg, db = Fn.bn_bwd(da, d['masks'][m], d['ys'][m], d['gamma'][m], d['st'][m][0],
                                  d['st'][m][1], None, Fn.ACT_RELU, True, want_dres=False)
        out[f'se_{name}'] = (dw1, db1, dw2, db2)
        out[f'dy_{name}'], out[f'dgamma_{name}'], out[f'dbeta_{name}'] = dy, dg, db
    return out


def _fused_bwd(d):
    Fn = _fn()
    h, w = d['h'], d['w']
    ys, aff, st, s = d['ys'], d['aff'], d['st'], d['s']
    sums, ds_r, ds_d = Fn.stem_stage_bwd_reduce(d['gf'], d['idx_f'], d['gd'], d['idx_d'], ys[0], ys[1],
                                                aff[0], aff[1], st[0], st[1])
    out, dgaps = {}, []
    for m, (name, ds) in enumerate((('rgb', ds_r), ('depth', ds_d))):
        w1, _, w2, _ = d['se'][m]
        dgap, dw1, db1, dw2, db2 = Fn.se_mlp_bwd(d['gap'][m], w1, w2, d['hid'][m], s[m], ds)
        dgaps.append(dgap)
        out[f'se_{name}'] = (dw1, db1, dw2, db2)
    dgb = Fn.stem_stage_bwd_finalize(sums, h * w, s[0], s[1], dgaps[0], dgaps[1])
    dy_r, dy_d = Fn.stem_stage_bwd_apply(d['gf'], d['idx_f'], d['gd'], d['idx_d'], ys[0], ys[1], aff[0],
                                         aff[1], st[0], st[1], d['gamma'][0], d['gamma'][1], s[0], s[1],
                                         dgaps[0], dgaps[1], dgb)
    out.update(dy_rgb=dy_r, dy_depth=dy_d, dgamma_rgb=dgb[0], dbeta_rgb=dgb[1], dgamma_depth=dgb[2],
               dbeta_depth=dgb[3])
    return out


def _flat(res):
    """name -> tensor of every backward result (the SE tuples spread out)"""
    out = {}
    for k, v in res.items():
        if isinstance(v, tuple):
            for name, t in zip(('dw1', 'db1', 'dw2', 'db2'), v):
                out[f'{k}.{name}'] = t
        else:
            out[k] = v
    return out


def _err(got, ref):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max())


@pytest.mark.parametrize('n,h,w', SHAPES)
def test_squeeze_from_y(n, h, w):
    """forward pass 1 against channel_mean(bn_act(y)): 4 ulp x sqrt(pixels per image) of max|gap|
    (the kernel keeps channel_dot's partition and order, so the difference is expected to be 0)"""
    Fn = _fn()
    d = _case(n, h, w)
    gr, gd, hr, hd, sr, sd = Fn.stem_stage_se(d['ys'][0], d['ys'][1], d['aff'][0], d['aff'][1],
                                              d['se'][0], d['se'][1])
    for m, gap in enumerate((gr, gd)):
        ref = d['gap_means'][m]
        err = float((gap - ref).abs().max())
        lim = 4 * ULP * math.sqrt(h * w) * float(ref.abs().max())
        print(f"squeeze {('rgb', 'depth')[m]} ({n},{h},{w}): max err {err:.3e}, bound {lim:.3e}")
        assert err <= lim
    # (and with equal gap the pair MLP gives the unfused path's hidden units and weights)
    for a, b in ((hr, d['hid'][0]), (hd, d['hid'][1]), (sr, d['s'][0]), (sd, d['s'][1])):
        assert float((a - b).abs().max()) <= 4 * ULP * math.sqrt(h * w) * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('n,h,w', SHAPES)
def test_forward_bit_equal(n, h, w):
    """forward pass 2, fed the unfused path's s: P_f, P_d and both argmax maps bit for bit"""
    Fn = _fn()
    d = _case(n, h, w)
    pf, idx_f, pd, idx_d = Fn.stem_stage_fwd(d['ys'][0], d['ys'][1], d['aff'][0], d['aff'][1],
                                             d['s'][0], d['s'][1])
    assert torch.equal(idx_f, d['idx_f']) and torch.equal(idx_d, d['idx_d'])
    assert torch.equal(pf.view(torch.int32), d['pf'].view(torch.int32))
    assert torch.equal(pd.view(torch.int32), d['pd'].view(torch.int32))
    # the all-negative channel: pooled value 0 and the first in-range tap (0 inside, 4 at the corner)
    assert float(pd[0, 7].abs().max()) == 0.0
    assert int(idx_d[0, 0, 0, 7]) == 4 and (h < 4 or w < 4 or int(idx_d[0, 1, 1, 7]) == 0)


@pytest.mark.parametrize('n,h,w', SHAPES)
def test_backward_against_fp64(n, h, w):
    """every gradient of the stage, fused and unfused from the same saved state and the same G_f, G_d,
    against the fp64 restatement: err(fused) <= max(2 err(unfused), 1e-6 max|reference|)"""
    d = _case(n, h, w)
    fu, un = _flat(_fused_bwd(d)), _flat(_unfused_bwd(d))
    ref = _flat(d['ref'])
    assert set(fu) == set(un) == set(ref) and len(ref) == 14
    bad = []
    for k in sorted(ref):
        ef, eu, top = _err(fu[k], ref[k]), _err(un[k], ref[k]), float(ref[k].abs().max())
        lim = max(2 * eu, 1e-6 * top)
        print(f"({n},{h},{w}) {k:18s} fused {ef:.3e}  unfused {eu:.3e}  max|ref| {top:.3e}")
        if ef > lim:
            bad.append(f"{k}: fused {ef:.3e} > max(2 x {eu:.3e}, 1e-6 x {top:.3e})")
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('n,h,w', [(2, 5, 7), (3, 34, 46)])
def test_fused_stage_is_deterministic(n, h, w):
    """two runs of the fused path: outputs and all gradients bit-equal"""
    Fn = _fn()
    d = _case(n, h, w)

    def run():
        se = Fn.stem_stage_se(d['ys'][0], d['ys'][1], d['aff'][0], d['aff'][1], d['se'][0], d['se'][1])
        fwd = Fn.stem_stage_fwd(d['ys'][0], d['ys'][1], d['aff'][0], d['aff'][1], se[4], se[5])
        return list(se) + list(fwd) + [t for _, t in sorted(_flat(_fused_bwd(d)).items())]
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_host_side_refusals():
    """other channel counts are refused on the host, before any launch"""
    from emsanet_amd import _lib
    L = _lib.lib()
    one = torch.zeros(16, device=DEV).data_ptr()
    assert L.emsa_stem_stage_squeeze(*([one] * 7), 2, 4, 32, None) == _lib.E_SHAPE
    assert L.emsa_stem_stage_fwd(*([one] * 12), 2, 2, 2, 128, None) == _lib.E_SHAPE
    assert L.emsa_stem_stage_bwd_reduce(*([one] * 17), 2, 2, 2, 32, None) == _lib.E_SHAPE
    assert L.emsa_stem_stage_bwd_finalize(*([one] * 9), 2, 4, 32, None) == _lib.E_SHAPE
    assert L.emsa_stem_stage_bwd_apply(*([one] * 26), 2, 2, 2, 32, None) == _lib.E_SHAPE
    assert L.emsa_stem_stage_fwd(*([None] * 12), 2, 2, 2, 64, None) == -2


def _encoders(seed=0):
    """engine and oracle (fp64) dual ResNet-18 encoders with the same weights, no dropout"""
    from emsanet_amd import nn as E
    from oracle import emsanet_oracle as O
    from oracle.emsanet_oracle import deterministic_state_dict

    def make(mod):
        return mod.FusedEncoder(mod.ResNetNBt1D('resnet18', 3, 0.0), mod.ResNetNBt1D('resnet18', 1, 0.0),
                                'se-add-uni-rgb', (4, 8, 16))
    oracle = make(O)
    sd = deterministic_state_dict(oracle, seed)
    oracle.load_state_dict(sd)
    enc = make(E)
    enc.load_state_dict(sd)
    return enc.to(DEV).train(), oracle.double().train()


def _encoder_outputs(outs, skips):
    return [outs['rgb'], outs['depth']] + [skips[k]['rgb'] for k in sorted(skips)]


def test_encoder_fused_vs_unfused(monkeypatch):
    """the whole stage through FusedEncoder (n = 2, 32 x 48 input), STEM_FUSE True vs False against
    the fp64 oracle encoder: outputs and parameter gradients within the 2x rule of the backward
    test; the fused run must not fall back"""
    Fn = _fn()
    enc, oracle = _encoders()
    feeds = {'rgb': rnd(2, 3, 32, 48, seed=5), 'depth': rnd(2, 1, 32, 48, seed=6)}
    ro = _encoder_outputs(*oracle({k: v.double() for k, v in feeds.items()}))
    cots = [rnd(*t.shape, seed=50 + i, scale=0.1) for i, t in enumerate(ro)]
    torch.autograd.backward(ro, [c.double() for c in cots])
    gfeeds = {k: v.to(DEV) for k, v in feeds.items()}
    runs = {}
    calls = []
    real = Fn.stem_stage_fwd
    monkeypatch.setattr(Fn, 'stem_stage_fwd', lambda *a: (calls.append(1), real(*a))[1])
    for fuse in (True, False):
        monkeypatch.setattr(Fn, 'STEM_FUSE', fuse)
        before = (Fn.STEM_FUSE_FALLBACKS, len(calls))
        e = copy.deepcopy(enc)
        outs = _encoder_outputs(*e(gfeeds))
        torch.autograd.backward(outs, [c.to(DEV) for c in cots])
        torch.cuda.synchronize()
        assert Fn.STEM_FUSE_FALLBACKS == before[0] and len(calls) == before[1] + (1 if fuse else 0)
        runs[fuse] = ([o.detach() for o in outs], {k: p.grad for k, p in e.named_parameters()})
    refs = [(f'out{i}', a, b, r.detach()) for i, (a, b, r) in enumerate(zip(runs[True][0], runs[False][0], ro))]
    for k, p in oracle.named_parameters():
        assert runs[True][1][k] is not None, k
        refs.append((k, runs[True][1][k], runs[False][1][k], p.grad))
    bad = []
    for k, a, b, r in refs:
        ef, eu, top = _err(a, r), _err(b, r), float(r.abs().max())
        if ef > max(2 * eu, 1e-6 * top):
            bad.append(f"{k}: fused {ef:.3e} > max(2 x {eu:.3e}, 1e-6 x {top:.3e})")
    assert not bad, '\n'.join(bad)


def test_forced_switch_falls_back_and_counts(monkeypatch):
    """STEM_FUSE = True in configurations the kernels do not cover (16-bit storage; eval) runs
    today's path and counts the fallback; with the rule alone nothing is counted"""
    Fn = _fn()
    enc, _ = _encoders()
    feeds = {'rgb': rnd(2, 3, 64, 128, seed=5).to(DEV), 'depth': rnd(2, 1, 64, 128, seed=6).to(DEV)}
    calls = []
    real = Fn.stem_stage_fwd
    monkeypatch.setattr(Fn, 'stem_stage_fwd', lambda *a: (calls.append(1), real(*a))[1])

    def run(e):
        outs, _ = e(feeds)
        torch.cuda.synchronize()
        assert torch.isfinite(outs['rgb'].float()).all()
        return outs['rgb']
    monkeypatch.setattr(Fn, 'STEM_FUSE', True)
    before = Fn.STEM_FUSE_FALLBACKS
    e16 = copy.deepcopy(enc)
    for bb in (e16.backbone_rgb, e16.backbone_depth):
        bb.compute_dtype = torch.bfloat16
    assert run(e16).dtype == torch.bfloat16
    assert Fn.STEM_FUSE_FALLBACKS == before + 1 and not calls
    ev = copy.deepcopy(enc).eval()
    with torch.no_grad():
        run(ev)
    assert Fn.STEM_FUSE_FALLBACKS == before + 2 and not calls
    monkeypatch.setattr(Fn, 'STEM_FUSE', None)
    monkeypatch.setattr(Fn, '_STEM_FUSE_ENV', None)
    with torch.no_grad():
        run(ev)                                        # the rule says no: not a fallback
    run(copy.deepcopy(enc))                            # below the rule's size floor: neither
    assert Fn.STEM_FUSE_FALLBACKS == before + 2 and not calls
    monkeypatch.setattr(Fn, '_STEM_FUSE_MIN_BYTES', 2 * 64 * 32 * 64 * 4)
    run(copy.deepcopy(enc))                            # the rule says yes: the fused stage runs
    assert Fn.STEM_FUSE_FALLBACKS == before + 2 and len(calls) == 1


def test_graphed_train_step_with_fused_stage_equals_eager(monkeypatch):
    """a training step with the fused stage captured and replayed from GraphedTrainStep == its eager
    twin (learning rate 0: the loss bit for bit, the gradients to the atomics jitter of other kernels)"""
    import test_model_gpu as T
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.graph import GraphedTrainStep
    from emsanet_amd.model import EMSANet
    from emsanet_amd.optim import FusedSGD
    from emsanet_amd.parallel import GradientBuckets
    from oracle.emsanet_oracle import synthetic_batch
    Fn = _fn()
    monkeypatch.setattr(Fn, 'STEM_FUSE', True)
    calls = []
    real = Fn.stem_stage_fwd
    monkeypatch.setattr(Fn, 'stem_stage_fwd', lambda *a: (calls.append(1), real(*a))[1])
    fallbacks0 = Fn.STEM_FUSE_FALLBACKS
    args = full_args(input_height=96, input_width=128)

    def build():
        torch.manual_seed(0)
        m = EMSANet(args, nyuv2_config()).to(DEV).train()
        m.dropout_seed = 99
        b = GradientBuckets([p for p in m.parameters() if p.requires_grad])
        return m, b, FusedSGD(b, lr=0.0, momentum=0.9, weight_decay=0.0)
    batches = [{k: v.to(DEV) for k, v in synthetic_batch(2, 96, 128, seed=s).items()} for s in (1, 2)]

    def loss_of(out):
        return sum((t * t).mean() for t in T._flatten(out))
    m2, b2, o2 = build()
    m3, b3, o3 = build()
    g = GraphedTrainStep(m2, batches[0], b2, o2, loss_fn=loss_of, warmup=3)
    l2, _ = g.replay(batches[1])
    b3.reset()
    loss = loss_of(m3(batches[1]))
    loss.backward()
    b3.finish()
    o3.step()
    torch.cuda.synchronize()
    assert calls and Fn.STEM_FUSE_FALLBACKS == fallbacks0
    assert float(l2) == float(loss.detach()), (float(l2), float(loss.detach()))
    gmax = max(float(p.grad.abs().max()) for p in m3.parameters())
    for (k, p2), (_, p3) in zip(m2.named_parameters(), m3.named_parameters()):
        d = float((p2.grad - p3.grad).abs().max())
        assert d <= 1e-4 * gmax, f"grad {k}: {d:.3e} vs max {gmax:.3e}"
