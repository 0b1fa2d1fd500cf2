"""2-D Winograd F(2x2,3x3) kernel of the dense 3x3 convs (csrc/conv_wino2d.hip): forward and data
gradient against an fp64 direct convolution and against the row-Winograd kernel, the fused
epilogues, the BatchNorm statistics rows, the weight transforms, host-side rejection, batch
invariance, and a small full model (eager and replayed from a hipGraph) with the 2-D form on."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, close, rnd, to_act

pytestmark = pytest.mark.gpu

# (cin, cout, n, h, w)
SHAPES = [
    (64, 64, 2, 12, 20),        # baseline, all even
    (128, 40, 1, 9, 13),        # odd H and W, partial N tile
    (96, 8, 2, 5, 7),           # N = 8
    (8, 96, 1, 6, 6),           # K shorter than a K step
    (72, 64, 1, 3, 40),         # K tail, H = 3
    (20, 36, 2, 5, 7),          # K and N both partial
    (64, 64, 1, 1, 1),          # single pixel
    (64, 64, 3, 2, 2),          # one tile per image: a workgroup spans images
    (64, 64, 1, 4, 66),         # 33 tiles per row: a workgroup's tiles wrap lines
    (512, 512, 1, 15, 20),      # the /32 stage's geometry, long K
]


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def _case(cfg):
    """inputs and the fp64 references of one shape, computed once and shared by the tests"""
    cin, cout, n, h, w = cfg
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=0.1)
    b = rnd(cout, seed=3)
    xd = x.double().requires_grad_(True)
    y_nobias = F.conv2d(xd, wt.double(), None, padding=1)
    dy = rnd(*y_nobias.shape, seed=7)
    y_nobias.backward(dy.double())
    ref = (y_nobias + b.double()[None, :, None, None]).detach()
    return x, wt, b, ref, dy, xd.grad.detach()


def _spec(cin, cout):
    Fn = _fn()
    spec = Fn.ConvSpec(cin, cout, (3, 3), (1, 1), (1, 1))
    assert Fn.wino2d_eligible(spec)
    return spec


@pytest.mark.parametrize('cfg', SHAPES)
def test_wino2d_fwd(cfg):
    """== direct convolution (fp64) with bias, with the statistics rows, with scale / shift /
    residual / ReLU; == the row-Winograd kernel to the kernel-versus-kernel bound"""
    Fn = _fn()
    cin, cout, n, h, w = cfg
    x, wt, b, ref, _, _ = _case(cfg)
    spec = _spec(cin, cout)
    u2 = Fn.pack_wino2d(wt.to(DEV))[0]
    y = Fn.conv_fwd(to_act(x), None, spec, bias=b.to(DEV), wino2d_u=u2)
    torch.cuda.synchronize()
    print('fwd err', close(y, ref, what='wino2d conv'))
    y1, stats = Fn.conv_fwd(to_act(x), None, spec, bias=b.to(DEV), want_stats=True, wino2d_u=u2)
    assert torch.equal(y1, y)
    assert stats.shape[1] == -(-(n * ((h + 1) // 2) * ((w + 1) // 2)) // 32)
    cnt = ref.numel() / cout
    assert float(stats[2][:, 0].sum()) == cnt
    assert bool((stats[2] == stats[2][:, :1]).all())
    mean = stats[0].sum(0) / cnt
    close(mean, ref.mean((0, 2, 3)), what='stats mean')
    tile_mean = stats[0] / stats[2].clamp(min=1)
    m2 = stats[1].sum(0) + (stats[2] * (tile_mean - mean[None]) ** 2).sum(0)
    close(m2 / cnt, ref.var((0, 2, 3), unbiased=False), tol=2e-4, what='stats var')
    sc, sh = rnd(cout, seed=4), rnd(cout, seed=5)
    res = rnd(*ref.shape, seed=6)
    y2 = Fn.conv_fwd(to_act(x), None, spec, bias=b.to(DEV), scale=sc.to(DEV), shift=sh.to(DEV),
                     residual=to_act(res), act=Fn.ACT_RELU, wino2d_u=u2)
    ref2 = F.relu(ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None] + res)
    close(y2, ref2, what='wino2d epilogue')
    # the row-Winograd kernel on the same inputs
    u = Fn.pack_wino(wt.to(DEV))[0]
    y3 = Fn.conv_fwd(to_act(x), None, spec, bias=b.to(DEV), wino_u=u)
    print('vs row err', close(y, y3.double(), tol=2e-5, what='wino2d vs row-Winograd'))


@pytest.mark.parametrize('cfg', SHAPES)
def test_wino2d_dgrad(cfg):
    Fn = _fn()
    cin, cout, n, h, w = cfg
    x, wt, _, _, dy, dx_ref = _case(cfg)
    spec = _spec(cin, cout)
    ud2 = Fn.pack_wino2d(wt.to(DEV), fwd=False, dgrad=True)[1]
    dx = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), wino2d_u=ud2)
    torch.cuda.synchronize()
    print('dgrad err', close(dx, dx_ref, what='wino2d dgrad'))
    mask = rnd(n, cin, h, w, seed=8)
    res = rnd(n, cin, h, w, seed=9)
    dx2 = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), mask_src=to_act(mask), wino2d_u=ud2)
    close(dx2, dx_ref * (mask > 0), what='wino2d dgrad mask')
    dx3 = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), residual=to_act(res), wino2d_u=ud2)
    close(dx3, dx_ref + res, what='wino2d dgrad residual')
    dx4 = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), mask_src=to_act(mask),
                        residual=to_act(res), wino2d_u=ud2)
    close(dx4, (dx_ref + res) * (mask > 0), what='wino2d dgrad residual + mask')
    ud = Fn.pack_wino(wt.to(DEV), fwd=False, dgrad=True)[1]
    dx5 = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), wino_u=ud)
    close(dx, dx5.double(), tol=2e-5, what='wino2d dgrad vs row-Winograd')


@pytest.mark.parametrize('cfg', SHAPES)
def test_wino2d_pack_routes_bit_equal(cfg):
    """U2 from the OIHW parameter == U2 from the packed [tap][n][k] layout, forward and flipped; and
    U2 is the row-Winograd U transformed across the three kernel rows"""
    Fn = _fn()
    cin, cout = cfg[:2]
    wt = _case(cfg)[1].to(DEV)
    u2, ud2 = Fn.pack_wino2d(wt, fwd=True, dgrad=True)
    a = Fn.pack_wino2d_packed(Fn.pack_weight(wt, 'fwd'), cout, cin, flip=False)
    assert torch.equal(u2, a)
    bflip = Fn.pack_wino2d_packed(Fn.pack_weight(wt, 'dgrad'), cin, cout, flip=True)
    assert torch.equal(ud2, bflip)
    u = Fn.pack_wino(wt)[0].view(4, cout, 3, cin)                  # [j][n][r][k]
    r0, r1, r2 = u[:, :, 0], u[:, :, 1], u[:, :, 2]
    s, hh = 0.5 * (r0 + r2), 0.5 * r1
    want = torch.stack([r0, s + hh, s - hh, r2])                   # [i][j][n][k]
    def plain(t, n, k):                       # [16][ceil(k/8)][n][8] -> [4][4][n][k]
        return t.view(16, -1, n, 8).permute(0, 2, 1, 3).reshape(4, 4, n, -1)[..., :k]
    assert u2.numel() == Fn.wino2d_numel(cout, cin) and ud2.numel() == Fn.wino2d_numel(cin, cout)
    assert torch.equal(plain(u2, cout, cin), want)
    # the data-gradient form: kernel flipped (components 0 <-> 3 both ways), channels transposed
    perm = [3, 1, 2, 0]
    assert torch.equal(plain(ud2, cin, cout), plain(u2, cout, cin)[perm][:, perm].transpose(2, 3))


def test_wino2d_host_side_rejection():
    """unsupported geometries and operand combinations return EMSA_E_SHAPE before any launch, and
    conv_fwd then goes on with the row kernel"""
    from emsanet_amd import _lib
    Fn = _fn()
    L = _lib.lib()

    def rc(spec, n=1, h=8, w=8):
        g = spec.geom_fwd(n, h, w, spec.cin, spec.cout)
        assert L.emsa_conv_wino2d_supported(g) == 0
        assert L.emsa_conv_wino2d_stats_rows(g) == _lib.E_SHAPE
        return L.emsa_conv_wino2d(g, None, None, None, None, None, None, None, None, 0, None, 0, 0,
                                  None)
    assert rc(Fn.ConvSpec(64, 64, (3, 3), (2, 2), (1, 1))) == _lib.E_SHAPE          # stride 2
    assert rc(Fn.ConvSpec(6, 64, (3, 3), (1, 1), (1, 1))) == _lib.E_SHAPE           # cin % 4
    assert rc(Fn.ConvSpec(64, 64, (1, 3), (1, 1), (0, 1))) == _lib.E_SHAPE          # not 3x3
    # statistics together with an activation: not a combination the epilogue takes
    cfg = SHAPES[0]
    cin, cout, n, h, w = cfg
    x, wt, b, ref, _, _ = _case(cfg)
    spec = _spec(cin, cout)
    xa = to_act(x)
    out = torch.full_like(to_act(ref.float()), 7.0)
    g = spec.geom_fwd(n, h, w, Fn.ld_of(xa), Fn.ld_of(out))
    assert L.emsa_conv_wino2d_supported(g) == 1
    rows = L.emsa_conv_wino2d_stats_rows(g)
    assert rows == 4
    u2 = Fn.pack_wino2d(wt.to(DEV))[0]
    stats = torch.zeros(3, rows, cout, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.emsa_conv_wino2d(g, p(xa), p(u2), p(out), None, p(stats), None, None, None, 0, None, 0,
                              Fn.ACT_RELU, None) == _lib.E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 0).all())             # nothing ran
    # conv_fwd: the refused combination runs on the row kernel (handed over lazily)
    asked = []

    def row_u():
        asked.append(1)
        return Fn.pack_wino(wt.to(DEV))[0]
    before = Fn.WINO2D_FALLBACKS
    y, st = Fn.conv_fwd(xa, None, spec, bias=b.to(DEV), want_stats=True, act=Fn.ACT_RELU,
                        wino2d_u=u2, wino_u=row_u)
    assert asked == [1] and Fn.WINO2D_FALLBACKS == before + 1     # and the fallback is counted
    yr, sr = Fn.conv_fwd(xa, None, spec, bias=b.to(DEV), want_stats=True, act=Fn.ACT_RELU,
                         wino_u=row_u())
    assert torch.equal(y, yr) and torch.equal(st, sr)


@pytest.mark.parametrize('cfg', [(64, 64, 3, 2, 2), (128, 40, 3, 9, 13), (64, 64, 3, 12, 20),
                                 (72, 64, 3, 3, 40)])
def test_wino2d_batch_invariant(cfg):
    """image 0 of a 3-image batch == the same image run alone, bit for bit (forward and data
    gradient): the K summation order does not depend on the batch or on the tile's position"""
    Fn = _fn()
    cin, cout, n, h, w = cfg
    x = rnd(n, cin, h, w, seed=11)
    wt = rnd(cout, cin, 3, 3, seed=12, scale=0.1).to(DEV)
    spec = _spec(cin, cout)
    u2, ud2 = Fn.pack_wino2d(wt, fwd=True, dgrad=True)
    y3 = Fn.conv_fwd(to_act(x), None, spec, wino2d_u=u2)
    y1 = Fn.conv_fwd(to_act(x[:1]), None, spec, wino2d_u=u2)
    assert torch.equal(y3[:1], y1)
    dy = rnd(n, cout, h, w, seed=13)
    d3 = Fn.conv_dgrad(to_act(dy), None, spec, (h, w), wino2d_u=ud2)
    d1 = Fn.conv_dgrad(to_act(dy[:1]), None, spec, (h, w), wino2d_u=ud2)
    assert torch.equal(d3[:1], d1)


def test_wino2d_switch_and_rule(monkeypatch):
    """Fn.WINO2D overrides the per-shape rule both ways; the rule itself names 3x3 shapes only"""
    Fn = _fn()
    s33 = Fn.ConvSpec(512, 512, (3, 3), (1, 1), (1, 1))
    s13 = Fn.ConvSpec(64, 64, (1, 3), (1, 1), (0, 1))
    monkeypatch.setattr(Fn, 'WINO2D', True)
    assert Fn.wino2d_selected(s33) and not Fn.wino2d_selected(s13)
    monkeypatch.setattr(Fn, 'WINO2D', False)
    assert not Fn.wino2d_selected(s33)
    monkeypatch.setattr(Fn, 'WINO2D', None)
    monkeypatch.setattr(Fn, '_WINO2D_ENV', None)
    assert Fn.wino2d_selected(s33) == ((512, 512) in Fn.WINO2D_SHAPES)


def test_wino2d_full_model_train_step(monkeypatch):
    """small full model, bs 2, all heads, train mode, every dense 3x3 conv on the 2-D kernel:
    outputs and parameter gradients against the oracle with the comparison and bounds of
    test_model_gpu.test_full_model_small; PackPlan's one-launch U2 == the stand-alone transforms"""
    import test_model_gpu as T
    from emsanet_amd import full_args
    from oracle.emsanet_oracle import synthetic_batch
    Fn = _fn()
    monkeypatch.setattr(Fn, 'WINO2D', True)
    fallbacks0 = Fn.WINO2D_FALLBACKS
    h, w, bs = 96, 128, 2
    args = full_args(input_height=h, input_width=w)
    model, o32, o64 = T._triple(args)
    plan = model._pack_plan
    rts2 = [rt for rt in plan.rts if rt.wino2d]
    multi2 = [m for m in plan.multi if m.wino2d]
    assert len(rts2) >= 3 and len(multi2) >= 1
    batch = synthetic_batch(bs, h, w)
    batch64 = {k: v.double() for k, v in batch.items()}
    gbatch = {k: v.to(DEV) for k, v in batch.items()}
    for m in (model, o32, o64):
        m.train(True)
        m.dropout_seed = 1234
    r32, r64, out = o32(batch), o64(batch64), model(gbatch)
    for rt in rts2:
        u2, ud2 = Fn.pack_wino2d(rt.conv.weight.detach(), fwd=True, dgrad=True)
        got_u2, got_ud2 = rt.packs.peek('wino2d', torch.float32, rt.key_now())
        assert torch.equal(got_u2, u2) and torch.equal(got_ud2, ud2)
    for m in multi2:
        s = m.spec
        got_u2, got_ud2 = m.packs.peek('wino2d', torch.float32, m.key_now())
        assert got_u2 is not None and got_ud2 is not None
        assert torch.equal(got_u2, Fn.pack_wino2d_packed(m._assemble(0, torch.float32), s.cout, s.cin,
                                                         flip=False))
        assert torch.equal(got_ud2, Fn.pack_wino2d_packed(m._assemble(1, torch.float32), s.cin, s.cout,
                                                          flip=True))
    f32, f64, fo = T._flatten(r32), T._flatten(r64), T._flatten(out)
    assert len(f32) == len(fo) == len(f64)
    for i, (a, b, c) in enumerate(zip(fo, f32, f64)):
        lim = max(T.TOL, 4 * T._rel(b, c))
        e = T._rel(a, c)
        assert e <= lim, f"train output {i}: err vs fp64 {e:.3e} > {lim:.3e}"
    T._argmax_check(fo[0], f64[0], 'semantic')
    cots = [rnd(*t.shape, seed=100 + i, scale=1e-1) for i, t in enumerate(f32)]
    torch.autograd.backward(f32, cots)
    torch.autograd.backward(f64, [c.double() for c in cots])
    torch.autograd.backward(fo, [c.to(DEV) for c in cots])
    p32, p64 = dict(o32.named_parameters()), dict(o64.named_parameters())
    # chaos yardstick: fp64 oracle again with a 1e-5 relative input perturbation
    g64 = {k: p.grad.clone() for k, p in p64.items() if p.grad is not None}
    for p in o64.parameters():
        p.grad = None
    o64.dropout_step = 0
    gen = torch.Generator().manual_seed(1)
    pert = {k: v * (1 + 1e-5 * torch.randn(v.shape, generator=gen, dtype=torch.float64))
            for k, v in batch64.items()}
    torch.autograd.backward(T._flatten(o64(pert)), [c.double() for c in cots])
    chaos = torch.tensor([(p64[k].grad - g64[k]).norm().item() / max(1e-30, g64[k].norm().item())
                          for k in g64])
    e_gpu_all, e_cpu_all, names = [], [], []
    gmax = max(g.abs().max().item() for g in g64.values())
    for k, p in model.named_parameters():
        assert p.grad is not None, f"no grad for {k}"
        assert torch.isfinite(p.grad).all(), f"non-finite grad for {k}"
        r = g64[k]
        before_bn = k.endswith(('conv1x3_1.bias', 'conv1x3_2.bias'))   # bias feeding a train-mode BN
        if before_bn or r.abs().max().item() < 1e-9 * gmax:
            continue
        den = max(1e-30, r.norm().item())
        e_gpu_all.append((p.grad.detach().cpu().double() - r).norm().item() / den)
        e_cpu_all.append((p32[k].grad.double() - r).norm().item() / den)
        names.append(k)
    eg, ec = torch.tensor(e_gpu_all), torch.tensor(e_cpu_all)
    med_g, med_c = eg.median().item(), ec.median().item()
    p95_g, p95_c = eg.quantile(0.95).item(), ec.quantile(0.95).item()
    msg = (f"rel-L2 grad error vs fp64  gpu median {med_g:.2e} p95 {p95_g:.2e} max "
           f"{eg.max().item():.2e} ({names[int(eg.argmax())]}) | cpu-fp32 median {med_c:.2e} p95 "
           f"{p95_c:.2e} max {ec.max().item():.2e} | fp64 chaos(1e-5) median "
           f"{chaos.median().item():.2e} p95 {chaos.quantile(0.95).item():.2e}")
    print(msg)
    assert med_g <= max(2e-3, 4 * med_c, 2 * chaos.median().item()), msg
    assert p95_g <= max(1e-2, 8 * p95_c, 2 * chaos.quantile(0.95).item()), msg
    assert eg.max().item() <= 0.1, msg
    assert Fn.WINO2D_FALLBACKS == fallbacks0, "a 3x3 conv of the step fell back to the row kernel"


def test_wino2d_graphed_train_step_equals_eager(monkeypatch):
    """the same step captured and replayed from GraphedTrainStep == its eager twin (learning rate 0:
    the loss bit for bit, the gradients to the atomics jitter of the other kernels)"""
    import test_model_gpu as T
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.graph import GraphedTrainStep
    from emsanet_amd.model import EMSANet
    from emsanet_amd.optim import FusedSGD
    from emsanet_amd.parallel import GradientBuckets
    from oracle.emsanet_oracle import synthetic_batch
    Fn = _fn()
    monkeypatch.setattr(Fn, 'WINO2D', True)
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
    assert sum(rt.wino2d for rt in m2._pack_plan.rts) >= 3
    g = GraphedTrainStep(m2, batches[0], b2, o2, loss_fn=loss_of, warmup=3)
    l2, _ = g.replay(batches[1])
    b3.reset()
    loss = loss_of(m3(batches[1]))
    loss.backward()
    b3.finish()
    o3.step()
    torch.cuda.synchronize()
    assert float(l2) == float(loss.detach()), (float(l2), float(loss.detach()))
    gmax = max(float(p.grad.abs().max()) for p in m3.parameters())
    for (k, p2), (_, p3) in zip(m2.named_parameters(), m3.named_parameters()):
        d = float((p2.grad - p3.grad).abs().max())
        assert d <= 1e-4 * gmax, f"grad {k}: {d:.3e} vs max {gmax:.3e}"
