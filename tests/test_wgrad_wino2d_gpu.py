"""2-D Winograd F(3x3,2x2) weight gradient of the dense 3x3 convs (csrc/conv_wgrad_wino2d.hip)
against fp64 `torch.nn.grad.conv2d_weight` and against the row form F(3,2) on the same inputs.

Bound, per case and per output (the rule of test_stem_stage_gpu for a re-ordered fp32 summation):
    err_2D <= max(2 * err_row, 1e-6 * max|reference|)
with err_row the error of the row kernel measured in the same test.  Inputs: a seeded normal x after a
ReLU, dy of magnitude 1e-3 (the benchmark's cotangents)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

# (n, h, w, cin, cout): the smallest shapes at which each mechanism can fail
SHAPES = [
    (1, 2, 2, 8, 8),          # one tile, everything else out of range
    (2, 7, 9, 96, 8),         # both sizes odd, channel tails on both sides
    (3, 15, 20, 64, 40),      # the /32 map's odd H, tiles wrapping lines and images, Cout tail
    (2, 16, 66, 128, 96),     # a tile range that ends inside a line
    (2, 34, 46, 64, 64),      # several K splits
    (3, 19, 29, 64, 64),      # 57 K steps, 8 per split: the last split is ONE step (of 2 tiles)
    (3, 3, 21, 64, 64),       # 9 K steps, 5 per split: the last split is one step SHORT
]


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _spec(cin, cout):
    return _fn().ConvSpec(cin, cout, (3, 3), (1, 1), (1, 1))


@functools.lru_cache(maxsize=None)
def _case(cfg):
    """inputs and fp64 references of one shape, computed once and shared"""
    n, h, w, cin, cout = cfg
    x = F.relu(rnd(n, cin, h, w, seed=1))
    dy = rnd(n, cout, h, w, seed=7, scale=1e-3)
    dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
    db = dy.double().sum((0, 2, 3))
    return x, dy, dw, db


def _err(got, ref):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float((got - ref).abs().max())


def _offset_view(A, shape):
    """a parameter-shaped view that starts 16 bytes into a guarded allocation (a gradient-bucket view)"""
    numel = 1
    for s in shape:
        numel *= s
    return A.alloc((numel + 4,), DEV)[4:].view(shape)


def _run(Fn, monkeypatch, on, x, dy, spec, bias, like=None, dw_out=None, db_out=None):
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', on)
    return Fn.conv_wgrad(x, dy, spec, bias, like=like, dw_out=dw_out, db_out=db_out)


def test_split_boundary_shapes_sit_where_the_launcher_splits():
    from emsanet_amd import _lib
    L = _lib.lib()
    for cfg, last in (((3, 19, 29, 64, 64), 1), ((3, 3, 21, 64, 64), -1), ((2, 34, 46, 64, 64), None)):
        n, h, w, cin, cout = cfg
        g = _spec(cin, cout).geom_fwd(n, h, w, cin, cout)
        sps = L.emsa_conv_wgrad_wino2d_split_steps(0, g)
        steps = -(-(n * ((h + 1) // 2) * ((w + 1) // 2)) // 8)
        splits = -(-steps // sps)
        assert splits >= 2
        if last is not None:
            assert steps - (splits - 1) * sps == (1 if last == 1 else sps - 1), (cfg, steps, sps)


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('cfg', SHAPES)
def test_wgrad_wino2d_against_fp64_and_row(cfg, bias, guard_allocations, monkeypatch):
    """OIHW form into an offset, 16-byte-aligned view and the packed form, with and without bias;
    two runs bit-equal; switched off == the row kernel bit for bit"""
    Fn, A = _fn(), guard_allocations
    n, h, w, cin, cout = cfg
    x, dy, dw_ref, db_ref = _case(cfg)
    spec = _spec(cin, cout)
    xa, dya = A.put(to_act(x)), A.put(to_act(dy))
    like = torch.empty(cout, cin, 3, 3, device=DEV)
    before = Fn.WGRAD_WINO2D_FALLBACKS
    # row kernel (the switch forced off): the yardstick, and what Fn.conv_wgrad ran before
    dw_r, db_r, packed = _run(Fn, monkeypatch, False, xa, dya, spec, bias, like=like)
    assert not packed
    e_row = _err(dw_r, dw_ref)
    # 2-D form, parameter layout, written in place
    tw = _offset_view(A, (cout, cin, 3, 3))
    tb = _offset_view(A, (cout,)) if bias else None
    dw2, db2, packed = _run(Fn, monkeypatch, True, xa, dya, spec, bias, like=like, dw_out=tw, db_out=tb)
    assert not packed and dw2.data_ptr() == tw.data_ptr()
    e_2d = _err(dw2, dw_ref)
    top = float(dw_ref.abs().max())
    print(f"{cfg} bias={bias} dw: 2-D {e_2d:.3e} row {e_row:.3e} max|ref| {top:.3e}")
    assert e_2d <= max(2 * e_row, 1e-6 * top), (e_2d, e_row, top)
    if bias:
        eb_row, eb_2d, btop = _err(db_r, db_ref), _err(db2, db_ref), float(db_ref.abs().max())
        print(f"{cfg} db: 2-D {eb_2d:.3e} row {eb_row:.3e} max|ref| {btop:.3e}")
        assert eb_2d <= max(2 * eb_row, 1e-6 * btop), (eb_2d, eb_row, btop)
    else:
        assert db2 is None
    # packed [tap][cout][cin] form (the merged heads' entry): the same bits
    dwp, dbp, packed = _run(Fn, monkeypatch, True, xa, dya, spec, bias)
    assert packed
    assert torch.equal(dwp.view(9, cout, cin).permute(1, 2, 0).reshape(cout, cin, 3, 3), dw2)
    assert torch.equal(Fn.unpack_wgrad(dwp, like), dw2)
    if bias:
        assert torch.equal(dbp, db2)
    # bit-reproducible
    dw3, db3, _ = _run(Fn, monkeypatch, True, xa, dya, spec, bias, like=like)
    assert torch.equal(dw3, dw2) and (not bias or torch.equal(db3, db2))
    # switched off: the row kernel again, bit for bit
    dw4, db4, _ = _run(Fn, monkeypatch, False, xa, dya, spec, bias, like=like)
    assert torch.equal(dw4, dw_r) and (not bias or torch.equal(db4, db_r))
    assert Fn.WGRAD_WINO2D_FALLBACKS == before
    A.check()


def test_wgrad_wino2d_refusals_leave_outputs_untouched(guard_allocations, monkeypatch):
    """stride 2, dilation, 16-bit storage, 1-D kernels, channel counts that are no multiple of 4:
    EMSA_E_SHAPE before any launch; Fn.conv_wgrad then runs what it ran before and counts it"""
    from emsanet_amd import _lib
    Fn, A = _fn(), guard_allocations
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n, h, w, c = 1, 8, 8, 16
    x = A.put(to_act(rnd(n, c, h, w, seed=1)))
    dy = A.put(to_act(rnd(n, c, h, w, seed=2)))
    dw = A.alloc((9 * c * c,), DEV)
    db = A.alloc((c,), DEV)
    ws = A.alloc((1 << 16,), DEV)
    ok = _spec(c, c).geom_fwd(n, h, w, c, c)
    assert L.emsa_conv_wgrad_wino2d_supported(0, ok) == 1
    dil = _spec(c, c).geom_fwd(n, h, w, c, c)
    dil.step_h = dil.step_w = 2
    dil.off_h = dil.off_w = -2
    refused = [
        (0, Fn.ConvSpec(c, c, (3, 3), (2, 2), (1, 1)).geom_fwd(n, h, w, c, c)),      # stride 2
        (0, dil),                                                                    # dilation 2
        (1, ok), (2, ok),                                                            # bf16 / fp16 storage
        (0, Fn.ConvSpec(c, c, (1, 3), (1, 1), (0, 1)).geom_fwd(n, h, w, c, c)),      # 1-D kernels
        (0, Fn.ConvSpec(c, c, (3, 1), (1, 1), (1, 0)).geom_fwd(n, h, w, c, c)),
        (0, Fn.ConvSpec(6, c, (3, 3), (1, 1), (1, 1)).geom_fwd(n, h, w, 6, c)),      # cin % 4
    ]
    for dtype, g in refused:
        assert L.emsa_conv_wgrad_wino2d_supported(dtype, g) == 0
        assert L.emsa_conv_wgrad_wino2d_ws_bytes(dtype, g) == 0
        assert L.emsa_conv_wgrad_wino2d_split_steps(dtype, g) == _lib.E_SHAPE
        for packed in (0, 1):
            assert L.emsa_conv_wgrad_wino2d(dtype, g, p(x), p(dy), p(dw), p(db), p(ws), packed,
                                            None) == _lib.E_SHAPE
    torch.cuda.synchronize()
    for t in (dw, db, ws):
        assert bool(torch.isnan(t).all())                 # the poison: nothing ran
    # a misaligned destination is refused as well
    assert L.emsa_conv_wgrad_wino2d(0, ok, p(x), p(dy), p(dw[1:]), p(db), p(ws), 0, None) == _lib.E_SHAPE
    # Fn.conv_wgrad with the switch on: a 3x3 conv the library refuses runs the row / generic path
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', True)
    monkeypatch.setattr(L, 'emsa_conv_wgrad_wino2d_supported', lambda *a: 0)
    before = Fn.WGRAD_WINO2D_FALLBACKS
    like = torch.empty(c, c, 3, 3, device=DEV)
    dw1, _, packed = Fn.conv_wgrad(x, dy, _spec(c, c), False, like=like)
    assert not packed and Fn.WGRAD_WINO2D_FALLBACKS == before + 1
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', False)
    dw0, _, _ = Fn.conv_wgrad(x, dy, _spec(c, c), False, like=like)
    assert torch.equal(dw0, dw1)
    # a 1-D conv is not selected at all: no fall-back counted
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', True)
    s13 = Fn.ConvSpec(c, c, (1, 3), (1, 1), (0, 1))
    Fn.conv_wgrad(x, dy, s13, False, like=torch.empty(c, c, 1, 3, device=DEV))
    assert Fn.WGRAD_WINO2D_FALLBACKS == before + 1
    A.check()


def test_wgrad_wino2d_switch_and_rule(monkeypatch):
    Fn = _fn()
    s33, s13 = _spec(512, 256), Fn.ConvSpec(64, 64, (1, 3), (1, 1), (0, 1))
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', True)
    assert Fn.wgrad_wino2d_selected(s33) and not Fn.wgrad_wino2d_selected(s13)
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', False)
    assert not Fn.wgrad_wino2d_selected(s33)
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', None)
    monkeypatch.setattr(Fn, '_WGRAD_WINO2D_ENV', None)
    assert Fn.wgrad_wino2d_selected(s33) == ((512, 256) in Fn.WGRAD_WINO2D_SHAPES)
    monkeypatch.setattr(Fn, '_WGRAD_WINO2D_ENV', '0')
    assert not Fn.wgrad_wino2d_selected(s33)


def _block(seed):
    """a decoder module and the two prediction heads (the merged 96->8 task convs among them).  The
    skip has the module's width: no 1x1 skip-fusion conv, whose fp32 weight gradient accumulates with
    atomics and is not bit-reproducible from run to run"""
    from emsanet_amd.decoder import DecoderModule, InstanceHead, SemanticHead
    torch.manual_seed(seed)
    mods = torch.nn.ModuleDict({
        'dec': DecoderModule(64, 128, 1, 0.0, 128),
        'sem': SemanticHead(128, 40),
        'ins': InstanceHead(128, True),
    })
    return mods.to(DEV).train()


def _block_step(Fn, monkeypatch, on):
    """-> outputs, gradients by parameter name, names of the dense 3x3 convs' parameters, and the
    (x, dy, spec, dw OIHW, db) of every dense 3x3 weight gradient of the backward pass"""
    monkeypatch.setattr(Fn, 'WGRAD_WINO2D', on)
    calls = []
    inner = Fn.conv_wgrad

    def recording(x, dy, spec, want_bias, *a, **kw):
        r = inner(x, dy, spec, want_bias, *a, **kw)
        if (spec.kh, spec.kw) == (3, 3):
            dw = r[0].view(9, spec.cout, spec.cin).permute(1, 2, 0) if r[2] else r[0]
            calls.append((x.detach().cpu(), dy.detach().cpu(), spec,
                          dw.reshape(spec.cout, spec.cin, 3, 3).detach().cpu().clone(),
                          None if r[1] is None else r[1].detach().cpu().clone()))
        return r
    monkeypatch.setattr(Fn, 'conv_wgrad', recording)
    m = _block(0)
    n, h, w = 2, 32, 48
    x = to_act(rnd(n, 64, h, w, seed=21)).requires_grad_(True)
    skip = to_act(F.relu(rnd(n, 128, 2 * h, 2 * w, seed=22)))
    y, _ = m['dec'](x, skip, lambda t: None)
    outs = [m['sem'](y), m['ins'](y)]
    cots = [rnd(*o.shape, seed=30 + i, scale=1e-3).to(DEV) for i, o in enumerate(outs)]
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    monkeypatch.setattr(Fn, 'conv_wgrad', inner)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    grads['x'] = x.grad.detach().clone()
    dense = set()
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (3, 3) and mod.groups == 1:
            dense |= {f"{name}.{k}" for k, _ in mod.named_parameters()}
    return [o.detach().clone() for o in outs], grads, dense, calls


def test_block_level_decoder_module_and_heads(monkeypatch):
    """a decoder module and the prediction heads (128->40, 128->96 and the merged 96->8 task convs),
    forward + backward at 2 x 32 x 48 (fp32, eager) with the 2-D weight gradient forced on and forced
    off: every output and every gradient except the dense 3x3 weight / bias gradients bit-equal, those
    within the rule against fp64 on the recorded operands, and no fall-back.
    A few gradients outside the dense convs are accumulated with fp32 atomics (the depthwise
    up-sampling conv's weight and bias) and differ between two runs of the SAME build; which ones is
    read from a second run with the switch off, not listed here.  For those the switch may move no
    more than a re-ordered fp32 sum does: 1e-5 of the gradient's maximum (what the issue expects of a
    re-ordered summation; the stem fusion moved 1.5e-5 of the maximum over far longer sums)"""
    Fn = _fn()
    before = Fn.WGRAD_WINO2D_FALLBACKS
    out_off, g_off, dense, c_off = _block_step(Fn, monkeypatch, False)
    _, g_off2, _, _ = _block_step(Fn, monkeypatch, False)
    out_on, g_on, _, c_on = _block_step(Fn, monkeypatch, True)
    assert Fn.WGRAD_WINO2D_FALLBACKS == before
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    assert set(g_on) == set(g_off) and len(dense & set(g_on)) >= 6
    jitter = [k for k in sorted(g_on) if k not in dense and not torch.equal(g_off[k], g_off2[k])]
    print('not bit-reproducible between two runs with the switch off:', jitter)
    assert all('.upsampling.' in k for k in jitter), jitter      # the depthwise convs' atomics only
    for k in sorted(g_on):
        if k in dense:
            continue
        if k in jitter:
            top = float(g_off[k].abs().max())
            d = float((g_on[k] - g_off[k]).abs().max())
            assert d <= 1e-5 * top, (k, d, top)
        else:
            assert torch.equal(g_on[k], g_off[k]), k
    assert len(c_on) == len(c_off) == 4
    shapes = set()
    for (x, dy, spec, dw_on, db_on), (x0, dy0, _, dw_off, db_off) in zip(c_on, c_off):
        assert torch.equal(x, x0) and torch.equal(dy, dy0)           # the same operands both times
        shapes.add((spec.cin, spec.cout))
        ref = torch.nn.grad.conv2d_weight(x.double(), (spec.cout, spec.cin, 3, 3), dy.double(), padding=1)
        e_on, e_off, top = _err(dw_on, ref), _err(dw_off, ref), float(ref.abs().max())
        print(f"{spec.cin}->{spec.cout} dw: 2-D {e_on:.3e} row {e_off:.3e} max|ref| {top:.3e}")
        assert not torch.equal(dw_on, dw_off), "the 2-D weight gradient did not run"
        assert e_on <= max(2 * e_off, 1e-6 * top), (spec.cin, spec.cout, e_on, e_off, top)
        if db_on is not None:
            rb = dy.double().sum((0, 2, 3))
            eb_on, eb_off, btop = _err(db_on, rb), _err(db_off, rb), float(rb.abs().max())
            assert eb_on <= max(2 * eb_off, 1e-6 * btop), (spec.cin, spec.cout, eb_on, eb_off, btop)
    assert shapes == {(64, 128), (128, 40), (128, 96), (96, 8)}
