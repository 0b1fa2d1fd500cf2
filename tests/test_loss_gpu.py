"""The loss kernels (csrc/loss.hip) against plain PyTorch fp64 on the CPU, at the sizes, class
counts, layouts and label patterns where such kernels go wrong: every template instantiation and
its boundaries, block counts beyond one pass of the finalize kernels, grid-strided instance
losses, strided views, labels outside 1..n_classes, confident pixels under a common logit offset.

Reference: `oracle.instance_loss_oracle.smoothed_ce` / `instance_losses` in fp64 on exactly the
fp32 values the kernel reads, evaluated per sample (or per group of samples) and combined as
sum of numerators / sum of denominators so that the batch-32 cases stay near 100 MB of fp64 at a
time.  Tolerances are those of tests/test_loss.py: loss 1e-5 relative, gradient max-abs error
<= 1e-5 * max |reference gradient| + 1e-12.  Every comparison prints its figures before it asserts.
"""
import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, to_act

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL, GRAD_ATOL = 1e-5, 1e-12


def _loss_mod():
    from emsanet_amd import loss
    return loss


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _emsa_error():
    from emsanet_amd._lib import EmsaError
    return EmsaError


def _class_weights(c, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(c, generator=g) + 0.5            # non-uniform, 0.5 .. 1.5


def _clean(t, c):
    """what the kernel promises for labels outside 0..c: exactly void"""
    t = t.long()
    return torch.where((t < 0) | (t > c), torch.zeros_like(t), t)


def _ref_ce(x, t, w, eps, gscale=1.0, den_total=None):
    """x (N,C,H,W) fp32 on the CPU, t (N,H,W) labels in 0..C -> (loss, fp64 gradient of
    gscale * loss), one sample at a time; `den_total`: the divisor of a larger batch these samples
    are part of (then the returned loss is this part's numerator / den_total)"""
    from oracle.instance_loss_oracle import smoothed_ce
    wd = w.double()
    t = t.long()
    dens = [float(wd[ti[ti > 0] - 1].sum()) for ti in t]
    den = sum(dens) if den_total is None else den_total
    num, grads = 0.0, []
    for xi, ti, di in zip(x, t, dens):
        if di == 0.0:
            grads.append(torch.zeros(xi.shape, dtype=torch.float64))
            continue
        xr = xi[None].double().requires_grad_(True)
        li = smoothed_ce(xr, ti[None], wd, eps)
        num += float(li.detach()) * di
        (li * (gscale * di / den)).backward()
        grads.append(xr.grad[0])
    return (num / den if den > 0 else 0.0), torch.stack(grads)


def _check_loss(got, ref, what):
    got, ref = float(got), float(ref)
    rel = abs(got - ref) / abs(ref) if ref != 0.0 else abs(got)
    print(f"{what}: loss {got:.9e} ref {ref:.9e} rel err {rel:.2e}")
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), (what, got, ref, rel)
    return rel


def _check_grad(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, mag = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: grad max err {err:.2e} max |ref| {mag:.2e} ratio {err / mag if mag else 0:.2e}")
    assert err <= GRAD_RTOL * mag + GRAD_ATOL, (what, err, mag)


def _ce(x_dev, t_dev, w, eps, gscale=1.0):
    """-> (loss tensor, gradient of gscale * loss) through CrossEntropyLossSemantic"""
    crit = _loss_mod().CrossEntropyLossSemantic(w, label_smoothing=eps).to(DEV)
    x_dev.grad = None
    l = crit([x_dev], [t_dev])[0][0]
    (gscale * l).backward()
    return l.detach(), x_dev.grad


SHAPES = {1: (1, 1, 1), 255: (1, 15, 17), 256: (1, 16, 16), 257: (1, 1, 257), 2460: (2, 30, 41)}


def _ce_case(c, shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * 3
    t = torch.randint(0, c + 1, (n, h, w), generator=g)
    t.view(-1)[0] = c                       # at least one labelled pixel, of the last class
    return x, t


# ---- 1. every dispatch path -------------------------------------------------------------------

@pytest.mark.parametrize('layout', ['act', 'nchw'])
@pytest.mark.parametrize('pixels', sorted(SHAPES))
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('c', [2, 3, 10, 16, 17, 37, 40, 41, 64])
def test_ce_every_dispatch_path(c, eps, pixels, layout):
    """<4> serves 1..16 classes, <10> 17..40, <16> 41..64; class counts off the multiples of 4
    exercise the `c < n_classes` guards; 255 / 256 / 257 pixels the partial last block"""
    x, t = _ce_case(c, SHAPES[pixels], seed=c * 1000 + pixels)
    w = _class_weights(c)
    xd = (to_act(x) if layout == 'act' else x.to(DEV)).requires_grad_(True)
    l, gx = _ce(xd, t.to(DEV), w, eps, gscale=2.5)
    ref, gref = _ref_ce(x, t, w, eps, gscale=2.5)
    what = f"ce c={c} eps={eps} px={pixels} {layout}"
    _check_loss(l, ref, what)
    assert gx.shape[1] == c and gx.shape == x.shape
    _check_grad(gx, gref, what)


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('c', [3, 10, 37, 41])
def test_ce_backward_pad_channels_are_zero(c, eps):
    """the gradient's rows are pad4(c) wide (the first c channels are what autograd sees): the pad
    channels must be written, with zeros, and nothing beyond them -- a poisoned buffer shows all"""
    from emsanet_amd import _lib
    Fn, L = _fn(), _lib.lib()
    x, t = _ce_case(c, SHAPES[2460], seed=c)
    w = _class_weights(c)
    n, _, h, wd = x.shape
    pixels, cp = n * h * wd, Fn.pad4(c)
    ld = cp + 8                             # both buffers are slices of wider rows
    xp = torch.full((pixels, ld), float('nan'))
    xp[:, :c] = x.permute(0, 2, 3, 1).reshape(pixels, c)
    xp, td, wdev = xp.to(DEV), t.reshape(-1).to(DEV), w.to(DEV)
    partial = torch.empty(2 * L.emsa_ce_semantic_blocks(pixels), device=DEV)
    out = torch.empty(2, device=DEV)
    g = torch.tensor([2.5], device=DEV)
    d = torch.full((pixels, ld), float('nan'), device=DEV)
    ws = float(w.double().sum())
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.emsa_ce_semantic_fwd(xp.data_ptr(), ld, td.data_ptr(), wdev.data_ptr(), c, pixels,
                                      eps, ws, partial.data_ptr(), out.data_ptr(), st), 'fwd')
    _lib.check(L.emsa_ce_semantic_bwd(xp.data_ptr(), ld, td.data_ptr(), wdev.data_ptr(), c, pixels,
                                      eps, ws, out.data_ptr(), g.data_ptr(), d.data_ptr(), ld, st),
               'bwd')
    torch.cuda.synchronize()
    ref, gref = _ref_ce(x, t, w, eps, gscale=2.5)
    _check_loss(out[0], ref, f"raw ce c={c}")
    assert cp > c and torch.equal(d[:, c:cp].cpu(), torch.zeros(pixels, cp - c))
    assert torch.isnan(d[:, cp:]).all(), "channels beyond the padded class count are not the kernel's"
    _check_grad(d[:, :c].cpu().reshape(n, h, wd, c).permute(0, 3, 1, 2), gref, f"raw ce c={c}")


# ---- 2. channel slices of a wider tensor ------------------------------------------------------

@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('lo,c', [(0, 10), (0, 40), (3, 10), (5, 40), (4, 37)])
def test_ce_on_channel_slice_of_wider_tensor(lo, c, eps):
    """pixel stride 64 > padded class count; a slice that starts off a 16-byte boundary (lo = 3, 5)
    either matches or is refused, never a different number; nothing outside the slice is touched"""
    g = torch.Generator().manual_seed(lo * 100 + c)
    full = torch.randn(2, 64, 30, 41, generator=g) * 3
    t = torch.randint(0, c + 1, (2, 30, 41), generator=g)
    w = _class_weights(c)
    wide = to_act(full).requires_grad_(True)
    before = wide.detach().clone()
    xs = wide[:, lo:lo + c]
    assert _fn().ld_of(xs) == 64
    crit = _loss_mod().CrossEntropyLossSemantic(w, label_smoothing=eps).to(DEV)
    try:
        l = crit([xs], [t.to(DEV)])[0][0]
    except _emsa_error():
        assert lo % 4, "an aligned slice must be served"
        return
    (2.5 * l).backward()
    ref, gref = _ref_ce(full[:, lo:lo + c], t, w, eps, gscale=2.5)
    what = f"ce slice [{lo}:{lo + c}] of 64"
    _check_loss(l, ref, what)
    _check_grad(wide.grad[:, lo:lo + c], gref, what)
    outside = torch.cat([wide.grad[:, :lo], wide.grad[:, lo + c:]], 1)
    assert float(outside.abs().max()) == 0.0
    assert torch.equal(wide.detach(), before)


# ---- 3. training size -------------------------------------------------------------------------

@pytest.mark.parametrize('n,eps', [(4, 0.1), (32, 0.0)])
def test_ce_at_training_size(n, eps):
    """4 and 32 x 40 x 480 x 640 (the latter is what `bench.py --losses` runs): 4,800 / 38,400
    partial sums, so every thread of the finalize kernel strides; bit-identical when repeated"""
    from emsanet_amd import _lib
    Fn = _fn()
    c, h, w = 40, 480, 640
    assert _lib.lib().emsa_ce_semantic_blocks(n * h * w) > 256
    wts = _class_weights(c)
    xg = Fn.act_empty(n, c, h, w, DEV)
    ts = torch.empty(n, h, w, dtype=torch.uint8)
    for i in range(n):                       # one sample at a time on the host
        g = torch.Generator().manual_seed(1000 + i)
        xg.permute(0, 2, 3, 1)[i].copy_(torch.randn(h, w, c, generator=g) * 3)
        ts[i] = torch.randint(0, c + 1, (h, w), generator=g).to(torch.uint8)
    xg.requires_grad_(True)
    tg = ts.to(DEV)
    l1, g1 = _ce(xg, tg, wts, eps)
    l2, g2 = _ce(xg, tg, wts, eps)
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "fixed-order reductions: bit-identical"
    del g2
    wd = wts.double()
    den = sum(float(wd[ti[ti > 0].long() - 1].sum()) for ti in ts)
    loss = 0.0
    for i in range(n):
        xi = xg[i:i + 1].detach().cpu()
        part, gref = _ref_ce(xi, ts[i:i + 1], wts, eps, den_total=den)
        loss += part
        _check_grad(g1[i:i + 1], gref, f"ce {n}x40x480x640 sample {i}")
    _check_loss(l1, loss, f"ce {n}x40x480x640 eps={eps}")


# ---- 4. label edges ---------------------------------------------------------------------------

@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('kind', ['uint8', 'int32', 'int64', 'view'])
def test_ce_target_types_and_labels_outside_the_classes(kind, eps):
    """labels above n_classes and negative labels behave exactly like void"""
    c = 37
    x, t = _ce_case(c, SHAPES[2460], seed=11)
    g = torch.Generator().manual_seed(12)
    odd = torch.rand(t.shape, generator=g)
    t[odd < 0.10] = c + 1
    t[(odd >= 0.10) & (odd < 0.15)] = 255
    if kind != 'uint8':
        t[(odd >= 0.15) & (odd < 0.20)] = -1
        t[(odd >= 0.20) & (odd < 0.25)] = -100
        t[(odd >= 0.25) & (odd < 0.27)] = 2 ** 31 - 1
    if kind == 'view':
        big = torch.zeros(2, 30, 82, dtype=torch.int32)
        big[:, :, ::2] = t.to(torch.int32)
        big[:, :, 1::2] = 5
        td = big.to(DEV)[:, :, ::2]
        assert not td.is_contiguous()
    else:
        td = t.to(getattr(torch, kind)).to(DEV)
    w = _class_weights(c)
    xd = to_act(x).requires_grad_(True)
    l, gx = _ce(xd, td, w, eps, gscale=2.5)
    tc = _clean(t, c)
    assert int((tc != t).sum()) > 100
    ref, gref = _ref_ce(x, tc, w, eps, gscale=2.5)
    what = f"ce labels {kind} eps={eps}"
    _check_loss(l, ref, what)
    _check_grad(gx, gref, what)
    rows = gx.cpu().permute(0, 2, 3, 1)[tc == 0]
    assert rows.shape[0] > 100 and float(rows.abs().max()) == 0.0


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('fill', [0, 255, -3])
def test_ce_all_pixels_void(fill, eps):
    x, t = _ce_case(40, SHAPES[2460], seed=13)
    t.fill_(fill)
    xd = to_act(x).requires_grad_(True)
    l, gx = _ce(xd, t.to(DEV), _class_weights(40), eps)
    assert float(l) == 0.0
    assert float(gx.abs().max()) == 0.0


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('k', [1, 300])
def test_ce_single_labelled_pixel_in_last_partial_block(k, eps):
    """pixel 256 k + 3 of 256 k + 5: the last block holds 5 pixels; with k = 300 its partial sum is
    the 301st, beyond the first pass of the finalize kernel"""
    c, pixels = 40, 256 * k + 5
    g = torch.Generator().manual_seed(k)
    x = torch.randn(1, c, 1, pixels, generator=g) * 3
    t = torch.zeros(1, 1, pixels, dtype=torch.long)
    t[0, 0, 256 * k + 3] = 17
    w = _class_weights(c)
    xd = to_act(x).requires_grad_(True)
    l, gx = _ce(xd, t.to(DEV), w, eps, gscale=2.5)
    ref, gref = _ref_ce(x, t, w, eps, gscale=2.5)
    assert ref > 0.0
    _check_loss(l, ref, f"ce single pixel k={k}")
    _check_grad(gx, gref, f"ce single pixel k={k}")
    gx = gx.cpu()
    gx[0, :, 0, 256 * k + 3] = 0.0
    assert float(gx.abs().max()) == 0.0


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('n,void', [(1, False), (257, False), (6, True), (257, True)])
def test_scene_head_batch_sizes_and_void(n, void, eps):
    from oracle.instance_loss_oracle import smoothed_ce
    g = torch.Generator().manual_seed(n)
    xs = torch.randn(n, 10, generator=g) * 2
    ts = torch.zeros(n, dtype=torch.long) if void else torch.randint(0, 11, (n,), generator=g)
    if not void:
        ts[0] = 10
    xd = xs.to(DEV).requires_grad_(True)
    l = _loss_mod().CrossEntropyLossScene(10, label_smoothing=eps).to(DEV)(xd, ts.to(DEV))
    l.backward()
    if void:
        assert float(l) == 0.0 and float(xd.grad.abs().max()) == 0.0
        return
    xr = xs.double().requires_grad_(True)
    ref = smoothed_ce(xr, ts, torch.ones(10, dtype=torch.float64), eps)
    ref.backward()
    _check_loss(l, ref, f"scene n={n}")
    assert xd.grad.shape == (n, 10)
    _check_grad(xd.grad, xr.grad, f"scene n={n}")
    assert float(xd.grad[(ts == 0).to(DEV)].abs().sum()) == 0.0


# ---- 5. shift invariance, confident pixels ----------------------------------------------------

OFFSETS = (100.0, -100.0, 30.0, -30.0, 0.0)


def _confident_case(labelled, seed):
    """a 4 x 5 image whose first `labelled` pixels carry a label; the label's logit leads every
    other class by 12 .. 14; pixel p gets the common offset OFFSETS[p % 5]"""
    c, pixels = 40, 20
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(pixels, c, generator=g) * 3
    cls = torch.randint(0, c, (pixels,), generator=g)
    idx = torch.arange(pixels)
    x[idx, cls] = -1e9
    x[idx, cls] = x.max(1).values + 12 + 2 * torch.rand(pixels, generator=g)
    x = x + torch.tensor(OFFSETS)[idx % 5][:, None]
    t = torch.zeros(pixels, dtype=torch.long)
    t[:labelled] = cls[:labelled] + 1
    others = x.clone()
    others[idx, cls] = -float('inf')
    assert float((x[idx, cls] - others.max(1).values).min()) >= 12.0 - 1e-4
    return x.t().reshape(1, c, 4, 5).contiguous(), t.reshape(1, 4, 5)


def _ce_fp32_log1p(x, t, w, eps):
    """cross-entropy in fp32 throughout, written so that no step cancels:
    -log p_c = (m - x_c) + log1p(sum of the other classes' exp(x - m))"""
    n, c = x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
    xs, tt = x.permute(0, 2, 3, 1).reshape(n, c), t.reshape(n)
    m, am = xs.max(1)
    e = torch.exp(xs - m[:, None])
    e[torch.arange(n), am] = 0.0
    nlp = (m[:, None] - xs) + torch.log1p(e.sum(1))[:, None]
    valid = tt > 0
    ti = (tt - 1).clamp(min=0)
    per = (1 - eps) * w[ti] * nlp[torch.arange(n), ti] + eps / c * (nlp * w[None]).sum(1)
    return (per * valid).sum() / (w[ti] * valid).sum()


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('labelled', [1, 4, 16])
def test_ce_confident_pixels_under_common_offsets(labelled, eps):
    """Loss ~ 1e-5 (eps 0) on logits near +-100: a formula that forms log-sum-exp + max and then
    subtracts the label's logit keeps none of it, and 1/s - 1 keeps nothing of the gradient.

    The inputs are checked first, on the CPU and in fp32: with eps 0.1 torch's own fp32
    F.cross_entropy is inside the tolerance.  With eps 0 it is NOT, on any input that meets
    'leads by >= 12': the loss is then <= log(1 + 39 e^-12) = 2.4e-4, which torch takes as the
    log of a sum rounded to 6e-8 (measured 3e-4 .. 2e-2 relative on these inputs; this is printed).
    There the check that the inputs can be served in fp32 is the cancellation-free form above."""
    import torch.nn.functional as F
    x, t = _confident_case(labelled, seed=labelled)
    w = _class_weights(40)
    ref, gref = _ref_ce(x, t, w, eps, gscale=2.5)
    f32 = float(F.cross_entropy(x, t - 1, weight=w, ignore_index=-1, label_smoothing=eps))
    safe = float(_ce_fp32_log1p(x, t, w, eps))
    print(f"inputs, fp32 on the CPU: F.cross_entropy rel err {abs(f32 - ref) / ref:.2e}, "
          f"cancellation-free form {abs(safe - ref) / ref:.2e} (loss {ref:.3e})")
    if eps:
        assert abs(f32 - ref) <= LOSS_RTOL * ref
    assert abs(safe - ref) <= LOSS_RTOL * ref
    xd = to_act(x).requires_grad_(True)
    l, gx = _ce(xd, t.to(DEV), w, eps, gscale=2.5)
    what = f"ce confident labelled={labelled} eps={eps}"
    _check_loss(l, ref, what)
    _check_grad(gx, gref, what)


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_ce_ordinary_logits_under_offset_1e4(sign, eps):
    x, t = _ce_case(40, SHAPES[2460], seed=21)
    x = x + sign * 1e4
    w = _class_weights(40)
    xd = to_act(x).requires_grad_(True)
    l, gx = _ce(xd, t.to(DEV), w, eps, gscale=2.5)
    ref, gref = _ref_ce(x, t, w, eps, gscale=2.5)
    _check_loss(l, ref, f"ce offset {sign * 1e4:+.0e}")
    _check_grad(gx, gref, f"ce offset {sign * 1e4:+.0e}")


# ---- 6. / 7. instance losses ------------------------------------------------------------------

WTS = {'instance_center': 6.0, 'instance_offset': 3.0, 'instance_orientation': 0.5}


def _inst_case(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    return dict(center=r(n, 1, h, w), offset=r(n, 2, h, w) * 2 - 1,
                orient=torch.randn(n, 2, h, w, generator=g), cgt=r(n, 1, h, w) ** 4,
                ogt=r(n, 2, h, w) * 2 - 1, rgt=(r(n, h, w) * 2 - 1) * 3.14159,
                fg=r(n, h, w) > 0.6, fgo=r(n, h, w) > 0.8, cm=r(n, h, w) > 0.1)


def _ref_inst(d, with_o, with_cm, group=4):
    """fp64 oracle over groups of samples: losses as sum of numerators / sum of denominators,
    gradients of sum_k WTS[k] * loss_k"""
    from oracle.instance_loss_oracle import instance_losses
    n = d['center'].shape[0]
    keys = ['instance_center', 'instance_offset'] + (['instance_orientation'] if with_o else [])

    def dens(s):
        px = d['cgt'][s].numel()
        return {'instance_center': float(d['cm'][s].sum()) if with_cm else float(px),
                'instance_offset': 2.0 * float(d['fg'][s].sum()),
                'instance_orientation': float(d['fgo'][s].sum())}
    total = dens(slice(0, n))
    num = {k: 0.0 for k in keys}
    grads = [[], [], []]
    for i in range(0, n, group):
        s = slice(i, min(n, i + group))
        part = dens(s)
        preds = [d[k][s].double().requires_grad_(True) for k in ('center', 'offset', 'orient')]
        out = instance_losses(preds[0], preds[1], preds[2] if with_o else None, d['cgt'][s].double(),
                              d['ogt'][s].double(), d['fg'][s], d['rgt'][s].double(), d['fgo'][s],
                              center_mask=d['cm'][s] if with_cm else None, kappa=1.0)
        obj = 0.0
        for k in keys:
            num[k] += float(out[k]) * part[k]
            if total[k] > 0:
                obj = obj + out[k] * (WTS[k] * part[k] / total[k])
        obj.backward()
        for lst, p in zip(grads, preds):
            lst.append(p.grad if p.grad is not None else torch.zeros_like(p))
    losses = {k: (num[k] / total[k] if total[k] > 0 else 0.0) for k in keys}
    return losses, [torch.cat(g) for g in grads[:3 if with_o else 2]]


def _run_inst(preds, d, with_o, with_cm):
    """preds: device tensors (leaves or views of one) -> dict of detached losses; gradients of
    sum_k WTS[k] * loss_k are left on the leaves"""
    crit = _loss_mod().InstanceLosses(kappa=1.0)
    got = crit(preds[0], preds[1], preds[2] if with_o else None, d['cgt'].to(DEV), d['ogt'].to(DEV),
               d['fg'].to(DEV), d['rgt'].to(DEV) if with_o else None,
               d['fgo'].to(DEV) if with_o else None,
               center_mask=d['cm'].to(DEV) if with_cm else None)
    sum(WTS[k] * v for k, v in got.items()).backward()
    return {k: v.detach().clone() for k, v in got.items()}


def _inst_twice_vs_oracle(d, with_o, with_cm, what):
    preds = [to_act(d[k]).requires_grad_(True) for k in ('center', 'offset', 'orient')]
    got = _run_inst(preds, d, with_o, with_cm)
    g1 = [p.grad for p in preds]
    for p in preds:
        p.grad = None
    again = _run_inst(preds, d, with_o, with_cm)
    ref, gref = _ref_inst(d, with_o, with_cm)
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k], again[k]), k
        if ref[k] == 0.0:
            assert float(got[k]) == 0.0, k
        else:
            _check_loss(got[k], ref[k], f"{what} {k}")
    for a, b, p, name in zip(g1, gref, preds, ('center', 'offset', 'orientation')):
        assert torch.equal(a, p.grad), name
        _check_grad(a, b, f"{what} d_{name}")
    assert with_o or g1[2] is None
    return got, g1


@pytest.mark.parametrize('with_cm', [True, False])
@pytest.mark.parametrize('with_o', [True, False])
@pytest.mark.parametrize('n', [4, 32])
def test_instance_losses_at_training_size(n, with_o, with_cm):
    """more than 2048 x 256 pixels: both kernels grid-stride (19 pixels per thread at batch 32)
    and the finalize kernel strides its 2048 partial sums 32 times"""
    from emsanet_amd import _lib
    h, w = 480, 640
    assert n * h * w > 524288 and _lib.lib().emsa_instance_loss_blocks(n * h * w) == 2048
    d = _inst_case(n, h, w, seed=n)
    _inst_twice_vs_oracle(d, with_o, with_cm, f"inst {n}x480x640 o={with_o} cm={with_cm}")


def test_instance_losses_foreground_only_beyond_first_grid_stride():
    """the only foreground lies in the last 1,000 pixels of the last sample"""
    n, h, w = 4, 480, 640
    d = _inst_case(n, h, w, seed=5)
    for k in ('fg', 'fgo'):
        flat = d[k].view(-1)
        flat[:-1000] = False
        flat[-1000:] = True
    assert n * h * w - 1000 > 524288
    got, grads = _inst_twice_vs_oracle(d, True, True, "inst last-1000 foreground")
    assert float(got['instance_offset']) > 0 and float(got['instance_orientation']) > 0
    go = grads[1].cpu().permute(0, 2, 3, 1).reshape(-1, 2)
    assert float(go[:-1000].abs().max()) == 0.0 and float(go[-1000:].abs().min()) > 0.0


def test_instance_losses_all_zero_center_mask():
    """centre loss 0 with a zero gradient; offset and orientation exactly as without a mask"""
    d = _inst_case(4, 480, 640, seed=6)
    base, gbase = _inst_twice_vs_oracle(d, True, False, "inst no mask")
    d['cm'] = torch.zeros_like(d['cm'])
    got, grads = _inst_twice_vs_oracle(d, True, True, "inst zero mask")
    assert float(got['instance_center']) == 0.0 and float(grads[0].abs().max()) == 0.0
    for k in ('instance_offset', 'instance_orientation'):
        assert torch.equal(got[k], base[k]), k
    assert torch.equal(grads[1], gbase[1]) and torch.equal(grads[2], gbase[2])


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 15, 17), (1, 1, 257), (2, 24, 40)])
def test_instance_losses_on_strided_views_with_gradients(shape):
    """the instance head's channel slices of one 8-wide NHWC tensor (pixel stride 8), gradients
    included; a (0, 0) orientation prediction inside the orientation foreground"""
    n, h, w = shape
    Fn = _fn()
    d = _inst_case(n, h, w, seed=h * w)
    zero_px = (n - 1, h - 1, w // 2)
    d['orient'][zero_px[0], :, zero_px[1], zero_px[2]] = 0.0
    d['fgo'][zero_px] = True
    d['fg'][0, 0, 0] = True
    filler = torch.randn(n, 3, h, w)
    wide = Fn.act_empty(n, 8, h, w, DEV)
    wide.copy_(torch.cat([d['center'], d['offset'], d['orient'], filler], 1).to(DEV))
    wide.requires_grad_(True)
    before = wide.detach().clone()
    preds = [wide[:, 0:1], wide[:, 1:3], wide[:, 3:5]]
    if h * w > 1:
        assert Fn.ld_of(preds[1]) == 8
    got = _run_inst(preds, d, True, True)
    ref, gref = _ref_inst(d, True, True)
    for k in ref:
        _check_loss(got[k], ref[k], f"inst ld=8 {shape} {k}")
    gw = wide.grad.cpu()
    assert torch.isfinite(gw).all()
    assert float(gw[:, 5:].abs().max()) == 0.0, "channels outside the slices receive nothing"
    assert torch.equal(wide.detach(), before)
    _check_grad(gw[:, 0:1], gref[0], f"inst ld=8 {shape} d_center")
    _check_grad(gw[:, 1:3], gref[1], f"inst ld=8 {shape} d_offset")
    # the (0, 0) pixel's gradient is 1e6 x the others' (the clamp's 1 / sqrt(1e-12)): it is held to
    # the oracle on its own so that it does not set the scale for every other pixel
    z = (zero_px[0], slice(None), zero_px[1], zero_px[2])
    gz, rz = gw[:, 3:5][z].double(), gref[2][z]
    assert torch.isfinite(gz).all()
    assert float((gz - rz).abs().max()) <= GRAD_RTOL * float(rz.abs().max()) + GRAD_ATOL
    gr, rr = gw[:, 3:5].clone(), gref[2].clone()
    gr[z], rr[z] = 0.0, 0.0
    _check_grad(gr, rr, f"inst ld=8 {shape} d_orientation")


# ---- 8. refusals ------------------------------------------------------------------------------

def test_refusals():
    """none of these may return a number"""
    L, E = _loss_mod(), _emsa_error()
    x = to_act(torch.randn(1, 65, 4, 4))
    with pytest.raises(E):
        L.CrossEntropyLossSemantic(torch.ones(65)).to(DEV)([x], [torch.ones(1, 4, 4).long().to(DEV)])
    x = to_act(torch.randn(2, 40, 4, 4))
    crit = L.CrossEntropyLossSemantic(torch.ones(40)).to(DEV)
    for bad in ((2, 4, 3), (1, 4, 4), (2, 4, 5)):
        with pytest.raises(E):
            crit([x], [torch.ones(bad).long().to(DEV)])
    d = {k: v.to(DEV) for k, v in _inst_case(2, 6, 8, seed=1).items()}
    inst = L.InstanceLosses()
    ok = dict(center=d['center'], offset=d['offset'], orientation=d['orient'], center_gt=d['cgt'],
              offset_gt=d['ogt'], foreground=d['fg'], orientation_gt=d['rgt'],
              orientation_foreground=d['fgo'], center_mask=d['cm'])
    assert set(inst(**ok)) == set(WTS)
    for key in ('center_gt', 'offset_gt', 'foreground', 'orientation_gt', 'orientation_foreground',
                'center_mask', 'offset', 'orientation'):
        with pytest.raises(E):
            inst(**dict(ok, **{key: ok[key][:1]}))
