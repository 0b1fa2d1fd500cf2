"""GPU: the tile-and-step-major U of the 1-D Winograd convs (conv_wino.hip, `wino_u_tiled` in
common.h): `[n/64][K/16][4][64][16]` where R = 1, n % 64 == 0 and K % 16 == 0, `[4][n][R*K]` everywhere
else.  `emsa_wino_set_u_tiled(0)` restores the second layout for every shape and is the reference here.

  pack    the tiled operand is a permutation of the classic one, bit for bit, from all three writers
          (emsa_pack_wino, emsa_pack_wino_packed, kind 1 of emsa_pack_batch), forward and data gradient;
          shapes the rule does not take pack the same bits either way
  conv    2x5x7 (odd lines, 40 / 42 pairs = one full and one partial pixel tile), along W and along H,
          forward and data gradient: switch on == switch off bit for bit (same operands, same summation
          order), both within 1e-4 * max|ref| of the fp64 convolution

A channel case K->n names the LAUNCH's GEMM K and its output channels: the forward launch of a conv with
c_in = K, c_out = n, and the data-gradient launch of a conv with c_out = K, c_in = n -- the rule looks at
each side's own (n, K), and only so do both directions take the tiled layout in every case."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import guard
from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = [(1, 3), (3, 1)]
TILED = [(64, 16), (64, 32), (128, 80), (192, 64)]             # (n, K)
#         K -> n:  one K step, one tile | both halves of a line | five steps, second tile's base |
#                  three tiles | eight steps
CONV = [(16, 64), (32, 64), (80, 128), (64, 192), (128, 64)]
NHW = (2, 5, 7)


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _lib():
    from emsanet_amd import _lib as lib
    return lib.lib()


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = _lib().emsa_wino_set_u_tiled(1)
    yield
    _lib().emsa_wino_set_u_tiled(prev)


def _with_switch(on, fn):
    L = _lib()
    prev = L.emsa_wino_set_u_tiled(on)
    try:
        return fn()
    finally:
        L.emsa_wino_set_u_tiled(prev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == torch.float32:
        a, b = _bits(a), _bits(b)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


# ---- the three writers: (u forward, u data gradient) of one OIHW weight ---------------------------
def _w_pack_wino(wt):
    return _fn().pack_wino(wt, fwd=True, dgrad=True)


def _w_packed(wt):
    Fn = _fn()
    cout, cin, kh, kw = wt.shape
    rows = 3 if (kh, kw) == (3, 3) else 1
    return (Fn.pack_wino_packed(guard.put(Fn.pack_weight(wt, 'fwd')), cout, cin, rows, flip=False),
            Fn.pack_wino_packed(guard.put(Fn.pack_weight(wt, 'dgrad')), cin, cout, rows, flip=True))


def _w_batch(wt):
    from emsanet_amd import _lib as lib
    Fn = _fn()
    cout, cin, kh, kw = wt.shape
    rows = 3 if (kh, kw) == (3, 3) else 1
    u, ud = Fn._empty((4 * rows * cout * cin,), wt.device), Fn._empty((4 * rows * cout * cin,), wt.device)
    jobs = (lib.EmsaPackJob * 1)(lib.EmsaPackJob(wt.data_ptr(), u.data_ptr(), ud.data_ptr(), cout, cin, kh,
                                                 kw, lib.PACK_WINO, 0, 0, 0, 0, 0))
    raw = guard.put(torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(wt.device))
    blocks = max(1, min(64, (cout * cin * kh * kw + 2047) // 2048))
    Fn.check(lib.lib().emsa_pack_batch(raw.data_ptr(), 1, blocks, Fn._stream()), 'emsa_pack_batch')
    torch.cuda.synchronize()
    return u, ud


WRITERS = {'pack_wino': _w_pack_wino, 'pack_wino_packed': _w_packed, 'pack_batch': _w_batch}


def _tiled_view(classic, n, k):
    return classic.view(4, n // 64, 64, k // 16, 16).permute(1, 3, 0, 2, 4).reshape(-1)


@pytest.mark.parametrize('writer', list(WRITERS))
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('n,k', TILED)
def test_tiled_pack_is_a_permutation_of_the_classic_pack(n, k, kernel, writer):
    """forward operand of the conv k->n and data-gradient operand of the conv n->k: both have n rows of
    k columns"""
    pack = WRITERS[writer]
    w_f = guard.put(rnd(n, k, *kernel, seed=2, scale=0.1).to(DEV))       # c_out = n, c_in = k
    w_d = guard.put(rnd(k, n, *kernel, seed=3, scale=0.1).to(DEV))       # c_out = k, c_in = n
    for side, wt in ((0, w_f), (1, w_d)):
        classic = _with_switch(0, lambda: pack(wt))[side]
        tiled = _with_switch(1, lambda: pack(wt))[side]
        assert torch.isfinite(tiled).all()
        _same_bits(tiled, _tiled_view(classic, n, k), f"{writer} side {side} n={n} k={k}")
        assert (n, k) == (64, 16) or not torch.equal(tiled, classic)      # (one block: the same order)


@pytest.mark.parametrize('writer', list(WRITERS))
@pytest.mark.parametrize('n,k,kernel', [(64, 24, (1, 3)), (40, 64, (3, 1)), (96, 64, (1, 3)),
                                        (64, 64, (3, 3))])
def test_other_shapes_keep_their_layout(n, k, kernel, writer):
    """a channel tail, an n below 64, an n that is no multiple of 64, the three-row form"""
    pack = WRITERS[writer]
    w_f = guard.put(rnd(n, k, *kernel, seed=2, scale=0.1).to(DEV))
    w_d = guard.put(rnd(k, n, *kernel, seed=3, scale=0.1).to(DEV))
    for side, wt in ((0, w_f), (1, w_d)):
        classic = _with_switch(0, lambda: pack(wt))[side]
        same = _with_switch(1, lambda: pack(wt))[side]
        assert torch.isfinite(same).all()
        _same_bits(same, classic, f"{writer} side {side} n={n} k={k} {kernel}")


# ---- convolution ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(k, n, kernel, dgrad):
    """operands and fp64 reference of the launch K = k -> n (see the module docstring), made once"""
    Fn = _fn()
    b, h, w = NHW
    pad = (kernel[0] // 2, kernel[1] // 2)
    if dgrad:
        spec = Fn.ConvSpec(n, k, kernel, (1, 1), pad)
        wt, x = rnd(k, n, *kernel, seed=2, scale=0.1), rnd(b, k, h, w, seed=3)
        ref = F.conv_transpose2d(x.double(), wt.double(), padding=pad)
    else:
        spec = Fn.ConvSpec(k, n, kernel, (1, 1), pad)
        wt, x = rnd(n, k, *kernel, seed=2, scale=0.1), rnd(b, k, h, w, seed=1)
        ref = F.conv2d(x.double(), wt.double(), padding=pad)
    return dict(spec=spec, wt=wt.to(DEV), x=to_act(x), x_cpu=x, wt_cpu=wt, ref=ref, pad=pad)


def _on_off(run, wt, dgrad):
    """run(u) with U packed and read under the switch off, then on -> (off, on), flat tensor lists"""
    def go():
        u = _fn().pack_wino(guard.put(wt), fwd=not dgrad, dgrad=dgrad)[1 if dgrad else 0]
        res = run(u)
        res = res if isinstance(res, (tuple, list)) else (res,)
        torch.cuda.synchronize()
        return [r.clone() for r in res if torch.is_tensor(r)]
    off = _with_switch(0, go)
    on = _with_switch(1, go)
    assert len(off) == len(on) >= 1
    for a, b in zip(off, on):
        _same_bits(b, a, 'switch on vs off')
    return off, on


def _within(got, ref, what):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err, lim = (got - ref).abs().max().item(), 1e-4 * ref.abs().max().item()
    print(f"{what}: max abs err {err:.3e}, bound {lim:.3e}")
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


@pytest.mark.parametrize('dgrad', [False, True], ids=['fwd', 'dgrad'])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('k,n', CONV)
def test_conv_equals_the_classic_layout_and_fp64(k, n, kernel, dgrad):
    Fn, d = _fn(), _case(k, n, kernel, dgrad)
    if dgrad:
        run = lambda u: Fn.conv_dgrad(guard.put(d['x']), None, d['spec'], NHW[1:], wino_u=u)   # noqa: E731
    else:
        run = lambda u: Fn.conv_fwd(guard.put(d['x']), None, d['spec'], wino_u=u)              # noqa: E731
    off, on = _on_off(run, d['wt'], dgrad)
    _within(off[0], d['ref'], 'classic U')
    _within(on[0], d['ref'], 'tiled U')


@pytest.mark.parametrize('kernel', KERNELS)
def test_conv_with_the_input_batchnorm_folded_in(kernel):
    """INBN, forward 80->128: relu(x * scale + shift) formed in the loader"""
    Fn, d = _fn(), _case(80, 128, kernel, False)
    sc, sh = rnd(80, seed=7).abs() + 0.5, rnd(80, seed=8) + 0.3
    bias = rnd(128, seed=6)
    a = torch.relu(d['x_cpu'].double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    ref = F.conv2d(a, d['wt_cpu'].double(), bias.double(), padding=d['pad'])
    aff, gb = (guard.put(sc.to(DEV)), guard.put(sh.to(DEV))), guard.put(bias.to(DEV))
    off, on = _on_off(lambda u: Fn.conv_fwd(guard.put(d['x']), None, d['spec'], bias=gb, wino_u=u,
                                            in_affine=aff), d['wt'], False)
    _within(off[0], ref, 'classic U, INBN')
    _within(on[0], ref, 'tiled U, INBN')


@pytest.mark.parametrize('kernel', KERNELS)
def test_data_gradient_with_the_batchnorm_backward_sums(kernel):
    """BNB, data gradient 80->128: g = dz * (t * scale + shift > 0) and the two sums per tile"""
    Fn, d = _fn(), _case(80, 128, kernel, True)
    b, h, w = NHW
    t = rnd(b, 128, h, w, seed=5)
    sc, sh = rnd(128, seed=11).abs() + 0.5, rnd(128, seed=12)
    mean, invstd = rnd(128, seed=13, scale=0.1), rnd(128, seed=14).abs() + 0.5
    keep = (t.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)) > 0
    ref = d['ref'] * keep
    gt = to_act(t)
    dev = [guard.put(v.to(DEV)) for v in (sc, sh, mean, invstd)]

    def run(u):
        g, partial, rows = Fn.conv_dgrad_bnb(guard.put(d['x']), None, d['spec'], (h, w), guard.put(gt),
                                             *dev, wino_u=u)
        return g, partial[:, :rows]
    off, on = _on_off(run, d['wt'], True)
    _within(off[0], ref, 'classic U, BNB')
    _within(on[0], ref, 'tiled U, BNB')
    # the rows summed over the tiles = the BatchNorm's two backward sums
    xhat = (t.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
    sums = torch.stack([ref.sum((0, 2, 3)), (ref * xhat).sum((0, 2, 3))])
    got = on[1].cpu().double().sum(1)
    assert (got - sums).abs().max().item() <= 1e-4 * sums.abs().max().item()


@pytest.mark.parametrize('kernel', KERNELS)
def test_data_gradient_with_a_residual_gated_by_bits(kernel):
    """mask_res, data gradient 80->128: out = dz + (bit ? residual : 0)"""
    Fn, d = _fn(), _case(80, 128, kernel, True)
    b, h, w = NHW
    res, m = rnd(b, 128, h, w, seed=4), rnd(b, 128, h, w, seed=15)
    words = torch.zeros(b * h * w, 2, dtype=torch.int64)
    flat = (m > 0).permute(0, 2, 3, 1).reshape(b * h * w, 128)
    for c in range(128):
        bit = (c & 3) * 16 + ((c >> 2) & 15)
        shv = torch.tensor(1 << bit if bit < 63 else -(1 << 63), dtype=torch.int64)
        words[:, c // 64] |= flat[:, c].to(torch.int64) * shv
    ref = d['ref'] + torch.where(m > 0, res, torch.zeros_like(res)).double()
    gres = to_act(res)

    def run(u):
        bits = guard.put(words.flatten().to(DEV))
        bits._emsa_wbits = True
        return Fn.conv_dgrad(guard.put(d['x']), None, d['spec'], (h, w), wino_u=u,
                             residual=guard.put(gres), res_bits=bits)
    off, on = _on_off(run, d['wt'], True)
    _within(off[0], ref, 'classic U, mask_res')
    _within(on[0], ref, 'tiled U, mask_res')


_WN32_CODE = '''
import sys, torch
sys.path.insert(0, "tests")
import torch.nn.functional as F
from util import DEV, rnd, to_act
from emsanet_amd import functional as Fn, _lib
L = _lib.lib()
for kernel in ((1, 3), (3, 1)):
    pad = (kernel[0] // 2, kernel[1] // 2)
    for dgrad in (False, True):
        # the launch K = 32 -> n = 64: two 32-wide tiles, each one half of the 64-row block
        spec = Fn.ConvSpec(64, 32, kernel, (1, 1), pad) if dgrad else Fn.ConvSpec(32, 64, kernel, (1, 1), pad)
        wt = rnd(32, 64, *kernel, seed=2, scale=0.1) if dgrad else rnd(64, 32, *kernel, seed=2, scale=0.1)
        x = rnd(2, 32, 5, 7, seed=1)
        ref = (F.conv_transpose2d if dgrad else F.conv2d)(x.double(), wt.double(), padding=pad)
        out = []
        for on in (0, 1):
            L.emsa_wino_set_u_tiled(on)
            u = Fn.pack_wino(wt.to(DEV), fwd=not dgrad, dgrad=dgrad)[1 if dgrad else 0]
            y = (Fn.conv_dgrad(to_act(x), None, spec, (5, 7), wino_u=u) if dgrad
                 else Fn.conv_fwd(to_act(x), None, spec, wino_u=u))
            torch.cuda.synchronize()
            err = (y.cpu().double() - ref).abs().max().item()
            assert torch.isfinite(y).all() and err <= 1e-4 * ref.abs().max().item(), (kernel, dgrad, on, err)
            out.append(y.contiguous().view(torch.int32).clone())
        assert torch.equal(out[0], out[1]), (kernel, dgrad)
        assert L.emsa_conv1d_wino_spec_launches() == 0        # 32-wide tiles: the generic kernel
print("WN32_OK")
'''


def test_32_wide_tile_reads_its_half_of_the_block_subprocess():
    """EMSA_WINO_WN=32 is read once per process: a fresh child runs 32->64 on both layouts"""
    env = dict(os.environ, EMSA_WINO_WN='32', EMSA_POISON='1')
    r = subprocess.run([sys.executable, '-c', _WN32_CODE], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert 'WN32_OK' in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_switch_entry_point():
    L = _lib()
    assert L.emsa_wino_set_u_tiled(0) == 1 and L.emsa_wino_set_u_tiled(0) == 0
    assert L.emsa_wino_set_u_tiled(7) == 0 and L.emsa_wino_set_u_tiled(1) == 1
