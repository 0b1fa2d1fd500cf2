"""GPU: every convolution entry family, the pointwise families, the fused stem stage and one whole
training step on poisoned, guard-banded memory (tests/guard.py) with the INPUTS next to NaN too.

Outputs and scratch come from the guarded arena through the `guard_allocations` fixture; every
operand a kernel reads (activation, packed weight, bias, scale / shift, residual, mask source, dy) is
placed with `arena.put()`, flush between two bands of 0xFF bytes.  Then

* an output element the launch did not write is NaN and `close()` fails on it,
* a store past either end of an output is named by `arena.check()`,
* a read past either end of an operand that reaches the result makes it NaN.

References are fp64 `F.conv2d` / autograd on the values the kernel reads (16-bit: the rounded ones),
computed once per shape and shared; tolerances are those of the existing parity tests: 1e-4 for fp32,
TOL[dtype] for 16-bit storage, 2e-4 for fp32 results from 16-bit inputs.  A geometry a family does
not take is asserted to be refused on the host.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from guard import GUARD_BYTES_MODEL, GuardedArena, GuardError, install
from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, close, rnd, to_act

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TOL = {BF16: 6e-3, F16: 1e-3}

# cin, cout, kernel, stride, padding, n, h, w: the ragged rows of the existing tables
EDGE = [
    (40, 72, (1, 3), (1, 1), (0, 1), 1, 5, 7),
    (72, 40, (3, 1), (1, 1), (1, 0), 2, 7, 5),
    (8, 8, (1, 3), (1, 1), (0, 1), 1, 1, 2),
    (24, 136, (3, 3), (1, 1), (1, 1), 1, 5, 3),
    (96, 8, (3, 3), (1, 1), (1, 1), 2, 5, 7),
    (16, 32, (3, 3), (2, 2), (1, 1), 1, 9, 11),
    (256, 12, (1, 1), (1, 1), (0, 0), 4, 1, 1),
]
# n * h * w one below, at and one above a tile edge: 127 / 128 / 129 (64- and 128-row tiles) and
# 255 / 256 / 257 (128- and 256-row tiles)
TRIO = [(64, 64, (1, 3), (1, 1), (0, 1), n, h, w)
        for n, h, w in ((1, 1, 127), (2, 8, 8), (1, 3, 43), (1, 3, 85), (4, 8, 8), (1, 1, 257))]
SHAPES = EDGE + TRIO
PAIRS16 = [(-1, 0), (0, 0), (1, 0), (2, 0), (-1, 1), (1, 1), (2, 2)]      # tile, staging of test_conv16_fwd


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _lib():
    from emsanet_amd import _lib
    return _lib


def _ids(cfg):
    cin, cout, k, s, _, n, h, w = cfg
    return f"{cin}-{cout}-{k[0]}x{k[1]}s{s[0]}-{n}x{h}x{w}"


@functools.lru_cache(maxsize=None)
def _ref(cfg, dtype=None):
    """operands (rounded to `dtype` where the kernels read 16-bit storage) and the fp64 results of
    one shape; computed once, shared by the tests, left unchanged"""
    cin, cout, k, s, p, n, h, w = cfg
    r = (lambda t: t.to(dtype).float()) if dtype is not None else (lambda t: t)
    x, wt, b = r(rnd(n, cin, h, w, seed=1)), r(rnd(cout, cin, *k, seed=2, scale=0.1)), rnd(cout, seed=3)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wt, b))
    y = F.conv2d(xd, wd, bd, stride=s, padding=p)
    dy = r(rnd(*y.shape, seed=7))
    y.backward(dy.double())
    sc, sh = rnd(cout, seed=4), rnd(cout, seed=5)
    res = r(rnd(*y.shape, seed=6))
    v = lambda t: t.double()[None, :, None, None]                  # noqa: E731
    y2 = F.relu(y.detach() * v(sc) + v(sh) + res.double())
    mask, resx = r(rnd(n, cin, h, w, seed=8)), r(rnd(n, cin, h, w, seed=9))
    return dict(x=x, wt=wt, b=b, y=y.detach(), dy=dy, dx=xd.grad, dw=wd.grad, db=bd.grad, sc=sc, sh=sh,
                res=res, y2=y2, mask=mask, resx=resx)


class _Ops:
    """the operands of one case on the device, each flush between NaN guards"""

    def __init__(self, arena, r, dtype=F32):
        self.A, self.r, self.dtype = arena, r, dtype

    def act(self, name):
        return self.A.put(to_act(self.r[name]).to(self.dtype))

    def vec(self, name):
        return self.A.put(self.r[name].to(DEV))

    def put(self, t):
        return self.A.put(t)


def _spec(Fn, cfg):
    cin, cout, k, s, p = cfg[:5]
    return Fn.ConvSpec(cin, cout, k, s, p)


def _check_stats(stats, r, cout, tol_mean=1e-4, tol_var=2e-4):
    assert bool(torch.isfinite(stats).all()), 'statistics rows with unwritten entries'
    cnt = r['y'].numel() / cout
    assert float(stats[2][:, 0].sum()) == cnt
    mean = stats[0].sum(0) / cnt
    close(mean, r['y'].mean((0, 2, 3)), tol=tol_mean, what='stats mean')
    tile_mean = stats[0] / stats[2].clamp(min=1)
    m2 = stats[1].sum(0) + (stats[2] * (tile_mean - mean[None]) ** 2).sum(0)
    close(m2 / cnt, r['y'].var((0, 2, 3), unbiased=False), tol=tol_var, what='stats var')


# ---------------------------------------------------------------------------------------------
# convolution families
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_igemm_fp32(cfg, tile, monkeypatch, guard_allocations):
    """fp32 implicit GEMM, forward (statistics; folded BN + residual + ReLU) and data gradient
    (mask + residual) at every forced tile"""
    Fn, A = _fn(), guard_allocations
    monkeypatch.setenv('EMSA_CONV_TILE', str(tile))
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg), _spec(Fn, cfg)
    o = _Ops(A, r)
    wp = o.put(Fn.pack_weight(r['wt'].to(DEV), 'fwd'))
    x = o.act('x')
    y, stats = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'), want_stats=True)
    close(y, r['y'], what='igemm')
    _check_stats(stats, r, cout)
    y2 = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                     residual=o.act('res'), act=Fn.ACT_RELU)
    close(y2, r['y2'], what='igemm epilogue')
    wpd = o.put(Fn.pack_weight(r['wt'].to(DEV), 'dgrad'))
    dx = Fn.conv_dgrad(o.act('dy'), wpd, spec, (h, w), mask_src=o.act('mask'), residual=o.act('resx'))
    close(dx, (r['dx'] + r['resx']) * (r['mask'] > 0), what='igemm dgrad residual+mask')
    A.check()


@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_winograd_rows_fp32(cfg, guard_allocations):
    """row Winograd F(2,3): forward (statistics, epilogue, ReLU bits) and data gradient"""
    Fn, A = _fn(), guard_allocations
    L, lib = _lib().lib(), _lib()
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg), _spec(Fn, cfg)
    if not Fn.wino_eligible(spec):
        g = spec.geom_fwd(n, h, w, cin, cout)
        assert L.emsa_conv1d_wino_stats_rows(g) == lib.E_SHAPE
        with pytest.raises(lib.EmsaError):
            Fn.conv_fwd(to_act(r['x']), None, spec, wino_u=torch.zeros(16, device=DEV))
        return
    o = _Ops(A, r)
    u, ud = Fn.pack_wino(r['wt'].to(DEV), fwd=True, dgrad=True)
    u, ud = o.put(u), o.put(ud)
    x = o.act('x')
    y, stats = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), want_stats=True, wino_u=u)
    close(y, r['y'], what='wino')
    _check_stats(stats, r, cout)
    y2, bits = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                           residual=o.act('res'), act=Fn.ACT_RELU, wino_u=u, want_relu_bits=True)
    close(y2, r['y2'], what='wino epilogue')
    # the bit mask: word per (pixel, 64-channel tile), bit = (c % 4) * 16 + (c % 64) // 4
    assert bits.numel() == n * h * w * ((cout + 63) // 64)
    words = bits.cpu().numpy().view('uint64').reshape(n * h * w, -1)
    yb = (y2.permute(0, 2, 3, 1).reshape(-1, cout) > 0).cpu().numpy()
    import numpy as np
    for c in range(cout):
        got = (words[:, c // 64] >> np.uint64((c % 4) * 16 + (c % 64) // 4)) & np.uint64(1)
        assert np.array_equal(got.astype(bool), yb[:, c]), f'relu bit of channel {c}'
    dx = Fn.conv_dgrad(o.act('dy'), None, spec, (h, w), mask_src=o.act('mask'), wino_u=ud)
    close(dx, r['dx'] * (r['mask'] > 0), what='wino dgrad mask')
    dx = Fn.conv_dgrad(o.act('dy'), None, spec, (h, w), residual=o.act('resx'), wino_u=ud)
    close(dx, r['dx'] + r['resx'], what='wino dgrad residual')
    A.check()


@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_winograd_2d_fp32(cfg, guard_allocations):
    """2-D Winograd F(2x2,3x3): forward (statistics; epilogue) and data gradient"""
    Fn, A = _fn(), guard_allocations
    L, lib = _lib().lib(), _lib()
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg), _spec(Fn, cfg)
    g = spec.geom_fwd(n, h, w, cin, cout)
    if not Fn.wino2d_eligible(spec):
        assert L.emsa_conv_wino2d_supported(g) == 0
        assert L.emsa_conv_wino2d_stats_rows(g) == lib.E_SHAPE
        return
    assert L.emsa_conv_wino2d_supported(g) == 1
    o = _Ops(A, r)
    u2, ud2 = Fn.pack_wino2d(r['wt'].to(DEV), fwd=True, dgrad=True)
    u2, ud2 = o.put(u2), o.put(ud2)
    x = o.act('x')
    before = Fn.WINO2D_FALLBACKS
    y, stats = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), want_stats=True, wino2d_u=u2)
    close(y, r['y'], what='wino2d')
    _check_stats(stats, r, cout)
    y2 = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                     residual=o.act('res'), act=Fn.ACT_RELU, wino2d_u=u2)
    close(y2, r['y2'], what='wino2d epilogue')
    dx = Fn.conv_dgrad(o.act('dy'), None, spec, (h, w), mask_src=o.act('mask'), residual=o.act('resx'),
                       wino2d_u=ud2)
    close(dx, (r['dx'] + r['resx']) * (r['mask'] > 0), what='wino2d dgrad residual+mask')
    assert Fn.WINO2D_FALLBACKS == before, 'ran on the row kernel instead'
    A.check()


def _h_ok(cfg):
    return cfg[0] % 8 == 0 and cfg[1] % 8 == 0         # conv_h.hip h_geom_ok: 16-byte channel groups


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('tile,staging', PAIRS16)
@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_conv_h_16bit(cfg, tile, staging, dtype, monkeypatch, guard_allocations):
    """16-bit implicit GEMM (conv_h.hip) at the tile x staging pairs of test_conv16_fwd"""
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    if tile >= 0:
        monkeypatch.setenv('EMSA_CONVH_TILE', str(tile))
    monkeypatch.setenv('EMSA_CONVH_PF', str(staging))
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, dtype), _spec(Fn, cfg)
    o = _Ops(A, r, dtype)
    if not _h_ok(cfg):
        g = spec.geom_fwd(n, h, w, cin, cout)
        assert lib.lib().emsa_conv_stats_rows_t(Fn.DT[dtype], g) == lib.E_SHAPE
        with pytest.raises(lib.EmsaError):
            Fn.conv_fwd(o.act('x'), torch.zeros(k[0] * k[1] * cout * cin, device=DEV, dtype=dtype), spec)
        return
    wp, wpd = Fn.pack_weight_t(r['wt'].to(DEV), dtype, fwd=True, dgrad=True)
    wp, wpd = o.put(wp), o.put(wpd)
    x = o.act('x')
    y, stats = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'), want_stats=True)
    assert y.dtype == dtype
    close(y, r['y'], tol=TOL[dtype], what='conv_h')
    _check_stats(stats, r, cout, tol_mean=2e-4, tol_var=4e-4)
    y2 = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                     residual=o.act('res'), act=Fn.ACT_RELU)
    close(y2, r['y2'], tol=TOL[dtype], what='conv_h epilogue')
    dx = Fn.conv_dgrad(o.act('dy'), wpd, spec, (h, w), mask_src=o.act('mask'))
    close(dx, r['dx'] * (r['mask'] > 0), tol=TOL[dtype], what='conv_h dgrad mask')
    dx = Fn.conv_dgrad(o.act('dy'), wpd, spec, (h, w), residual=o.act('resx'))
    close(dx, r['dx'] + r['resx'], tol=TOL[dtype], what='conv_h dgrad residual')
    A.check()


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_conv_rs_16bit(cfg, dtype, guard_allocations):
    """register-stationary 3-tap kernel (conv_rs.hip): C_in = C_out in {64, 128, 256, 512} only"""
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, dtype), _spec(Fn, cfg)
    g = spec.geom_fwd(n, h, w, cin, cout)
    if not Fn.rs_eligible(spec):
        assert lib.lib().emsa_conv1d_rs_supported(Fn.DT[dtype], g) == 0
        return
    assert Fn.rs_supported(Fn.DT[dtype], g), 'the rs kernel must take this case'
    o = _Ops(A, r, dtype)
    wf, wfd = Fn.pack_weight_frag_t(r['wt'].to(DEV), dtype, fwd=True, dgrad=True)
    wf, wfd = o.put(wf), o.put(wfd)
    x = o.act('x')
    y, stats = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), want_stats=True, wfrag=wf)
    assert y.dtype == dtype and stats.shape[1] == g._rs[2]
    close(y, r['y'], tol=TOL[dtype], what='conv_rs')
    _check_stats(stats, r, cout, tol_mean=2e-4, tol_var=4e-4)
    y2 = Fn.conv_fwd(x, None, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                     residual=o.act('res'), act=Fn.ACT_RELU, wfrag=wf)
    close(y2, r['y2'], tol=TOL[dtype], what='conv_rs epilogue')
    assert Fn.rs_supported(Fn.DT[dtype], spec.geom_dgrad(n, h, w, cout, cin))
    dx = Fn.conv_dgrad(o.act('dy'), None, spec, (h, w), residual=o.act('resx'), mask_src=o.act('mask'),
                       wfrag=wfd)
    close(dx, (r['dx'] + r['resx']) * (r['mask'] > 0), tol=TOL[dtype], what='conv_rs dgrad res+mask')
    A.check()


# few output tiles and a long K: the two ragged rows of test_conv16_tap_split's table
SPLIT = [(128, 96, (3, 3), (1, 1), (1, 1), 2, 9, 11), (512, 512, (3, 1), (1, 1), (1, 0), 1, 5, 7)]


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('cfg', SHAPES + SPLIT, ids=_ids)
def test_tap_split_16bit(cfg, dtype, guard_allocations):
    """the tap-split launch + finish pass (emsa_conv_igemm_splitk_t); a geometry the plan does not
    split has a workspace of 0 bytes and the direct call is refused"""
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, dtype), _spec(Fn, cfg)
    g = spec.geom_fwd(n, h, w, cin, cout)
    ws_bytes = Fn._splitk_ws_bytes(Fn.DT[dtype], g)
    if cfg in SPLIT:
        assert ws_bytes > 0, 'this case must take the tap-split path'
    if ws_bytes <= 0:
        assert ws_bytes == 0
        assert lib.lib().emsa_conv_igemm_splitk_t(Fn.DT[dtype], g, None, None, None, None, None, None,
                                                  None, 0, 0, None, None) == lib.E_SHAPE
        return
    o = _Ops(A, r, dtype)
    wp = o.put(Fn.pack_weight_t(r['wt'].to(DEV), dtype, fwd=True)[0])
    x = o.act('x')
    y = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'))
    close(y, r['y'], tol=TOL[dtype], what='tap-split')
    y2 = Fn.conv_fwd(x, wp, spec, bias=o.vec('b'), scale=o.vec('sc'), shift=o.vec('sh'),
                     residual=o.act('res'), act=Fn.ACT_RELU)
    close(y2, r['y2'], tol=TOL[dtype], what='tap-split epilogue')
    A.check()


@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_wgrad_fp32(cfg, guard_allocations):
    """fp32 weight + bias gradient: the packed accumulator form and the two-pass form"""
    Fn, A = _fn(), guard_allocations
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg), _spec(Fn, cfg)
    o = _Ops(A, r)
    x, dy = o.act('x'), o.act('dy')
    like = torch.empty(cout, cin, *k, device=DEV)
    dwp, db, packed = Fn.conv_wgrad(x, dy, spec, True, two_pass=False)
    assert packed
    close(Fn.unpack_wgrad(dwp, like), r['dw'], what='wgrad')
    close(db, r['db'], what='bgrad')
    dw2, db2, packed2 = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=True)
    assert packed2 == (not (k in ((3, 1), (1, 3), (3, 3)) and s == (1, 1)))
    close(Fn.unpack_wgrad(dw2, like) if packed2 else dw2, r['dw'], what='wgrad two-pass')
    close(db2, r['db'], what='bgrad two-pass')
    A.check()


@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_wgrad_bf16(cfg, guard_allocations):
    """fp32 weight + bias gradient from bf16 activations, both forms"""
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, BF16), _spec(Fn, cfg)
    o = _Ops(A, r, BF16)
    x, dy = o.act('x'), o.act('dy')
    like = torch.empty(cout, cin, *k, device=DEV)
    for two_pass in (True, False):
        try:
            dw, db, packed = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=two_pass)
        except lib.EmsaError:
            # refused on the host: only a geometry off the 8-channel rule of the 16-bit loaders
            assert not _h_ok(cfg), 'a supported geometry was refused'
            continue
        if packed:
            dw = Fn.unpack_wgrad(dw, like)
        close(dw, r['dw'], tol=2e-4, what=f'wgrad16 (two_pass={two_pass})')
        close(db, r['db'], tol=2e-4, what=f'dbias16 (two_pass={two_pass})')
    A.check()


@pytest.mark.parametrize('n_jobs', [2, 4])
@pytest.mark.parametrize('cfg', SHAPES, ids=_ids)
def test_wgrad_multi_bf16(cfg, n_jobs, guard_allocations):
    """several weight gradients in one launch (emsa_conv_wgrad_multi_t), a job without a bias"""
    Fn, A = _fn(), guard_allocations
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, BF16), _spec(Fn, cfg)
    o = _Ops(A, r, BF16)
    like = torch.empty(cout, cin, *k, device=DEV)
    jobs = [(o.act('x'), o.act('dy'), spec, like, None, None, j != 1) for j in range(n_jobs)]
    out = Fn.conv_wgrad_multi(jobs)
    if out is None:
        # no multi-job form (the caller launches job by job): only where the wrapper's rule says so
        assert not Fn.wgrad_multi_eligible(jobs[0][0], spec), 'an eligible set was refused'
        return
    for j, (dw, db) in enumerate(out):
        close(dw, r['dw'], tol=2e-4, what=f'multi wgrad job {j}')
        if j != 1:
            close(db, r['db'], tol=2e-4, what=f'multi dbias job {j}')
        else:
            assert db is None
    A.check()


@pytest.mark.parametrize('dtype', [F32, F16])
@pytest.mark.parametrize('cfg', [EDGE[0], EDGE[2], TRIO[0], TRIO[4]], ids=_ids)
def test_wgrad_multi_has_no_fp32_or_fp16_form(cfg, dtype, guard_allocations):
    """the multi-job launch exists for bf16 storage only: fp32 and fp16 jobs of geometries it takes in
    bf16 are refused on the host (workspace of 0 bytes -> None), the caller launches job by job"""
    Fn, A = _fn(), guard_allocations
    cin, cout, k = cfg[:3]
    r, spec = _ref(cfg, None if dtype == F32 else dtype), _spec(Fn, cfg)
    o = _Ops(A, r, dtype)
    like = torch.empty(cout, cin, *k, device=DEV)
    jobs = [(o.act('x'), o.act('dy'), spec, like, None, None, True) for _ in range(2)]
    assert Fn.wgrad_multi_eligible(jobs[0][0].to(BF16), spec) and not Fn.wgrad_multi_eligible(jobs[0][0], spec)
    assert Fn.conv_wgrad_multi(jobs) is None
    A.check()


@pytest.mark.parametrize('k,dtype,wino2d', [(1, F32, False), (3, F32, False), (3, F32, True), (1, BF16, False),
                                           (3, BF16, False)])
def test_merged_head_repack_paths(k, dtype, wino2d, monkeypatch, guard_allocations):
    """ops.MultiConvRT without a PackPlan in front of it: the operand of two convs (5 + 2 output
    channels in an 8-wide head) is assembled by its own re-pack path -- `_assemble`, once per side,
    in the activations' dtype, into zeroed buffers; U and U2 (2-D Winograd) are
    made from those same two operands -- forward and data gradient against the fp64 convs; the
    padding channel is the zero the buffers started with"""
    from emsanet_amd import ops
    Fn, A = _fn(), guard_allocations
    monkeypatch.setattr(Fn, 'WINO2D', wino2d)
    n, cin, h, w = 2, 16, 5, 7
    lo = dtype != F32
    r_ = (lambda t: t.to(dtype).float()) if lo else (lambda t: t)
    convs, off, places = [], 0, []
    for j, co in enumerate((5, 2)):
        c = torch.nn.Conv2d(cin, co, k, padding=k // 2)
        with torch.no_grad():
            c.weight.copy_(r_(rnd(co, cin, k, k, seed=10 + j, scale=0.1)))
            c.bias.copy_(rnd(co, seed=20 + j))
        convs.append(c.to(DEV))
        places.append((convs[-1], off, 0))
        off += co
    rt = ops.MultiConvRT(places, Fn.pad8(off), cin, k, k // 2)
    assert rt.wino2d == (wino2d and k == 3)
    x, dy = r_(rnd(n, cin, h, w, seed=1)), r_(rnd(n, 8, h, w, seed=2))
    xd = x.double().requires_grad_(True)
    ref = torch.cat([F.conv2d(xd, c.weight.detach().cpu().double(), c.bias.detach().cpu().double(),
                              padding=k // 2) for c in convs], 1)
    ref.backward(dy[:, :off].double())
    tol = TOL[dtype] if lo else 1e-4
    y = rt.forward(A.put(to_act(x).to(dtype)))
    close(y[:, :off], ref.detach(), tol=tol, what='merged head')
    assert float(y[:, off:].float().abs().max()) == 0.0, 'padding channel of the merged head'
    dx = rt.dgrad(A.put(to_act(dy).to(dtype)), (h, w))
    close(dx, xd.grad, tol=tol, what='merged head dgrad')
    sites = [(e[3].rsplit(':', 1)[0], e[5]) for e in A._live]
    want = {('ops.py:_assemble', dtype)}
    if rt.wino2d:
        # U2 of both sides was made under the guard, from the operands the row form was made from
        want.add(('functional.py:_wino2d_buf', F32))
        assert rt.packs.peek('wino2d', F32, rt.key_now()) != (None, None)
    assert want <= set(sites), (want, sorted(s_ for s_ in sites if s_[0].startswith('ops.py')))
    for site in sorted(want):
        # each operand (forward, data gradient) is assembled once, whichever forms are made from it
        assert sites.count(site) == 2, (site, sites)
    A.check()


@pytest.mark.parametrize('cin,cout,k,dtype,wino2d,shape,form', [
    (64, 64, (3, 1), F32, None, (2, 6, 10), 'wino'),
    (16, 8, (3, 3), F32, True, (2, 6, 10), 'wino2d'),
    (12, 20, (3, 3), F32, True, (2, 5, 7), 'wino2d'),        # U2 with K-step padding
    (16, 8, (1, 1), F32, None, (2, 6, 10), 'gemm'),
    (64, 64, (3, 1), BF16, None, (2, 6, 10), None),          # 'frag', or 'gemm' where conv_rs refuses
], ids=['wino', 'wino2d', 'wino2d-padded', 'gemm', 'bf16'])
def test_frozen_conv_caches_its_data_gradient_pack(cin, cout, k, dtype, wino2d, shape, form, monkeypatch,
                                                   guard_allocations):
    """ops.ConvRT without a PackPlan in front of it, weight trainable / frozen: the same data
    gradient bit for bit (== fp64), and the frozen conv's data-gradient operand -- packed at the
    first request, the forward miss left it out -- is the SAME tensor at the second request"""
    from emsanet_amd import ops
    Fn, A = _fn(), guard_allocations
    if wino2d is not None:
        monkeypatch.setattr(Fn, 'WINO2D', wino2d)
    n, h, w = shape
    lo = dtype != F32
    r_ = (lambda t: t.to(dtype).float()) if lo else (lambda t: t)
    pad = (k[0] // 2, k[1] // 2)
    conv = torch.nn.Conv2d(cin, cout, k, padding=pad, bias=False)
    with torch.no_grad():
        conv.weight.copy_(r_(rnd(cout, cin, *k, seed=3, scale=0.1)))
    conv.to(DEV)
    x, dy = r_(rnd(n, cin, h, w, seed=1)), r_(rnd(n, cout, h, w, seed=2))
    xd = x.double().requires_grad_(True)
    F.conv2d(xd, conv.weight.detach().cpu().double(), padding=pad).backward(dy.double())
    gx, gdy = A.put(to_act(x).to(dtype)), A.put(to_act(dy).to(dtype))

    def dgrad_packs(rt):
        sides = {f: rt.packs.peek(f, dtype, rt.key_now())[1] for f in ('gemm', 'wino', 'wino2d', 'frag')}
        return {f: t.data_ptr() for f, t in sides.items() if t is not None}
    dxs = []
    for trainable in (True, False):
        conv.weight.requires_grad_(trainable)
        rt = ops.ConvRT(conv)
        assert rt.wino2d == bool(wino2d)
        rt.forward(gx)
        # the forward miss packed the data-gradient side along iff the weight is trainable
        assert bool(dgrad_packs(rt)) == trainable
        dx = rt.dgrad(gdy, (h, w))
        packs = dgrad_packs(rt)
        assert (form in packs) if form else bool(packs), packs
        dx2 = rt.dgrad(gdy, (h, w))
        assert torch.equal(dx, dx2) and dgrad_packs(rt) == packs
        dxs.append(dx)
    close(dxs[0], xd.grad, tol=TOL[dtype] if lo else 1e-4, what='data gradient')
    assert torch.equal(dxs[0], dxs[1])
    A.check()


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('shape', [(1, 22, 26), (2, 7, 9)])
@pytest.mark.parametrize('cin,rows', [(3, True), (1, True), (1, False)])
def test_stem_routes(cin, rows, shape, dtype, monkeypatch, guard_allocations):
    """7x7/2 stem, forward + statistics + weight gradient: the NHWC4 route (seven row taps) and the
    rows-as-channels route of the one-channel stem; packed image, packed weight and dy between guards"""
    Fn, A = _fn(), guard_allocations
    monkeypatch.setattr(Fn, 'STEM_ROWS', rows)
    n, h, w = shape
    lo = dtype != F32
    r_ = (lambda t: t.to(dtype).float()) if lo else (lambda t: t)
    x = r_(rnd(n, cin, h, w, seed=1))
    wt = r_(rnd(64, cin, 7, 7, seed=2, scale=0.1))
    wd = wt.double().requires_grad_(True)
    y = F.conv2d(x.double(), wd, None, stride=2, padding=3)
    dy = r_(rnd(*y.shape, seed=3))
    y.backward(dy.double())
    spec = Fn.StemSpec(cin)
    assert spec.rows == (cin == 1 and rows)
    xp = Fn.stem_pack_input(A.put(x.to(DEV)), dtype)             # (guarded: the arena's own)
    wp = Fn.stem_pack_weight(A.put(wt.to(DEV)), dtype)
    if lo and w % 2:
        # conv_h.hip h_geom_ok: 16-byte accesses need the padded NHWC4 image's row stride (w + 8) * 4
        # to be a multiple of 8 elements, i.e. an even width -- refused before any launch
        with pytest.raises(_lib().EmsaError):
            Fn.stem_fwd(xp, wp, spec, n, h, w)
        return
    out, stats = Fn.stem_fwd(xp, wp, spec, n, h, w)
    close(out, y.detach(), tol=TOL[dtype] if lo else 1e-4, what='stem fwd')
    assert bool(torch.isfinite(stats).all())
    close(stats[0].sum(0) / (y.numel() / 64), y.detach().mean((0, 2, 3)), tol=2e-4 if lo else 1e-4,
          what='stem mean')
    dw = Fn.stem_wgrad(xp, A.put(to_act(dy).to(dtype)), spec, n, h, w, wt.to(DEV))
    close(dw, wd.grad, tol=2e-4 if lo else 1e-4, what='stem wgrad')
    A.check()


# ---------------------------------------------------------------------------------------------
# pointwise families with ragged totals
# ---------------------------------------------------------------------------------------------
# channel counts 5 / 8 / 40 on the maps 1x1x1, 1x9x33, 3x4x4: element counts 5 .. 11,880, none a
# multiple of 256 and (c = 5) none a multiple of a 4- or 8-element vector.  The map 2x4x4 is added
# for the exact multiples of 256: 8 channels = 256 elements, 40 channels = 1,280.
PW = [(c, m) for c in (5, 8, 40) for m in ((1, 1, 1), (1, 9, 33), (3, 4, 4))] + [(8, (2, 4, 4)), (40, (2, 4, 4))]
PW_IDS = [f"c{c}-{m[0]}x{m[1]}x{m[2]}" for c, m in PW]
pw = pytest.mark.parametrize('c,m', PW, ids=PW_IDS)
pw_dtype = pytest.mark.parametrize('dtype', [F32, BF16])


def _vec_ok(c, dtype):
    """pointwise.hip cv_ok<T>: whole 16-byte channel vectors (4 fp32 / 8 16-bit elements)"""
    return c % (4 if dtype == F32 else 8) == 0


def _q(t, dtype):
    return t.to(dtype).double()


def _tol(dtype, f32=1e-4):
    return f32 if dtype == F32 else TOL[dtype]


def _put_act(A, t, dtype=F32):
    return A.put(to_act(t).to(dtype))


@pw
@pw_dtype
def test_bn_act_mask_and_bn_bwd(c, m, dtype, guard_allocations):
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    n, h, w = m
    x, res, dy = (rnd(n, c, h, w, seed=s_) for s_ in (1, 2, 3))
    gamma, mean = rnd(c, seed=4).abs() + 0.5, rnd(c, seed=5) * 0.1
    invstd, beta = rnd(c, seed=6).abs() + 0.5, rnd(c, seed=7)
    scale = gamma * invstd
    shift = beta - mean * scale
    args = (_put_act(A, x, dtype), A.put(scale.to(DEV)), A.put(shift.to(DEV)), None, _put_act(A, res, dtype))
    if not _vec_ok(c, dtype):
        with pytest.raises(lib.EmsaError):
            Fn.bn_act(*args, Fn.ACT_RELU, want_mask=True)
        return
    y, bits = Fn.bn_act(*args, Fn.ACT_RELU, want_mask=True)
    v = lambda t: t.double()[None, :, None, None]                  # noqa: E731
    ref = F.relu(_q(x, dtype) * v(scale) + v(shift) + _q(res, dtype))
    close(y, ref, tol=_tol(dtype), what='bn_act')
    assert bits.dtype == torch.int64 and bits.numel() == lib.lib().emsa_relu_mask_words(n * c * h * w)
    # backward (frozen statistics) from the bit mask and from y itself: the same bits; against the
    # closed form with the ReLU decisions of the engine's own forward
    outs = []
    for msk in (bits, y):
        outs.append(Fn.bn_bwd(_put_act(A, dy, dtype), msk, args[0], A.put(gamma.to(DEV)), A.put(mean.to(DEV)),
                              A.put(invstd.to(DEV)), None, Fn.ACT_RELU, False, want_dres=True))
    for a, b, name in zip(outs[0], outs[1], ('dx', 'dres', 'dgamma', 'dbeta')):
        assert torch.equal(a, b), f'bit-mask path differs: {name}'
    g = _q(dy, dtype) * (y.detach().cpu().double() > 0)
    xhat = (_q(x, dtype) - v(mean)) * v(invstd)
    dx, dres, dg, db = outs[0]
    close(dres, g, tol=_tol(dtype), what='bn dres')
    close(dx, g * v(gamma * invstd), tol=_tol(dtype) * (1 if dtype == F32 else 3), what='bn dx')
    close(dg, (g * xhat).sum((0, 2, 3)), tol=1e-4 if dtype == F32 else 2e-4, what='bn dgamma')
    close(db, g.sum((0, 2, 3)), tol=1e-4 if dtype == F32 else 2e-4, what='bn dbeta')
    A.check()


@pw
@pw_dtype
def test_maxpool_and_index_map(c, m, dtype, guard_allocations):
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    n, h, w = m
    x = rnd(n, c, h, w, seed=1)
    xa = _put_act(A, x, dtype)
    if not _vec_ok(c, dtype):
        with pytest.raises(lib.EmsaError):
            Fn.maxpool_fwd(xa)
        return
    xr = _q(x, dtype).requires_grad_(True)
    ref = F.max_pool2d(xr, 3, stride=2, padding=1)
    dy = rnd(*ref.shape, seed=2)
    ref.backward(_q(dy, dtype))
    y, idx = Fn.maxpool_fwd(xa)
    close(y, ref.detach(), tol=0, what='maxpool')
    assert idx.dtype == torch.int8 and int(idx.min()) >= 0 and int(idx.max()) <= 8, 'index map not written'
    dx = Fn.maxpool_bwd(_put_act(A, dy, dtype), A.put(idx), (h, w))
    close(dx, xr.grad, tol=1e-6 if dtype == F32 else TOL[dtype], what='maxpool bwd')
    A.check()


@pw
@pw_dtype
def test_se_scale_add(c, m, dtype, guard_allocations):
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    n, h, w = m
    a, b = rnd(n, c, h, w, seed=1), rnd(n, c, h, w, seed=2)
    sa, sb = rnd(n, c, seed=3).abs() + 0.1, rnd(n, c, seed=4).abs() + 0.1
    args = (_put_act(A, a, dtype), A.put(sa.to(DEV)), _put_act(A, b, dtype), A.put(sb.to(DEV)))
    if not _vec_ok(c, dtype):
        with pytest.raises(lib.EmsaError):
            Fn.se_scale_add(*args)
        return
    out = Fn.se_scale_add(*args)
    close(out, _q(a, dtype) * sa.double()[:, :, None, None] + _q(b, dtype) * sb.double()[:, :, None, None],
          tol=_tol(dtype), what='se_scale_add')
    A.check()


@pw
@pw_dtype
def test_up2x_dw_forward_and_one_pass_backward(c, m, dtype, monkeypatch, guard_allocations):
    Fn, A = _fn(), guard_allocations
    lib = _lib()
    n, h, w = m
    x, wt, b = rnd(n, c, h, w, seed=1), rnd(c, 1, 3, 3, seed=2, scale=0.3), rnd(c, seed=3)
    skip, dy = rnd(n, c, 2 * h, 2 * w, seed=4), rnd(n, c, 2 * h, 2 * w, seed=5)
    xa = _put_act(A, x, dtype)
    wd_, bd_ = A.put(wt.to(DEV)), A.put(b.to(DEV))
    if c % 4:                                            # pointwise.hip c4_ok
        with pytest.raises(lib.EmsaError):
            Fn.up2x_dw_fwd(xa, wd_, bd_, None)
        return
    assert _vec_ok(c, dtype)                             # (8 and 40 are multiples of 4 and of 8)
    xr, wr, br = _q(x, dtype).requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    up = F.conv2d(F.interpolate(xr, scale_factor=2, mode='nearest'), wr, br, padding=1, groups=c)
    y = Fn.up2x_dw_fwd(xa, wd_, bd_, _put_act(A, skip, dtype))
    close(y, up.detach() + _q(skip, dtype), tol=_tol(dtype), what='up2x fwd')
    up.backward(_q(dy, dtype))
    assert lib.lib().emsa_up2x_dw3x3_bwd_supported(c, xa.element_size()) == 1
    monkeypatch.setattr(Fn, 'UP2X_FUSED_BWD', True)
    dx, dw, db = Fn.up2x_dw_bwd(_put_act(A, dy, dtype), xa, wd_)
    assert dx.dtype == dtype
    close(dx, xr.grad, tol=1e-4 if dtype == F32 else 1e-2, what='one-pass dx')
    close(dw.view(c, 1, 3, 3), wr.grad, tol=2e-4, what='one-pass dw')
    close(db, br.grad, tol=2e-4, what='one-pass db')
    A.check()


@pw
def test_bilinear_and_nearest_both_ways(c, m, guard_allocations):
    Fn, A = _fn(), guard_allocations
    n, ih, iw = m
    oh, ow = 2 * ih + 1, 2 * iw + 3
    for mode, fwd, bwd, tf, tb in (('bilinear', Fn.bilinear_fwd, Fn.bilinear_bwd, 1e-4, 2e-5),
                                   ('nearest', Fn.nearest_fwd, Fn.nearest_bwd, 0.0, 2e-6)):
        x = rnd(n, c, ih, iw, seed=1).double().requires_grad_(True)
        y = F.interpolate(x, (oh, ow), mode=mode, **({'align_corners': False} if mode == 'bilinear' else {}))
        dy = rnd(n, c, oh, ow, seed=2)
        y.backward(dy.double())
        out = Fn.act_empty(n, c, oh, ow, DEV)
        close(fwd(_put_act(A, x.detach().float()), out), y.detach(), tol=tf, what=f'{mode} fwd')
        close(bwd(_put_act(A, dy), (ih, iw)), x.grad, tol=tb, what=f'{mode} bwd')
    A.check()


@pw
def test_head_act(c, m, guard_allocations):
    Fn, A = _fn(), guard_allocations
    n, h, w = m
    x = rnd(n, c, h, w, seed=1).double().requires_grad_(True)
    y = torch.cat([torch.sigmoid(x[:, :1]), torch.tanh(x[:, 1:3]), x[:, 3:]], 1)
    dy = rnd(n, c, h, w, seed=2)
    y.backward(dy.double())
    yg = Fn.head_act_fwd(_put_act(A, x.detach().float()), 1, 2)
    close(yg, y.detach(), what='head act')
    dx = Fn.head_act_bwd(_put_act(A, dy), A.put(yg), 1, 2)
    close(dx, x.grad, what='head act bwd')
    A.check()


@pw
@pw_dtype
def test_copy_cast_to_nhwc_add_axpy(c, m, dtype, guard_allocations):
    Fn, A = _fn(), guard_allocations
    n, h, w = m
    x, b = rnd(n, c, h, w, seed=1), rnd(n, c, h, w, seed=2)
    xa = _put_act(A, x, dtype)
    # copy into the first c columns of an ld-wide buffer: columns c..ld keep their sentinel
    ld = c + 3
    wide = A.alloc((n, h, w, ld), DEV, dtype)
    wide.fill_(7.0)
    Fn.copy_channels(xa, wide[..., :c].permute(0, 3, 1, 2))
    assert torch.equal(wide[..., :c].permute(0, 3, 1, 2), xa)
    assert bool((wide[..., c:] == 7.0).all()), 'columns c..ld were written'
    # cast both ways
    other = BF16 if dtype == F32 else F32
    assert torch.equal(Fn.cast(xa, other), xa.to(other))
    # any layout -> dense NHWC: contiguous NCHW memory
    nchw = A.put(x.to(dtype).to(DEV))
    got = Fn.to_nhwc(nchw)
    if h * w == 1:
        assert got is nchw                               # one pixel: NCHW memory is NHWC memory, no launch
    else:
        assert got.data_ptr() != nchw.data_ptr() and Fn.ld_of(got) == c and torch.equal(got, nchw)
    # add, axpy_
    ba = _put_act(A, b, dtype)
    close(Fn.add(xa, ba), _q(x, dtype) + _q(b, dtype), tol=1e-6 if dtype == F32 else TOL[dtype], what='add')
    if dtype == F32:
        yv = A.put(x.reshape(-1).to(DEV))
        Fn.axpy_(yv, A.put(b.reshape(-1).to(DEV)), 0.5)
        close(yv, x.reshape(-1).double() + 0.5 * b.reshape(-1).double(), tol=1e-6, what='axpy')
    A.check()


# ---------------------------------------------------------------------------------------------
# the fused stem stage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,h,w', [(2, 2, 2), (2, 5, 7), (2, 6, 10), (3, 9, 4), (3, 34, 46)])
def test_stem_stage_between_guards(n, h, w, guard_allocations):
    """the five shapes of test_stem_stage_gpu.py with both y maps, both index maps and G_f, G_d
    between guards: forward bit-equal to the unfused kernels, backward within that module's rule"""
    import test_stem_stage_gpu as S
    assert (n, h, w) in S.SHAPES and len(S.SHAPES) == 5
    Fn, A = _fn(), guard_allocations
    d = dict(S._case(n, h, w))
    d['ys'] = [A.put(t) for t in d['ys']]
    for key in ('idx_f', 'idx_d', 'gf', 'gd'):
        d[key] = A.put(d[key])
    pf, idx_f, pd, idx_d = Fn.stem_stage_fwd(d['ys'][0], d['ys'][1], d['aff'][0], d['aff'][1],
                                             d['s'][0], d['s'][1])
    assert torch.equal(idx_f, d['idx_f']) and torch.equal(idx_d, d['idx_d'])
    assert torch.equal(pf.view(torch.int32), d['pf'].view(torch.int32))
    assert torch.equal(pd.view(torch.int32), d['pd'].view(torch.int32))
    fu, un, ref = S._flat(S._fused_bwd(d)), S._flat(S._unfused_bwd(d)), S._flat(d['ref'])
    assert set(fu) == set(un) == set(ref) and len(ref) == 14
    bad = []
    for k in sorted(ref):
        ef, eu, top = S._err(fu[k], ref[k]), S._err(un[k], ref[k]), float(ref[k].abs().max())
        if ef > max(2 * eu, 1e-6 * top):
            bad.append(f"{k}: fused {ef:.3e} > max(2 x {eu:.3e}, 1e-6 x {top:.3e})")
    assert not bad, '\n'.join(bad)
    A.check()


# ---------------------------------------------------------------------------------------------
# the whole engine, eager
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_whole_engine_train_step(dtype, monkeypatch):
    """one training step at 64 x 96, batch 2, with every wrapper allocation in the arena (4 KiB
    bands, see guard.GUARD_BYTES_MODEL) and without it: finite outputs and gradients, intact guards,
    and the two runs agree as test_train_step_gradients_are_reproducible_run_to_run demands of two
    runs (outputs bit-equal; gradients equal, or roundoff-sized, or rel-L2 <= 1e-5; at most a
    quarter of them different at all)"""
    import test_timed_size_gpu as T
    from emsanet_amd import full_args
    batch = T._inputs(2, 64, 96, seed=2)

    def build():
        m = T._model(full_args(input_height=64, input_width=96), None if dtype == F32 else dtype)
        m.train()
        m.dropout_seed = 23
        return m
    model = build()
    model.dropout_step = 0
    with torch.no_grad():
        shapes = [t.shape for t in T._flatten(model(batch))]
    g = torch.Generator().manual_seed(77)
    cots = [(torch.randn(s, generator=g) * 1e-1).to(DEV) for s in shapes]
    model.dropout_step = 5
    g0, o0 = T._grads(model, batch, cots, with_outputs=True)
    # the guarded step runs on a model of its own with the same weights, so that it is this step that
    # builds PackPlan's arena and the merged-head operands and packs every weight (a model that has
    # run before finds its packed weights cached on the parameters' versions and packs nothing)
    twin = build()
    arena = GuardedArena(GUARD_BYTES_MODEL)
    with monkeypatch.context() as mp:
        install(mp, arena)
        twin.dropout_step = 5
        g1, o1 = T._grads(twin, batch, cots, with_outputs=True)
        sites = [(e[3], e[5]) for e in arena._live]
        checked = arena.check()
    ops_sites = sorted({s_.rsplit(':', 1)[0] for s_, _ in sites if s_.startswith('ops.py:')})
    print(f"whole engine {dtype}: allocation sites in ops.py: {ops_sites}")
    assert any(s_.startswith('ops.py:_build:') and d_ == torch.uint8 for s_, d_ in sites), \
        "PackPlan's arena was not allocated under the guard"
    assert any(s_.startswith('ops.py:_build:') and d_ != torch.uint8 for s_, d_ in sites), \
        "the merged-head operands were not allocated under the guard"
    print(f"whole engine {dtype}: {checked} guarded allocations")
    assert checked > 500
    for t in o1:
        assert bool(torch.isfinite(t.float()).all()), 'non-finite output'
    assert set(g0) == set(g1)
    for k, t in g1.items():
        assert bool(torch.isfinite(t).all()), f'non-finite gradient {k}'
    loss0 = sum(float((a.double() * c.double()).sum()) for a, c in zip(o0, cots))
    loss1 = sum(float((a.double() * c.double()).sum()) for a, c in zip(o1, cots))
    assert loss0 == loss1
    for a, b in zip(o0, o1):
        assert torch.equal(a, b), 'forward differs between the guarded and the unguarded run'
    worst, n_diff = 0.0, 0
    gmax = max(float(v.abs().max()) for v in g0.values())
    for k, a in g0.items():
        b = g1[k]
        if torch.equal(a, b):
            continue
        n_diff += 1
        if float((a - b).abs().max()) <= 1e-6 * gmax and float(b.abs().max()) <= 1e-4 * gmax:
            continue
        e = float((a - b).norm() / max(float(b.norm()), 1e-30))
        worst = max(worst, e)
        assert e <= 1e-5, f"{k}: guarded vs unguarded rel-L2 {e:.3e}"
    print(f"whole engine {dtype}: {n_diff} of {len(g0)} gradients differ, worst rel-L2 {worst:.2e}")
    assert n_diff <= len(g0) // 4


# ---------------------------------------------------------------------------------------------
# positive controls: inside memory the test owns
# ---------------------------------------------------------------------------------------------
def _memset(t, nbytes):
    lib = _lib()
    lib.check(lib.lib().emsa_memset_async(t.data_ptr(), 0, nbytes, torch.cuda.current_stream().cuda_stream),
              'emsa_memset_async')


def test_control_overrun_by_four_bytes_is_reported():
    arena = GuardedArena()
    t = arena.alloc((5, 7), DEV)
    _memset(t, t.numel() * 4 + 4)
    with pytest.raises(GuardError) as e:
        arena.check()
    msg = str(e.value)
    print(msg)
    assert 'test_memory_edges_gpu.py:test_control_overrun_by_four_bytes_is_reported' in msg
    assert 'shape (5, 7) torch.float32: rear band damaged, first byte at offset 0 ' in msg and ', 4 bytes' in msg
    assert 'front band' not in msg


def test_control_short_write_leaves_the_last_element_nan():
    arena = GuardedArena()
    t = arena.alloc((5, 7), DEV)
    _memset(t, t.numel() * 4 - 4)
    torch.cuda.synchronize()
    flat = t.view(-1)
    assert bool(torch.isnan(flat[-1])) and bool((flat[:-1] == 0).all())
    with pytest.raises(AssertionError, match='non-finite'):
        close(t, torch.zeros(5, 7), what='short write')
    arena.check()


@pytest.mark.parametrize('dtype', [F32, BF16, torch.int8, torch.int64])
def test_control_put_is_an_exact_copy_with_intact_guards(dtype):
    arena = GuardedArena()
    src = (rnd(2, 5, 3, 7, seed=1) * 8).to(dtype).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    got = arena.put(src)
    assert got.data_ptr() != src.data_ptr() and got.data_ptr() % 256 == 0
    assert got.stride() == src.stride() and torch.equal(got, src)
    assert arena.check() == 1
