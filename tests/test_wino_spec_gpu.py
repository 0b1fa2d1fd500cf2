"""GPU: the 1-D Winograd conv's instantiations with a compile-time epilogue (conv_wino.hip,
`wino_spec_opt`) against the generic kernel of the same launch, bit for bit -- output tensor,
`relu_bits` words, `stats` rows, `bnb` rows -- for every specialised feature set, along W and along
H, on the smallest shapes at which the kernel can still go wrong:

  2x5x7   64->64    odd lines (virtual pixel); 40 (W) / 42 (H) pairs = one full and one partial
                    tile; tiles crossing line and image ends
  1x2x66  64->128   33 pairs per line along W; two channel tiles
  3x4x4   128->64   fewer than 32 pairs; 8 K steps
  1x1x2   64->64    a single pair
  2x5x7   64->40    a channel-tail tile (n_ch < 64) -- where the feature set allows it
  2x5x7   40->64    a partial last channel chunk: the dispatch must keep the generic kernel

and one launch per feature set that must stay on the generic kernel (eval-mode scale / shift, a
float mask_src).  `emsa_conv1d_wino_spec_launches()` counts the specialised launches, so each case also
shows which kernel the dispatch took."""
import functools

import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu

#          n, h, w, cin, cout
SHAPES = [(2, 5, 7, 64, 64), (1, 2, 66, 64, 128), (3, 4, 4, 128, 64), (1, 1, 2, 64, 64)]
TAIL_N = (2, 5, 7, 64, 40)
TAIL_K = (2, 5, 7, 40, 64)
KERNELS = [(1, 3), (3, 1)]


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


def _lib():
    from emsanet_amd import _lib as lib
    return lib.lib()


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = _lib().emsa_conv1d_wino_set_spec(1)
    yield
    _lib().emsa_conv1d_wino_set_spec(prev)


@functools.lru_cache(maxsize=None)
def _case(shape, kernel):
    """the operands of every launch of one (shape, direction), made once"""
    Fn = _fn()
    n, h, w, cin, cout = shape
    pad = (kernel[0] // 2, kernel[1] // 2)
    spec = Fn.ConvSpec(cin, cout, kernel, (1, 1), pad)
    wt = rnd(cout, cin, *kernel, seed=2, scale=0.1).to(DEV)
    u, ud = Fn.pack_wino(wt, fwd=True, dgrad=True)
    d = dict(spec=spec, u=u, ud=ud, hw=(h, w),
             x=to_act(rnd(n, cin, h, w, seed=1)), dy=to_act(rnd(n, cout, h, w, seed=3)),
             res=to_act(rnd(n, cin, h, w, seed=4)), t=to_act(rnd(n, cin, h, w, seed=5)),
             bias=rnd(cout, seed=6).to(DEV),
             in_aff=((rnd(cin, seed=7).abs() + 0.5).to(DEV), (rnd(cin, seed=8) + 0.3).to(DEV)),
             out_aff=((rnd(cout, seed=9).abs() + 0.5).to(DEV), rnd(cout, seed=10).to(DEV)),
             bn=((rnd(cin, seed=11).abs() + 0.5).to(DEV), rnd(cin, seed=12).to(DEV),
                 rnd(cin, seed=13, scale=0.1).to(DEV), (rnd(cin, seed=14).abs() + 0.5).to(DEV)))
    # ReLU bits of an activation with the data gradient's output shape (n, cin, h, w), in the
    # kernel's own layout: about half the bits set
    m = rnd(n, cin, h, w, seed=15)
    words = torch.zeros(n * h * w, (cin + 63) // 64, dtype=torch.int64)
    flat = (m > 0).permute(0, 2, 3, 1).reshape(n * h * w, cin)
    for c in range(cin):
        bit = (c & 3) * 16 + ((c >> 2) & 15)
        sh = torch.tensor(1 << bit if bit < 63 else -(1 << 63), dtype=torch.int64)
        words[:, c // 64] |= flat[:, c].to(torch.int64) * sh
    d['bits'] = words.flatten().to(DEV)
    d['bits']._emsa_wbits = True
    d['mask'] = to_act(m)
    return d


def _flat(res):
    out = []
    for r in res if isinstance(res, (tuple, list)) else (res,):
        if isinstance(r, (tuple, list)):
            out += _flat(r)
        elif torch.is_tensor(r):
            out.append(r)
    return out


def _both(run, specialised):
    """run() on the generic kernel and on the dispatch's choice: the same bits everywhere, and the
    dispatch took a specialised instantiation exactly where `specialised` says so"""
    L = _lib()
    L.emsa_conv1d_wino_set_spec(0)
    ref = [r.clone() for r in _flat(run())]
    assert L.emsa_conv1d_wino_set_spec(1) == 0
    before = L.emsa_conv1d_wino_spec_launches()
    got = _flat(run())
    torch.cuda.synchronize()
    took = L.emsa_conv1d_wino_spec_launches() - before
    assert took == (1 if specialised else 0), f"specialised launches: {took}"
    assert len(ref) == len(got) and len(got) >= 1
    for a, b in zip(ref, got):
        assert a.shape == b.shape and a.dtype == b.dtype
        if a.dtype == torch.float32:
            a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"
    return got


def _k_whole(shape, dgrad=False):
    """the launch's K (input channels; output channels for a data gradient) is whole 16-channel chunks"""
    return (shape[4] if dgrad else shape[3]) % 16 == 0


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('shape', SHAPES + [TAIL_N, TAIL_K])
@pytest.mark.parametrize('inbn', [False, True])
def test_bias_relu_bits(shape, kernel, inbn):
    Fn, d = _fn(), _case(shape, kernel)
    got = _both(lambda: Fn.conv_fwd(d['x'], None, d['spec'], bias=d['bias'], act=Fn.ACT_RELU,
                                    wino_u=d['u'], want_relu_bits=True,
                                    in_affine=d['in_aff'] if inbn else None), _k_whole(shape))
    y, bits = got
    assert torch.isfinite(y).all() and float(y.min()) == 0.0 and bits.dtype == torch.int64


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('shape', SHAPES + [TAIL_N, TAIL_K])
def test_bias_stats(shape, kernel):
    Fn, d = _fn(), _case(shape, kernel)
    y, stats = _both(lambda: Fn.conv_fwd(d['x'], None, d['spec'], bias=d['bias'], want_stats=True,
                                         wino_u=d['u']), _k_whole(shape))
    n, h, w = shape[:3]
    assert torch.isfinite(stats).all() and float(stats[2, :, 0].sum()) == n * h * w


# (emsa_conv1d_wino_resmask takes whole 64-channel output tiles only: not TAIL_K's 40 channels)
DGRAD = [(s, f) for s in SHAPES + [TAIL_N, TAIL_K] for f in ('plain', 'mask_bits', 'res_bits')
         if not (f == 'res_bits' and s[3] % 64)]


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('shape,form', DGRAD)
def test_data_gradient(shape, kernel, form):
    Fn, d = _fn(), _case(shape, kernel)
    kw = {'plain': {}, 'mask_bits': dict(mask_bits=d['bits']),
          'res_bits': dict(residual=d['res'], res_bits=d['bits'])}[form]
    (dx,) = _both(lambda: Fn.conv_dgrad(d['dy'], None, d['spec'], d['hw'], wino_u=d['ud'], **kw),
                  _k_whole(shape, dgrad=True))
    assert torch.isfinite(dx).all()
    if form == 'mask_bits':
        assert not bool(((dx != 0) & ~(d['mask'] > 0)).any()) and float(dx.abs().max()) > 0


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('shape', SHAPES + [TAIL_N, TAIL_K])
@pytest.mark.parametrize('with_res', [False, True])
def test_bnb(shape, kernel, with_res):
    Fn, d = _fn(), _case(shape, kernel)
    sc, sh, mean, invstd = d['bn']

    def run():
        g, partial, rows = Fn.conv_dgrad_bnb(d['dy'], None, d['spec'], d['hw'], d['t'], sc, sh, mean,
                                             invstd, residual=d['res'] if with_res else None,
                                             wino_u=d['ud'])
        return g, partial[:, :rows]               # (the 16 slice-sum rows behind are not the kernel's)
    g, rows = _both(run, _k_whole(shape, dgrad=True))
    assert torch.isfinite(g).all() and torch.isfinite(rows).all()


@pytest.mark.parametrize('kernel', KERNELS)
def test_nan_and_negative_inputs_through_the_relu(kernel):
    """the specialised ReLU is one v_med3 per element: NaN -> 0 like fmaxf, and the bits agree"""
    Fn, d = _fn(), _case(SHAPES[0], kernel)
    x = d['x'].clone()
    x[0, 3, 2, 3] = float('nan')
    x[1, :, 4, 6] = float('-inf')
    _both(lambda: Fn.conv_fwd(x, None, d['spec'], bias=d['bias'], act=Fn.ACT_RELU, wino_u=d['u'],
                              want_relu_bits=True), True)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('case', ['eval_affine', 'eval_affine_relu', 'float_mask', 'float_mask_res'])
def test_other_operand_sets_keep_the_generic_kernel(kernel, case):
    Fn, d = _fn(), _case(SHAPES[0], kernel)
    sc, sh = d['out_aff']
    if case.startswith('eval'):
        run = lambda: Fn.conv_fwd(d['x'], None, d['spec'], bias=d['bias'], scale=sc, shift=sh,   # noqa: E731
                                  act=Fn.ACT_RELU if case.endswith('relu') else Fn.ACT_NONE,
                                  wino_u=d['u'])
    else:
        run = lambda: Fn.conv_dgrad(d['dy'], None, d['spec'], d['hw'], mask_src=d['mask'],       # noqa: E731
                                    residual=d['res'] if case.endswith('res') else None,
                                    wino_u=d['ud'])
    (y,) = _both(run, False)
    assert torch.isfinite(y).all()


def test_switch_entry_point():
    L = _lib()
    assert L.emsa_conv1d_wino_set_spec(0) == 1 and L.emsa_conv1d_wino_set_spec(0) == 0
    assert L.emsa_conv1d_wino_set_spec(7) == 0 and L.emsa_conv1d_wino_set_spec(1) == 1
    n = L.emsa_conv1d_wino_spec_launches()
    assert n >= 0 and L.emsa_conv1d_wino_spec_launches() == n
