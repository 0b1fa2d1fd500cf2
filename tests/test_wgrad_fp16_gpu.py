"""fp32 weight / bias gradients from float16 activations (emsa_conv_wgrad_t with EMSA_DT_F16): the
16-bit weight-gradient family instantiated for fp16 -- the tap-group kernel, the direct 16-bit modes
(1x1, stride-2 3-tap, stem rows), the transposing-read kernel, both the two-pass deterministic form
and the atomic form.

Reference: fp64 conv2d on the operands rounded to fp16.  The tolerance is the bf16 tests' own 2e-4:
the product of two 11-bit mantissas is exact in fp32 as the product of two 8-bit ones is, what remains
is the fp32 accumulation order, which is the same kernel's.

The shape tables are imported from the bf16 tests, not copied: tests/test_ops16_gpu.py (CONVS) and
tests/test_memory_edges_gpu.py (EDGE: cout 8 / 12 / 40 / 72 / 136 and the 1x1x2 map; SPLIT).  Every
output and scratch buffer is poisoned and guard-banded (guard.py)."""
import pytest
import torch
import torch.nn.functional as F

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from test_memory_edges_gpu import EDGE, SPLIT, _h_ok, _ids, _Ops, _ref, _spec
from test_ops16_gpu import CONVS, act16, q
from util import DEV, close, rnd

pytestmark = pytest.mark.gpu

F16 = torch.float16


def _fn():
    from emsanet_amd import functional as Fn
    return Fn


@pytest.mark.parametrize('two_pass', [True, False])
@pytest.mark.parametrize('cfg', CONVS)
def test_conv_wgrad_fp16(cfg, two_pass):
    """the CONVS table of test_conv16_wgrad in fp16 storage, both forms"""
    Fn = _fn()
    cin, cout, k, s, p, n, h, w = cfg
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, *k, seed=2, scale=0.1).double().requires_grad_(True)
    b = rnd(cout, seed=3).double().requires_grad_(True)
    y = F.conv2d(q(x, F16), wt, b, stride=s, padding=p)
    dy = rnd(*y.shape, seed=7)
    y.backward(q(dy, F16))
    spec = Fn.ConvSpec(cin, cout, k, s, p)
    like = torch.empty(cout, cin, *k, device=DEV)
    dw, db, packed = Fn.conv_wgrad(act16(x, F16), act16(dy, F16), spec, True, like=like,
                                   two_pass=two_pass)
    if packed:
        dw = Fn.unpack_wgrad(dw, like)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    close(dw, wt.grad, tol=2e-4, what=f'wgrad fp16 (two_pass={two_pass})')
    close(db, b.grad, tol=2e-4, what=f'dbias fp16 (two_pass={two_pass})')


@pytest.mark.parametrize('cfg', EDGE + SPLIT, ids=_ids)
def test_conv_wgrad_fp16_ragged_between_guards(cfg, guard_allocations):
    """the ragged geometries and the two tap-split shapes of test_memory_edges_gpu.py, operands flush
    between NaN guards: the gate of its test_wgrad_bf16, guard bands intact"""
    from emsanet_amd import _lib
    Fn, A = _fn(), guard_allocations
    cin, cout, k, s, p, n, h, w = cfg
    r, spec = _ref(cfg, F16), _spec(Fn, cfg)
    o = _Ops(A, r, F16)
    x, dy = o.act('x'), o.act('dy')
    like = torch.empty(cout, cin, *k, device=DEV)
    for two_pass in (True, False):
        try:
            dw, db, packed = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=two_pass)
        except _lib.EmsaError:
            # refused on the host: only a geometry off the 8-channel rule of the 16-bit loaders
            assert not _h_ok(cfg), 'a supported geometry was refused'
            continue
        if packed:
            dw = Fn.unpack_wgrad(dw, like)
        close(dw, r['dw'], tol=2e-4, what=f'wgrad fp16 (two_pass={two_pass})')
        close(db, r['db'], tol=2e-4, what=f'dbias fp16 (two_pass={two_pass})')
    A.check()


@pytest.mark.parametrize('cin', [3, 1])
def test_stem_wgrad_fp16(cin):
    """the 16-bit stem weight gradient in fp16 (setup of test_stem16's bf16 branch): the NHWC4 route
    (cin 3) and the rows-as-channels route (cin 1)"""
    Fn = _fn()
    n, h, w = 2, 32, 48
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(64, cin, 7, 7, seed=2, scale=0.1)
    spec = Fn.StemSpec(cin, 64)
    assert spec.rows == (cin == 1)
    xp = Fn.stem_pack_input(x.to(DEV), F16)
    wd = wt.double().requires_grad_(True)
    yy = F.conv2d(q(x, F16), wd, None, stride=2, padding=3)
    dy = rnd(*yy.shape, seed=5)
    yy.backward(q(dy, F16))
    dw = Fn.stem_wgrad(xp, act16(dy, F16), spec, n, h, w, wt.to(DEV))
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32
    close(dw, wd.grad, tol=2e-4, what='stem wgrad fp16')


@pytest.mark.parametrize('cfg', [CONVS[0], CONVS[8], CONVS[18], CONVS[20]],
                         ids=['tr-3x1', 'tr-3x3', 'mode1-1x1', 'mode2-s2'])
def test_two_pass_fp16_is_bit_reproducible(cfg):
    """the two-pass form (split-K partial tiles + reduction pass, no atomics) run twice gives
    identical bits: the transposing-read kernel and the direct 16-bit modes 1 and 2"""
    Fn = _fn()
    cin, cout, k, s, p, n, h, w = cfg
    spec = Fn.ConvSpec(cin, cout, k, s, p)
    oh, ow = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    x, dy = act16(rnd(n, cin, h, w, seed=1), F16), act16(rnd(n, cout, oh, ow, seed=7), F16)
    like = torch.empty(cout, cin, *k, device=DEV)
    runs = []
    for _ in range(2):
        dw, db, packed = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=True)
        assert not packed, 'this geometry has a two-pass form in bf16'
        torch.cuda.synchronize()
        runs.append((dw.clone(), db.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all())
