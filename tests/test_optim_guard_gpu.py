"""The optimizer update kernels (csrc/optim_step.h: emsa_sgd_nesterov, emsa_sgd_nesterov_dev,
emsa_adam_step and their `_ls` forms) between guard bands, called through the wrappers of
emsanet_amd/optim.py: `FusedSGD.step`, `FusedAdam.step`, `LossScaler.step`.

optim.py keeps its parameter, gradient and moment buffers for the whole run and allocates them itself,
so the guarded allocator never sees them.  Here the flat parameter, gradient, momentum (and second
moment) vectors, the hyper-parameter rows and the scaler state are placed with `arena.put`, flush
between two bands of 0xFF: a vector store of the float4 body or a scalar store of the tail past the
n-th element changes a guard byte, a load past it reads NaN into the result.

Lengths: 1, 3 (tail only), 4 (body only), 5, 1023, 1025, and 4 * 256 * K + {0, 1, 2, 3} with K = 6145:
the launch is capped at 2048 workgroups of 256 threads, one float4 each, so 256 * K = 1,573,120 vectors
are three whole grid strides and 256 vectors of a fourth, with every tail length behind them.

Reference: the same formulas (torch.optim's SGD with Nesterov momentum, Adam, AdamW, RAdam, as
tests/test_optim.py compares against) evaluated in float64 with torch on the fp32 inputs.  Tolerance: the
one of tests/test_optim.py for these kernels, max |difference| <= 2e-6 * max(1, max |reference|), for the
parameters and for the moments.  With the loss scaler's skip flag set, parameters and moments are
bit-identical to their inputs."""
import math

import numpy as np
import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV

pytestmark = pytest.mark.gpu

K = 6145
LENGTHS = [1, 3, 4, 5, 1023, 1025] + [4 * 256 * K + r for r in range(4)]
RTOL = 2e-6                                   # tests/test_optim.py
LR, MU, WD = 0.03, 0.9, 1e-4
BETAS, EPS = (0.9, 0.999), 1e-8
SCALE = 2.0 ** 16                             # the scaler's initial scale: g * SCALE is exact


def _rand(n, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)).to(DEV)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _close(got, ref, what):
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), what
    err = float((got.double() - ref).abs().max())
    bound = RTOL * max(1.0, float(ref.abs().max()))
    print(f"{what}: max |kernel - float64| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)


class _OneBucket:
    """what the fused optimizers read of `GradientBuckets`: one flat gradient, whose only parameter's
    `.grad` is the bucket itself (nothing to gather); world = 2 without averaging makes the update
    kernel fold grad_scale = 0.5 in"""

    def __init__(self, g, world):
        self.par = torch.nn.Parameter(torch.zeros_like(g))
        self.par.grad = g
        self.buckets = [(g, [self.par], [g])]
        self.active, self.average, self.world = world > 1, False, world


def _guard_scaler(A, opt):
    from emsanet_amd.optim import LossScaler
    sc = LossScaler(opt, init_scale=SCALE)
    sc._f = A.put(sc._f)                      # the 32 bytes of device state between guards too
    sc._i, sc._scale = sc._f.view(torch.int32), sc._f[0]
    return sc


# ---- SGD ----------------------------------------------------------------------------------------------
def _sgd_reference(p, g, m, first, gs):
    p, g, m = p.double(), g.double(), m.double()
    d = g * gs + WD * p
    b = d if first else MU * m + d
    return p - LR * (d + MU * b), b


@pytest.mark.parametrize('ls', [False, True], ids=['plain', 'ls'])
@pytest.mark.parametrize('dev_hyper', [False, True], ids=['args', 'dev'])
@pytest.mark.parametrize('n', LENGTHS)
def test_sgd_nesterov_through_fused_sgd(n, dev_hyper, ls, guard_allocations):
    """two steps, the first with the first-step rule (momentum buffer not read), the second without"""
    from emsanet_amd.optim import FusedSGD
    A = guard_allocations
    world = 2
    p0, g0, m0 = _rand(n, 1), _rand(n, 2, 0.1), _rand(n, 3, 0.1)
    p, m = A.put(p0), A.put(m0)
    g = A.put(g0 * SCALE if ls else g0)
    b = _OneBucket(g, world)
    opt = FusedSGD(b, lr=LR, momentum=MU, weight_decay=WD)
    opt.flat_params, opt.flat_momentum = [p], [m]
    if dev_hyper:
        opt.use_device_hyperparameters()
        opt._hyper = A.put(opt._hyper)
    sc = _guard_scaler(A, opt) if ls else None
    for first in (True, False):
        assert opt._first == first
        before_p, before_m = p.clone(), m.clone()
        (sc or opt).step()
        ref_p, ref_m = _sgd_reference(before_p, g0, before_m, first, 1.0 / world)
        _close(p, ref_p, f"sgd n={n} first={first} p")
        _close(m, ref_m, f"sgd n={n} first={first} m")
        assert _same(g, g0 * SCALE if ls else g0)                   # the gradient is read only
    assert not _same(p, p0)
    if ls:
        assert sc.state()['skipped'] == 0 and sc.state()['steps'] == 2
    A.check()


@pytest.mark.parametrize('dev_hyper', [False, True], ids=['args', 'dev'])
@pytest.mark.parametrize('n', LENGTHS)
def test_sgd_skipped_step_moves_nothing(n, dev_hyper, guard_allocations):
    """an inf in the last element (the tail's, or the body's last lane): the scan finds it, the state
    update sets the skip flag, and the update kernel leaves p and m bit for bit"""
    from emsanet_amd.optim import FusedSGD
    A = guard_allocations
    p0, g0, m0 = _rand(n, 1), _rand(n, 2, 0.1) * SCALE, _rand(n, 3, 0.1)
    g0[n - 1] = float('inf')
    p, g, m = A.put(p0), A.put(g0), A.put(m0)
    opt = FusedSGD(_OneBucket(g, 1), lr=LR, momentum=MU, weight_decay=WD)
    opt.flat_params, opt.flat_momentum = [p], [m]
    opt._first = False                                              # (so that m would be read and written)
    if dev_hyper:
        opt.use_device_hyperparameters()
        opt._hyper = A.put(opt._hyper)
    sc = _guard_scaler(A, opt)
    sc.step()
    A.check()
    assert _same(p, p0) and _same(m, m0) and _same(g, g0)
    st = sc.state()
    assert st['skipped'] == 1 and st['steps'] == 1 and st['scale'] == SCALE / 2
    assert int(sc._i[sc._SKIP]) == 1


# ---- Adam family ----------------------------------------------------------------------------------------
def _adam_reference(p, g, m, v, mode, t, gs):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    b1, b2 = BETAS
    g = g * gs
    if mode == 'adamw':
        p = p * (1.0 - LR * WD)
    else:
        g = g + WD * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if mode != 'radam':
        return p - (LR / bc1) * m / (v.sqrt() / math.sqrt(bc2) + EPS), m, v
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * t * b2 ** t / bc2
    if rho_t > 5.0:
        rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
        return p - (m / bc1) * LR * (math.sqrt(bc2) / (v.sqrt() + EPS)) * rect, m, v
    return p - (m / bc1) * LR, m, v


def _adam(A, n, mode, world, g, p, m, v, steps_before):
    from emsanet_amd.optim import FusedAdam
    opt = FusedAdam(_OneBucket(g, world), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, mode=mode)
    opt.flat_params, opt.exp_avg, opt.exp_avg_sq = [p], [m], [v]
    opt._hyper, opt._state = A.put(opt._hyper), A.put(opt._state)
    opt._state[0] = float(steps_before)
    opt.flat_momentum = opt.exp_avg + opt.exp_avg_sq + [opt._state]
    return opt


@pytest.mark.parametrize('ls', [False, True], ids=['plain', 'ls'])
@pytest.mark.parametrize('mode,steps_before', [('adam', 0), ('adamw', 0), ('radam', 0), ('radam', 7)])
@pytest.mark.parametrize('n', LENGTHS)
def test_adam_step_through_fused_adam(n, mode, steps_before, ls, guard_allocations):
    """two steps; RAdam from step 1 (plain momentum) and from step 8 (rectified, rho_t > 5)"""
    A = guard_allocations
    world = 2
    p0, g0 = _rand(n, 1), _rand(n, 2, 0.1)
    m0, v0 = _rand(n, 3, 0.1), _rand(n, 4, 0.1).abs()
    p, m, v = A.put(p0), A.put(m0), A.put(v0)
    g = A.put(g0 * SCALE if ls else g0)
    opt = _adam(A, n, mode, world, g, p, m, v, steps_before)
    sc = _guard_scaler(A, opt) if ls else None
    for t in (steps_before + 1, steps_before + 2):
        before = p.clone(), m.clone(), v.clone()
        (sc or opt).step()
        assert opt.step_count == t
        ref_p, ref_m, ref_v = _adam_reference(before[0], g0, before[1], before[2], mode, t, 1.0 / world)
        for name, got, ref in (('p', p, ref_p), ('m', m, ref_m), ('v', v, ref_v)):
            _close(got, ref, f"{mode} n={n} t={t} {name}")
        assert _same(g, g0 * SCALE if ls else g0)
    if mode == 'radam':
        assert float(opt._state[5]) == (1.0 if steps_before else 0.0)   # the branch the case is about
    A.check()


@pytest.mark.parametrize('mode', ['adam', 'adamw', 'radam'])
@pytest.mark.parametrize('n', LENGTHS)
def test_adam_skipped_step_moves_nothing(n, mode, guard_allocations):
    A = guard_allocations
    p0, g0 = _rand(n, 1), _rand(n, 2, 0.1) * SCALE
    m0, v0 = _rand(n, 3, 0.1), _rand(n, 4, 0.1).abs()
    g0[n - 1] = float('nan')
    p, g, m, v = A.put(p0), A.put(g0), A.put(m0), A.put(v0)
    opt = _adam(A, n, mode, 1, g, p, m, v, 7)
    state0 = opt._state.clone()
    sc = _guard_scaler(A, opt)
    sc.step()
    A.check()
    assert _same(p, p0) and _same(m, m0) and _same(v, v0)
    assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
    assert opt.step_count == 7 and torch.equal(opt._state, state0)      # Adam's step count does not advance
    assert sc.state()['skipped'] == 1 and sc.state()['scale'] == SCALE / 2
