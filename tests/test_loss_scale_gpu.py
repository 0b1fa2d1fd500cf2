"""The loss-scaler kernels of csrc/loss_scale.hip on the device: the non-finite scan (exact flags,
read-only), the one-thread state update against the restatement of loss_scale_reference.py (every
field, every step), and the scaled optimizer updates against the plain ones (bit for bit at
power-of-two scales; nothing moves on a skipped step).  Operands lie flush between guard bands."""
import numpy as np
import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from loss_scale_reference import ScalerState
from util import DEV

pytestmark = pytest.mark.gpu

I32 = torch.int32
# +inf, -inf, a quiet NaN, a NaN with only the lowest mantissa bit set (int32 bit patterns)
NONFINITE = {'+inf': 0x7F800000, '-inf': 0xFF800000 - (1 << 32), 'qnan': 0x7FC00000, 'nan-lsb': 0x7F800001}
# finite values the scan must let pass: the largest magnitudes, both zeros, subnormals
FINITE_EDGES = np.array([3.4028235e38, -3.4028235e38, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38,
                         -1.1754942e-38, 1.17549435e-38], dtype=np.float32)


def _L():
    from emsanet_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _new_state(scale=1.0, skip=0, n=1):
    """n EmsaLossScale records: float32 view and int32 view of the same 32-byte records"""
    f = torch.zeros(n, 8, dtype=torch.float32, device=DEV)
    f[:, 0] = scale
    f[:, 1] = 1.0 / scale
    i = f.view(I32)
    i[:, 2] = skip
    return f, i


def _finite_fill(n, seed):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 1e3).astype(np.float32)
    k = min(n, FINITE_EDGES.size)
    v[rng.permutation(n)[:k]] = FINITE_EDGES[:k]
    if n >= 2:                       # the extremes sit at both ends too (head and tail paths)
        v[0], v[-1] = FINITE_EDGES[0], FINITE_EDGES[1]
    return torch.from_numpy(v)


def _positions(n, off):
    """first element, last element, last element of the float4 body, first of the tail (those that
    exist) for a view that starts `off` floats past a 16-byte boundary"""
    head = min((4 - off) % 4, n)
    n4 = (n - head) // 4
    pos = {0, n - 1}
    if n4 > 0:
        pos.add(head + 4 * n4 - 1)
    if head + 4 * n4 < n:
        pos.add(head + 4 * n4)
    return sorted(pos)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1025, 2 ** 20 + 3])
def test_nonfinite_scan_flags_are_exact_and_gradients_untouched(n, guard_allocations):
    L, A = _L(), guard_allocations
    lib = L.lib()
    cases = []          # (offset, what, position or None)
    same = []
    for off in (0, 1, 2, 3):                 # views 0 / 4 / 8 / 12 bytes past a 16-byte boundary
        host = torch.zeros(off + n)
        host[off:] = _finite_fill(n, seed=n + off)
        buf = A.put(host.to(DEV))            # the view ends flush against the rear guard
        g = buf[off:]
        assert g.data_ptr() % 16 == 4 * off
        want = g.view(I32).clone()
        gi = g.view(I32)
        jobs = [(None, None)] + [(name, p) for name in NONFINITE for p in _positions(n, off)]
        f, i = _new_state(n=len(jobs))
        for j, (name, p) in enumerate(jobs):
            expect = want
            if name is not None:
                expect = want.clone()
                expect[p] = NONFINITE[name]
                gi[p] = NONFINITE[name]
            L.check(lib.emsa_nonfinite_scan(g.data_ptr(), n, f[j].data_ptr(), _stream()), 'scan')
            same.append(torch.equal(gi, expect))          # read-only: the bits it scanned are still there
            if name is not None:
                gi[p] = want[p]
            cases.append((off, name, p))
        flags = i[:, 6].cpu().tolist()
        rest = torch.cat([i[:, :6], i[:, 7:]], 1).cpu()
        for (name, p), flag in zip(jobs, flags):
            assert flag == (0 if name is None else 1), f"n={n} offset={off}: {name} at {p} -> found={flag}"
        # nothing but `found` is written
        f0, i0 = _new_state(n=len(jobs))
        assert torch.equal(rest, torch.cat([i0[:, :6], i0[:, 7:]], 1).cpu())
        assert torch.equal(gi, want)
    assert all(same)
    A.check()


def test_nonfinite_scan_never_clears_the_flag_and_refuses_bad_arguments(guard_allocations):
    L, A = _L(), guard_allocations
    lib = L.lib()
    f, i = _new_state()
    i[0, 6] = 1
    g = A.put(torch.ones(37, device=DEV))
    L.check(lib.emsa_nonfinite_scan(g.data_ptr(), 37, f.data_ptr(), _stream()), 'scan')
    assert int(i[0, 6]) == 1
    assert lib.emsa_nonfinite_scan(None, 4, f.data_ptr(), _stream()) == -2
    assert lib.emsa_nonfinite_scan(g.data_ptr(), 4, None, _stream()) == -2
    assert lib.emsa_nonfinite_scan(g.data_ptr() + 2, 4, f.data_ptr(), _stream()) == -1
    assert lib.emsa_loss_scale_update(f.data_ptr(), 1.0, 0.5, 3, _stream()) == -2
    assert lib.emsa_loss_scale_update(f.data_ptr(), 2.0, 1.0, 3, _stream()) == -2
    assert lib.emsa_loss_scale_update(f.data_ptr(), 2.0, 0.5, 0, _stream()) == -2
    A.check()


SEQUENCES = {
    'clean': [False] * 12,
    'mixed': [False, False, True, False, False, False, True, True, False, False, False, False],
    'all-bad': [True] * 12,
    'alternating': [False, True] * 6,
}


@pytest.mark.parametrize('init,growth,backoff', [(2.0 ** 16, 2.0, 0.5), (2.0 ** 126, 2.0, 0.5), (1.5, 3.0, 0.25)])
@pytest.mark.parametrize('seq', list(SEQUENCES))
def test_state_update_equals_the_restatement(seq, init, growth, backoff, guard_allocations):
    """12 steps, growth_interval 3: every field after every step (2^126: growth suppressed where it
    would leave float32).  `found` is raised by real scans of a clean and a poisoned bucket."""
    L, A = _L(), guard_allocations
    lib = L.lib()
    good = A.put(torch.ones(9, device=DEV))
    bad = A.put(torch.tensor([1.0] * 8 + [float('inf')], device=DEV))
    ref = ScalerState(init, growth, backoff, 3)
    f, i = _new_state(scale=init)
    for step, found in enumerate(SEQUENCES[seq]):
        L.check(lib.emsa_nonfinite_scan(good.data_ptr(), 9, f.data_ptr(), _stream()), 'scan')
        if found:
            L.check(lib.emsa_nonfinite_scan(bad.data_ptr(), 9, f.data_ptr(), _stream()), 'scan')
            L.check(lib.emsa_nonfinite_scan(good.data_ptr(), 9, f.data_ptr(), _stream()), 'scan')
        L.check(lib.emsa_loss_scale_update(f.data_ptr(), growth, backoff, 3, _stream()), 'update')
        ref.update(found)
        hf, hi = f.cpu()[0], i.cpu()[0]
        got = {'scale': float(hf[0]), 'inv_scale': float(hf[1]), 'skip': int(hi[2]),
               'growth_tracker': int(hi[3]), 'steps': int(hi[4]), 'skipped': int(hi[5]), 'found': int(hi[6])}
        assert got == ref.fields(), f"{seq} step {step}: {got} != {ref.fields()}"
        assert int(hi[7]) == 0
    A.check()


# ---- scaled optimizer updates -------------------------------------------------------------------
SCALES = [1.0, 2.0 ** 16, 2.0 ** -3]
SIZES = [5, 4099]


def _rand(n, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)).to(DEV)


def _bits(t):
    return t.view(I32) if t.dtype == torch.float32 else t.view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('dev_hyper', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('first', [1, 0])
@pytest.mark.parametrize('n', SIZES)
def test_scaled_sgd_equals_plain_sgd_bit_for_bit(n, first, wd, dev_hyper, guard_allocations):
    L, A = _L(), guard_allocations
    lib = L.lib()
    lr, mu, gs = 0.03, 0.9, 0.5
    p0, g0, m0 = _rand(n, 1), _rand(n, 2, 0.1), _rand(n, 3, 0.1)
    hyper = A.put(torch.tensor([lr, mu, wd, gs, float(first), 0, 0, 0], device=DEV)) if dev_hyper else None
    hp = hyper.data_ptr() if dev_hyper else None
    p, g, m = A.put(p0), A.put(g0), A.put(m0)
    if dev_hyper:
        L.check(lib.emsa_sgd_nesterov_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, hp, _stream()), 'sgd')
    else:
        L.check(lib.emsa_sgd_nesterov(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, lr, mu, wd, gs, first,
                                      _stream()), 'sgd')
    assert not _same(p, p0)
    for S in SCALES:
        f, _ = _new_state(scale=S)
        ps, gS, ms = A.put(p0), A.put(g0 * S), A.put(m0)
        L.check(lib.emsa_sgd_nesterov_ls(ps.data_ptr(), gS.data_ptr(), ms.data_ptr(), n, lr, mu, wd, gs,
                                         first, hp, f.data_ptr(), _stream()), 'sgd_ls')
        assert _same(ps, p) and _same(ms, m), f"scale {S}"
        assert _same(gS, g0 * S)
        # skip = 1: nothing moves, whatever the gradient holds
        f, _ = _new_state(scale=S, skip=1)
        gbad = g0 * S
        gbad[n // 2] = float('nan')
        pk, gk, mk = A.put(p0), A.put(gbad), A.put(m0)
        L.check(lib.emsa_sgd_nesterov_ls(pk.data_ptr(), gk.data_ptr(), mk.data_ptr(), n, lr, mu, wd, gs,
                                         first, hp, f.data_ptr(), _stream()), 'sgd_ls')
        assert _same(pk, p0) and _same(mk, m0)
    A.check()


def _adam_hyper(mode, wd, gs):
    return torch.tensor([0.01, 0.9, 0.999, 1e-8, wd, gs, float(mode), 0.0], dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('steps_before', [0, 7])       # 7: RAdam's rectified branch (rho_t > 5)
@pytest.mark.parametrize('mode', [0, 1, 2], ids=['adam', 'adamw', 'radam'])
@pytest.mark.parametrize('n', SIZES)
def test_scaled_adam_equals_plain_adam_bit_for_bit(n, mode, steps_before, guard_allocations):
    L, A = _L(), guard_allocations
    lib = L.lib()
    hyper = A.put(_adam_hyper(mode, 1e-4, 0.5))
    st0 = A.put(torch.zeros(8, dtype=torch.float64, device=DEV))
    for _ in range(steps_before):
        L.check(lib.emsa_adam_advance(hyper.data_ptr(), st0.data_ptr(), _stream()), 'advance')
    p0, g0 = _rand(n, 1), _rand(n, 2, 0.1)
    m0, v0 = _rand(n, 3, 0.1), _rand(n, 4, 0.1).abs()
    p, g, m, v, st = A.put(p0), A.put(g0), A.put(m0), A.put(v0), A.put(st0)
    L.check(lib.emsa_adam_advance(hyper.data_ptr(), st.data_ptr(), _stream()), 'advance')
    L.check(lib.emsa_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(),
                               st.data_ptr(), _stream()), 'adam')
    assert float(st[0]) == steps_before + 1 and not _same(p, p0)
    if mode == 2:
        assert float(st[5]) == (1.0 if steps_before else 0.0)
    for S in SCALES:
        f, _ = _new_state(scale=S)
        ps, gS, ms, vs, sts = A.put(p0), A.put(g0 * S), A.put(m0), A.put(v0), A.put(st0)
        L.check(lib.emsa_adam_advance_ls(hyper.data_ptr(), sts.data_ptr(), f.data_ptr(), _stream()), 'advance_ls')
        L.check(lib.emsa_adam_step_ls(ps.data_ptr(), gS.data_ptr(), ms.data_ptr(), vs.data_ptr(), n,
                                      hyper.data_ptr(), sts.data_ptr(), f.data_ptr(), _stream()), 'adam_ls')
        assert _same(ps, p) and _same(ms, m) and _same(vs, v) and _same(sts, st), f"scale {S}"
        f, _ = _new_state(scale=S, skip=1)
        gbad = g0 * S
        gbad[n // 2] = float('inf')
        pk, gk, mk, vk, stk = A.put(p0), A.put(gbad), A.put(m0), A.put(v0), A.put(st0)
        L.check(lib.emsa_adam_advance_ls(hyper.data_ptr(), stk.data_ptr(), f.data_ptr(), _stream()), 'advance_ls')
        L.check(lib.emsa_adam_step_ls(pk.data_ptr(), gk.data_ptr(), mk.data_ptr(), vk.data_ptr(), n,
                                      hyper.data_ptr(), stk.data_ptr(), f.data_ptr(), _stream()), 'adam_ls')
        # parameters, both moments and the device step count: untouched
        assert _same(pk, p0) and _same(mk, m0) and _same(vk, v0) and _same(stk, st0)
    A.check()


def _tiny_problem(seed=0):
    from emsanet_amd.optim import FusedSGD
    from emsanet_amd.parallel import GradientBuckets
    ps = [torch.nn.Parameter(_rand(n, seed + k)) for k, n in enumerate(SIZES)]
    buckets = GradientBuckets(ps)
    return ps, buckets, FusedSGD(buckets, lr=0.03, momentum=0.9, weight_decay=1e-4)


def _step(ps, buckets, grads, do_step):
    buckets.reset()
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    buckets.finish()
    do_step()


@pytest.mark.parametrize('dev_hyper', [False, True])
def test_skipped_first_sgd_step_then_clean_one_equals_one_clean_first_step(dev_hyper):
    """FusedSGD's first-step flag is a host flag with no device twin: a skipped first step leaves the
    momentum buffers at zero, and the next step, run with first = 0, forms momentum * 0 + g = g"""
    from emsanet_amd.optim import LossScaler
    grads = [_rand(n, 10 + k, 0.1) for k, n in enumerate(SIZES)]
    ps_a, b_a, opt_a = _tiny_problem()
    ps_b, b_b, opt_b = _tiny_problem()
    if dev_hyper:
        opt_a.use_device_hyperparameters(True)
        opt_b.use_device_hyperparameters(True)
    _step(ps_a, b_a, grads, opt_a.step)                              # one clean first step
    scaler = LossScaler(opt_b, init_scale=4.0, growth_interval=100)
    before = [fp.clone() for fp in opt_b.flat_params]
    bad = [g * 4.0 for g in grads]
    bad[1][17] = float('inf')
    _step(ps_b, b_b, bad, scaler.step)                               # skipped: scale 4 -> 2
    assert scaler.state() == {'scale': 2.0, 'growth_tracker': 0, 'steps': 1, 'skipped': 1}
    assert all(_same(a, b) for a, b in zip(opt_b.flat_params, before))
    assert all(int((m != 0).sum()) == 0 for m in opt_b.flat_momentum)
    assert not opt_b._first
    _step(ps_b, b_b, [g * 2.0 for g in grads], scaler.step)          # clean, under scale 2
    assert scaler.state() == {'scale': 2.0, 'growth_tracker': 1, 'steps': 2, 'skipped': 1}
    for a, b in zip(opt_a.flat_params + opt_a.flat_momentum, opt_b.flat_params + opt_b.flat_momentum):
        assert _same(a, b)
    for a, b in zip(ps_a, ps_b):
        assert _same(a.data, b.data) and b._version > 0


def test_scaler_state_dict_round_trip():
    from emsanet_amd.optim import LossScaler
    ps, b, opt = _tiny_problem()
    s1 = LossScaler(opt, init_scale=8.0, growth_interval=1)
    _step(ps, b, [_rand(n, 20 + k, 0.1) for k, n in enumerate(SIZES)], s1.step)
    sd = s1.state_dict()
    s2 = LossScaler(opt, init_scale=1.0, growth_interval=1)
    s2.load_state_dict(sd)
    assert s2.state() == s1.state() == {'scale': 16.0, 'growth_tracker': 0, 'steps': 1, 'skipped': 0}
