"""GPU: a hand-made ops.PackPlan over four runtimes that between them have every form and every job
kind of `emsa_pack_batch`.  After `refresh(dtype)` each operand the plan installed -- a view of its
arena or a merged head's persistent operand, allocated poisoned and guard-banded (tests/guard.py) --
equals, bit for bit, the one a fresh runtime over the same parameters packs by itself."""
import ctypes

import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FORMS = ('gemm', 'wino', 'wino2d', 'frag', 'bias')
# job kinds of include/emsanet_hip.h each table must hold: [tap][n][k] (0 / 2 / 3), U (1), bias copy (4),
# fragment-ordered (5 / 6), U2 (7)
KINDS = {F32: {0, 1, 4, 7}, BF16: {2, 4, 5}, F16: {3, 4, 6}}


def _conv(cin, cout, k, pad, seed, bias=False):
    c = torch.nn.Conv2d(cin, cout, k, padding=pad, bias=bias)
    with torch.no_grad():
        c.weight.copy_(rnd(*c.weight.shape, seed=seed, scale=0.1))
        if bias:
            c.bias.copy_(rnd(cout, seed=seed + 50))
    return c.to(DEV)


@pytest.mark.parametrize('trainable', [True, False], ids=['trainable', 'frozen'])
@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=['fp32', 'bf16', 'fp16'])
def test_plan_installs_what_each_runtime_packs_itself(dtype, trainable, guard_allocations):
    """the smallest set that reaches every kind and both one- and two-sided operands: a 3x1 conv 64->64
    (U; 16-bit: [tap][n][k] + fragment-ordered), a 3x3 conv 128->40 of the per-shape rule (U + U2, both
    channel counts multiples of 8), a 1x1 conv 64->128 ([tap][n][k] only) and two biased 3x3 convs
    128->20 merged into one 128->40 head (U + U2 + bias; 16-bit: [tap][n][k] + bias)"""
    from emsanet_amd import _lib, functional as Fn, ops
    assert (128, 40) in Fn.WINO2D_SHAPES
    convs = [_conv(64, 64, (3, 1), (1, 0), 1), _conv(128, 40, 3, 1, 2), _conv(64, 128, 1, 0, 3)]
    heads = [_conv(128, 20, 3, 1, 4, bias=True), _conv(128, 20, 3, 1, 5, bias=True)]
    for c in convs + heads:
        for p in c.parameters():
            p.requires_grad_(trainable)

    def runtimes():
        return [ops.ConvRT(c) for c in convs] + \
            [ops.MultiConvRT([(heads[0], 0, 0), (heads[1], 20, 0)], 40, 128, 3, 1)]
    planned, alone = runtimes(), runtimes()
    assert [(rt.wino, rt.wino2d) for rt in planned] == [(True, False), (True, True), (False, False), (True, True)]
    assert planned[0].rs and Fn.CONV_RS
    plan = ops.PackPlan(planned)
    plan.refresh(dtype)
    assert not plan._lean                          # (a first table is always the full one)
    raw = plan._jobs.cpu().numpy().tobytes()
    jobs = (_lib.EmsaPackJob * (len(raw) // ctypes.sizeof(_lib.EmsaPackJob))).from_buffer_copy(raw)
    assert {j.kind for j in jobs} == KINDS[dtype]
    compared = 0
    for rt, fresh in zip(planned, alone):
        installed = {}
        for form in FORMS:
            for dt in (F32, BF16, F16):
                sides = rt.packs.peek(form, dt, rt.key_now())
                if sides != (None, None):
                    installed[form, dt] = sides
        # every form of the declaration that has a job, in its own element type, and nothing else
        assert set(installed) == {(f.name, f.dtype) for f in rt.forms(dtype) if f.kind is not None}
        for (form, dt), sides in installed.items():
            two_sided = form != 'bias' and (trainable or isinstance(rt, ops.MultiConvRT))
            assert sides[0] is not None and (sides[1] is not None) == two_sided, (form, dt)
            for side, got in enumerate(sides):
                if got is not None:
                    want = fresh.weights(form, side, dt)
                    assert got.dtype == want.dtype == dt and got.shape == want.shape, (form, side)
                    assert torch.equal(got, want), (type(rt).__name__, rt.spec, form, side)
                    compared += 1
    # the three convs have four forms between them in every dtype (fp32: U | U, U2 | gemm; 16-bit: gemm,
    # frag | gemm | gemm), one side each when frozen; the head always both sides of U, U2 (fp32) or of
    # gemm (16-bit), and the bias
    sides = 2 if trainable else 1
    assert compared == 4 * sides + (5 if dtype == F32 else 3)
    guard_allocations.check()
