"""A guarded, poisoned allocator for the kernel parity tests.

Every output and scratch buffer of the host wrappers comes from `functional._empty` (or its zeroed
twin `_zeros`).  While the `guard_allocations` fixture is active those two hand out memory from a
`GuardedArena`: the payload lies flush between two bands of 0xFF bytes inside one uint8 buffer and
is itself filled with 0xFF -- NaN in fp32 / bf16 / fp16, -1 in the int8 pool-index maps (valid: 0..8),
all-ones in the integer masks.  A parity assertion then means what it says:

* an element the kernel did not write is NaN (`close()` asserts finiteness), never the previous
  test variant's correct result handed back by the caching allocator;
* a store past either end of an output changes a guard byte, and `check()` names the allocation;
* an input placed with `put()` has NaN on both sides, so a read past its end that reaches the
  result shows as NaN.

This is a plain helper module (not a conftest): a test module switches the fixture on with
`from guard import guard_allocations  # noqa: F401`.  A module that compares integer, bool or uint8
outputs exactly runs every test once per payload byte, 0xFF and 0x00 (see PAYLOADS): a module written
new imports `guard_allocations_both` instead; a module whose tests exist already keeps their names for
the 0xFF run and ends with `guard.second_payload(globals())`, which adds a twin per test for 0x00.
"""
import os
import sys
import types

import pytest
import torch

POISON = 0xFF
ALIGN = 256          # start alignment of a payload (the caching allocator's blocks start 512-aligned)

# Guard width.  A stray store can at worst be a whole tile of one workgroup, so the band is as large as
# the largest tile any kernel stores from one workgroup (tile tables of emsanet_amd/csrc):
#   conv_h.hip     tap-split launch: the raw fp32 accumulator tile into ws[ksplit][M][n_ch];
#                  launch_h<256, 128, ..> (EMSA_CONVH_TILE=3) 256 rows x 128 channels x 4 B = 131,072 B
#   conv_mfma.hip  launch_igemm<128, 128, ..>          128 rows x 128 channels x 4 B = 65,536 B
#   conv_h.hip     launch_h<256, 128, ..> (HT_256x128) 256 rows x 128 channels x 2 B = 65,536 B
#   conv_mfma.hip  launch_wgrad<64, 32, 7, ..>         7 taps x 64 x 32 x 4 B        = 57,344 B
#                  launch_wgrad<64, 64, 3, ..>         3 taps x 64 x 64 x 4 B        = 49,152 B
#   conv_rs.hip / conv_wino.hip / conv_wino2d.hip      <= 128 rows x 64 channels x 4 B = 32,768 B
# Every other kernel (pointwise, reductions, pack) stores at most one 16-byte vector per thread of a
# 256-thread workgroup = 4,096 B.
GUARD_BYTES = 256 * 128 * 4

# The whole-engine test keeps every allocation of a training step alive (about two thousand):
# 4 KiB per band = 256 x the largest single vector store (16 B, global_store_dwordx4) = what one
# 256-thread workgroup stores in one instruction; misses only a stray store further than 4 KiB away.
GUARD_BYTES_MODEL = 4096

# Tests of the guarded modules that run WITHOUT the arena, one line of reason each.  Only tests that
# build the whole model or capture a hipGraph; no test of one kernel or one fused pair.
OPT_OUT = {
    'test_stem_stage_gpu.py::test_graphed_train_step_with_fused_stage_equals_eager':
        'captures a hipGraph: allocations made during capture belong to the graph\'s private pool',
    'test_conv_wino2d_gpu.py::test_wino2d_full_model_train_step':
        'whole model training step; test_memory_edges_gpu runs the same model under its own arena',
    'test_conv_wino2d_gpu.py::test_wino2d_graphed_train_step_equals_eager':
        'captures a hipGraph: allocations made during capture belong to the graph\'s private pool',
    'test_memory_edges_gpu.py::test_whole_engine_train_step':
        'whole model: installs its own arena with GUARD_BYTES_MODEL bands and runs the unguarded twin',
    'test_augment_gpu.py::test_training_step_on_an_augmented_batch':
        'builds the whole model and runs three forward passes; apply() runs guarded in every other test',
    'test_evaluation_gpu.py::test_evaluator_reads_fullres_entries_for_larger_label_maps':
        'runs the whole model\'s eval forward pass; the evaluator runs guarded in the tests beside it',
    'test_evaluation_gpu.py::test_evaluator_keys_follow_the_tasks':
        'builds a second whole model and runs its eval forward pass',
    'test_export_gpu.py::test_pack_replayed_from_a_graph_behind_the_eval_forward':
        'captures a hipGraph of the whole eval forward: allocations made during capture belong to the '
        'graph\'s private pool',
    'test_metrics_gpu.py::test_validation_loop_end_to_end':
        'builds the whole model for an eval forward pass; both metrics run guarded in every other test',
    'test_normal_gpu.py::test_training_step_with_the_normal_task':
        'builds the whole five-task model and runs a training step forward and backward',
    'test_normal_gpu.py::test_evaluator_reports_the_normal_error':
        'runs the whole model\'s eval forward pass',
    'test_targets_gpu.py::test_training_step_losses_equal_the_reference_targets':
        'builds the whole model and runs its forward pass; the target kernels run guarded in every other test',
}

_PKG = os.sep + 'emsanet_amd' + os.sep
_SKIP_FUNCS = ('_empty', '_zeros', 'act_empty', 'act_zeros')


def _call_site():
    """'file.py:function:line' of the innermost frame in emsanet_amd/ that is not one of the
    allocation helpers; the test's own frame when the package is not on the stack"""
    f = sys._getframe(2)
    first = None
    while f is not None:
        name = f.f_code.co_filename
        if first is None and os.sep + 'tests' + os.sep in name and os.path.basename(name) != 'guard.py':
            first = f
        if _PKG in name and f.f_code.co_name not in _SKIP_FUNCS:
            return f"{os.path.basename(name)}:{f.f_code.co_name}:{f.f_lineno}"
        f = f.f_back
    if first is not None:
        return f"{os.path.basename(first.f_code.co_filename)}:{first.f_code.co_name}:{first.f_lineno}"
    return '?'


class GuardError(AssertionError):
    pass


class GuardedArena:
    def __init__(self, guard_bytes=GUARD_BYTES, payload=POISON):
        assert guard_bytes > 0 and 0 <= int(payload) <= 0xFF
        self.guard_bytes = int(guard_bytes)
        self.payload = int(payload)  # the byte an `alloc` payload is filled with; the bands are always 0xFF
        self._live = []              # (buffer, payload offset, payload bytes, site, shape, dtype)
        self.checked = 0             # allocations checked so far (all check() calls)

    # -- allocation ---------------------------------------------------------------------------
    def _carve(self, shape, device, dtype, site):
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        if any(s < 0 for s in shape):                    # (as torch.empty: a status code used as a size)
            raise RuntimeError(f"negative dimension in shape {shape}")
        numel = 1
        for s in shape:
            numel *= s
        esz = torch.empty((), dtype=dtype).element_size()
        nbytes = numel * esz
        g = self.guard_bytes
        buf = torch.empty(2 * g + nbytes + ALIGN, device=device, dtype=torch.uint8)
        buf.fill_(POISON)
        off = g + (-(buf.data_ptr() + g)) % ALIGN
        if self.payload != POISON:
            buf[off:off + nbytes].fill_(self.payload)
        t = buf[off:off + nbytes].view(dtype).view(shape)
        self._live.append((buf, off, nbytes, site, shape, dtype))
        return t

    def alloc(self, shape, device, dtype=torch.float32):
        """stand-in for functional._empty: every payload byte is `self.payload` (0xFF by default)"""
        return self._carve(shape, device, dtype, _call_site())

    def zeros(self, shape, device, dtype=torch.float32):
        """stand-in for functional._zeros: payload zero, guards 0xFF"""
        t = self._carve(shape, device, dtype, _call_site())
        t.zero_()
        return t

    def put(self, t):
        """a copy of `t` (same shape, strides of a dense tensor in t's dimension order, dtype,
        device) flush against the guards: how a test places an input, weight or packed operand"""
        if t is None:
            return None
        # keep the memory order of a dense permuted tensor (an NHWC activation stays NHWC); any
        # other layout (a slice of a wider buffer) is placed as its contiguous copy
        order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
        if not t.permute(order).is_contiguous():
            order = list(range(t.dim()))
        src = t.permute(order).contiguous()
        g = self._carve(tuple(src.shape), t.device, t.dtype, 'put@' + _call_site())
        g.copy_(src)
        inv = [0] * len(order)
        for i, d in enumerate(order):
            inv[d] = i
        return g.permute(inv)

    # -- checking -----------------------------------------------------------------------------
    def check(self):
        """synchronize; every guard byte of every allocation made since the last check must still
        be 0xFF.  Releases the buffers."""
        live, self._live = self._live, []
        if not live:
            return 0
        if any(b.is_cuda for b, *_ in live):
            torch.cuda.synchronize()
        g = self.guard_bytes
        counts = []
        for buf, off, nbytes, *_ in live:
            counts.append((buf[off - g:off] != POISON).sum() + (buf[off + nbytes:off + nbytes + g] != POISON).sum())
        bad = torch.stack(counts).cpu()
        self.checked += len(live)
        if int(bad.sum()) == 0:
            return len(live)
        msgs = []
        for (buf, off, nbytes, site, shape, dtype), nb in zip(live, bad.tolist()):
            if not nb:
                continue
            for side, lo in (('front', off - g), ('rear', off + nbytes)):
                dam = (buf[lo:lo + g] != POISON).nonzero().flatten().cpu()
                if dam.numel():
                    first = int(dam[0]) + lo - off - (nbytes if side == 'rear' else 0)
                    where = f"payload end + {first}" if side == 'rear' else f"payload start - {-first}"
                    msgs.append(f"{site} shape {shape} {dtype}: {side} band damaged, first byte at "
                                f"offset {first} ({where}), {dam.numel()} bytes")
        raise GuardError("out-of-bounds write into a guard band:\n  " + "\n  ".join(msgs))


def install(monkeypatch, arena):
    """route functional._empty / _zeros to the arena (Fn._POISON and the environment untouched)"""
    from emsanet_amd import functional as Fn
    monkeypatch.setattr(Fn, '_empty', arena.alloc)
    monkeypatch.setattr(Fn, '_zeros', arena.zeros)


# allocations checked per test module in this process (memory discipline); the running
# total is printed at every teardown (pytest -s / -rP shows it)
COUNTS = {}


# the arena of the running test (none in an opted-out test): what the module-level helpers of a test
# module, which see no fixture argument, place their inputs with
_ACTIVE = []


def put(t):
    """`arena.put(t)` on the running test's arena: the input flush between two bands of 0xFF, so that a
    read past either end returns poison; `t` itself in a test that runs without the arena"""
    return _ACTIVE[-1].put(t) if _ACTIVE else t


def check():
    """`arena.check()` on the running test's arena (0 without one)"""
    return _ACTIVE[-1].check() if _ACTIVE else 0


def _guarded(request, monkeypatch, payload):
    mod = os.path.basename(str(request.node.fspath))
    name = getattr(request.node, 'originalname', None) or request.node.name
    if name.endswith(TWIN):                      # a twin made by second_payload()
        name, payload = name[:-len(TWIN)], PAYLOADS[1]
    if f"{mod}::{name}" in OPT_OUT:
        yield None
        return
    arena = GuardedArena(payload=payload)
    install(monkeypatch, arena)
    _ACTIVE.append(arena)
    yield arena
    _ACTIVE.remove(arena)
    try:
        arena.check()
    finally:
        COUNTS[mod] = COUNTS.get(mod, 0) + arena.checked
        print(f"GUARD_COUNT {mod} {COUNTS[mod]}")


# 0xFF is a legal VALUE in integer outputs: True in a bool mask, 255 in a uint8 map, -1 in int32 / int64
# where -1 is a sentinel ("no centre").  An element the kernel skipped escapes an exact comparison
# whenever the expected value happens to be the poison, so the modules whose tests compare integer,
# bool or uint8 outputs exactly import this fixture instead: every test runs twice, on 0xFF and on 0x00
# payloads, and an unwritten element differs from its expected value under at least one of the two.
PAYLOADS = (POISON, 0x00)
TWIN = '_poison00'


@pytest.fixture(autouse=True)
def guard_allocations(request, monkeypatch):
    """every test of the importing module runs on poisoned, guard-banded outputs; the guards are
    checked when the test is over (also when it failed: both reports are shown).  Payload 0xFF; 0x00
    for the twins that second_payload() made"""
    yield from _guarded(request, monkeypatch, POISON)


def second_payload(namespace):
    """called as `guard.second_payload(globals())` at the end of a test module that imports
    `guard_allocations`: every test function `test_x` of the module gets a twin `test_x_poison00` -- the
    same code, marks, parameters and fixtures -- which the fixture runs on 0x00 payloads.  The tests
    themselves keep their names and their 0xFF run.  Opted-out tests get no twin (they would run twice
    on the plain allocator).  -> the names added"""
    mod = os.path.basename(namespace['__file__'])
    added = []
    for name, f in list(namespace.items()):
        if not (name.startswith('test_') and isinstance(f, types.FunctionType)) or name.endswith(TWIN) \
                or name + TWIN in namespace or f.__module__ != namespace['__name__'] \
                or f"{mod}::{name}" in OPT_OUT:
            continue
        twin = types.FunctionType(f.__code__, f.__globals__, name + TWIN, f.__defaults__, f.__closure__)
        twin.__dict__.update(f.__dict__)
        if 'pytestmark' in f.__dict__:
            twin.pytestmark = list(f.pytestmark)
        twin.__kwdefaults__, twin.__doc__, twin.__module__ = f.__kwdefaults__, f.__doc__, f.__module__
        twin.__qualname__ = name + TWIN
        namespace[name + TWIN] = twin
        added.append(name + TWIN)
    return added


@pytest.fixture(autouse=True, params=PAYLOADS, ids=lambda b: f"poison{b:02X}")
def guard_allocations_both(request, monkeypatch):
    """`guard_allocations`, once per payload byte of PAYLOADS"""
    yield from _guarded(request, monkeypatch, request.param)
