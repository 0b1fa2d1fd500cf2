"""ops.PackPlan on the host (stubbed library, CPU tensors): the job table of `emsa_pack_batch`, the
arena layout and the views installed in the convs' caches, field for field against what the commit
before the entry-list refactor built (tests/golden/pack_table_parent.npz, recorded by
tests/golden/make_pack_table_golden.py with the functions of this module); and that the two users
of `forms(dtype)` -- PackPlan and the convs' own operand ladders -- agree on the set of forms."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_host_logic import _FakeLib, _GenerousLib, _bypass_device_check, _install, _model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pack_table_parent.npz')

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# name -> (activations' dtype, lean table, encoder layer1 convs frozen); the frozen ones last: they
# run on the same model, which stays frozen
CONFIGS = {'fp32': (F32, False, False), 'bf16_full': (BF16, False, False), 'bf16_lean': (BF16, True, False),
           'fp16_lean': (F16, True, False), 'fp32_frozen': (F32, False, True),
           'bf16_lean_frozen': (BF16, True, True)}
# Jobs and blocks of the 64 x 96 model's tables as the parent commit built them
TOTALS = {'fp32': (262, 10483), 'bf16_full': (444, 18710), 'bf16_lean': (444, 10338)}

FORMS = ('gemm', 'wino', 'wino2d', 'frag', 'bias')
NULL, PARAM, ARENA, OPERAND = 0, 1, 2, 3         # what a pointer of the table points into
JOB_COLUMNS = ('kind', 'cout', 'cin', 'kh', 'kw', 'first_block', 'cout_total', 'cout_off', 'cin_total',
               'cin_off')


def freeze_layer1(model):
    """the parameters test_dry_run_packs_every_weight_form_once freezes: one-sided operands"""
    n = 0
    for k, p in model.named_parameters():
        if 'encoder' in k and 'layer1' in k and 'conv' in k:
            p.requires_grad_(False)
            n += p.dim() == 4
    assert n == 24


def runtimes(plan):
    return list(plan.rts) + list(plan.multi)


def launch_args(plan):
    """(n_jobs, total_blocks) as `refresh` hands them to emsa_pack_batch"""
    b = getattr(plan, '_built', None)
    return (b.n_jobs, b.n_blocks) if b is not None else (plan._n_jobs, plan._n_blocks)


def record(plan, model, dtype, lean, install):
    """build the table for `dtype` on the host, run `install(plan)` (the install step of `refresh`) on
    fresh caches, and return the table, the totals, the persistent operands and the installed views as
    integer arrays with every pointer normalised: (PARAM, index in model.parameters()), (ARENA, byte
    offset), (OPERAND, ordinal of that zero-initialised operand in order of first appearance) or
    (NULL, -1)"""
    from emsanet_amd import _lib, functional as Fn
    for rt in runtimes(plan):
        rt.packs = type(rt.packs)()
    zeroed, zeros = {}, Fn._zeros

    def recording_zeros(shape, device, dtype=torch.float32):
        t = zeros(shape, device, dtype)
        zeroed[t.data_ptr()] = t
        return t
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Fn, '_zeros', recording_zeros)
        plan._build(torch.device('cpu'), dtype, lean)
    assert plan._lean == lean
    arena = plan._arena
    assert arena.dtype == torch.uint8 and arena.dim() == 1
    params = {p.data_ptr(): i for i, p in enumerate(model.parameters())}
    operands = {}

    def loc(ptr):
        if not ptr:
            return NULL, -1
        if ptr in params:
            return PARAM, params[ptr]
        if arena.data_ptr() <= ptr < arena.data_ptr() + arena.numel():
            return ARENA, ptr - arena.data_ptr()
        t = zeroed[ptr]                          # KeyError: a destination nobody allocated in _build
        return OPERAND, operands.setdefault(ptr, (len(operands), t.numel(), Fn.DT[t.dtype]))[0]

    raw = plan._jobs.numpy().tobytes()
    n_jobs, n_blocks = launch_args(plan)
    assert len(raw) == n_jobs * ctypes.sizeof(_lib.EmsaPackJob)
    jobs = (_lib.EmsaPackJob * n_jobs).from_buffer_copy(raw)
    table = [[getattr(j, c) for c in JOB_COLUMNS] + [*loc(j.src), *loc(j.dst0), *loc(j.dst1)]
             for j in jobs]
    install(plan)

    def tloc(t):
        return (NULL, -1, 0) if t is None else (*loc(t.data_ptr()), t.numel())
    installed = []
    for i, rt in enumerate(runtimes(plan)):
        for f, form in enumerate(FORMS):
            for dt in (F32, BF16, F16):
                fwd, dgrad = rt.packs.peek(form, dt, rt.key_now())
                if fwd is not None or dgrad is not None:
                    assert fwd is None or fwd.dtype == dt
                    installed.append([i, f, Fn.DT[dt], *tloc(fwd), *tloc(dgrad)])
    return {'jobs': np.array(table, dtype=np.int64),
            'totals': np.array([n_jobs, n_blocks, arena.numel()], dtype=np.int64),
            'operands': np.array([list(v) for v in operands.values()], dtype=np.int64).reshape(-1, 3),
            'installed': np.array(installed, dtype=np.int64)}


def make_model():
    """the full model at 64 x 96 on the host (the stub library is needed while it is constructed only)"""
    from emsanet_amd import full_args
    with pytest.MonkeyPatch.context() as mp:
        _install(mp, _FakeLib())
        return _model(full_args(input_height=64, input_width=96)).train()


def record_all(model, install):
    """{config: arrays of `record`} for every configuration of CONFIGS; leaves `model` frozen"""
    out = {}
    for name, (dtype, lean, frozen) in CONFIGS.items():
        if frozen and all(p.requires_grad for p in model.parameters()):
            freeze_layer1(model)
        assert frozen == (not all(p.requires_grad for p in model.parameters()))
        out[name] = record(model._pack_plan, model, dtype, lean, install)
    return out


@pytest.fixture(scope='module')
def engine():
    return make_model()


@pytest.fixture(scope='module')
def tables(engine):
    return record_all(engine, lambda plan: plan._install())


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('config', list(CONFIGS))
def test_pack_table_equals_the_parents(config, tables, golden):
    """same jobs in the same order with the same first_block, placements, sources and arena offsets;
    same launch arguments and arena size; same zero-initialised merged-head operands"""
    got = tables[config]
    for part in ('totals', 'operands', 'jobs'):
        want = golden[f'{config}/{part}']
        assert got[part].shape == want.shape, (part, got[part].shape, want.shape)
        diff = np.argwhere(got[part] != want)
        assert diff.size == 0, f"{part}: first difference at {diff[0]}: {got[part][tuple(diff[0])]} != " \
                               f"{want[tuple(diff[0])]}"
    if config in TOTALS:
        assert tuple(got['totals'][:2]) == TOTALS[config]
    assert len(got['jobs']) == got['totals'][0]


@pytest.mark.parametrize('config', list(CONFIGS))
def test_installed_views_equal_the_parents(config, tables, golden):
    """what `refresh` installs after a build: per conv the same (form, dtype) slots with the same sides,
    each side a view at the recorded arena offset and size or the recorded persistent operand"""
    got, want = tables[config]['installed'], golden[f'{config}/installed']
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize('config', list(CONFIGS))
def test_nothing_is_installed_outside_forms(config, engine, tables):
    """every slot a conv's cache holds after the install step is a form of that conv's `forms(dtype)`,
    and every form the plan has a job for was installed (a lean table leaves out the [tap][n][k]
    operand of the convs that have fragment-ordered weights)"""
    from emsanet_amd import functional as Fn
    dtype, lean, _ = CONFIGS[config]
    have = {(int(i), FORMS[f], int(d)) for i, f, d in tables[config]['installed'][:, :3]}
    for i, rt in enumerate(runtimes(engine._pack_plan)):
        forms = rt.forms(dtype)
        names = [f.name for f in forms]
        assert len(set(names)) == len(names) and set(names) <= set(FORMS)
        mine = {h for h in have if h[0] == i}
        declared = {(i, f.name, Fn.DT[f.dtype]) for f in forms}
        assert mine <= declared, (mine - declared)
        skipped = {'gemm'} if lean and 'frag' in names else set()
        planned = {(i, f.name, Fn.DT[f.dtype]) for f in forms if f.kind is not None and f.name not in skipped}
        assert mine == planned, (mine ^ planned)


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_every_operand_a_training_step_reads_is_a_declared_form(dtype, monkeypatch):
    """one training step of the 64 x 96 model on host tensors (`refresh` leaves those to the per-layer
    path): every (form, dtype) a conv's `weights()` is asked for is in that conv's `forms(dtype)` --
    the operand ladders and PackPlan read the same declaration"""
    import emsanet_amd.model as M
    from emsanet_amd import full_args, ops
    from oracle.emsanet_oracle import synthetic_batch
    half = dtype != 'float32'
    act = getattr(torch, dtype)
    _install(monkeypatch, _GenerousLib() if half else _FakeLib())
    asked = []
    for cls in (ops.ConvRT, ops.MultiConvRT):
        def weights(self, form, side, dtype=torch.float32, _orig=cls.weights):
            asked.append((self, form, dtype))
            return _orig(self, form, side, dtype)
        monkeypatch.setattr(cls, 'weights', weights)
    model = _model(full_args(input_height=64, input_width=96,
                             **({'compute_dtype': dtype} if half else {}))).train()
    monkeypatch.setattr(M.EMSANet, 'forward', _bypass_device_check(model))
    outs = model(synthetic_batch(2, 64, 96))
    flat = [t for o, sides in outs for t in (list(o) if isinstance(o, tuple) else [o])]
    flat += [t for _, sides in outs for s in sides for t in (list(s) if isinstance(s, tuple) else [s])]
    torch.autograd.backward(flat, [torch.zeros_like(t) for t in flat])
    plan = model._pack_plan
    known = set(map(id, runtimes(plan)))
    seen = set()
    for rt, form, dt in asked:
        declared = {(f.name, f.dtype) for f in rt.forms(act)}
        assert (form, dt) in declared, (type(rt).__name__, rt.spec, form, dt, declared)
        if id(rt) in known:
            seen.add(form)
    # the step went through every kind of form the model has in this dtype
    assert seen == ({'gemm', 'frag', 'bias'} if half else {'gemm', 'wino', 'wino2d', 'bias'})
