"""One allocation point: every device buffer that a kernel writes or uses as workspace comes from
`functional._empty` / `functional._zeros`, so that the guarded allocator of tests/guard.py sees it.

This walks emsanet_amd/*.py with `ast` and fails on a direct torch allocation on a device:
  torch.empty / zeros / full / ones (..., device=...)      an explicit device
  torch.empty_like / zeros_like (t)                        the device of a tensor
  t.new_empty / new_zeros / new_full (...)                 the device of a tensor
outside `functional._empty` / `_zeros`, unless ALLOWED names the site (module, function, reason).
A host allocation (no `device=`: pinned staging memory, NumPy-side tables) is not a device buffer and
is not looked at.
"""
import ast
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'emsanet_amd')

FACTORIES = ('empty', 'zeros', 'full', 'ones')
LIKE = ('empty_like', 'zeros_like')
NEW = ('new_empty', 'new_zeros', 'new_full')
EXEMPT = {('functional.py', '_empty'), ('functional.py', '_zeros')}

# (module, function): (the calls allowed there, reason).  The sites that stay direct torch allocations.
ALLOWED = {
    # parameter and bucket storage that lives for the whole run; the update kernels that write it are
    # tested between guards directly (test_optim_guard_gpu.py)
    ('optim.py', '_FlatOptimizer.__init__'): (('zeros_like',),
        'flat parameter storage that the parameters are re-homed into'),
    ('optim.py', 'FusedSGD.__init__'): (('zeros_like',),
        'momentum buffers: optimizer state for the whole run'),
    ('optim.py', 'FusedSGD.use_device_hyperparameters'): (('zeros',),
        'hyper-parameter row that the host uploads with copy_'),
    ('optim.py', 'FusedAdam.__init__'): (('zeros_like', 'zeros'),
        'moment buffers, step and hyper rows: optimizer state for the whole run'),
    ('optim.py', 'LossScaler.__init__'): (('zeros',), 'scaler state row: lives for the whole run'),
    ('parallel.py', 'GradientBuckets._close'): (('zeros',),
        'gradient bucket storage that the .grad tensors are views of'),
    ('parallel.py', 'GradientBuckets.reduce'): (('empty_like',),
        'communication copy of a bucket, filled by copy_ and handed to RCCL'),
    ('parallel.py', 'broadcast_parameters'): (('empty',),
        'broadcast staging buffer, filled by copy_ and handed to torch.distributed'),
    # operands that torch ops fill and consume, or that kernels only read
    ('nn.py', 'LearnedUpsampling._padded'): (('new_zeros',),
        'zero padding of a weight, consumed by torch.cat (autograd slices it back)'),
    ('loss.py', 'CrossEntropyLossScene.forward'): (('new_zeros',),
        'zero padding of the logits, consumed by torch.cat'),
    ('postprocessing.py', 'softmax_argmax'): (('new_zeros',),
        'zero padding of the logits, consumed by torch.cat'),
    ('ops.py', 'MultiConvRT._bias_vec'): (('zeros',),
        'bias operand filled with torch copy_; kernels only read it'),
    ('ops.py', 'StemStageFunction.backward'): (('zeros',),
        'zero gradient standing in for an unused output; kernels only read it'),
    ('ops.py', 'SEAddFunction.backward'): (('zeros_like',),
        'zero gradient standing in for an unused output; kernels only read it'),
    ('model.py', 'EMSANet.use_device_dropout_state'): (('zeros',),
        'dropout seed row: model state for the whole run'),
}

# the functions whose allocations were moved to the allocation point: never to be allow-listed
MOVED = {
    'targets.py': ('TrainingTargetGenerator._constants', 'TrainingTargetGenerator._slots'),
    'augment.py': ('TrainingAugmenter._slots',),
    'metrics.py': ('MeanIntersectionOverUnion._buffers', 'PanopticQuality._buffers', 'PanopticQuality._update',
                   'MeanAbsoluteAngularError._buffers', 'MeanAbsoluteNormalError._buffers', 'panoptic_targets'),
    'export.py': ('InferenceOutputPacker._state', 'InferenceOutputPacker._out',
                  'InferenceOutputPacker.instance_outputs'),
    'evaluation.py': ('ValidationEvaluator._buffer',),
    'postprocessing.py': ('instance_centers', 'instance_assign', 'panoptic_merge', 'instance_stats',
                          'panoptic_scores', 'instance_orientation_sums'),
    'staging.py': ('BatchStager._issue', 'BatchStager._issue_files'),
}
# softmax_argmax holds two moved sites (its index maps) next to the padding that stays: only the padding call
MOVED_KINDS = {('postprocessing.py', 'softmax_argmax'): ('empty', 'zeros')}


def _sites(path):
    """[(qualified function, line, call text)] of the direct device allocations in one file"""
    tree = ast.parse(open(path).read(), path)
    out = []

    def visit(node, scope, in_func=False):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef) and not in_func:
                visit(child, scope + [child.name])
                continue
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                # a nested helper counts as its enclosing method / function
                visit(child, scope if in_func else scope + [child.name], True)
                continue
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                f = child.func
                on_torch = isinstance(f.value, ast.Name) and f.value.id == 'torch'
                # `device=...` spelled out, or hidden in a `**kwargs` dictionary
                dev = any(k.arg == 'device' or k.arg is None for k in child.keywords)
                hit = (on_torch and f.attr in FACTORIES and dev) or (on_torch and f.attr in LIKE) or \
                    (f.attr in NEW)
                if hit:
                    out.append(('.'.join(scope) or '<module>', child.lineno, f.attr))
            visit(child, scope, in_func)

    visit(tree, [])
    return out


def _all_sites():
    found = {}
    for name in sorted(os.listdir(PKG)):
        if name.endswith('.py'):
            for func, line, what in _sites(os.path.join(PKG, name)):
                found.setdefault((name, func), []).append((line, what))
    return found


def test_walker_sees_the_calls_it_is_meant_to(tmp_path):
    src = tmp_path / 'm.py'
    src.write_text(
        "import torch\n"
        "def host():\n"
        "    return torch.empty(3, pin_memory=True), torch.zeros((2, 2)), np.zeros(3)\n"
        "def a(d):\n"
        "    return torch.empty(3, device=d)\n"
        "class K:\n"
        "    def b(self, t):\n"
        "        def inner():\n"
        "            return t.new_zeros(3)\n"
        "        kw = dict(device=t.device)\n"
        "        return torch.zeros_like(t), torch.full((2,), 1, **kw), inner()\n"
        "    def c(self, t):\n"
        "        return torch.ones(2, dtype=torch.int32, device=t.device), x.y.new_full((1,), 0)\n"
        "z = torch.empty_like(q)\n")
    got = sorted((f, w) for f, _l, w in _sites(str(src)))
    assert got == [('<module>', 'empty_like'), ('K.b', 'full'), ('K.b', 'new_zeros'), ('K.b', 'zeros_like'),
                   ('K.c', 'new_full'), ('K.c', 'ones'), ('a', 'empty')], got


def test_the_allocation_point_itself_is_found():
    found = _all_sites()
    for key in EXEMPT:
        assert key in found, f"{key}: the allocation helper no longer allocates with torch?"


def test_every_device_allocation_goes_through_the_allocation_point():
    found = _all_sites()
    bad = [f"emsanet_amd/{m}:{line} {func}: torch {what}" for (m, func), hits in sorted(found.items())
           if (m, func) not in EXEMPT for line, what in hits if what not in ALLOWED.get((m, func), ((),))[0]]
    assert not bad, ("direct device allocations (use functional._empty / _zeros, or give the site a reason "
                     "in ALLOWED):\n  " + "\n  ".join(bad))


def test_allow_list_is_current_and_reasoned():
    found = _all_sites()
    stale = [k for k in ALLOWED if k not in found]
    assert not stale, f"ALLOWED names sites that no longer allocate: {stale}"
    assert not (set(ALLOWED) & EXEMPT)
    for key, (kinds, reason) in ALLOWED.items():
        assert set(kinds) == {what for _line, what in found[key]}, f"{key}: allows more than is there"
        assert isinstance(reason, str) and len(reason.split()) >= 4, f"{key}: say why"


def test_allow_list_holds_no_data_path_site():
    for (m, func), (kinds, _reason) in ALLOWED.items():
        assert func not in MOVED.get(m, ()), f"{m} {func}: its buffers come from the allocation point"
        assert not set(kinds) & set(MOVED_KINDS.get((m, func), ())), (m, func, kinds)
    # and every moved function still exists under its name (a rename must move its entry along)
    for m, funcs in MOVED.items():
        tree = ast.parse(open(os.path.join(PKG, m)).read())
        names = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        for func in funcs:
            assert set(func.split('.')) <= names, (m, func)
