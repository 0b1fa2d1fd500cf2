"""bench.py: what `--dump-outputs` writes (on the host), and a plain run on the GPU -- the timed steps,
the result line and the dumped outputs, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench    # noqa: E402


def _step_result(channels_last):
    """(loss, outputs) shaped like one EMSANet training step: semantic (out, sides), instance
    ((centre, offset, orientation), ((centre, offset), ...)), scene (out, ())"""
    g = torch.Generator().manual_seed(5)

    def r(*shape):
        t = torch.randn(*shape, generator=g)
        return t.to(memory_format=torch.channels_last) if channels_last and t.dim() == 4 else t
    sem = (r(2, 40, 96, 128), (r(2, 40, 3, 4), r(2, 40, 6, 8)))
    inst = ((r(2, 1, 96, 128), r(2, 2, 96, 128), r(2, 2, 96, 128)),
            ((r(2, 1, 3, 4), r(2, 2, 3, 4)), (r(2, 1, 6, 8), r(2, 2, 6, 8))))
    return torch.tensor(2.5), [sem, inst, (r(2, 10), ())]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files(tmp_path):
    shapes = [(64, 3, 7, 7), (300,), (256, 256, 3, 3)]
    ids = torch.randperm(sum(int(np.prod(s)) for s in shapes)).float()    # every value once
    params = [torch.nn.Parameter(c.reshape(s)) for c, s in
              zip(ids.split([int(np.prod(s)) for s in shapes]), shapes)]
    params[0].grad = torch.randn(64, 3, 7, 7).to(memory_format=torch.channels_last)
    params[2].grad = torch.randn(256, 256, 3, 3)
    res = _step_result(channels_last=True)
    bench.dump_outputs(str(tmp_path / 'a'), res, params)
    a = _load(tmp_path / 'a')
    flat = bench.flatten_outputs(res[1])
    assert set(a) == {f'output_{i:02d}' for i in range(len(flat))} | {'loss', 'param_sample', 'grad_sample'}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert float(a['loss']) == 2.5
    for i, t in enumerate(flat):
        got = a[f'output_{i:02d}']
        if t.numel() <= 1 << 19:
            np.testing.assert_array_equal(got, t.numpy())          # small outputs: whole, NCHW
        else:
            assert got.shape == (1 << 19,)                         # large ones: a seeded sample
            assert np.isin(got, t.numpy()).all()
    n = sum(p.numel() for p in params)
    assert a['param_sample'].shape == a['grad_sample'].shape == (min(n, 1 << 20),)
    # the same elements of the parameters and of their gradients (zeros where a parameter has none)
    values = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    grads = torch.cat([torch.zeros(300) if p.grad is None else p.grad.contiguous().reshape(-1)
                       for p in params]).numpy()
    pos = {v: i for i, v in enumerate(values.tolist())}
    at = np.array([pos[v] for v in a['param_sample'].tolist()])
    assert (np.diff(at) >= 0).all()
    np.testing.assert_array_equal(a['grad_sample'], grads[at])

    # the same step in the other memory layout samples the same logical elements: identical files
    bench.dump_outputs(str(tmp_path / 'b'), _step_result(channels_last=False), params)
    b = _load(tmp_path / 'b')
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch-size', '2',
           '--height', '96', '--width', '128', '--steps', '3', '--warmup', '2',
           '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_times_and_dumps(tmp_path):
    """a plain run: the timed steps, `ms_per_step`, none of the --full figures, and the dumped outputs
    of its last step the same from one run to the next (same arguments, same inputs): the forward
    outputs bit for bit, parameters and gradients to the atomics jitter"""
    runs = [(_bench(tmp_path / f'run{i}'), _load(tmp_path / f'run{i}')) for i in range(2)]
    for d, files in runs:
        assert d['steps'] == 3 and d['warmup'] == 2 and d['ms_per_step'] > 0 and d['value'] > 0
        assert abs(d['value'] - 2 * 1e3 / d['ms_per_step']) <= 0.02 * d['value']
        assert d['roofline'] is None and d['whole_step'] is None and d['cpu_baseline'] is None
        assert d['conv_kernels'] == []
        assert {'param_sample', 'grad_sample', 'output_00'} <= set(files)
        assert all(np.isfinite(v).all() for v in files.values())
        assert np.abs(files['grad_sample']).max() > 0
    (_, a), (_, b) = runs
    assert set(a) == set(b)
    for k in a:
        if k.startswith('output_'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        lim = 1e-5 * float(np.abs(a[k]).max())
        assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= lim, k
