"""SHA-256 of dw and db of the two-pass (atomics-free) weight-gradient forms over a short case list,
one line per case, from inputs seeded on the host: two builds whose launchers choose the same
kernel, grid, workspace layout and reduction print the same lines (these forms are bit-reproducible).

    python tools/wgrad_dump.py            the default environment, then one switch at a time, each
                                          in a fresh child process (the switches are read once)
    python tools/wgrad_dump.py --child    the cases under the current environment

A case is the smallest that reaches its branch.  A refusal prints its message, a case that lands on
an atomics form prints `atomics` (not reproducible, not hashed)."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ({}, {'EMSA_WGRAD_WINO': '0'}, {'EMSA_WGRAD16': 'wino'}, {'EMSA_WGRAD16_TR': '0'},
            {'EMSA_BF16_MFMA': '1'})

# name, dtype, n, h, w, cin, cout, kernel, stride, padding, fold
CASES = [
    ('f32 1x3 c64 even line', 'f32', 1, 5, 8, 64, 64, (1, 3), (1, 1), (0, 1), False),
    ('f32 1x3 c64 15-pixel line', 'f32', 1, 4, 15, 64, 64, (1, 3), (1, 1), (0, 1), False),
    ('f32 3x1 c64', 'f32', 1, 6, 5, 64, 64, (3, 1), (1, 1), (1, 0), False),
    ('f32 3x3 128->40 row form', 'f32', 1, 6, 8, 128, 40, (3, 3), (1, 1), (1, 1), False),
    ('f32 1x3 c64 in_affine', 'f32', 1, 5, 8, 64, 64, (1, 3), (1, 1), (0, 1), True),
    ('f32 3x1 c512 1x8x10 rows reduction', 'f32', 1, 8, 10, 512, 512, (3, 1), (1, 1), (1, 0), False),
    ('bf16 3x1 c64', 'bf16', 1, 6, 5, 64, 64, (3, 1), (1, 1), (1, 0), False),
    ('bf16 3x1 c64 in_affine', 'bf16', 1, 6, 5, 64, 64, (3, 1), (1, 1), (1, 0), True),
    ('bf16 3x1 c12', 'bf16', 1, 6, 5, 12, 12, (3, 1), (1, 1), (1, 0), False),
    ('bf16 1x1 64->128 stride 1', 'bf16', 1, 6, 8, 64, 128, (1, 1), (1, 1), (0, 0), False),
    ('bf16 1x1 64->128 stride 2', 'bf16', 1, 6, 8, 64, 128, (1, 1), (2, 2), (0, 0), False),
    ('bf16 3x1 c64 stride (2,1)', 'bf16', 1, 6, 5, 64, 64, (3, 1), (2, 1), (1, 0), False),
    ('f16 3x1 c64', 'f16', 1, 6, 5, 64, 64, (3, 1), (1, 1), (1, 0), False),
    ('f16 3x1 c12', 'f16', 1, 6, 5, 12, 12, (3, 1), (1, 1), (1, 0), False),
]


def sha(t):
    return 'none' if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def operands(seed, dtype, n, h, w, cin, cout, kernel, stride, padding, fold):
    import numpy as np
    import torch
    from emsanet_amd import functional as Fn
    tdt = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}[dtype]
    rng = np.random.default_rng(seed)
    spec = Fn.ConvSpec(cin, cout, kernel, stride, padding)
    oh, ow = spec.out_hw(h, w)

    def act(c, hh, ww):
        t = torch.from_numpy(rng.standard_normal((n, c, hh, ww)).astype(np.float32)).to(tdt)
        return t.to('cuda:0').permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    x, dy = act(cin, h, w), act(cout, oh, ow)
    aff = None
    if fold:
        aff = tuple(torch.from_numpy(rng.standard_normal(cin).astype(np.float32)).to('cuda:0') for _ in range(2))
    like = torch.empty(cout, cin, *kernel, device='cuda:0')
    return x, dy, spec, like, aff


def run_cases():
    import torch
    from emsanet_amd import _lib, functional as Fn
    Fn.WGRAD_WINO2D = False
    for i, (name, *case) in enumerate(CASES):
        x, dy, spec, like, aff = operands(100 + i, *case)
        try:
            dw, db, packed = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=True, in_affine=aff)
            torch.cuda.synchronize()
            print(f"{name}: " + ('atomics' if packed else f"dw {sha(dw)} db {sha(db)}"), flush=True)
        except _lib.EmsaError as e:
            print(f"{name}: refused ({e})", flush=True)
    for n_jobs in (2, 4):
        jobs = []
        for j in range(n_jobs):          # 3x1 and 1x3 in turn; job 1 folded, the last without a bias
            k, p = (((3, 1), (1, 0)), ((1, 3), (0, 1)))[j & 1]
            x, dy, spec, like, aff = operands(200 + 10 * n_jobs + j, 'bf16', 1, 6, 5, 64, 64, k, (1, 1), p, j == 1)
            jobs.append((x, dy, spec, like, None, None, j != n_jobs - 1, aff))
        try:
            out = Fn.conv_wgrad_multi(jobs)
            torch.cuda.synchronize()
            res = 'no multi-job form' if out is None else ' | '.join(f"dw {sha(dw)} db {sha(db)}" for dw, db in out)
        except _lib.EmsaError as e:
            res = f"refused ({e})"
        print(f"bf16 multi {n_jobs} jobs c64: {res}", flush=True)


def main():
    if '--child' in sys.argv:
        run_cases()
        return 0
    for env in VARIANTS:
        print('== ' + (' '.join(f'{k}={v}' for k, v in env.items()) or 'default environment'), flush=True)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'],
                            env={**os.environ, **env}).returncode
        if rc != 0:
            print(f"child exited with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
