"""GPU: dW and db of the fp32 1-D Winograd weight gradient (conv_wgrad1d_wino_kernel, the
deterministic two-pass form without atomics; plain and with the input's BatchNorm + ReLU folded
into the loader) are bit-equal to arrays recorded from the build of the commit BEFORE the kernel's
per-step pixel decomposition moved to the scalar unit (tests/golden/wgrad1d_wino_parent.npz,
recorded by tests/golden/make_wgrad1d_golden.py from the same seeded inputs).  The lane-side
arithmetic borrows at most one line and one image per step, which must hold for every line length:

  2x5x7    64->64   along W and along H: odd lines (virtual pixel), 4-6 lines per 32-pixel step
  1x15x20  64->64   along W and along H: the /32 stage's lines of 20 and 15 (+1 virtual) pixels
  3x19x29  64->128  two output-channel tiles; several splits, the last one step short; a step
                    that crosses an image boundary
  1x2x2    64->64   a single step, 2-pixel lines: 16 lines and 8 images' worth of pixels per step"""
import os

import numpy as np
import pytest
import torch

from guard import guard_allocations  # noqa: F401  (autouse: poisoned, guard-banded allocations)
from util import DEV, rnd, to_act

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad1d_wino_parent.npz')

#         n, h,  w, cin, cout, kernel
CASES = [(2, 5, 7, 64, 64, (1, 3)), (2, 5, 7, 64, 64, (3, 1)),
         (1, 15, 20, 64, 64, (1, 3)), (1, 15, 20, 64, 64, (3, 1)),
         (3, 19, 29, 64, 128, (1, 3)),
         (1, 2, 2, 64, 64, (1, 3))]


def key(case, xbn):
    n, h, w, cin, cout, k = case
    return f"{n}x{h}x{w}_{cin}_{cout}_k{k[0]}{k[1]}_{'xbn' if xbn else 'plain'}"


def run_case(Fn, case, xbn):
    """(dw, db) of one case on the build `Fn` belongs to; the inputs depend on the case alone"""
    n, h, w, cin, cout, k = case
    spec = Fn.ConvSpec(cin, cout, k, (1, 1), (k[0] // 2, k[1] // 2))
    x = to_act(rnd(n, cin, h, w, seed=1))
    dy = to_act(rnd(n, cout, h, w, seed=2))
    like = torch.empty(cout, cin, *k, device=DEV)
    aff = ((rnd(cin, seed=3).abs() + 0.5).to(DEV), (rnd(cin, seed=4) + 0.3).to(DEV)) if xbn else None
    dw, db, packed = Fn.conv_wgrad(x, dy, spec, True, like=like, two_pass=True, in_affine=aff)
    torch.cuda.synchronize()
    assert not packed
    return dw, db


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('xbn', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_dw_and_db_equal_the_recorded_parent(case, xbn, golden):
    from emsanet_amd import functional as Fn
    dw, db = run_case(Fn, case, xbn)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    for got, name in ((dw, 'dw'), (db, 'db')):
        ref = golden[f"{key(case, xbn)}_{name}"]
        got = got.cpu().numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
        diff = got.view(np.int32) != ref.view(np.int32)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} elements differ in their bits"
