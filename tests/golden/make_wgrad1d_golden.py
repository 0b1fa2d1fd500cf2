"""Records tests/golden/wgrad1d_wino_parent.npz: dW and db of the fp32 1-D Winograd weight gradient
for the cases of tests/test_wgrad1d_lean_gpu.py, from the build that is to serve as the reference
(run once on the GPU box, on the commit BEFORE a change that must keep the results bit-equal):

    EMSANET_ROOT=<checkout of the reference commit, built> python tests/golden/make_wgrad1d_golden.py [out.npz]

Without EMSANET_ROOT the package of this checkout is recorded.  Cases, inputs and array names come
from the test module, so the recording and the test cannot drift apart."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.environ.get('EMSANET_ROOT') or os.path.dirname(TESTS))

from emsanet_amd import functional as Fn                               # noqa: E402
from test_wgrad1d_lean_gpu import CASES, GOLDEN, key, run_case         # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = {}
    for case in CASES:
        for xbn in (False, True):
            dw, db = run_case(Fn, case, xbn)
            arrays[f"{key(case, xbn)}_dw"] = dw.cpu().numpy()
            arrays[f"{key(case, xbn)}_db"] = db.cpu().numpy()
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes, package {os.path.dirname(Fn.__file__)}")


if __name__ == '__main__':
    main()
