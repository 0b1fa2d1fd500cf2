"""Records tests/golden/pack_table_parent.npz: PackPlan's job table, arena layout and installed views
for the configurations of tests/test_pack_table.py, from the checkout that is to serve as the
reference (host only: stubbed library, CPU tensors; run on the commit BEFORE a change that must
keep the table byte for byte):

    EMSANET_ROOT=<checkout of the reference commit> python tests/golden/make_pack_table_golden.py [out.npz]

Without EMSANET_ROOT the package of this checkout is recorded.  Configurations, normalisation and
array names come from the test module, so the recording and the test cannot drift apart."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.environ.get('EMSANET_ROOT') or os.path.dirname(TESTS))

import emsanet_amd                                                      # noqa: E402
from test_pack_table import GOLDEN, make_model, record_all              # noqa: E402


def install(plan):
    """the install step of `refresh`.  A plan from before the entry list keeps its views in four
    places and installs them in four loops at the end of `refresh`, which a host tensor never
    reaches: the same four loops, from that `refresh`"""
    if hasattr(plan, '_install'):
        return plan._install()
    dtype = plan._dtype
    for m, (d0, d1, bias, wino, d2, d3) in zip(plan.multi, plan._mviews):
        m.packs.put('wino' if wino else 'gemm', dtype, m.key_now(), d0, d1)
        m.packs.put('bias', torch.float32, m.key_now(), bias, None)
        if d2 is not None:
            m.packs.put('wino2d', dtype, m.key_now(), d2, d3)
    for rt, (f0, f1) in zip(*plan._frag):
        rt.packs.put('frag', dtype, rt.key_now(), f0, f1)
    for rt, (u0, u1) in zip(*plan._w2):
        rt.packs.put('wino2d', dtype, rt.key_now(), u0, u1)
    for rt, (v0, v1) in zip(plan.rts, plan._views):
        if v0 is None:
            continue
        rt.packs.put('wino' if rt.wino and dtype == torch.float32 else 'gemm', dtype, rt.key_now(), v0, v1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = {f'{config}/{part}': a for config, parts in record_all(make_model(), install).items()
              for part, a in parts.items()}
    np.savez_compressed(out, **arrays)
    for config in sorted({k.split('/')[0] for k in arrays}):
        n_jobs, n_blocks, arena = arrays[f'{config}/totals']
        print(f"{config}: {n_jobs} jobs, {n_blocks} blocks, arena {arena} bytes, "
              f"{len(arrays[config + '/operands'])} persistent operands, "
              f"{len(arrays[config + '/installed'])} installed slots")
    print(f"{out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes, package "
          f"{os.path.dirname(emsanet_amd.__file__)}")


if __name__ == '__main__':
    main()
