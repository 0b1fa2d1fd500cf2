"""Vector-instruction budgets of the fp32 Winograd kernels (cross-compiled, no GPU needed).  On gfx950
every VALU instruction of any wave takes four cycles away from the fp32 MFMA pipe, so
the instructions around a kernel's MFMAs are its overhead; tools/valu_count.py counts them per
instantiation and this test keeps them from growing back.  Every bound is the count reached when
the bound was set plus 5 % (rounded up): a compiler update may move a few instructions, a run-time
option that turns back into selects on every pixel moves dozens.

The generic conv1d_wino_kernel<64> (options read at run time) stands at 187 before the first MFMA,
642 after the last one and 14 + 7 + 7 per K step; it is the fallback and is not watched."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')),
                                 reason='hipcc not available')

# conv1d_wino_kernel<64, false, BNB, INBN, OPT>: (BNB, INBN, OPT) -> VALU bounds
#   pre: before the first MFMA, post: after the last one (static, all paths), step: per K step of 16 MFMAs
# OPT bits: 1 bias, 2 ReLU, 4 relu_bits, 8 stats, 16 mask_bits, 32 residual, 64 mask_res
WINO = {
    #                          reached: pre post step
    ('false', 'false', 7):   dict(pre=82, post=187, step=8),     # 78  178   7   bias + ReLU + relu_bits
    ('false', 'true', 7):    dict(pre=120, post=202, step=23),   # 114 192  21   ... with the input BatchNorm
    ('false', 'false', 9):   dict(pre=82, post=223, step=8),     # 78  212   7   bias + stats
    ('false', 'false', 16):  dict(pre=82, post=141, step=8),     # 78  134   7   gated by mask_bits
    ('false', 'false', 112): dict(pre=82, post=164, step=8),     # 78  156   7   residual gated by bits
    ('false', 'false', 0):   dict(pre=82, post=86, step=8),      # 78   81   7   no option
    ('true', 'false', 0):    dict(pre=82, post=244, step=8),     # 78  232   7   BatchNorm-backward sums
    ('true', 'false', 32):   dict(pre=82, post=265, step=8),     # 78  252   7   ... plus residual
}
# conv_wgrad1d_wino_kernel<64, 64, false, float, XBN>: XBN -> bounds (post: after the last MFMA; step: the
# loader's block + the MFMA block of one K step of 32 MFMAs).  The step stood at 46 + 14 (XBN 56 + 50)
# with a per-lane magic-division decomposition; with the decomposition on the scalar unit it is 35 + 14.
# "Under about 40" is not reachable in this structure: 14 are the operand transforms in the MFMA block,
# 6 the loads' channel-column adds, 10 the validity tests and line-end selects of the six row offsets,
# which leaves the lane-side borrow arithmetic and two byte offsets at 19.
WGRAD = {
    'false': dict(post=601, step=52),    # reached 572 (workspace and atomics paths together), 35 + 14 = 49
    'true': dict(post=640, step=100),    # reached 609, 45 + 50 = 95
}


def _measure(name):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import valu_count
    finally:
        sys.path.pop(0)
    return valu_count.measure(os.path.join(ROOT, 'emsanet_amd', 'csrc', name))


def _step(r, mfmas):
    blocks = [c for _, c in r['loop']]
    assert sum(c['mfma'] for c in blocks) == mfmas, r['loop']
    return sum(c['valu'] for c in blocks)


@needs_hipcc
def test_specialised_winograd_epilogues_stay_lean():
    res = _measure('conv_wino.hip')
    bad = []
    for (bnb, inbn, opt), lim in WINO.items():
        r = res[f"conv1d_wino_kernel<64, false, {bnb}, {inbn}, {opt}>"]
        got = dict(pre=r['pre']['valu'], post=r['post']['valu'], step=_step(r, 16))
        print(bnb, inbn, opt, got)
        bad += [f"<{bnb}, {inbn}, {opt}> {k}: {got[k]} > {lim[k]}" for k in lim if got[k] > lim[k]]
    assert not bad, '\n'.join(bad)


@needs_hipcc
def test_fp32_winograd_weight_gradient_stays_lean():
    res = _measure('conv_mfma.hip')
    bad = []
    for xbn, lim in WGRAD.items():
        r = res[f"conv_wgrad1d_wino_kernel<64, 64, false, float, {xbn}>"]
        got = dict(post=r['post']['valu'], step=_step(r, 32))
        print(xbn, got)
        bad += [f"XBN={xbn} {k}: {got[k]} > {lim[k]}" for k in lim if got[k] > lim[k]]
    assert not bad, '\n'.join(bad)
