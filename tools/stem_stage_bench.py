"""The half-resolution stage behind the two stem convolutions, fused (csrc/stem_stage.hip) against
the kernels it replaces, at the training shape 32 x 64 x 240 x 320 (GPU box, one process): per pass the
median of 20 device-event timings in us, and the achieved TB/s = the bytes the pass has to move
(every tensor operand once) / time.   usage: python tools/stem_stage_bench.py [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emsanet_amd import functional as Fn      # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps=20, warm=3):
    """-> (median us, algorithmic bytes of one call: every operand the wrappers hand to a launch)"""
    for _ in range(warm):
        fn()
    Fn.BYTES = [0]
    fn()
    nbytes, Fn.BYTES = Fn.BYTES[0], None
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--h', type=int, default=240)
    ap.add_argument('--w', type=int, default=320)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, c, cr, h, w = a.n, 64, 4, a.h, a.w
    torch.manual_seed(0)
    ys = [Fn.act_empty(n, c, h, w, DEV).normal_() for _ in range(2)]
    gam = [torch.rand(c, device=DEV) + 0.5 for _ in range(2)]
    st = [(y.mean((0, 2, 3)), 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + 1e-5)) for y in ys]
    aff = [(g * s[1], 0.1 - s[0] * g * s[1]) for g, s in zip(gam, st)]
    se = [(torch.randn(cr, c, device=DEV) * 0.3, torch.randn(cr, device=DEV) * 0.3,
           torch.randn(c, cr, device=DEV) * 0.3, torch.randn(c, device=DEV) * 0.3) for _ in range(2)]
    oh, ow = (h + 1) // 2, (w + 1) // 2
    gf, gd = (Fn.act_empty(n, c, oh, ow, DEV).normal_() for _ in range(2))
    R = Fn.ACT_RELU
    # ---- state both paths share ----
    acts, bits = zip(*(Fn.bn_act(y, sc, sh, None, None, R, want_mask=True) for y, (sc, sh) in zip(ys, aff)))
    gr, gdp, hr, hd, sr, sd = Fn.se_pair_fwd(acts[0], acts[1], se[0], se[1])
    fmap = Fn.se_scale_add(acts[0], sr, acts[1], sd)
    _, idx_f = Fn.maxpool_fwd(fmap)
    _, idx_d = Fn.maxpool_fwd(acts[1])
    gap, hid, s = (gr, gdp), (hr, hd), (sr, sd)

    def unfused_bwd():
        dout = Fn.maxpool_bwd(gf, idx_f, (h, w))
        ddn = Fn.maxpool_bwd(gd, idx_d, (h, w))
        for m in range(2):
            ds = Fn.se_scale_bwd_reduce(dout, acts[m])
            dgap = Fn.se_mlp_bwd(gap[m], se[m][0], se[m][2], hid[m], s[m], ds)[0]
            da = Fn.se_scale_bwd_apply(dout, s[m], dgap, ddn if m else None)
            Fn.bn_bwd(da, bits[m], ys[m], gam[m], st[m][0], st[m][1], None, R, True, want_dres=False)

    sums, ds_r, ds_d = Fn.stem_stage_bwd_reduce(gf, idx_f, gd, idx_d, ys[0], ys[1], aff[0], aff[1],
                                                st[0], st[1])
    dgaps = [Fn.se_mlp_bwd(gap[m], se[m][0], se[m][2], hid[m], s[m], ds)[0]
             for m, ds in enumerate((ds_r, ds_d))]
    dgb = Fn.stem_stage_bwd_finalize(sums, h * w, sr, sd, dgaps[0], dgaps[1])

    def fused_bwd():
        sm, d0, d1 = Fn.stem_stage_bwd_reduce(gf, idx_f, gd, idx_d, ys[0], ys[1], aff[0], aff[1],
                                              st[0], st[1])
        dg = [Fn.se_mlp_bwd(gap[m], se[m][0], se[m][2], hid[m], s[m], ds)[0]
              for m, ds in enumerate((d0, d1))]
        o = Fn.stem_stage_bwd_finalize(sm, h * w, sr, sd, dg[0], dg[1])
        Fn.stem_stage_bwd_apply(gf, idx_f, gd, idx_d, ys[0], ys[1], aff[0], aff[1], st[0], st[1], gam[0],
                                gam[1], sr, sd, dg[0], dg[1], o)

    def unfused_fwd():
        a2 = [Fn.bn_act(y, sc, sh, None, None, R, want_mask=True)[0] for y, (sc, sh) in zip(ys, aff)]
        r = Fn.se_pair_fwd(a2[0], a2[1], se[0], se[1])
        Fn.maxpool_fwd(Fn.se_scale_add(a2[0], r[4], a2[1], r[5]))
        Fn.maxpool_fwd(a2[1])

    def fused_fwd():
        r = Fn.stem_stage_se(ys[0], ys[1], aff[0], aff[1], se[0], se[1])
        Fn.stem_stage_fwd(ys[0], ys[1], aff[0], aff[1], r[4], r[5])

    passes = [
        ('unfused forward (bn_act x2, se_pair, se_scale_add, maxpool x2)', unfused_fwd),
        ('fused forward (both passes)', fused_fwd),
        ('  fused fwd 1: squeeze + pair MLP', lambda: Fn.stem_stage_se(ys[0], ys[1], aff[0], aff[1], se[0], se[1])),
        ('  fused fwd 2: scale-add + max pools', lambda: Fn.stem_stage_fwd(ys[0], ys[1], aff[0], aff[1], sr, sd)),
        ('unfused backward (maxpool_bwd x2, SE bwd x2, bn_bwd x2)', unfused_bwd),
        ('fused backward (both passes + SE MLP bwd + finalize)', fused_bwd),
        ('  fused bwd 1: reduce + merge', lambda: Fn.stem_stage_bwd_reduce(
            gf, idx_f, gd, idx_d, ys[0], ys[1], aff[0], aff[1], st[0], st[1])),
        ('  fused bwd 2: apply', lambda: Fn.stem_stage_bwd_apply(
            gf, idx_f, gd, idx_d, ys[0], ys[1], aff[0], aff[1], st[0], st[1], gam[0], gam[1], sr, sd,
            dgaps[0], dgaps[1], dgb)),
    ]
    rows = []
    print(f"shape {n} x {c} x {h} x {w} fp32 ({ys[0].numel() * 4 / 1e6:.0f} MB per tensor)")
    for name, fn in passes:
        us, nbytes = timed(fn)
        rows.append({'pass': name.strip(), 'us': round(us, 1), 'gbytes': round(nbytes / 1e9, 3),
                     'tb_per_s': round(nbytes / us / 1e6, 2)})
        print(f"{name:62s} {us:8.1f} us  {nbytes / 1e9:6.2f} GB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'shape': [n, c, h, w], 'reps': 20, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
