"""Writes tests/golden/wgrad_ws_bytes.json: what emsa_conv_wgrad_ws_bytes_t and
emsa_conv_wgrad_multi_ws_bytes (pure host functions, no GPU needed) answer over a geometry table.

    python tools/gen_wgrad_ws_golden.py <commit the library was built from> [out.json]

tests/test_wgrad_plan_host.py holds every later library to these answers.  A case is
[n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, ld_in, ld_out]; ld 0 = dense (the channel count).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DTYPES = ('f32', 'bf16', 'f16')           # EMSA_DT_* codes 0, 1, 2


def geom(case):
    from emsanet_amd.functional import ConvSpec
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, ld_in, ld_out = case
    return ConvSpec(cin, cout, (kh, kw), (sh, sw), (ph, pw)).geom_fwd(n, h, w, ld_in or cin, ld_out or cout)


def ws_bytes(dtype, case):
    from emsanet_amd import _lib
    return int(_lib.lib().emsa_conv_wgrad_ws_bytes_t(dtype, geom(case)))


def multi_ws_bytes(dtype, cases):
    import ctypes
    from emsanet_amd import _lib
    geoms = (_lib.EmsaConvGeom * len(cases))()
    for j, c in enumerate(cases):
        ctypes.memmove(ctypes.byref(geoms[j]), ctypes.byref(geom(c)), ctypes.sizeof(_lib.EmsaConvGeom))
    return int(_lib.lib().emsa_conv_wgrad_multi_ws_bytes(dtype, len(cases), geoms))


def c31(n, h, w, c, cout=None, **kw):
    return [n, h, w, c, cout or c, 3, 1, kw.get('sh', 1), 1, 1, 0, kw.get('ld_in', 0), kw.get('ld_out', 0)]


def c13(n, h, w, c, cout=None, **kw):
    return [n, h, w, c, cout or c, 1, 3, 1, kw.get('sw', 1), 0, 1, kw.get('ld_in', 0), kw.get('ld_out', 0)]


def single_cases():
    out = []
    # the NBt1D convs: every channel count on every map (odd lines at 15x20), batch 1 / 2 / 8
    for c in (64, 128, 256, 512):
        for h, w in ((120, 160), (60, 80), (30, 40), (15, 20)):
            for n in (1, 2, 8):
                out += [c31(n, h, w, c), c13(n, h, w, c)]
    # the dense 3x3 shapes of Fn.WGRAD_WINO2D_SHAPES at their resolutions
    for cin, cout, h, w in ((512, 512, 15, 20), (512, 256, 30, 40), (256, 128, 60, 80), (128, 40, 120, 160),
                            (128, 96, 120, 160), (96, 8, 120, 160)):
        out.append([2, h, w, cin, cout, 3, 3, 1, 1, 1, 1, 0, 0])
    out += [[2, 30, 40, 64, 128, 1, 1, 1, 1, 0, 0, 0, 0],          # 1x1, stride 1 and 2
            [2, 30, 40, 64, 128, 1, 1, 2, 2, 0, 0, 0, 0],
            c31(2, 30, 40, 64, sh=2), c13(2, 30, 40, 64, sw=2),      # down-sampling 3-tap convs
            c31(2, 30, 40, 12), c13(2, 30, 40, 12),                  # 4-channel rule, not the 8-channel one
            c31(2, 30, 40, 6),                                       # refused: 0
            c31(2, 30, 40, 64, ld_out=128), c13(2, 15, 20, 64, ld_in=96, ld_out=72),
            c31(2, 30, 40, 64, ld_out=68)]                           # (68: 4-, not 8-aligned rows)
    seen, uniq = set(), []
    for c in out:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            uniq.append(c)
    return uniq


def multi_cases():
    a, b = c31(2, 30, 40, 64), c13(2, 30, 40, 64)      # lines of 30 and of 40 pixels
    o = c13(2, 15, 20, 64)                             # odd lines, a quarter of the pixels
    w = c31(2, 15, 20, 512)
    return [('bf16', [a, b]), ('bf16', [a, b, o]), ('bf16', [a, b, a, b]), ('bf16', [o, b, a, o]),
            ('bf16', [w, c13(2, 15, 20, 512)]), ('bf16', [w] * 4),
            ('bf16', [a, b, a, b, a]),                 # the rest answer 0: five jobs,
            ('bf16', [a, c31(2, 30, 40, 128)]),        # unequal channel counts,
            ('f32', [a, b]), ('f16', [a, b])]          # other storage types


def main():
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'wgrad_ws_bytes.json')
    single = [[c, [ws_bytes(d, c) for d in range(3)]] for c in single_cases()]
    multi = [[dt, cs, multi_ws_bytes(DTYPES.index(dt), cs)] for dt, cs in multi_cases()]
    with open(path, 'w') as f:
        f.write('{"generated_by": "tools/gen_wgrad_ws_golden.py on the library of commit %s",\n' % commit)
        f.write(' "case": "[n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, ld_in, ld_out], bytes for f32 / bf16 / f16",\n')
        f.write(' "single": [\n  ' + ',\n  '.join(json.dumps(s) for s in single) + '],\n')
        f.write(' "multi": [\n  ' + ',\n  '.join(json.dumps(m) for m in multi) + ']}\n')
    print(f"{len(single)} geometries x 3 dtypes, {len(multi)} multi-job sets -> {path}")


if __name__ == '__main__':
    main()
