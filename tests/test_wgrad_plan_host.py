"""CPU, the real library: the workspace plan of the weight-gradient launchers.

emsa_conv_wgrad_ws_bytes_t and emsa_conv_wgrad_multi_ws_bytes are pure host functions; their answer
is the split-K plan (which kernel family takes the geometry, how many splits, the workspace layout).
tests/golden/wgrad_ws_bytes.json records the answers of the commit named in its first key
(tools/gen_wgrad_ws_golden.py): the launcher's selection code must keep them."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_wgrad_ws_golden as G  # noqa: E402

with open(os.path.join(ROOT, 'tests', 'golden', 'wgrad_ws_bytes.json')) as _f:
    GOLDEN = json.load(_f)


def test_table_is_the_generators():
    assert [s[0] for s in GOLDEN['single']] == G.single_cases()
    assert [[m[0], m[1]] for m in GOLDEN['multi']] == [list(m) for m in G.multi_cases()]
    assert 'commit' in GOLDEN['generated_by']


def test_hand_checked_figures():
    """hand-checked answers: 64 -> 64 3x1 at 2x30x40 runs 10 splits of one tile in every storage
    type; a 1x1 conv has a two-pass form in 16-bit storage only (3 splits of two one-tap tiles)"""
    by_case = {tuple(c): b for c, b in GOLDEN['single']}
    assert by_case[tuple(G.c31(2, 30, 40, 64))] == [494080] * 3
    assert by_case[(2, 30, 40, 64, 128, 1, 1, 2, 2, 0, 0, 0, 0)] == [0, 99840, 99840]
    assert by_case[tuple(G.c31(2, 30, 40, 6))] == [0, 0, 0]
    same = G.c31(2, 30, 40, 64)
    assert [G.multi_ws_bytes(d, [same, same]) for d in range(3)] == [0, 988160, 0]


@pytest.mark.parametrize('dtype', range(3), ids=G.DTYPES)
def test_single_ws_bytes(dtype):
    got = [G.ws_bytes(dtype, c) for c, _ in GOLDEN['single']]
    assert got == [b[dtype] for _, b in GOLDEN['single']]
    if dtype == 0:      # the fp32 twin entry point
        from emsanet_amd import _lib
        assert got == [int(_lib.lib().emsa_conv_wgrad_ws_bytes(G.geom(c))) for c, _ in GOLDEN['single']]


def test_multi_ws_bytes():
    got = [G.multi_ws_bytes(G.DTYPES.index(dt), cs) for dt, cs, _ in GOLDEN['multi']]
    assert got == [b for _, _, b in GOLDEN['multi']]
    assert all(b > 0 for b in got[:6]) and got[6:] == [0, 0, 0, 0]


def _ceil(a, b):
    return (a + b - 1) // b


def test_equal_jobs_one_layout_formula():
    """n equal jobs with a common split ks take n * ks * (per-split floats): partial tiles
    [R][n_tiles][taps][64][64] + bias rows [n_co_tiles][64], ks from the shared budget of 768
    workgroups with at least four 64-pixel K steps per split"""
    checked = 0
    for case, _ in GOLDEN['single']:
        n_img, h, w, cin, cout, kh, kw, sh, sw = case[:9]
        if (kh, kw) not in ((3, 1), (1, 3)) or sh != 1 or sw != 1:
            continue
        for n in (2, 3, 4):
            got = G.multi_ws_bytes(1, [case] * n)
            if cin % 8 or cout % 8 or case[11] % 8 or case[12] % 8:
                assert got == 0, (case, n)
                continue
            n_tiles = _ceil(cout, 64) * _ceil(cin, 64)
            per_split = n_tiles * 3 * 4096 + _ceil(cout, 64) * 64
            line, lines = (h, w) if kh == 3 else (w, h)
            steps = _ceil(n_img * lines * (line + 1), 64)      # one virtual zero pixel behind every line
            ks = max(1, min(768 // (n * n_tiles), _ceil(steps, 4)))
            ks = _ceil(steps, _ceil(steps, ks))
            assert got == n * ks * per_split * 4, (case, n, ks)
            checked += 1
    assert checked >= 3 * 96
