"""Device-side training augmentation (emsanet_amd/augment.py, csrc/augment.hip) against the NumPy
restatement of tests/augment_reference.py, under the parameter table the engine drew or a forced one.

Gates: the drawn table, every label map, the raw depth crop and the orientation table are equal bit for
bit.  With the HSV amplitudes 0 `rgb` is bit-equal to the engine's `normalize_rgb` of the reference's
resized uint8 crop (and to the NumPy restatement of that expression) and `depth` to `normalize_depth`
of the reference's crop.  With the jitter on, |difference| <= 1e-4 on the normalised values against
the float64 reference: one grey level is 1 / (255 * 0.229) = 1.7e-2 there; under 30 fp32 roundings on
values <= 1 (hue <= 6 enters scaled by v * s <= 1), divided by std >= 0.224, give <= 8e-6, so the gate
is about 10x the round-off bound and 170x below a wrong pixel (the float32 NumPy twin stays under
2.5e-5 of the float64 reference on the CPU, tests/test_augment.py).

Shapes: 37x53 -> 32x48 (one tile, the clamped border rows and columns of an up-scale), 60x80 -> 32x48
(down-scaling), 96x128 = crop, 480x640 bs 2 (many tiles in x and y, whole and partial), and a crop width
of 50 (no multiple of 4: the scalar-store path and a 2-pixel vector tail).

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (label maps of every
integer dtype and the drawn table are compared exactly): the ring slots lie between two bands of 0xFF,
and the raw frames, label maps and forced parameter rows are placed with `guard.put`, so that a gather
past the last source row or column reads poison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R   # noqa: E402
import guard   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STATS = (2000.0, 900.0)
AMPS = (10 / 180, 20 / 255, 50 / 255)
ALL_TASKS = ('semantic', 'scene', 'instance', 'orientation')
NP_DTYPES = {torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8, torch.int16: np.int16,
             torch.uint16: np.uint16}
# 40 classes + void; every third class is stuff, every second thing class has orientations
IS_THING = (False,) + tuple(bool(i % 3) for i in range(40))
USE_ORIENTATION = tuple(t and i % 2 == 0 for i, t in enumerate(IS_THING))


def _args(h, w, smin=1.0, smax=1.4, tasks=ALL_TASKS, modalities=('rgb', 'depth')):
    from emsanet_amd import full_args
    return full_args(input_height=h, input_width=w, aug_scale_min=smin, aug_scale_max=smax, tasks=tasks,
                     input_modalities=modalities)


def _aug(h, w, smin=1.0, smax=1.4, tasks=ALL_TASKS, modalities=('rgb', 'depth'), **kw):
    from emsanet_amd import TrainingAugmenter
    return TrainingAugmenter(_args(h, w, smin, smax, tasks, modalities), STATS, **kw)


def _dev(batch, keys=None):
    return {k: guard.put(torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in batch.items()
            if keys is None or k in keys}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(x, y):
    """bit-equal tensors of any dtype (NaNs compare by their bits)"""
    return x.dtype == y.dtype and x.shape == y.shape and \
        torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def assert_augmented(got, batch, table, h, w, hsv):
    """`got`: the dictionary of apply(); `batch`: the NumPy inputs; `table`: int32 (N, 8)"""
    from emsanet_amd.postprocessing import normalize_depth, normalize_rgb
    keys = [k for k in batch if k in got]
    ref = R.reference_apply({k: batch[k] for k in keys}, table, h, w, STATS, hsv=hsv)
    n = len(table)
    if 'rgb' in keys:
        g = got['rgb']
        assert g.dtype == torch.float32 and tuple(g.shape) == (n, 3, h, w) and g.is_contiguous()
        if hsv:
            err = float(np.abs(g.cpu().numpy().astype(np.float64) - ref['rgb']).max())
            print(f"hsv on, {h}x{w}: max |device - float64 reference| = {err:.3e}")
            assert err <= 1e-4
        else:
            want = normalize_rgb(torch.from_numpy(ref['rgb_u8']).to(DEV))
            assert torch.equal(g.view(torch.int32), want.view(torch.int32)), "rgb bits vs normalize_rgb"
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(ref['rgb'])), "rgb bits vs NumPy"
    if 'depth' in keys:
        g = got['depth']
        assert g.dtype == torch.float32 and tuple(g.shape) == (n, 1, h, w)
        want = normalize_depth(torch.from_numpy(ref['depth_u16']).to(DEV), *STATS)
        assert torch.equal(g.view(torch.int32), want.view(torch.int32)), "depth bits vs normalize_depth"
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(ref['depth']))
        assert not g.cpu().numpy()[:, 0][ref['depth_u16'] == 0].any()
    for k in ('semantic', 'instance'):
        if k in keys:
            assert got[k].dtype == torch.from_numpy(batch[k][:0]).dtype and tuple(got[k].shape) == (n, h, w)
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    if 'orientations' in keys:
        g, want = got['orientations'].cpu().numpy(), ref['orientations']
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(g), nan)
        assert np.array_equal(_bits(g)[~nan], _bits(want)[~nan]), "orientation bits"
    if 'scene' in keys:
        assert np.array_equal(got['scene'].cpu().numpy(), batch['scene'])
    return ref


CASES = {
    'up_37x53': (3, 37, 53, 32, 48, 1.0, 1.4),
    'down_60x80': (3, 60, 80, 32, 48, 0.6, 1.0),
    'same_96x128': (2, 96, 128, 96, 128, 1.0, 1.4),
    'full_480x640': (2, 480, 640, 480, 640, 1.0, 1.4),
    'width_50': (3, 37, 53, 32, 50, 1.0, 1.4),
}


@pytest.fixture(scope='module')
def batches():
    return {name: R.random_batch(c[0], c[1], c[2], seed=i) for i, (name, c) in enumerate(CASES.items())}


@pytest.mark.parametrize('hsv', [False, True], ids=['hsv_off', 'hsv_on'])
@pytest.mark.parametrize('case', list(CASES))
def test_drawn_parameters(batches, case, hsv):
    n, hs, ws, h, w, smin, smax = CASES[case]
    amps = AMPS if hsv else (0.0, 0.0, 0.0)
    aug = _aug(h, w, smin, smax, seed=11, hsv_jitter=amps)
    got = aug.apply(_dev(batches[case]))
    guard.check()
    table = aug.last_params().numpy()
    want = R.draw_table(11, 0, n, hs, ws, h, w, aug.q_min, aug.q_max, 0.5, amps)
    assert np.array_equal(table, want)
    assert_augmented(got, batches[case], table, h, w, hsv)


def test_draw_matches_numpy_over_three_steps(batches):
    n, hs, ws, h, w, _smin, _smax = CASES['up_37x53']
    aug = _aug(h, w, seed=0xDEADBEEF, flip_p=0.25)
    b = _dev(batches['up_37x53'])
    seen = []
    for step in range(3):
        aug.apply(b)
        t = aug.last_params().numpy()
        assert np.array_equal(t, R.draw_table(0xDEADBEEF, step, n, hs, ws, h, w, 1024, 1434, 0.25, AMPS)), step
        seen.append(t)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert aug.state_dict() == {'seed': 0xDEADBEEF, 'step': 3}
    # a resumed run continues the sequence
    other = _aug(h, w, flip_p=0.25)
    other.load_state_dict({'seed': 0xDEADBEEF, 'step': 1})
    other.apply(b)
    assert np.array_equal(other.last_params().numpy(), seen[1])
    other.load_state_dict({'seed': 0xDEADBEEF, 'step': 0})          # after the device state exists
    other.apply(b)
    assert np.array_equal(other.last_params().numpy(), seen[0])


@pytest.mark.parametrize('dt_sem,dt_inst', [(torch.uint8, torch.int64), (torch.int16, torch.uint16),
                                            (torch.uint16, torch.int32), (torch.int32, torch.int16),
                                            (torch.int64, torch.uint8)])
@pytest.mark.parametrize('w', [48, 50])
def test_every_label_dtype(batches, dt_sem, dt_inst, w):
    b = dict(batches['up_37x53'])
    b['semantic'] = b['semantic'].astype(NP_DTYPES[dt_sem])
    b['instance'] = b['instance'].astype(NP_DTYPES[dt_inst])
    aug = _aug(32, w, seed=3)
    got = aug.apply(_dev(b))
    guard.check()
    assert got['semantic'].dtype == dt_sem and got['instance'].dtype == dt_inst
    assert_augmented(got, b, aug.last_params().numpy(), 32, w, True)


def test_single_modalities_and_no_instance(batches):
    b = batches['up_37x53']
    for modalities in (('rgb',), ('depth',)):
        aug = _aug(32, 48, modalities=modalities, seed=4)
        got = aug.apply(_dev(b))
        assert sorted(got) == sorted(list(modalities) + ['instance', 'orientations', 'scene', 'semantic'])
        assert_augmented(got, b, aug.last_params().numpy(), 32, 48, True)
    aug = _aug(32, 48, tasks=('semantic',), seed=4)
    got = aug.apply(_dev(b, ('rgb', 'depth', 'semantic')))
    assert sorted(got) == ['depth', 'rgb', 'semantic']
    assert_augmented(got, b, aug.last_params().numpy(), 32, 48, True)


def _stripes(n, hs, ws):
    """top half: stripes of black, white, grey and the six saturated colours; bottom half: noise"""
    colours = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [255, 255, 0], [0, 255, 0],
                        [0, 255, 255], [0, 0, 255], [255, 0, 255]], np.uint8)
    b = R.random_batch(n, hs, ws, seed=77)
    b['rgb'][:, :hs // 2] = colours[(np.arange(ws) * len(colours)) // ws][None, None]
    return b


def test_forced_parameter_rows():
    """through params=: flip on and off, the crop at both corners, the maximum scale, and the extreme
    HSV deltas of both signs on pure black, white, grey and the six saturated colours"""
    hs, ws, h, w = 37, 53, 32, 48
    hm, wm = (hs * 1434 + 512) >> 10, (ws * 1434 + 512) >> 10
    a = [np.float32(v) for v in AMPS]
    rows = [(hs, ws, 0, 0, 0, a[0], a[1], a[2]),
            (hs, ws, hs - h, ws - w, 1, -a[0], -a[1], -a[2]),
            (hm, wm, 0, 0, 1, a[0], -a[1], a[2]),
            (hm, wm, hm - h, wm - w, 0, -a[0], a[1], -a[2]),
            (hm, wm, 0, wm - w, 1, a[0], a[1], -a[2]),
            (hs, ws, 0, 2, 0, 0.0, 0.0, 0.0)]
    table = R.pack_rows(rows)
    b = _stripes(len(rows), hs, ws)
    dev = _dev(b)
    params = guard.put(torch.from_numpy(table).to(DEV))
    for hsv in (True, False):
        aug = _aug(h, w, hsv_jitter=AMPS if hsv else (0.0, 0.0, 0.0))
        got = aug.apply(dev, params=params)
        guard.check()
        assert np.array_equal(aug.last_params().numpy(), table)
        ref = assert_augmented(got, b, table, h, w, hsv)
        assert aug.state_dict()['step'] == 0                      # a forced table draws nothing
    # the pure colours are in the crop of the un-scaled rows
    assert {(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 0, 255)} <= \
        {tuple(c) for c in ref['rgb_u8'][0, 0]}
    # repeated apply with the same params is bit-identical, in the other ring slot
    aug = _aug(h, w)
    first = aug.apply(dev, params=params)
    second = aug.apply(dev, params=params)
    for k in first:
        assert first[k].data_ptr() != second[k].data_ptr(), k
        assert _same(first[k], second[k]), k


@pytest.mark.parametrize('w', [48, 50])
def test_forced_far_corner_with_flip(w):
    """the crop in the far corner of the resized frame, flipped, at scale 1 and at the maximum scale: the
    last source row and column are the last ones gathered (the bilinear taps beyond are clamped), at a
    crop width that is a multiple of the 4-pixel vector and at one that is not (50)"""
    hs, ws, h = 37, 53, 32
    hm, wm = (hs * 1434 + 512) >> 10, (ws * 1434 + 512) >> 10
    a = [np.float32(v) for v in AMPS]
    rows = [(hs, ws, hs - h, ws - w, 1, a[0], -a[1], a[2]),
            (hm, wm, hm - h, wm - w, 1, -a[0], a[1], -a[2]),
            (hm, wm, hm - h, wm - w, 0, 0.0, 0.0, 0.0)]
    table = R.pack_rows(rows)
    b = _stripes(len(rows), hs, ws)
    params = guard.put(torch.from_numpy(table).to(DEV))
    for hsv in (True, False):
        aug = _aug(h, w, hsv_jitter=AMPS if hsv else (0.0, 0.0, 0.0))
        got = aug.apply(_dev(b), params=params)
        guard.check()
        assert np.array_equal(aug.last_params().numpy(), table)
        assert_augmented(got, b, table, h, w, hsv)


def test_ring_keeps_the_previous_outputs(batches):
    b = _dev(batches['up_37x53'])
    aug = _aug(32, 48, seed=8, ring=2)
    first = aug.apply(b)
    table = aug.last_params().numpy()
    kept = {k: v.clone() for k, v in first.items()}
    second = aug.apply(b)
    assert not np.array_equal(aug.last_params().numpy(), table)
    torch.cuda.synchronize()
    for k in first:
        assert first[k].data_ptr() != second[k].data_ptr(), k
        assert _same(first[k], kept[k]), k
    assert_augmented(first, batches['up_37x53'], table, 32, 48, True)
    third = aug.apply(b)                                           # ring = 2: the first slot again
    assert third['rgb'].data_ptr() == first['rgb'].data_ptr()


def test_resize_normalize(batches):
    b = batches['up_37x53']
    aug = _aug(32, 48)
    got = aug.resize_normalize(_dev(b), 24, 32)
    table = R.pack_rows([(24, 32, 0, 0, 0, 0.0, 0.0, 0.0)] * 3)
    assert np.array_equal(aug.last_params().numpy(), table)
    assert_augmented(got, b, table, 24, 32, False)
    assert aug.state_dict()['step'] == 0
    same = aug.resize_normalize(_dev(b), 37, 53)                   # the identity: a plain normalisation
    assert np.array_equal(same['semantic'].cpu().numpy(), b['semantic'])
    assert_augmented(same, b, R.pack_rows([(37, 53, 0, 0, 0, 0.0, 0.0, 0.0)] * 3), 37, 53, False)


def _generator(args, **kw):
    from emsanet_amd import TrainingTargetGenerator
    return TrainingTargetGenerator(args, IS_THING, USE_ORIENTATION, max_instances=16, **kw)


def _same_targets(a, b):
    assert sorted(a) == sorted(b)
    for x, y in zip(a['semantic'], b['semantic']):
        assert torch.equal(x, y)
    for dx, dy in zip(a['instance'], b['instance']):
        assert sorted(dx) == sorted(dy)
        for k in dx:
            assert _same(dx[k], dy[k]), k
    assert torch.equal(a['scene'], b['scene'])


def test_apply_and_generate_capture_into_a_graph():
    """warm up, capture apply + generate, replay twice: the two replays' tables are the reference's steps
    k and k + 1, and the outputs are those of these tables"""
    n, hs, ws, h, w = 2, 110, 140, 96, 128
    b = R.random_batch(n, hs, ws, seed=21)
    dev = _dev(b)
    args = _args(h, w)
    aug = _aug(h, w, seed=13)
    gen, eager_gen = _generator(args), _generator(args)
    gen.generate(aug.apply(dev))                                   # step 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            got = aug.apply(dev)
            targets = gen.generate(got)
    torch.cuda.current_stream().wait_stream(stream)
    tables = []
    for step in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        table = aug.last_params().numpy()
        assert np.array_equal(table, R.draw_table(13, step, n, hs, ws, h, w)), step
        assert_augmented(got, b, table, h, w, True)
        _same_targets(targets, eager_gen.generate({k: v.clone() for k, v in got.items()}))
        tables.append(table)
    assert not np.array_equal(tables[0], tables[1])
    gen.check()
    guard.check()                            # (every captured buffer was made by the warm-up step)


def test_batch_stager_augments_and_generates():
    """three pinned batches of raw frames in: what the stager hands out equals apply + generate on the
    same raw tensors (a second augmenter with the same seed draws the same sequence)"""
    from emsanet_amd.staging import BatchStager
    n, hs, ws, h, w = 2, 110, 140, 96, 128
    raw = [R.random_batch(n, hs, ws, seed=30 + j, sem_dtype=np.uint8, inst_dtype=np.int16) for j in range(3)]

    def host_batches():
        for j, b in enumerate(raw):
            hb = {k: torch.from_numpy(v).pin_memory() for k, v in b.items()}
            hb['name'] = f'batch{j}'
            yield hb

    args = _args(h, w)
    staged = list(BatchStager(host_batches(), DEV, augmenter=_aug(h, w, seed=5, ring=3),
                              target_generator=_generator(args, ring=3)))
    torch.cuda.synchronize()
    guard.check()                            # the stager's device buffers, the augmenter's and the generator's rings
    aug, gen = _aug(h, w, seed=5), _generator(args)
    assert len(staged) == 3
    for j, (s, b) in enumerate(zip(staged, raw)):
        assert sorted(s) == ['depth', 'instance', 'name', 'orientations', 'rgb', 'scene', 'semantic', 'targets']
        assert s['name'] == f'batch{j}'
        want = aug.apply(_dev(b))
        table = aug.last_params().numpy()
        assert np.array_equal(table, R.draw_table(5, j, n, hs, ws, h, w))
        for k in want:
            assert _same(s[k], want[k]), (j, k)
        _same_targets(s['targets'], gen.generate(want))
        assert_augmented(s, b, table, h, w, True)
    # without the argument nothing changes: the raw label maps and the plain normalisation
    plain = next(iter(BatchStager(host_batches(), DEV, depth_stats=STATS)))
    assert tuple(plain['rgb'].shape) == (n, 3, hs, ws) and tuple(plain['semantic'].shape) == (n, hs, ws)


def test_training_step_on_an_augmented_batch():
    """96x128, bs 2, all tasks, fp32.  With params forcing the identity and the amplitudes 0 the losses
    of a step are bit-equal to the step on the un-augmented batch through the existing path
    (normalize_rgb, normalize_depth, generate on the raw maps); a drawn augmentation of larger raw frames
    gives finite losses"""
    from emsanet_amd import nyuv2_config
    from emsanet_amd.loss import TrainingLosses
    from emsanet_amd.model import EMSANet
    from emsanet_amd.postprocessing import normalize_depth, normalize_rgb
    n, h, w = 2, 96, 128
    args = _args(h, w)
    torch.manual_seed(0)
    model = EMSANet(args, nyuv2_config()).to(DEV).train()
    g = torch.Generator(device='cpu').manual_seed(99)
    crit = TrainingLosses(args, torch.rand(40, generator=g) * 2 + 0.3, 10).to(DEV)
    gen = _generator(args, ring=3)
    raw = _dev(R.random_batch(n, h, w, seed=40))

    def losses(inputs, labels):
        targets = gen.generate(labels)
        model.dropout_step = 0
        with torch.no_grad():
            total, parts = crit(model({'rgb': inputs['rgb'], 'depth': inputs['depth']}), targets)
        return {k: float(v) for k, v in parts.items()}, float(total)

    plain = {'rgb': normalize_rgb(raw['rgb']), 'depth': normalize_depth(raw['depth'], *STATS)}
    l_plain, t_plain = losses(plain, raw)
    identity = torch.tensor([[h, w, 0, 0, 0, 0, 0, 0]] * n, dtype=torch.int32, device=DEV)
    same = _aug(h, w, hsv_jitter=(0.0, 0.0, 0.0)).apply(raw, params=identity)
    l_same, t_same = losses(same, same)
    gen.check()
    assert sorted(l_plain) == ['instance_center', 'instance_offset', 'instance_orientation', 'scene', 'semantic']
    for k in l_plain:
        print(f"{k}: existing path {l_plain[k]!r}, identity augmentation {l_same[k]!r}")
        assert np.isfinite(l_plain[k]) and l_plain[k] == l_same[k], k
    assert t_plain == t_same
    big = _dev(R.random_batch(n, 120, 150, seed=41))
    out = _aug(h, w, seed=1).apply(big)
    l_aug, t_aug = losses(out, out)
    gen.check()
    assert all(np.isfinite(v) for v in l_aug.values()) and np.isfinite(t_aug) and t_aug > 0
    assert l_aug['semantic'] != l_plain['semantic']


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
