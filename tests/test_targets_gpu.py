"""Device-side training targets (emsanet_amd/targets.py, csrc/targets.hip) against the brute-force NumPy
reference of tests/targets_reference.py.

Gates: the label maps, both foreground masks and the centres are equal; `center` is bit-equal (both
sides take exp in float64 and round to fp32 once, per integer d2); `offset` and `orientation` within
1 fp32 ulp (the one rounding of the division; the angle is a copy); everything off the foreground is
exactly 0.

The edge scene (targets_reference.edge_scene, 96x128, N = 3: side scales 12x16, 6x8, 3x4) holds: an
image without any instance; non-contiguous ids including max_instances - 1; a one-pixel instance; an
instance touching two borders (clipped window); two instances whose windows overlap (the maximum); an
instance on a stuff class and one on void (both cleared); an instance that vanishes at /32; a mean of
exactly x.5 in both directions with an even and with an odd integer part; orientations present, NaN,
and on a class that uses none -- tests/test_targets.py checks that it does.

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (the label maps, both
bool masks and the centre table are compared exactly, and True / -1 are what 0xFF reads as): outputs,
ring slots and the workspace lie between two bands of 0xFF, the inputs are placed with `guard.put`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard   # noqa: E402
import targets_reference as R   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_DTYPES = {torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8, torch.int16: np.int16,
             torch.uint16: np.uint16}


def _args(**kw):
    from emsanet_amd import full_args
    return full_args(**kw)


def _gen(args=None, **kw):
    from emsanet_amd import TrainingTargetGenerator
    return TrainingTargetGenerator(args or _args(), R.IS_THING, R.USE_ORIENTATION, **kw)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(NP_DTYPES[dtype])))
    return guard.put(t.to(DEV))                  # flush between two bands of 0xFF: a read past its end is poison


def _batch(sem, inst, ori=None, scene=None, dt_sem=None, dt_inst=None):
    b = {'semantic': _dev(sem, dt_sem), 'instance': _dev(inst, dt_inst)}
    if ori is not None:
        b['orientations'] = _dev(ori)
    if scene is not None:
        b['scene'] = _dev(scene)
    return b


def _ulp_close(got, want):
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


def assert_targets(got, ref, n_scales=4, inst_scales=None, centers=None):
    """`got`: the dictionary of generate(); `ref`: reference_targets() of the same labels"""
    inst_scales = n_scales if inst_scales is None else inst_scales
    assert len(got['semantic']) == n_scales and len(got['instance']) == inst_scales
    for z, (g, want) in enumerate(zip(got['semantic'], ref['semantic'])):
        assert g.dtype == torch.int64 and g.is_contiguous(), z
        assert np.array_equal(g.cpu().numpy(), want), f"semantic, scale {z}"
    for z, (g, want) in enumerate(zip(got['instance'], ref['instance'])):
        fg = want['foreground']
        assert g['foreground'].dtype == torch.bool and g['center'].dtype == torch.float32
        assert np.array_equal(g['foreground'].cpu().numpy(), fg), f"foreground, scale {z}"
        c = g['center'].cpu().numpy()
        assert c.shape == want['center'].shape
        assert np.array_equal(c.view(np.int32), want['center'].view(np.int32)), f"center bits, scale {z}"
        assert g['offset'].shape == want['offset'].shape
        assert g['offset'].permute(0, 2, 3, 1).is_contiguous()
        o = g['offset'].cpu().numpy()
        assert _ulp_close(o, want['offset']), f"offset, scale {z}"
        assert not o[:, 0][~fg].any() and not o[:, 1][~fg].any(), f"offset off the foreground, scale {z}"
        if 'orientation' in want:
            a = g['orientation'].cpu().numpy()
            assert _ulp_close(a, want['orientation']), f"orientation, scale {z}"
            assert not a[~fg].any()
            assert np.array_equal(g['orientation_foreground'].cpu().numpy(), want['orientation_foreground'])
        else:
            assert 'orientation' not in g
    if ref['scene'] is not None and 'scene' in got:
        assert got['scene'].dtype == torch.int64 and np.array_equal(got['scene'].cpu().numpy(), ref['scene'])
    if centers is not None:
        for z, (table, want) in enumerate(zip(centers, ref['centers'])):
            t = table.cpu().numpy()
            for i, per_image in enumerate(want):
                have = {int(k): (int(t[i, k, 0]), int(t[i, k, 1])) for k in np.nonzero(t[i, :, 0] >= 0)[0]}
                assert have == per_image, f"centres, scale {z}, image {i}"


@pytest.fixture(scope='module')
def edge():
    sem, inst, ori, scene = R.edge_scene()
    return sem, inst, ori, scene, R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene)


@pytest.mark.parametrize('dt_inst', [torch.uint8, torch.int16, torch.uint16, torch.int32, torch.int64])
@pytest.mark.parametrize('dt_sem', [torch.uint8, torch.int32, torch.int64])
def test_edge_scene_every_label_dtype(edge, dt_sem, dt_inst):
    sem, inst, ori, scene, ref = edge
    gen = _gen()
    got = gen.generate(_batch(sem, inst, ori, scene, dt_sem, dt_inst))
    gen.check()
    guard.check()
    assert got.get('center_mask') is None
    assert_targets(got, ref, centers=gen.last_centers())


@pytest.fixture(scope='module')
def corner():
    sem, inst, ori, scene = R.corner_scene()
    return sem, inst, ori, scene, R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene)


@pytest.mark.parametrize('dt_sem, dt_inst', [(torch.uint8, torch.uint8), (torch.int64, torch.int16),
                                             (torch.int32, torch.int64)])
def test_corner_scene_one_pixel_scale_maps(corner, dt_sem, dt_inst):
    """32x32: scale maps of 1x1, 2x2 and 4x4 pixels (1, 4, 16: no multiple of 64, one partial wave),
    Gaussian windows clipped at each of the four image corners, the last id of the table in the last
    pixel of image 0 and as the only instance of image 1 (tests/test_targets.py: the scene's claims)"""
    sem, inst, ori, scene, ref = corner
    gen = _gen()
    got = gen.generate(_batch(sem, inst, ori, scene, dt_sem, dt_inst))
    gen.check()
    guard.check()
    assert [tuple(t.shape[1:]) for t in got['semantic']] == [(32, 32), (1, 1), (2, 2), (4, 4)]
    assert_targets(got, ref, centers=gen.last_centers())


def test_last_table_entry_beside_the_first_refused_id(corner):
    """max_instances = 200 on the corner scene with its ids moved: 199, the last entry of every
    per-instance table (acc[3][m], the list, centre_of), is stored; 200, on its neighbour pixels, is
    flagged and stored nowhere -- the guards stand behind each table"""
    sem, inst, ori, scene, _ = corner
    m = 200
    inst = np.where(inst == 255, m - 1, np.where(inst == 254, m, inst))
    assert (inst[0, 29:, 29:] == m - 1).all() and (inst[0, 29:, :3] == m).all() and (inst[1] == m - 1).all()
    ori = np.ascontiguousarray(ori[:, :m])
    ori[:, m - 1] = 0.5
    ref = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene, max_instances=m)
    assert ref['bad_id'] and ref['centers'][0][0] == {1: (1, 1), 2: (1, 30), m - 1: (30, 30)}
    gen = _gen(max_instances=m)
    got = gen.generate(_batch(sem, inst, ori, scene, torch.uint8, torch.uint8))
    guard.check()
    assert_targets(got, ref, centers=gen.last_centers())
    with pytest.raises(ValueError, match='instance id'):
        gen.check()


def test_large_instance_and_many_small_ones():
    """480x640, N = 2: one instance covering a whole image (75 workgroups of partial sums merged with
    global atomics, count 307200, sum_x 98 million) and 200 small ones; two eager calls on the same
    inputs are bit-identical"""
    sem, inst = R.rectangles_scene(2, 480, 640, 200, seed=3, big_first=True)
    ref = R.reference_targets(sem, inst, R.IS_THING)
    assert ref['centers'][0][0] == {255: (240, 320)} and len(ref['centers'][0][1]) == 200   # 239.5 -> 240
    gen = _gen(_args(tasks=('semantic', 'instance')))
    batch = _batch(sem, inst, dt_sem=torch.uint8, dt_inst=torch.int32)
    first = gen.generate(batch)
    assert_targets(first, ref, centers=gen.last_centers())
    guard.check()
    second = gen.generate(batch)                     # the other ring slot: `first` stays valid
    gen.check()
    for a, b in zip(first['instance'], second['instance']):
        for k in a:
            assert a[k].data_ptr() != b[k].data_ptr() and torch.equal(a[k], b[k]), k
    third = gen.generate(batch)                      # ring = 2: the first slot again, accumulators re-zeroed
    assert third['instance'][0]['center'].data_ptr() == first['instance'][0]['center'].data_ptr()
    assert_targets(third, ref, centers=gen.last_centers())


def test_deeplab_pixel_offsets(edge):
    sem, inst, ori, scene, _ = edge
    ref = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene, normalized_offset=False)
    gen = _gen(_args(instance_offset_encoding='deeplab'))
    got = gen.generate(_batch(sem, inst, ori, scene))
    assert_targets(got, ref)
    assert float(got['instance'][0]['offset'].abs().max()) >= 10.0


def test_single_scale_generator(edge):
    """both no-multiscale switches set: every task gets its full-scale entry only"""
    sem, inst, ori, scene, ref = edge
    gen = _gen(_args(semantic_no_multiscale_supervision=True, instance_no_multiscale_supervision=True))
    got = gen.generate(_batch(sem, inst, ori, scene))
    gen.check()
    assert_targets(got, ref, n_scales=1)
    # one switch only: four semantic maps, one set of instance targets
    got = _gen(_args(instance_no_multiscale_supervision=True)).generate(_batch(sem, inst, ori, scene))
    assert_targets(got, ref, n_scales=4, inst_scales=1)


def test_semantic_only_generator(edge):
    sem, _inst, _ori, _scene, ref = edge
    got = _gen(_args(tasks=('semantic',))).generate({'semantic': _dev(sem, torch.uint8)})
    assert sorted(got) == ['semantic']
    for g, want in zip(got['semantic'], ref['semantic']):
        assert np.array_equal(g.cpu().numpy(), want)


def _partition_equal(got_ids, inst):
    """the recovered ids equal the ground truth up to a renaming, on every foreground pixel"""
    fg = inst != 0
    pairs = np.unique(np.stack([inst[fg], got_ids[fg]]), axis=1)
    return (got_ids[fg] != 0).all() and len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


def test_inverse_of_the_postprocessing():
    """the full-scale `center` / `offset` of a scene of rectangles, fed to the engine's instance
    post-processing (threshold 0.1, kernel 17), give the ground-truth partition back: this ties the [U]
    conventions (centre rounding, (dy, dx) order, normalisation by H_s / W_s, heat map peak) to code the
    project already tests.  20 rectangles per image, centres >= 17 apart in the Chebyshev sense.  The
    scene is checked on the CPU first, with the NumPy reference and oracle.postprocessing_oracle."""
    from emsanet_amd.postprocessing import instance_assign, instance_centers
    from oracle import postprocessing_oracle as O
    sem, inst = R.rectangles_scene(2, 96, 128, 20, seed=11)
    ref = R.reference_targets(sem, inst, R.IS_THING, scales=(1,))
    for per_image in ref['centers'][0]:
        pts = np.array(list(per_image.values()))
        d = np.abs(pts[:, None] - pts[None]).max(-1)
        assert len(pts) == 20 and d[~np.eye(20, dtype=bool)].min() > 8
    r0 = ref['instance'][0]
    cpu_centers = O.instance_centers(torch.from_numpy(r0['center']), 0.1, 17, 64)
    cpu_ids = O.instance_assign(torch.from_numpy(r0['offset']), cpu_centers,
                                torch.from_numpy(r0['foreground'])).numpy()
    for i in range(2):
        assert len(cpu_centers[i][0]) == 20 and _partition_equal(cpu_ids[i], inst[i])

    gen = _gen(_args(tasks=('semantic', 'instance')), scales=(1,))
    t = gen.generate(_batch(sem, inst))['instance'][0]
    centers, _scores, n_centers = instance_centers(t['center'], threshold=0.1, nms_kernel_size=17, top_k=64)
    ids = instance_assign(t['offset'], centers, n_centers, t['foreground'], normalized_offset=True)
    assert n_centers.tolist() == [20, 20]
    ids = ids.cpu().numpy()
    for i in range(2):
        assert _partition_equal(ids[i], inst[i])
        assert not ids[i][inst[i] == 0].any()


@pytest.mark.parametrize('what', ['id', 'label'])
def test_error_flag(edge, what):
    """an id >= max_instances or a label outside the table: check() raises, the flagged pixels carry no
    instance and do not disturb the others; after clean batches check() returns"""
    sem, inst, ori, scene, ref = edge
    sem, inst = sem.copy(), inst.copy()
    if what == 'id':
        inst[1, 20:24, 60:64] = 256              # on the stuff background, beside the instances
        inst[1, 15, 15] = 300                    # inside instance 255: that pixel drops out of it
    else:
        sem[1, 20:24, 60:64] = len(R.IS_THING)
        sem[1, 15, 15] = 77
    bad = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene, max_instances=256)
    assert bad['bad_id'] == (what == 'id') and bad['bad_label'] == (what == 'label')
    assert set(bad['centers'][0][1]) == set(ref['centers'][0][1])
    gen = _gen()
    gen.check()
    got = gen.generate(_batch(sem, inst, ori, scene, dt_inst=torch.int32))
    guard.check()
    assert_targets(got, bad, centers=gen.last_centers())
    with pytest.raises(ValueError, match='instance id' if what == 'id' else 'semantic label'):
        gen.check()
    gen.check()                                  # reported once
    clean = gen.generate(_batch(*edge[:4]))
    gen.generate(_batch(*edge[:4]))
    gen.check()
    assert_targets(clean, ref)


def test_negative_labels_are_flagged(edge):
    sem, inst, ori, scene, _ = edge
    sem, inst = sem.copy(), inst.copy()
    inst[2, 0, 0] = -1
    sem[2, 95, 127] = -3
    bad = R.reference_targets(sem, inst, R.IS_THING, R.USE_ORIENTATION, ori, scene)
    gen = _gen()
    assert_targets(gen.generate(_batch(sem, inst, ori, scene, torch.int32, torch.int16)), bad)
    with pytest.raises(ValueError, match='instance id.*and.*semantic label'):
        gen.check()


def test_generate_captures_into_a_graph(edge):
    """after one warm-up call generate() is captured; the input buffers are overwritten with a second
    scene and the replay gives that scene's targets"""
    sem, inst, ori, scene, ref = edge
    sem2 = np.ascontiguousarray(sem[::-1, :, ::-1])          # images reversed, mirrored
    inst2 = np.ascontiguousarray(inst[::-1, :, ::-1])
    ori2, scene2 = np.ascontiguousarray(ori[::-1]), np.ascontiguousarray(scene[::-1])
    ref2 = R.reference_targets(sem2, inst2, R.IS_THING, R.USE_ORIENTATION, ori2, scene2)
    gen = _gen()
    batch = _batch(sem, inst, ori, scene, torch.uint8, torch.int32)
    assert_targets(gen.generate(batch), ref)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            got = gen.generate(batch)
    torch.cuda.current_stream().wait_stream(stream)
    for key, new in (('semantic', sem2), ('instance', inst2), ('orientations', ori2), ('scene', scene2)):
        batch[key].copy_(_dev(new).to(batch[key].dtype))
    graph.replay()
    torch.cuda.synchronize()
    guard.check()                                    # (every buffer was made by the warm-up call, before the capture)
    assert_targets(got, ref2, centers=gen.last_centers())
    batch['semantic'].copy_(_dev(sem).to(torch.uint8))
    batch['instance'].copy_(_dev(inst).to(torch.int32))
    batch['orientations'].copy_(_dev(ori))
    batch['scene'].copy_(_dev(scene))
    graph.replay()
    torch.cuda.synchronize()
    assert_targets(got, ref)
    gen.check()


def _ref_to_device(ref):
    return {'semantic': [_dev(t) for t in ref['semantic']],
            'instance': [{k: _dev(v) for k, v in d.items()} for d in ref['instance']],
            'scene': _dev(ref['scene'])}


def test_training_step_losses_equal_the_reference_targets():
    """96x128, bs 2, all tasks, fp32: TrainingLosses on the generated targets == on the NumPy reference's
    targets moved to the device, 1e-6 relative per loss (the tolerance of tests/test_loss_gpu.py for these
    kernels); the offsets arrive in the layout the loss kernel reads"""
    from emsanet_amd import nyuv2_config
    from emsanet_amd.loss import TrainingLosses
    from emsanet_amd.model import EMSANet
    from oracle.emsanet_oracle import synthetic_batch
    args = _args(input_height=96, input_width=128)
    args.tasks_weighting = (1.0, 0.25, 3.0, 0.5)
    torch.manual_seed(0)
    model = EMSANet(args, nyuv2_config()).to(DEV).train()
    g = torch.Generator(device='cpu').manual_seed(99)
    crit = TrainingLosses(args, torch.rand(40, generator=g) * 2 + 0.3, 10).to(DEV)
    # 40 classes + void; every third class is stuff, every second thing class has orientations
    is_thing = (False,) + tuple(bool(i % 3) for i in range(40))
    use_o = tuple(t and i % 2 == 0 for i, t in enumerate(is_thing))
    esem, einst, eori, _ = R.edge_scene()
    sem = np.array([0, 6, 5, 7, 8, 9])[esem[1:]]                # 7 is stuff; 6 and 8 use orientations
    assert not is_thing[7] and all(is_thing[c] for c in (5, 6, 8, 9)) and use_o[6] and use_o[8] and not use_o[5]
    inst, ori, scene = einst[1:], eori[1:], np.array([3, 0], np.int64)
    ref = R.reference_targets(sem, inst, is_thing, use_o, ori, scene)
    assert all(d['foreground'].any() for d in ref['instance'][1:]) and ref['instance'][0]['orientation_foreground'].any()
    from emsanet_amd import TrainingTargetGenerator
    gen = TrainingTargetGenerator(args, is_thing, use_o)
    targets = gen.generate(_batch(sem, inst, ori, scene, torch.uint8, torch.uint16))
    gen.check()
    for d in targets['instance']:
        assert d['offset'].permute(0, 2, 3, 1).is_contiguous()
    batch = {k: v.to(DEV) for k, v in synthetic_batch(2, 96, 128).items()}
    model.dropout_step = 0
    with torch.no_grad():
        out = model(batch)
        t_dev, l_dev = crit(out, targets)
        t_ref, l_ref = crit(out, _ref_to_device(ref))
    assert sorted(l_dev) == sorted(l_ref) == ['instance_center', 'instance_offset', 'instance_orientation',
                                              'scene', 'semantic']
    for k in l_ref:
        a, b = float(l_dev[k]), float(l_ref[k])
        print(f"{k}: device targets {a!r}, reference targets {b!r}")
        assert b > 0 and abs(a - b) <= 1e-6 * abs(b), k
    assert abs(float(t_dev) - float(t_ref)) <= 1e-6 * abs(float(t_ref))


def test_batch_stager_hands_out_targets(edge):
    """three pinned batches of raw label maps in: 'targets' equals the reference for each; without the
    argument the handed-out dictionaries have the keys they have today"""
    from emsanet_amd import orientation_table
    from emsanet_amd.staging import BatchStager, pinned_raw_batch
    sem, inst, ori, scene, ref = edge
    scenes = [(sem, inst, ori, scene), (sem[::-1], inst[::-1], ori[::-1], scene[::-1]),
              (np.roll(sem, 1, 0), np.roll(inst, 1, 0), np.roll(ori, 1, 0), np.roll(scene, 1, 0))]
    refs = [ref] + [R.reference_targets(s, i, R.IS_THING, R.USE_ORIENTATION, o, c) for s, i, o, c in scenes[1:]]

    def host_batches():
        for j, (s, i, o, c) in enumerate(scenes):
            b = pinned_raw_batch(3, 96, 128, seed=j)
            b['semantic'] = torch.from_numpy(s.astype(np.uint8)).pin_memory()
            b['instance'] = torch.from_numpy(i.astype(np.int16)).pin_memory()
            b['orientations'] = orientation_table(
                [{k: float(v) for k, v in enumerate(row) if not np.isnan(v)} for row in o], 256)
            b['scene'] = torch.from_numpy(np.ascontiguousarray(c)).pin_memory()
            b['name'] = f'batch{j}'
            yield b

    plain = list(BatchStager(host_batches(), DEV))
    gen = _gen(ring=3)                            # the test keeps all three batches
    staged = list(BatchStager(host_batches(), DEV, target_generator=gen))
    torch.cuda.synchronize()
    gen.check()
    guard.check()                                 # the stager's device buffers and the three ring slots
    assert len(staged) == len(plain) == 3
    for b, p, want in zip(staged, plain, refs):
        assert sorted(p) == ['depth', 'instance', 'name', 'orientations', 'rgb', 'scene', 'semantic']
        assert sorted(b) == sorted(list(p) + ['targets'])
        assert_targets(b['targets'], want)
        assert torch.equal(b['rgb'], p['rgb']) and torch.equal(b['semantic'], p['semantic'])


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
