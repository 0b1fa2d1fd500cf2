"""Device-side packing of the inference outputs (emsanet_amd/export.py, csrc/export.hip) against the NumPy
restatement of tests/export_reference.py.  Every output is integer or ONE fp32 add of exactly
representable operands' images, so every comparison is exact equality (np.array_equal), the fp32
outputs included; the counters must agree as well.

Every test runs on the guarded arena of tests/guard.py, once per payload byte -- as
`test_x` on 0xFF and as its twin `test_x_poison00` on 0x00 -- (uint8 maps hold 255 and
the rank tables -1: what 0xFF reads as): the packer's ring buffers, the rank / count / start tables and
the mask stack -- sized by a count read back from the device -- lie between two bands of 0xFF, and the
source maps, tables and the destinations a test hands in are placed with `guard.put`.  The model whose
prediction three tests pack is built by a module fixture, before the arena is installed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_reference as X   # noqa: E402
import guard   # noqa: E402
from guard import guard_allocations  # noqa: E402,F401  (autouse: poisoned, guard-banded allocations)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_LABEL = {'int64': np.int64, 'int32': np.int32, 'uint8': np.uint8}


def _dev(a):
    return guard.put(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))    # flush between two bands of 0xFF


def _np(t):
    return t.detach().cpu().numpy()


def _table(size=41, mod=251):
    t = ((np.arange(size) * 7 + 3) % mod).astype(np.uint8)
    t[0] = 0
    return t


def _case(n, h, w, H, W, label, seed):
    """source maps (n, h, w) with a few values no format can hold, raw depth (n, H, W) in both types"""
    rng = np.random.RandomState(seed)
    small = label == 'uint8'
    sem = rng.randint(0, 41, (n, h, w))
    inst = rng.randint(0, 200 if small else 3000, (n, h, w))
    div = 16 if small else 1000
    pan = rng.randint(0, 15, (n, h, w)) * div + rng.randint(0, div, (n, h, w))
    sem[0, 0, 0] = 41                                                    # outside the table (also + 1)
    sem[-1, -1, -1] = 40                                                 # + 1 outside
    if not small:
        inst[0, 1, 1] = 70000
        sem[0, 2, 2], inst[0, 2, 2] = 40, 65535                          # 40 * 1000 + 65535 wraps
        pan[0, 0, 1] = 300 * div + 5                                     # class 300 in the BGR
    score = (rng.rand(n, h, w) * 1.2 - 0.1).astype(np.float32)
    score[0, 0, 0] = 1.0
    depth = rng.randint(2400, 2600, (n, H, W)).astype(np.uint16)
    depth[0, 0, :3] = (2499, 2500, 2501)
    depth[0, 1, 1] = depth[0, 2, 2] = 0                                  # (the pixels built for the counters stay)
    t = NP_LABEL[label]
    return sem.astype(t), inst.astype(t if small else np.int32), pan.astype(np.int64 if not small else t), \
        div, score, depth


def _run_all_kinds(n, h, w, H, W, label, seed, max_depth=2500.5):
    from emsanet_amd import export as E
    sem, inst, pan, div, score, depth = _case(n, h, w, H, W, label, seed)
    table = _table()
    lut = _dev(table)
    d16, d32 = _dev(depth), _dev(depth.astype(np.float32))
    counters = guard.put(torch.zeros(4, dtype=torch.int64, device=DEV))
    def new(dt, *tail):                                                  # pre-filled: every byte must be written
        shape = (n, H, W) + tail
        return guard.put(torch.full(shape[:-1] + (shape[-1] * dt.itemsize,), 77, dtype=torch.uint8,
                                    device=DEV)).view(dt)
    s, i, p, sc = _dev(sem), _dev(inst), _dev(pan), _dev(score)
    jobs = [E.PackJob(E.LABEL_U8, s, new(torch.uint8), lut=lut, lut_size=41, add=1),
            E.PackJob(E.LABEL_U8, s, new(torch.uint8), lut_size=41, depth=d16, max_depth=max_depth),
            E.PackJob(E.PANOPTIC_BGR, s, new(torch.uint8, 3), src1=i, lut=lut, lut_size=41, depth=d32,
                      max_depth=max_depth),
            E.PackJob(E.PANOPTIC_BGR, p, new(torch.uint8, 3), divisor=div, depth=d16, max_depth=max_depth),
            E.PackJob(E.SEM_INST_U16, s, new(torch.uint16), src1=i, lut_size=256, depth=d16, max_depth=2499.5),
            E.PackJob(E.SEM_INST_U16, s, new(torch.uint16), src1=i, lut=lut, lut_size=41, depth=d32,
                      max_depth=2499.99999999),
            E.PackJob(E.CLASS_SCORE_F32, s, new(torch.float32), src1=sc, lut=lut, lut_size=41, add=1),
            E.PackJob(E.CLASS_SCORE_F32, i, new(torch.float32), src1=sc)]
    E.export_pack(jobs, counters)
    c = X.new_counters()
    hw = (H, W)
    want = [X.label_u8(sem, hw, c, table, add=1),
            X.label_u8(sem, hw, c, None, 41, depth=depth, max_depth=max_depth),
            X.panoptic_bgr(sem, inst, hw, c, table, depth=depth.astype(np.float32), max_depth=max_depth),
            X.panoptic_bgr(pan, None, hw, c, divisor=div, depth=depth, max_depth=max_depth),
            X.sem_inst_u16(sem, inst, hw, c, None, 256, depth=depth, max_depth=2499.5),
            X.sem_inst_u16(sem, inst, hw, c, table, depth=depth.astype(np.float32), max_depth=2499.99999999),
            X.class_score_f32(sem, score, hw, c, table, add=1),
            X.class_score_f32(inst, score, hw, c, lut_size=0)]
    torch.cuda.synchronize()
    guard.check()
    for k, (j, ref) in enumerate(zip(jobs, want)):
        got = _np(j.dst)
        assert got.dtype == ref.dtype and got.shape == ref.shape, (k, got.dtype, got.shape, ref.shape)
        assert np.array_equal(got, ref), (k, int((got != ref).sum()))
    assert counters.cpu().tolist() == c.tolist(), (counters.cpu().tolist(), c.tolist())
    return c


@pytest.mark.parametrize('label', ['int64', 'int32', 'uint8'])
@pytest.mark.parametrize('h,w,H,W', [(6, 10, 15, 23), (16, 12, 8, 6), (15, 13, 15, 13), (9, 16, 9, 16),
                                     (7, 13, 14, 16)])
def test_every_kind_in_one_launch(h, w, H, W, label):
    """N = 2; widths 13 (the flat size is odd: scalar tail, groups across rows) and 16 (whole groups);
    a non-integer ratio up, a down-sampling, equal sizes (vector loads), every label type, depth as
    uint16 and as fp32 with fractional thresholds, values every counter fires on"""
    c = _run_all_kinds(2, h, w, H, W, label, seed=h * 100 + W)
    assert c[X.CAUSE_LUT] > 0
    if label != 'uint8' and (h, w) == (H, W):
        assert all(c > 0), c


def test_larger_maps_480x640():
    """the full grid (grid-stride loop, 32-bit pixel indices): 2 x 480 x 640, equal and half-size sources"""
    _run_all_kinds(2, 480, 640, 480, 640, 'int64', seed=1)
    _run_all_kinds(2, 240, 320, 480, 640, 'int32', seed=2)


def test_an_unaligned_source_view_takes_the_gather_path():
    from emsanet_amd import export as E
    rng = np.random.RandomState(3)
    flat = rng.randint(0, 40, 2 * 8 * 16 + 1).astype(np.uint8)
    src = _dev(flat)[1:].view(2, 8, 16)                                  # 1 byte off the allocation
    dst = guard.put(torch.full((2, 8, 16), 77, dtype=torch.uint8, device=DEV))
    counters = guard.put(torch.zeros(4, dtype=torch.int64, device=DEV))
    E.export_pack([E.PackJob(E.LABEL_U8, src, dst, lut_size=256, add=1)], counters)
    guard.check()
    assert np.array_equal(_np(dst), flat[1:].reshape(2, 8, 16) + 1) and not counters.any()


def test_packing_a_network_resolution_map_equals_packing_its_fullres_twin():
    from emsanet_amd import export as E
    from emsanet_amd.postprocessing import add_fullres_predictions
    rng = np.random.RandomState(4)
    n, h, w, H, W = 2, 24, 32, 61, 83
    r = {'panoptic_segmentation_deeplab_semantic_idx': _dev(rng.randint(0, 41, (n, h, w)).astype(np.int64)),
         'panoptic_segmentation_deeplab_instance_idx': _dev(rng.randint(0, 65, (n, h, w)).astype(np.int32)),
         'panoptic_segmentation_deeplab_panoptic_score': _dev(rng.rand(n, h, w).astype(np.float32))}
    add_fullres_predictions(r, (H, W))
    sem, inst, score = (r['panoptic_segmentation_deeplab_' + k] for k in
                        ('semantic_idx', 'instance_idx', 'panoptic_score'))
    SEM, INST, SCORE = (r['panoptic_segmentation_deeplab_' + k + '_fullres'] for k in
                        ('semantic_idx', 'instance_idx', 'panoptic_score'))
    assert SEM.shape == (n, H, W)
    counters = torch.zeros(4, dtype=torch.int64, device=DEV)
    outs = []
    for a, b, c in ((sem, inst, score), (SEM, INST, SCORE)):
        new = lambda dt, *tail: torch.empty((n, H, W) + tail, dtype=dt, device=DEV)   # noqa: E731
        jobs = [E.PackJob(E.LABEL_U8, a, new(torch.uint8), lut_size=256),
                E.PackJob(E.PANOPTIC_BGR, a, new(torch.uint8, 3), src1=b),
                E.PackJob(E.CLASS_SCORE_F32, b, new(torch.float32), src1=c)]
        E.export_pack(jobs, counters)
        outs.append([_np(j.dst) for j in jobs])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[0][0], X.resample(_np(sem), (H, W)))


# ---- scannet-instance: ranks and masks ------------------------------------------------------------
class _Meta(list):
    device_tables = None


@pytest.mark.parametrize('label', ['int64', 'int32', 'uint8'])
@pytest.mark.parametrize('h,w,H,W', [(15, 13, 15, 13), (8, 16, 8, 16), (6, 10, 15, 23), (16, 12, 8, 6)])
def test_instance_outputs_small(h, w, H, W, label):
    """top_k + 1 = 9 slots; sample 0 carries ids 0, 1, 8 and (in the table only) 5, id 3 has area 0;
    sample 1 has no instance: an empty slice of the stack and no line"""
    from emsanet_amd import InferenceOutputPacker
    rng = np.random.RandomState(h + W)
    inst = np.zeros((2, h, w), NP_LABEL[label])
    inst[0] = rng.choice([0, 1, 8], (h, w))
    inst[0, :2, :2] = (1, 8)
    inst[0, -1, -1] = 9                                                  # an id beyond the slots: no plane
    area = np.zeros((2, 9), np.int32)
    for j in (0, 1, 8):
        area[0, j] = (inst[0] == j).sum()
    area[0, 5] = 4                                                       # ranked, though no pixel shows it
    area[1, 0] = h * w
    cls = np.full((2, 9), -1, np.int32)
    cls[0, [1, 5, 8]] = (4, 39, 0)
    score = rng.rand(2, 9).astype(np.float32)
    table = _table()
    meta = _Meta([{j: {'area': int(area[i, j]), **({'semantic_idx': int(cls[i, j]) + 1,
                                                    'panoptic_score': float(score[i, j])} if area[i, j] else {})}
                   for j in range(1, 9)} for i in range(2)])
    pred = {'panoptic_segmentation_deeplab_instance_idx': _dev(inst),
            'panoptic_segmentation_deeplab_semantic_idx': _dev(inst),
            'panoptic_segmentation_deeplab_instance_meta': meta}
    rank, count, start = X.instance_ranks(area)
    assert rank[0].tolist() == [-1, 0, -1, -1, -1, 1, -1, -1, 2] and count.tolist() == [3, 0]
    want = X.instance_masks(inst, rank, count, start, (H, W))
    lines = [X.instance_lines(meta[i], b, table) for i, b in enumerate(('s_000', 's_001'))]
    packer = InferenceOutputPacker(formats='scannet-instance', semantic_class_mapping=table)
    for tables in (None, {'area': _dev(area), 'instance_class': _dev(cls), 'panoptic_score': _dev(score)}):
        meta.device_tables = tables                                     # host-built ranks, then the kernel
        out = packer.instance_outputs(pred, None, ['s_000', 's_001'], output_size=(H, W))
        masks, got_lines = out
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (3, H, W)
        assert np.array_equal(_np(masks), want)
        assert got_lines == lines and len(lines[0]) == 3 and lines[1] == []
        assert out.start == [0, 3, 3] and masks[out.start[1]:out.start[2]].shape[0] == 0
        guard.check()
    assert want[1].sum() == 0 and want[0].sum() > 0 and want[2].sum() > 0
    packer.check()
    # nobody owns a pixel: an empty stack
    meta.device_tables = {'area': _dev(area * 0), 'instance_class': _dev(cls), 'panoptic_score': _dev(score)}
    out = packer.instance_outputs(pred, None, ['a', 'b'])
    assert tuple(out.masks.shape) == (0, h, w) and out.lines == [[], []]
    guard.check()


@pytest.mark.parametrize('label', ['int32', 'uint8'])
@pytest.mark.parametrize('used', ['every_slot', 'one', 'none'])
def test_instance_ranks_table_ends_and_stack_totals(used, label):
    """9 slots, N = 3, 7 x 13 -> 7 x 13.  every_slot: all eight ids of every sample are ranked, the last
    rank of the last sample is the last entry of every table and the last plane of a 24-plane stack.
    one: a single instance in the last sample, id 8: a stack of exactly one plane behind two empty
    slices.  none: no slot used at all: a stack of 0 planes, and the mask kernel gets no pointer"""
    from emsanet_amd import InferenceOutputPacker
    n, h, w, slots = 3, 7, 13, 9
    rng = np.random.RandomState(len(used))
    inst = np.zeros((n, h, w), NP_LABEL[label])
    area = np.zeros((n, slots), np.int32)
    if used == 'every_slot':
        inst[:] = rng.randint(0, slots, (n, h, w))
        inst[:, 0, :slots] = np.arange(slots)                            # every id has a pixel
        inst[-1, -1, -1] = slots - 1
    elif used == 'one':
        inst[-1, -2:, -3:] = slots - 1
    for i in range(n):
        for j in range(1, slots):
            area[i, j] = (inst[i] == j).sum()
    cls = np.where(area > 0, rng.randint(0, 40, (n, slots)), -1).astype(np.int32)
    score = rng.rand(n, slots).astype(np.float32)
    table = _table()
    meta = _Meta([{j: {'area': int(area[i, j]), 'semantic_idx': int(cls[i, j]) + 1,
                       'panoptic_score': float(score[i, j])} for j in range(1, slots) if area[i, j]}
                  for i in range(n)])
    meta.device_tables = {'area': _dev(area), 'instance_class': _dev(cls), 'panoptic_score': _dev(score)}
    names = ['s_000', 's_001', 's_002']
    rank, count, start = X.instance_ranks(area)
    total = {'every_slot': n * (slots - 1), 'one': 1, 'none': 0}[used]
    assert int(start[-1]) == total and (used != 'every_slot' or (rank[:, 1:] >= 0).all())
    want = X.instance_masks(inst, rank, count, start, (h, w))
    lines = [X.instance_lines(meta[i], b, table) for i, b in enumerate(names)]
    pred = {'panoptic_segmentation_deeplab_instance_idx': _dev(inst),
            'panoptic_segmentation_deeplab_instance_meta': meta}
    packer = InferenceOutputPacker(formats='scannet-instance', semantic_class_mapping=table)
    out = packer.instance_outputs(pred, None, names)
    guard.check()
    assert out.masks.dtype == torch.uint8 and tuple(out.masks.shape) == (total, h, w)
    assert np.array_equal(_np(out.masks), want)
    assert out.lines == lines and out.start == start.tolist()
    if total:
        assert want[-1].any() and want[-1, -1, -1] == 255                # the last plane's last byte is set
    packer.check()


# ---- counters -------------------------------------------------------------------------------------
def test_each_counter_fires_and_check_names_the_cause():
    from emsanet_amd import InferenceOutputPacker
    from emsanet_amd import export as E
    n, h, w = 2, 5, 13
    z = lambda dt, v=0: torch.full((n, h, w), v, dtype=dt, device=DEV)   # noqa: E731
    base = {'semantic_segmentation_idx': z(torch.int64, 3), 'semantic_segmentation_score': z(torch.float32, 0.5),
            'panoptic_segmentation_deeplab_semantic_idx': z(torch.int64, 4),
            'panoptic_segmentation_deeplab_instance_idx': z(torch.int32, 2),
            'panoptic_segmentation_deeplab_semantic_score': z(torch.float32, 0.5),
            'panoptic_segmentation_deeplab_panoptic_score': z(torch.float32, 0.5),
            'scene_class_idx': torch.zeros(n, dtype=torch.int64, device=DEV),
            'scene_class_score': torch.zeros(n, device=DEV)}
    gt = {'semantic': z(torch.uint8, 7), 'instance': z(torch.int32, 9)}
    cases = [('outside the class mapping table', {'semantic_segmentation_idx': z(torch.int64, 40)}, {}, 1000,
              np.arange(41, dtype=np.uint8)),
             ('semantic class above 255', {'panoptic_segmentation_deeplab_semantic_idx': z(torch.int64, 256)}, {},
              1000, None),
             ('instance id above 65535', {'panoptic_segmentation_deeplab_instance_idx': z(torch.int32, 65536)}, {},
              1000, None),
             ('does not fit uint16', {}, {'semantic': z(torch.uint8, 65), 'instance': z(torch.int32, 537)}, 1000,
              None)]
    for cause, p, b, shift, mapping in cases:
        packer = InferenceOutputPacker(shift=shift, semantic_class_mapping=mapping, write_ground_truth=True)
        packer.pack(base, gt)
        packer.check()                                                   # nothing to report
        out = packer.pack({**base, **p}, {**gt, **b})
        with pytest.raises(ValueError, match=cause) as e:
            packer.check()
        others = [c for c in E.CAUSES if cause not in c]
        if cause != 'semantic class above 255':                          # (class 256 is also outside uint8 maps)
            assert not any(o in str(e.value) for o in others), str(e.value)
        packer.check()                                                   # counting starts afresh
        assert out['scannet_instance/gt_path'].dtype == torch.uint16
    # the wrap stores the reference's uint16 arithmetic
    assert int(out['scannet_instance/gt_path'][0, 0, 0]) == 1


# ---- the model's prediction -----------------------------------------------------------------------
_CACHE = {}


def _setup():
    """the tiny golden configuration the other GPU tests use (96 x 128, 4 images, all tasks, panoptic,
    deterministic weights), a batch with `rgb_fullres` at twice the size, blocky labels (image 0: the
    model's own panoptic prediction) and raw depth at that size, and the eval prediction -- built once,
    never modified"""
    if 'full' in _CACHE:
        return _CACHE['full']
    from util import deterministic_state_dict
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.model import EMSANet
    n, h, w = 4, 96, 128
    H, W = 2 * h, 2 * w
    cfg = nyuv2_config()
    labels = cfg.semantic_label_list_without_void
    labels.classes_is_thing = tuple(bool(i % 3) for i in range(len(labels)))
    model = EMSANet(full_args(input_height=h, input_width=w, enable_panoptic=True), cfg)
    model.load_state_dict(deterministic_state_dict(model))
    model.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    batch = {'rgb': torch.randn(n, 3, h, w, generator=g).to(DEV),
             'depth': torch.randn(n, 1, h, w, generator=g).to(DEV)}
    div = model.decoders['panoptic_helper'].postprocessing.max_instances_per_category
    with torch.no_grad():
        first = model(batch, do_postprocessing=True)
    sem = torch.randint(0, len(labels) + 1, (n, H // 16, W // 16), generator=g).repeat_interleave(16, 1) \
        .repeat_interleave(16, 2).to(torch.uint8).to(DEV)
    inst = torch.randint(0, 5, (n, H // 32, W // 32), generator=g).repeat_interleave(32, 1) \
        .repeat_interleave(32, 2).to(torch.int32).to(DEV)
    up = lambda t: t.repeat_interleave(2, -2).repeat_interleave(2, -1)   # noqa: E731
    sem[0] = up(first['panoptic_segmentation_deeplab_semantic_idx'][0]).to(torch.uint8)
    inst[0] = up(first['panoptic_segmentation_deeplab_instance_idx'][0])
    big = {'rgb': batch['rgb'], 'depth': batch['depth'],
           'rgb_fullres': torch.zeros(n, 3, H, W, device=DEV),
           'semantic_fullres': sem, 'instance_fullres': inst,
           'panoptic_fullres': sem.long() * div + inst.long(),
           '_no_preprocessing': {'depth': _dev(np.random.RandomState(9).randint(0, 5000, (n, H, W))
                                               .astype(np.uint16))}}
    with torch.no_grad():
        prediction = model({k: big[k] for k in ('rgb', 'depth', 'rgb_fullres')}, do_postprocessing=True)
    assert prediction['panoptic_segmentation_deeplab_instance_idx_fullres'].shape == (n, H, W)
    _CACHE['full'] = (model, big, prediction, div)
    return _CACHE['full']


@pytest.fixture(scope='module')
def full_setup():
    """`_setup()` ahead of the function-scoped guard fixture: the model and its eval forward pass (the
    whole model) run on the plain allocator, the packer under test on the arena"""
    return _setup()


def _host(d):
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            out[k] = _np(v)
        elif isinstance(v, dict):
            out[k] = _host(v)
    return out


@pytest.mark.usefixtures('full_setup')
@pytest.mark.parametrize('shift,mapped', [(1000, True), (1 << 16, False)])
def test_packer_end_to_end_on_the_model_prediction(shift, mapped):
    from emsanet_amd import InferenceOutputPacker
    from emsanet_amd import export as E
    model, batch, prediction, div = _setup()
    table = _table(mod=41) if mapped else None                           # ids <= 40: sem * 1000 + inst fits uint16
    kw = dict(shift=shift, max_depth=2500.5, write_ground_truth=True, instance_use_panoptic_score=mapped)
    packer = InferenceOutputPacker(E.FORMATS, div, table, n_semantic_classes=41, **kw)
    packed = packer.pack(prediction, batch)
    host = packer.to_host(packed)
    packer.check()
    got = host.synchronize()
    guard.check()
    want, c = X.pack_reference(_host(prediction), _host(batch), E.FORMATS, div, table, **kw)
    assert not c.any()
    assert set(want) == set(got) - {'mapping/pred_panoptic_instance_meta'} and len(want) == 10
    for k, ref in want.items():
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (k, got[k].shape, ref.shape)
        assert np.array_equal(got[k], ref), (k, int((got[k] != ref).sum()))
        assert np.array_equal(_np(packed[k]), ref), k
    n, H, W = prediction['semantic_segmentation_idx_fullres'].shape
    assert got['mapping/pred_semantic'].shape == (n, 1, H, W) and got['mapping/pred_scene'].shape == (n,)
    assert got['scannet_panoptic/pred_path'].shape == (n, H, W, 3)
    assert got['scannet_instance/gt_path'].dtype == (np.uint16 if shift == 1000 else np.uint8)
    assert (got['scannet_semantic/gt_path'] == 0).any() and got['scannet_panoptic/pred_path'][..., 0].any()
    assert all(v.is_pinned() for v in host.values() if torch.is_tensor(v))
    assert list(got['mapping/pred_panoptic_instance_meta']) == \
        list(prediction['panoptic_segmentation_deeplab_instance_meta'])

    # scannet-instance prediction: device ranks, and the same from the plain dictionaries
    names = [f'scene{i:04d}_00_{i:06d}' for i in range(n)]
    meta = list(prediction['panoptic_segmentation_deeplab_instance_meta'])
    area = np.zeros((n, max([2] + [max(m) + 1 for m in meta if m])), np.int64)
    for i, m in enumerate(meta):
        for j, e in m.items():
            area[i, j] = e['area']
    rank, count, start = X.instance_ranks(area)
    assert count.sum() >= 1
    inst = _np(prediction['panoptic_segmentation_deeplab_instance_idx_fullres'])
    masks = X.instance_masks(inst, rank, count, start, (H, W))
    lines = [X.instance_lines(m, b, table) for m, b in zip(meta, names)]
    for p in (prediction, {**prediction, 'panoptic_segmentation_deeplab_instance_meta': meta}):
        out = packer.instance_outputs(p, batch, names)
        assert np.array_equal(_np(out.masks), masks) and out.lines == lines and out.start == start.tolist()
        guard.check()
    packer.check()


@pytest.mark.usefixtures('full_setup')
def test_pack_replayed_from_a_graph_behind_the_eval_forward():
    """`GraphedInference(..., do_postprocessing=True, after=packer.pack)`: the replay's packed outputs are
    the eager ones on two inputs, in the same buffers every time; eager calls allocate nothing after the
    first turn of the ring"""
    from emsanet_amd import InferenceOutputPacker
    from emsanet_amd.graph import GraphedInference
    model, batch, _, div = _setup()
    b1 = {k: batch[k] for k in ('rgb', 'depth')}
    b2 = {k: v.roll(1, 0) for k, v in b1.items()}
    eager_packer = InferenceOutputPacker(max_instances_per_category=div, ring=2)
    eager, ptrs = [], []
    with torch.no_grad():
        preds = [model(b, do_postprocessing=True) for b in (b1, b2)]
    for turn in range(3):
        if turn == 1:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
        out = [eager_packer.pack(p, b) for p, b in zip(preds, (b1, b2))]     # ring turns 0, 1
        ptrs.append([{k: v.data_ptr() for k, v in o.items() if torch.is_tensor(v)} for o in out])
        eager = [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in out]
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                       # (the clones of a turn replace the last)
    assert ptrs[0] == ptrs[1] == ptrs[2]
    assert all(ptrs[0][0][k] != ptrs[0][1][k] for k in ptrs[0][0])       # two sets of buffers
    eager_packer.check()

    packer = InferenceOutputPacker(max_instances_per_category=div, ring=2)
    gi = GraphedInference(model, b1, do_postprocessing=True, after=packer.pack)
    static = {k: v for k, v in gi.static_after.items() if torch.is_tensor(v)}
    assert set(static) == set(eager[0]) and len(static) == 7
    where = {k: v.data_ptr() for k, v in static.items()}
    for b, ref in ((b2, eager[1]), (b1, eager[0]), (b2, eager[1])):
        gi(b)
        torch.cuda.synchronize()
        assert gi.static_after is not None and {k: v.data_ptr() for k, v in static.items()} == where
        for k, v in static.items():
            assert np.array_equal(_np(v), _np(ref[k])), k
    assert not np.array_equal(_np(eager[0]['scannet_panoptic/pred_path']), _np(eager[1]['scannet_panoptic/pred_path']))
    packer.check()


@pytest.mark.usefixtures('full_setup')
def test_to_host_copies_into_the_ring_set_the_outputs_came_from():
    from emsanet_amd import InferenceOutputPacker
    model, batch, prediction, div = _setup()
    packer = InferenceOutputPacker('scannet-panoptic', div, ring=2)
    p0 = packer.pack(prediction, batch)
    want0 = _np(p0['scannet_panoptic/pred_path'])
    flipped = dict(prediction)
    for k in ('panoptic_segmentation_deeplab_instance_idx', 'panoptic_segmentation_deeplab_instance_idx_fullres'):
        flipped[k] = prediction[k].flip(0)
    p1 = packer.pack(flipped, batch)
    assert (p0.turn, p1.turn) == (0, 1)
    h1 = packer.to_host(p1)
    h0 = packer.to_host(p0)                                              # after a later pack(): still set 0
    a0, a1 = h0.synchronize(), h1.synchronize()
    assert h0['scannet_panoptic/pred_path'].data_ptr() != h1['scannet_panoptic/pred_path'].data_ptr()
    assert np.array_equal(a0['scannet_panoptic/pred_path'], want0)
    assert np.array_equal(a1['scannet_panoptic/pred_path'], _np(p1['scannet_panoptic/pred_path']))
    assert not np.array_equal(a0['scannet_panoptic/pred_path'], a1['scannet_panoptic/pred_path'])
    packer.release()
    assert not packer._buf and not packer._pinned


def test_instance_outputs_refuses_malformed_device_tables():
    from emsanet_amd import InferenceOutputPacker
    inst = torch.zeros((2, 4, 8), dtype=torch.int32, device=DEV)
    good = {'area': torch.zeros((2, 9), dtype=torch.int32, device=DEV),
            'instance_class': torch.zeros((2, 9), dtype=torch.int32, device=DEV),
            'panoptic_score': torch.zeros((2, 9), device=DEV)}
    packer = InferenceOutputPacker('scannet-instance')
    for key, bad in (('area', good['area'].long()), ('instance_class', good['instance_class'][:, :5]),
                     ('panoptic_score', good['panoptic_score'].cpu()), ('area', good['area'][:1])):
        meta = _Meta([{}, {}])
        meta.device_tables = {**good, key: bad}
        with pytest.raises(TypeError, match=r"device_tables\['"):
            packer.instance_outputs({'panoptic_segmentation_deeplab_instance_idx': inst,
                                     'panoptic_segmentation_deeplab_instance_meta': meta}, None, ['a', 'b'])


# every test above once more as `<name>_poison00`, on 0x00 payloads (True, 255 and -1 are legal values)
guard.second_payload(globals())
