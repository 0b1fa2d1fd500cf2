"""CPU: the NumPy restatement of the inference output formats (tests/export_reference.py) against images a
few pixels large computed by hand from /root/reference/inference_dataset.py:139-552, the host-side
refusals of emsanet_amd/export.py and the `mapping` file tree.  No GPU, no kernel."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_reference as X   # noqa: E402


def _maps(*rows, dtype=np.int64):
    return np.array(rows, dtype)[None]                                   # (1, 1, w)


def test_bgr_bytes_of_instance_0x1234_with_class_7():
    c = X.new_counters()
    out = X.panoptic_bgr(_maps([7, 0]), _maps([0x1234, 0]), (1, 2), c)
    assert out.dtype == np.uint8 and out.shape == (1, 1, 2, 3)
    assert out[0, 0, 0].tolist() == [0x34, 0x12, 7] and out[0, 0, 1].tolist() == [0, 0, 0]
    assert not c.any()
    # the same pixel from the merged panoptic id (id // divisor, id % divisor), both divisors in use
    for div in (1000, 1 << 16):
        assert X.panoptic_bgr(_maps([7 * div + 0x234]), None, (1, 1), c, divisor=div)[0, 0, 0].tolist() == \
            [0x34, 0x02, 7]
    assert not c.any()


def test_bgr_counts_what_three_channels_cannot_hold():
    c = X.new_counters()
    out = X.panoptic_bgr(_maps([256, 3, 3]), _maps([1, 65536, 65535]), (1, 3), c)
    assert c.tolist() == [0, 1, 1, 0]
    assert out[0, 0, 2].tolist() == [0xFF, 0xFF, 3]
    c = X.new_counters()
    X.panoptic_bgr(_maps([-5]), None, (1, 1), c, divisor=1000)           # a negative panoptic id
    assert c.tolist() == [1, 0, 0, 0]


def test_39_plus_1_through_a_mapping_table():
    table = np.arange(41, dtype=np.uint8)
    table[40] = 39                                                       # the benchmark id of class 40
    c = X.new_counters()
    out = X.label_u8(_maps([39, 0, 40]), (1, 3), c, lut=table, add=1)
    assert out.dtype == np.uint8 and out[0, 0].tolist() == [39, 1, 0]    # 40 + 1 lies outside the table
    assert c.tolist() == [1, 0, 0, 0]
    c = X.new_counters()
    assert X.label_u8(_maps([39, 255]), (1, 2), c, add=0)[0, 0].tolist() == [39, 255] and not c.any()
    assert X.label_u8(_maps([255]), (1, 1), c, add=1)[0, 0].tolist() == [0] and c[0] == 1


def test_65_times_1000_plus_537_wraps_and_is_counted():
    c = X.new_counters()
    out = X.sem_inst_u16(_maps([65, 65, 2]), _maps([537, 535, 7]), (1, 3), c)
    assert out.dtype == np.uint16
    want = (np.array([65], np.uint16) * 1000 + np.array([537], np.uint16))[0]      # the reference's arithmetic
    assert out[0, 0].tolist() == [1, 65535, 2007] and int(want) == 1
    assert c.tolist() == [0, 0, 0, 1]


def test_score_one_is_clamped_so_that_the_class_survives_the_cast():
    c = X.new_counters()
    score = np.array([[[1.0, -0.25, 0.5, 0.9995]]], np.float32)
    out = X.class_score_f32(_maps([12, 12, 0, 39]), score, (1, 4), c, add=1)
    assert out.dtype == np.float32
    want = np.array([13, 13, 1, 40], np.float32) + np.array([0.999, 0.0, 0.5, 0.999], np.float32)
    assert np.array_equal(out[0, 0], want)
    assert out.astype(np.uint8)[0, 0].tolist() == [13, 13, 1, 40]        # inference_dataset.py:477
    ids = X.class_score_f32(_maps([300]), np.array([[[2.0]]], np.float32), (1, 1), c, lut_size=0)
    assert ids[0, 0, 0] == np.float32(300) + np.float32(0.999) and not c.any()
    assert np.isnan(X.class_score_f32(_maps([1]), np.array([[[np.nan]]], np.float32), (1, 1), c)[0, 0, 0])


def test_fractional_max_depth_against_depths_below_equal_and_above():
    sem, inst = _maps([5, 5, 5, 5]), _maps([9, 9, 9, 9])
    c = X.new_counters()
    for dtype in (np.uint16, np.float32):
        depth = np.array([[[2499, 2500, 2501, 65535]]]).astype(dtype)
        assert X.depth_mask(depth, 2500.5)[0, 0].tolist() == [False, False, True, True]
        assert X.depth_mask(depth, 2500.0)[0, 0].tolist() == [False, False, True, True]
        assert X.depth_mask(depth, 2499.5)[0, 0].tolist() == [False, True, True, True]
        assert X.label_u8(sem, (1, 4), c, depth=depth, max_depth=2499.5)[0, 0].tolist() == [5, 0, 0, 0]
        assert X.sem_inst_u16(sem, inst, (1, 4), c, depth=depth, max_depth=2500.5)[0, 0].tolist() == \
            [5009, 5009, 0, 0]
        assert X.panoptic_bgr(sem, inst, (1, 4), c, depth=depth, max_depth=2500.5)[0, 0].tolist() == \
            [[9, 0, 5], [9, 0, 5], [0, 0, 0], [0, 0, 0]]
    # a threshold that float32 rounds onto an integer: the uint16 map compares exactly, as NumPy does
    d16 = np.array([[[2500]]], np.uint16)
    assert X.depth_mask(d16, 2499.99999999)[0, 0, 0] and bool((d16 > 2499.99999999)[0, 0, 0])
    d32 = d16.astype(np.float32)
    assert not X.depth_mask(d32, 2499.99999999)[0, 0, 0] and not bool((d32 > np.float32(2499.99999999))[0, 0, 0])
    assert not c.any()


def test_nearest_rule_and_resampling():
    assert X.nearest_index(4, 2).tolist() == [0, 0, 1, 1]
    assert X.nearest_index(3, 6).tolist() == [0, 2, 4]
    assert X.nearest_index(23, 10).tolist() == \
        torch.nn.functional.interpolate(torch.arange(10.)[None, None], size=23, mode='nearest')[0, 0].long().tolist()
    a = np.arange(6 * 10).reshape(1, 6, 10)
    want = torch.nn.functional.interpolate(torch.from_numpy(a).float()[None], size=(15, 23), mode='nearest')[0]
    assert np.array_equal(X.resample(a, (15, 23)), want.numpy().astype(np.int64))
    assert X.resample(a, (6, 10)) is a


def test_rank_order_with_an_empty_instance_in_the_middle():
    area = np.array([[50, 4, 0, 7, 0, 0, 0, 0, 2], [9, 0, 0, 0, 0, 0, 0, 0, 0]])   # slot 0 = no instance
    rank, count, start = X.instance_ranks(area)
    assert rank.tolist() == [[-1, 0, -1, 1, -1, -1, -1, -1, 2], [-1] * 9]
    assert count.tolist() == [3, 0] and start.tolist() == [0, 3, 3]
    inst = np.array([[[0, 1, 3], [8, 8, 2]], [[0, 0, 0], [0, 0, 0]]])
    stack = X.instance_masks(inst, rank, count, start, (2, 3))
    assert stack.shape == (3, 2, 3) and stack.dtype == np.uint8
    assert stack.tolist() == [[[0, 255, 0], [0, 0, 0]], [[0, 0, 255], [0, 0, 0]], [[0, 0, 0], [255, 255, 0]]]


def test_the_text_line():
    meta = {1: {'area': 4, 'semantic_idx': 5, 'panoptic_score': 0.72344},
            2: {'area': 0},
            3: {'area': 7, 'semantic_idx': 33, 'panoptic_score': 0.90381}}
    lines = X.instance_lines(meta, 'scene0707_00_000000')
    assert lines == ['predicted_masks/scene0707_00_000000_000.png 5 0.7234\n',
                     'predicted_masks/scene0707_00_000000_001.png 33 0.9038\n']
    table = np.arange(41, dtype=np.uint8)[::-1].copy()
    assert X.instance_lines(meta, 'a', table)[1] == 'predicted_masks/a_001.png 7 0.9038\n'
    from emsanet_amd.export import instance_entries, instance_line
    assert [instance_line('a', r, c, s) for r, (_, c, s) in enumerate(instance_entries(meta, table))] == \
        X.instance_lines(meta, 'a', table)
    assert X.instance_lines({}, 'a') == []


# ---- host-side refusals ---------------------------------------------------------------------------
def test_constructor_refusals():
    from emsanet_amd import InferenceOutputPacker as P
    with pytest.raises(ValueError, match="unknown output format 'scannet-depth'"):
        P(formats=('scannet-semantic', 'scannet-depth'))
    for shift in (999, 1 << 15, 0):
        with pytest.raises(ValueError, match='shift'):
            P(shift=shift)
    P(shift=1 << 16)
    with pytest.raises(TypeError, match='uint8'):
        P(semantic_class_mapping=np.arange(41))
    with pytest.raises(TypeError, match='uint8'):
        P(semantic_class_mapping=torch.arange(41))
    with pytest.raises(ValueError, match='40 entries, the label list with void has 41'):
        P(semantic_class_mapping=np.arange(40, dtype=np.uint8), n_semantic_classes=41)
    P(semantic_class_mapping=np.arange(41, dtype=np.uint8), n_semantic_classes=41)


def _cpu_prediction(n=2, h=4, w=6):
    z = torch.zeros(n, h, w)
    return {'semantic_segmentation_idx': z.long(), 'semantic_segmentation_score': z,
            'panoptic_segmentation_deeplab_semantic_idx': z.long(),
            'panoptic_segmentation_deeplab_instance_idx': z.int(),
            'panoptic_segmentation_deeplab_semantic_score': z, 'panoptic_segmentation_deeplab_panoptic_score': z,
            'panoptic_segmentation_deeplab_instance_score': z, 'scene_class_idx': torch.zeros(n).long(),
            'scene_class_score': torch.zeros(n), 'panoptic_segmentation_deeplab_instance_meta': [{}] * n}


def test_pack_refuses_cpu_tensors_and_missing_panoptic_keys():
    from emsanet_amd import InferenceOutputPacker as P
    p = _cpu_prediction()
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        P().pack(p, {})
    with pytest.raises(NotImplementedError, match='CPU tensor'):
        P(formats='scannet-instance').instance_outputs(p, {}, ['a', 'b'])
    for fmt in ('scannet-panoptic', 'scannet-instance', 'mapping'):
        for key in ('panoptic_segmentation_deeplab_semantic_idx', 'panoptic_segmentation_deeplab_instance_idx'):
            q = {k: v for k, v in p.items() if k not in (key, key + '_fullres')}
            with pytest.raises(KeyError, match=f"format '{fmt}' needs prediction\\['{key}'\\]"):
                P(formats=(fmt,)).pack(q, {})
    q = {k: v for k, v in p.items() if k != 'panoptic_segmentation_deeplab_instance_meta'}
    with pytest.raises(KeyError, match='instance_meta'):
        P().instance_outputs(q, {}, ['a', 'b'])


# ---- the mapping tree -----------------------------------------------------------------------------
@pytest.mark.parametrize('compressed', [True, False])
def test_write_mapping_output_round_trip(tmp_path, compressed):
    from emsanet_amd import write_mapping_output
    rng = np.random.RandomState(0)
    host = {'mapping/pred_semantic': rng.rand(2, 1, 3, 5).astype(np.float32) + 4,
            'mapping/pred_panoptic_semantic': torch.from_numpy(rng.rand(2, 1, 3, 5).astype(np.float32)),
            'mapping/pred_panoptic_instance': rng.rand(2, 3, 5).astype(np.float32),
            'mapping/pred_scene': np.array([3.25, 0.999], np.float32),
            'mapping/pred_panoptic_instance_meta': [
                {1: {'area': 3, 'center': [1.0, 2.0], 'score': 0.5, 'semantic_idx': 2, 'semantic_score': 0.25,
                     'panoptic_score': 0.125}, 2: {'area': 0, 'center': [0.0, 0.0], 'score': 0.75}}, {}],
            'scannet_semantic/pred_path_semantic': np.zeros((2, 3, 5), np.uint8)}
    idents = [('kitchen', 'cam0', '000012'), ('000013',)]
    table = np.array([0, 11, 22, 33], np.uint8)
    out = str(tmp_path / 'mapping')
    written = write_mapping_output(host, idents, out, compressed=compressed, semantic_class_mapping=table)
    assert len(written) == 10
    for key in ('pred_semantic', 'pred_panoptic_semantic', 'pred_panoptic_instance', 'pred_scene'):
        want = host['mapping/' + key]
        want = want.numpy() if torch.is_tensor(want) else want
        a = np.load(os.path.join(out, key, 'kitchen', 'cam0', '000012.npz'))['arr_0']
        b = np.load(os.path.join(out, key, '000013.npz'))['arr_0']
        assert a.dtype == np.float32 and np.array_equal(a, want[0]) and np.array_equal(b, want[1])
    assert np.load(os.path.join(out, 'pred_semantic', '000013.npz'))['arr_0'].shape == (1, 3, 5)
    assert not os.path.exists(os.path.join(out, 'pred_path_semantic'))
    with open(os.path.join(out, 'pred_panoptic_instance_meta', 'kitchen', 'cam0', '000012.json')) as f:
        meta = json.load(f)
    assert meta == {'1': {'area': 3, 'center': [1.0, 2.0], 'score': 0.5, 'semantic_idx': 22,
                          'semantic_score': 0.25, 'panoptic_score': 0.125},
                    '2': {'area': 0, 'center': [0.0, 0.0], 'score': 0.75}}
    with open(os.path.join(out, 'pred_panoptic_instance_meta', '000013.json')) as f:
        assert json.load(f) == {}
    assert host['mapping/pred_panoptic_instance_meta'][0][1]['semantic_idx'] == 2      # not modified in place
    with pytest.raises(ValueError, match='identifiers'):
        write_mapping_output(host, idents[:1], out)
