"""NumPy restatement of the inference output formats (emsanet_amd/export.py, csrc/export.hip), written
from the rules of /root/reference/inference_dataset.py:139-552 as the issue states them -- one function
per job kind, plain array operations, no device.  tests/test_export.py checks it against hand-computed
images; tests/test_export_gpu.py checks the device against it, bit for bit."""
import numpy as np

SCORE_MAX = np.float32(0.999)
CAUSE_LUT, CAUSE_CLASS, CAUSE_INSTANCE, CAUSE_WRAP = range(4)


def new_counters():
    return np.zeros(4, np.int64)


def nearest_index(out, size):
    """source index of every output index: floor(dst * in / out) in float32, clamped ('nearest' of
    torch.nn.functional.interpolate, the rule of emsa_nearest_fwd_t)"""
    scale = np.float32(size) / np.float32(out)
    i = np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(i, size - 1)


def resample(a, hw):
    """(N, h, w) -> (N, H, W), nearest neighbour"""
    a = np.asarray(a)
    if tuple(a.shape[1:]) == tuple(hw):
        return a
    return a[:, nearest_index(hw[0], a.shape[1])][:, :, nearest_index(hw[1], a.shape[2])]


def depth_mask(depth, max_depth):
    """depth > max_depth as NumPy compares an array with a Python float: a uint16 array exactly, a
    float32 array in float32"""
    if depth is None:
        return None
    depth = np.asarray(depth)
    if depth.dtype == np.float32:
        return depth > np.float32(max_depth)
    return depth.astype(np.float64) > float(max_depth)


def map_class(v, lut, lut_size, counters):
    """lut[v] (lut None: the identity on [0, lut_size); lut_size 0: no table, no bound); a value outside
    is counted and becomes 0"""
    v = np.asarray(v).astype(np.int64)
    if lut is None and lut_size == 0:
        return v
    size = len(lut) if lut is not None else lut_size
    bad = (v < 0) | (v >= size)
    counters[CAUSE_LUT] += int(bad.sum())
    v = np.where(bad, 0, v)
    out = np.asarray(lut).astype(np.int64)[v] if lut is not None else v
    return np.where(bad, 0, out)


def label_u8(label, hw, counters, lut=None, lut_size=256, add=0, depth=None, max_depth=None):
    c = map_class(resample(label, hw).astype(np.int64) + add, lut, lut_size, counters)
    m = depth_mask(depth, max_depth)
    if m is not None:
        c = np.where(m, 0, c)
    return c.astype(np.uint8)


def bgr(sem, inst, counters):
    """B = inst & 0xFF, G = inst >> 8, R = sem; what does not fit is counted, the low bits are kept"""
    counters[CAUSE_CLASS] += int(((sem < 0) | (sem > 255)).sum())
    counters[CAUSE_INSTANCE] += int(((inst < 0) | (inst > 65535)).sum())
    return np.stack([inst & 0xFF, (inst >> 8) & 0xFF, sem & 0xFF], axis=-1).astype(np.uint8)


def panoptic_bgr(sem, inst, hw, counters, lut=None, lut_size=0, divisor=0, depth=None, max_depth=None):
    """sources (semantic, instance), or with divisor > 0 (panoptic id, None)"""
    sem = resample(sem, hw).astype(np.int64)
    if divisor > 0:
        neg = sem < 0
        counters[CAUSE_LUT] += int(neg.sum())
        sem = np.where(neg, 0, sem)
        sem, inst = sem // divisor, sem % divisor
    else:
        inst = resample(inst, hw).astype(np.int64)
    sem = map_class(sem, lut, lut_size, counters)
    m = depth_mask(depth, max_depth)
    if m is not None:
        sem, inst = np.where(m, 0, sem), np.where(m, 0, inst)
    return bgr(sem, inst, counters)


def sem_inst_u16(sem, inst, hw, counters, lut=None, lut_size=256, add=0, depth=None, max_depth=None):
    sem = map_class(resample(sem, hw).astype(np.int64) + add, lut, lut_size, counters)
    inst = resample(inst, hw).astype(np.int64)
    m = depth_mask(depth, max_depth)
    if m is not None:
        sem, inst = np.where(m, 0, sem), np.where(m, 0, inst)
    full = sem * 1000 + inst
    counters[CAUSE_WRAP] += int(((full < 0) | (full > 65535)).sum())
    return (full & 0xFFFF).astype(np.uint16)


def class_score_f32(label, score, hw, counters, lut=None, lut_size=256, add=0):
    """float32(class) + clip(score, 0, 0.999): one float32 add; lut_size 0: float32(label + add)"""
    c = map_class(resample(label, hw).astype(np.int64) + add, lut, lut_size, counters)
    s = np.clip(resample(score, hw).astype(np.float32), np.float32(0), SCORE_MAX)
    return (c.astype(np.float32) + s).astype(np.float32)


# ---- scannet-instance prediction ------------------------------------------------------------------
def instance_ranks(area):
    """area (N, slots) -> rank (N, slots) int32 (-1 absent; id 0 never ranked), count (N,), start (N + 1,)"""
    area = np.asarray(area)
    rank = np.full(area.shape, -1, np.int32)
    count = np.zeros(area.shape[0], np.int32)
    for i in range(area.shape[0]):
        for j in range(1, area.shape[1]):
            if area[i, j] > 0:
                rank[i, j] = count[i]
                count[i] += 1
    return rank, count, np.concatenate([[0], np.cumsum(count)]).astype(np.int32)


def instance_masks(inst, rank, count, start, hw):
    """stack (total, H, W) uint8: plane start[i] + r = 255 where the map carries the id of rank r"""
    inst = resample(inst, hw).astype(np.int64)
    stack = np.zeros((int(start[-1]),) + tuple(hw), np.uint8)
    for i in range(inst.shape[0]):
        for j in range(rank.shape[1]):
            if rank[i, j] >= 0:
                stack[start[i] + rank[i, j]] = (inst[i] == j) * 255
    return stack


def instance_lines(meta, basename, mapping=None):
    """the text lines of one sample from its meta dictionary {id: {'area', 'semantic_idx',
    'panoptic_score', ...}}: ascending ids, instances without pixels skipped"""
    lines = []
    for j in sorted(meta):
        if meta[j]['area'] == 0:
            continue
        c = meta[j]['semantic_idx']
        c = int(c if mapping is None else mapping[c])
        lines.append(f"predicted_masks/{basename}_{len(lines):03d}.png {c} {meta[j]['panoptic_score']:0.4f}\n")
    return lines


# ---- the packer -----------------------------------------------------------------------------------
def _full(d, key):
    return d[key + '_fullres'] if key + '_fullres' in d else d[key]


def pack_reference(prediction, batch, formats, divisor, mapping=None, shift=1000, max_depth=None,
                   write_ground_truth=False, instance_use_panoptic_score=True):
    """every key of InferenceOutputPacker.pack from host arrays -> (dict, counters)"""
    c = new_counters()
    out = {}
    hw = tuple(_full(prediction, 'semantic_segmentation_idx').shape[1:])
    pan_sem = 'panoptic_segmentation_deeplab_semantic_idx'
    pan_inst = 'panoptic_segmentation_deeplab_instance_idx'
    depth = batch['_no_preprocessing']['depth'] if (max_depth is not None and write_ground_truth) else None
    dm = dict(depth=depth, max_depth=max_depth)
    has = lambda k: batch is not None and (k in batch or k + '_fullres' in batch)   # noqa: E731
    if 'scannet-semantic' in formats:
        out['scannet_semantic/pred_path_semantic'] = label_u8(_full(prediction, 'semantic_segmentation_idx'), hw,
                                                             c, mapping, add=1)
        if pan_sem in prediction or pan_sem + '_fullres' in prediction:
            out['scannet_semantic/pred_path_panoptic_semantic'] = label_u8(_full(prediction, pan_sem), hw, c,
                                                                          mapping)
        if write_ground_truth and has('semantic'):
            g = _full(batch, 'semantic')
            out['scannet_semantic/gt_path'] = label_u8(g, g.shape[1:], c, mapping, **dm)
    if 'scannet-panoptic' in formats:
        out['scannet_panoptic/pred_path'] = panoptic_bgr(_full(prediction, pan_sem), _full(prediction, pan_inst),
                                                         hw, c, mapping)
        if write_ground_truth and has('panoptic'):
            g = _full(batch, 'panoptic')
            out['scannet_panoptic/gt_path'] = panoptic_bgr(g, None, g.shape[1:], c, mapping, divisor=divisor, **dm)
    if 'scannet-instance' in formats and write_ground_truth and has('semantic') and has('instance'):
        s, i = _full(batch, 'semantic'), _full(batch, 'instance')
        out['scannet_instance/gt_path'] = sem_inst_u16(s, i, s.shape[1:], c, mapping, **dm) if shift == 1000 \
            else panoptic_bgr(s, i, s.shape[1:], c, mapping, **dm)
    if 'mapping' in formats:
        score = 'panoptic_segmentation_deeplab_' + ('panoptic_score' if instance_use_panoptic_score
                                                    else 'instance_score')
        out['mapping/pred_semantic'] = class_score_f32(
            _full(prediction, 'semantic_segmentation_idx'), _full(prediction, 'semantic_segmentation_score'), hw, c,
            mapping, add=1)[:, None]
        out['mapping/pred_panoptic_semantic'] = class_score_f32(
            _full(prediction, pan_sem), _full(prediction, 'panoptic_segmentation_deeplab_semantic_score'), hw, c,
            mapping)[:, None]
        out['mapping/pred_panoptic_instance'] = class_score_f32(
            _full(prediction, pan_inst), _full(prediction, score), hw, c, lut_size=0)
        n = prediction['scene_class_idx'].shape[0]
        out['mapping/pred_scene'] = class_score_f32(
            prediction['scene_class_idx'].reshape(1, 1, n), prediction['scene_class_score'].reshape(1, 1, n),
            (1, n), c, lut_size=0).reshape(n)
    return out, c
