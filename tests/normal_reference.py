"""NumPy / plain-torch restatement of the surface-normal rules the engine states in emsanet_amd/loss.py,
targets.py, augment.py, postprocessing.py and metrics.py ([U]: the reference's task code lives in the
un-vendored nicr_mt_scene_analysis library).  Ground-truth maps here are (N, H, W, 3) float32 arrays,
channel 0 the image-x component; predictions (N, 3, H, W)."""
import numpy as np
import torch

from augment_reference import nearest_axis, source_coords

ANGLE_ONE = 1 << 20          # the engine adds round(angle * 2^20): at most 2^-21 = 4.8e-7 rad per pixel
UNIT_EPS = 1e-12
DEFAULT_SCALES = (1, 32, 16, 8)


def valid_mask(target):
    """(N, H, W) bool: the vector is not exactly (0, 0, 0) (-0.0 counts as 0)"""
    return (np.asarray(target) != 0).any(-1)


def to_hwc(target):
    """(N, 3, H, W) -> (N, H, W, 3)"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(target), 1, -1))


# ---- loss ------------------------------------------------------------------------------------------
def l1_loss(pred, target, grad_out=1.0):
    """pred (N, 3, H, W), target (N, H, W, 3) -> (loss, gradient of grad_out * loss), float64:
    loss = sum over valid pixels and channels of |p - t| / (3 n_valid), 0 without a valid pixel;
    gradient = grad_out * sign(p - t) / (3 n_valid) on valid pixels, 0 elsewhere"""
    p = np.moveaxis(np.asarray(pred, np.float64), 1, -1)
    t = np.asarray(target, np.float64)
    m = valid_mask(target)
    n_valid = int(m.sum())
    if n_valid == 0:
        return 0.0, np.zeros(np.asarray(pred).shape, np.float64)
    d = (p - t) * m[..., None]
    loss = np.abs(d).sum() / (3.0 * n_valid)
    grad = grad_out * np.sign(d) / (3.0 * n_valid)
    return float(loss), np.moveaxis(grad, -1, 1)


def l1_loss_autograd(pred, target, grad_out=1.0):
    """the same masked expression through torch autograd in fp64 (the check of `l1_loss`)"""
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.moveaxis(np.asarray(target, np.float64), -1, 1).copy())
    m = torch.from_numpy(valid_mask(target))[:, None].expand_as(p)
    if not bool(m.any()):
        return 0.0, np.zeros(p.shape, np.float64)
    loss = (p - t).abs()[m].sum() / m.sum()
    (grad_out * loss).backward()
    return float(loss.detach()), p.grad.numpy()


# ---- targets ---------------------------------------------------------------------------------------
def multiscale_targets(target, scales=DEFAULT_SCALES):
    """[(N, H/s, W/s, 3)]: the vector at (y, x) of scale s is the one at (y * s, x * s)"""
    return [np.ascontiguousarray(np.asarray(target)[:, ::s, ::s]) for s in scales]


# ---- augmentation ----------------------------------------------------------------------------------
def augment(target, table, h, w):
    """target (N, Hs, Ws, 3), table int32 (N, 8) rows (Hr, Wr, cy, cx, flip, ...) -> (N, h, w, 3): the
    composed index and the nearest rule of depth and the labels; channel 0 negated on a flipped row"""
    target = np.asarray(target)
    out = np.empty((target.shape[0], h, w, 3), target.dtype)
    for i, row in enumerate(np.asarray(table)):
        hr, wr, cy, cx, flip = (int(v) for v in row[:5])
        Y, X = source_coords(h, w, cy, cx, flip)
        yn = np.minimum(nearest_axis(Y, target.shape[1], hr), target.shape[1] - 1)
        xn = np.minimum(nearest_axis(X, target.shape[2], wr), target.shape[2] - 1)
        out[i] = target[i][yn][:, xn]
        if flip:
            out[i, ..., 0] = -out[i, ..., 0]
    return out


# ---- post-processing -------------------------------------------------------------------------------
def unit_vectors(pred):
    """torch.nn.functional.normalize(dim=1) on the CPU, on the fp32 values: v / max(|v|_2, 1e-12)"""
    return torch.nn.functional.normalize(torch.as_tensor(pred, dtype=torch.float32), dim=1,
                                         eps=UNIT_EPS).numpy()


# ---- metric ----------------------------------------------------------------------------------------
def nearest_source(n_out, n_in):
    """source index of every output coordinate: floor(o * (n_in / n_out)) in fp32, clamped -- the rule of
    torch.nn.functional.interpolate(mode='nearest')"""
    scale = np.float32(n_in) / np.float32(n_out)
    i = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(i, n_in - 1)


def angles(pred, target):
    """pred (N, 3, h, w), target (N, H, W, 3) -> the float64 angles atan2(|p x t|, p . t) of the valid
    target pixels (1-D); a smaller prediction is read with nearest neighbour"""
    p = np.moveaxis(np.asarray(pred, np.float64), 1, -1)
    t = np.asarray(target, np.float64)
    if p.shape[1:3] != t.shape[1:3]:
        p = p[:, nearest_source(t.shape[1], p.shape[1])][:, :, nearest_source(t.shape[2], p.shape[2])]
    m = valid_mask(target)
    p, t = p[m], t[m]
    return np.arctan2(np.linalg.norm(np.cross(p, t), axis=-1), (p * t).sum(-1))


def angular_error(pairs):
    """pairs: iterable of (pred, target) updates -> (mean angle in rad or NaN, number of valid pixels)"""
    total, count = 0.0, 0
    for pred, target in pairs:
        a = angles(pred, target)
        total += float(a.sum())
        count += a.size
    return (total / count if count else float('nan')), count


def angles_acos(pred, target):
    """the same angles as acos of the clipped cosine similarity (ill-conditioned near 0 and pi)"""
    p = np.moveaxis(np.asarray(pred, np.float64), 1, -1)
    t = np.asarray(target, np.float64)
    m = valid_mask(target)
    p, t = p[m], t[m]
    cos = (p * t).sum(-1) / (np.linalg.norm(p, axis=-1) * np.linalg.norm(t, axis=-1))
    return np.arccos(np.clip(cos, -1.0, 1.0))


# ---- inputs ----------------------------------------------------------------------------------------
def random_normals(n, h, w, seed=0, invalid=0.3):
    """(N, H, W, 3) float32 unit vectors, about `invalid` of the pixels exactly (0, 0, 0)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, h, w, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v = v.astype(np.float32)
    v[rng.random((n, h, w)) < invalid] = 0.0
    return v
