"""CPU references for tests/test_reduce_pool_gpu.py: the launch rules of the SE channel reductions and
of the adaptive average pool restated in Python, integer-valued inputs whose sums are exact in fp32,
and fp64 / int64 references of the reductions, the excitation MLP, both pools and the max pool's tie
rule.  Nothing here touches the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}     # elements of a 16-byte vector


# -- channel reductions ---------------------------------------------------------------------------
def channel_splits(hw, n, invariant=False):
    """(splits, chunk) of csrc/pointwise.hip channel_splits + the chunk of channel_dot_kernel: 512
    pixels per workgroup, at most 64 per image; where that leaves the launch with <= 64 workgroups
    (and the partition may depend on the batch), 64 pixels, at most 256"""
    splits = min((hw + 511) // 512, 64)
    if n * splits <= 64 and not invariant:
        splits = min((hw + 63) // 64, 256)
    splits = max(splits, 1)
    return splits, (hw + splits - 1) // splits


def reduction_route(dtype, c):
    """('narrow', lanes, idle threads) or ('wide', channel-vector groups, live threads of the last)"""
    cvn = c // VEC[dtype]
    if cvn > 256:
        return 'wide', (cvn + 255) // 256, cvn - (cvn - 1) // 256 * 256
    return 'narrow', 256 // cvn, 256 - 256 // cvn * cvn


def int_map(n, c, h, w, seed, chunk):
    """int64 (n, c, h, w) with values in -3 .. 3 (exact in fp32, bf16 and fp16): a random part in
    -2 .. 2 plus an offset in -1 .. 1 that changes with the image and with the chunk of `chunk` pixels
    the pixel lies in, so chunks of different images or positions have different sums"""
    rng = np.random.default_rng(seed)
    base = torch.from_numpy(rng.integers(-2, 3, (n, c, h, w)))
    pix = torch.arange(h * w).view(1, 1, h, w)
    img = torch.arange(n).view(n, 1, 1, 1)
    return (base + ((pix // max(chunk, 1) + img) % 3 - 1)).clamp_(-3, 3)


def mean_bits(total, hw):
    """what channel_dot_finish_kernel stores for an exact sum: float32(sum) * float32(1 / hw)"""
    scale = np.float32(1.0) / np.float32(hw)
    return torch.from_numpy(total.numpy().astype(np.float32) * scale)


# -- excitation MLP -------------------------------------------------------------------------------
def se_mlp_reference(gap, w1, b1, w2, b2, ds):
    """fp64 sigmoid(W2 relu(W1 g + b1) + b2) and its autograd (ReLU' = 0 at 0)
    -> hid, s, dgap, dw1, db1, dw2, db2"""
    g, a1, c1, a2, c2 = (t.double().clone().requires_grad_(True) for t in (gap, w1, b1, w2, b2))
    hid = torch.relu(g @ a1.t() + c1)
    s = torch.sigmoid(hid @ a2.t() + c2)
    s.backward(ds.double())
    return (hid.detach(), s.detach(), g.grad, a1.grad, c1.grad, a2.grad, c2.grad)


# -- adaptive average pool ------------------------------------------------------------------------
def bin_range(i, size, bins):
    return (i * size) // bins, ((i + 1) * size + bins - 1) // bins


def pool_route(dtype, c, h, w, bins):
    """'wg256' / 'wg1024' (adaptive_avgpool_fwd_wg_kernel and its thread count) or 'general'"""
    v = VEC[dtype]
    vec_ok = c >= 4 and c % 4 == 0 and c <= 4096 and c % v == 0
    if vec_ok and c // v <= 1024 and h * w >= 4 * bins * bins:
        return 'wg1024' if c // v >= 64 else 'wg256'
    return 'general'


def pool_sums(x, bins):
    """(sum over each bin (n, c, bins, bins) in x's dtype, pixels per bin (bins, bins) int64)"""
    n, c, h, w = x.shape
    sums = x.new_zeros((n, c, bins, bins))
    count = torch.zeros((bins, bins), dtype=torch.int64)
    for i in range(bins):
        h0, h1 = bin_range(i, h, bins)
        for j in range(bins):
            w0, w1 = bin_range(j, w, bins)
            sums[:, :, i, j] = x[:, :, h0:h1, w0:w1].sum((2, 3))
            count[i, j] = (h1 - h0) * (w1 - w0)
    return sums, count


def pool_mean_bits(sums, count, dtype):
    """an exact bin sum through the kernel's arithmetic: float32(sum) / float32(pixels), one correctly
    rounded fp32 division, then one rounding to the storage type"""
    q = sums.numpy().astype(np.float32) / count.numpy().astype(np.float32)
    return torch.from_numpy(q).to(dtype)


def pool_bwd_reference(dy, h, w):
    """fp64 gradient of F.adaptive_avg_pool2d for the cotangent dy (n, c, bins, bins)"""
    x = torch.zeros(dy.shape[0], dy.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    F.adaptive_avg_pool2d(x, dy.shape[-1]).backward(dy.double())
    return x.grad


# -- max pool 3x3 / 2, padding 1 ------------------------------------------------------------------
def maxpool_reference(x):
    """F.max_pool2d of the fp64 map x: y, the flat input index of each maximum (a tie goes to the first
    tap in row-major window order, an all -inf window to its first in-range tap) and that index as the
    tap number 0 .. 8 the kernel stores"""
    h, w = x.shape[2:]
    y, ind = F.max_pool2d(x, 3, stride=2, padding=1, return_indices=True)
    oh = torch.arange(y.shape[2]).view(1, 1, -1, 1)
    ow = torch.arange(y.shape[3]).view(1, 1, 1, -1)
    tap = (ind // w - (2 * oh - 1)) * 3 + (ind % w - (2 * ow - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    return y, ind, tap


def maxpool_bwd_reference(dy, ind, h, w):
    """int64 scatter of the integer cotangent dy to the positions `ind`"""
    n, c = dy.shape[:2]
    dx = torch.zeros(n, c, h * w, dtype=torch.int64)
    dx.scatter_add_(2, ind.reshape(n, c, -1), dy.reshape(n, c, -1))
    return dx.view(n, c, h, w)
