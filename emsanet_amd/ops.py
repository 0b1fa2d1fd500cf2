# -*- coding: utf-8 -*-
"""
Fused forward/backward operators of the EMSANet engine as torch.autograd.Functions.

Granularity follows the fusion plan of DESIGN.md, not the reference's module list: one Function
per NonBottleneck1D block (4 MFMA convs + 2 BatchNorms + Dropout2d + residual, hand-written
backward with the ReLU masks and the residual add fused into the data-gradient epilogues), one
per conv+BN+act, per SE fusion, per learned upsampling ...  Every Function only sequences calls
into libemsanet_hip.so (emsanet_amd/functional.py); autograd is used for graph bookkeeping only.
What travels between these host functions is a named record: _ConvBN, _NBtSaved, _WgradJob.
"""
import collections
import contextlib
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as Fn
from ._lib import check
from .functional import ACT_NONE, ACT_RELU
from .parallel import grad_target

# debug: set to a list to record (tag, tensor clone) for every backward's inputs and outputs
TRACE = None
# tests: set to a list to record every sign decision of the forward pass (ReLU outputs > 0) in
# execution order -- tests/test_model_gpu.py replays them inside the fp64 oracle so that the
# engine's gradients can be compared at a TIGHT tolerance (same piecewise-linear branch on both
# sides; without it a single ReLU flipped by fp32 roundoff moves every upstream gradient by ~1e-2)
MASK_TRACE = None


# tools/actgrad_compare.py: set to a dict to record, per convolution module (key: id(module)), the
# gradient w.r.t. that convolution's OUTPUT as its backward kernels receive it -- the quantity a
# tensor hook on the conv output gives in plain PyTorch -- to localise where activation gradients
# of engine and oracle part
GRAD_TRACE = None


def _trace_grad(module, dy):
    if GRAD_TRACE is not None:
        GRAD_TRACE[id(module)] = dy.detach().float().cpu()


def _trace_mask(tag, t):
    if MASK_TRACE is not None:
        MASK_TRACE.append((tag, t > 0))


def _traced(fn):
    """wrap a Function.backward: with ops.TRACE = [] every incoming / outgoing gradient is cloned
    into the list (tools/determinism.py uses it to find the first diverging tensor)."""
    def wrapper(ctx, *grads):
        if TRACE is None:
            return fn(ctx, *grads)
        tag = fn.__qualname__.split('.')[0]
        for i, g in enumerate(grads):
            if torch.is_tensor(g):
                TRACE.append((f'{tag}.in{i}', g.detach().clone()))
        out = fn(ctx, *grads)
        for i, g in enumerate(out if isinstance(out, tuple) else (out,)):
            if torch.is_tensor(g):
                TRACE.append((f'{tag}.out{i}', g.detach().clone()))
        return out
    wrapper.__qualname__ = fn.__qualname__
    return wrapper


# ---------------------------------------------------------------------------------------------
# runtime views of parameter containers
# ---------------------------------------------------------------------------------------------
class _PackCache:
    """The packed forms of one conv's weights: (form, dtype) -> [key_fwd, fwd, key_dgrad, dgrad].  A
    side is valid while its key equals the conv's current one (the parameters' versions and
    addresses); the owner packs into it on a miss (`get`), PackPlan installs its views (`put`)."""

    def __init__(self):
        self._slots = {}

    def get(self, form, dtype, side, key, pack, both):
        """side 0: forward operand, 1: data-gradient operand.  A forward miss calls
        pack(fwd=True, dgrad=both) -- `both`: the data gradient will be wanted too, one launch for
        the two -- a data-gradient miss pack(fwd=False, dgrad=True); pack returns (fwd, dgrad)"""
        ent = self._slots.get((form, dtype))
        if ent is None:
            ent = self._slots[(form, dtype)] = [None, None, None, None]
        if ent[2 * side] != key:
            if side == 0:
                ent[1], d = pack(fwd=True, dgrad=both)
                ent[0] = key
                if d is not None:
                    ent[2], ent[3] = key, d
            else:
                ent[3] = pack(fwd=False, dgrad=True)[1]
                ent[2] = key
        return ent[2 * side + 1]

    def put(self, form, dtype, key, fwd, dgrad):
        """overwrites the whole slot: an older data-gradient operand is dropped, never kept beside a
        newer forward one (it would pin the arena it is a view of)"""
        self._slots[(form, dtype)] = [key, fwd, key if dgrad is not None else None, dgrad]

    def peek(self, form, dtype, key):
        """(fwd, dgrad) as stored under `key`, None for a side that is absent or stale; never packs"""
        ent = self._slots.get((form, dtype), (None, None, None, None))
        return ent[1] if ent[0] == key else None, ent[3] if ent[2] == key else None


# One packed form of a conv's weights as a packer has to know it: the slot's name in `_PackCache`, the
# EmsaPackJob kind (None: no job of emsa_pack_batch makes it, the runtime derives it itself), the
# element type of the result, the elements of the forward and of the data-gradient operand, and
# whether the operands hold padding no pack writes (zeroed once, so that two packs compare equal)
_Form = collections.namedtuple('_Form', 'name kind dtype n_fwd n_dgrad zero_pad')


def _weight_forms(rt, n, dtype):
    """the forms of the n-element [tap][n][k] operand of `rt` that spec and dtype alone decide"""
    s, f32 = rt.spec, torch.float32
    if dtype != f32:
        return [_Form('gemm', _lib.PACK_GEMM_16[Fn.DT[dtype]], dtype, n, n, False)]
    if not rt.wino:
        return [_Form('gemm', _lib.PACK_GEMM, f32, n, n, False)]
    fs = [_Form('wino', _lib.PACK_WINO, f32, n * 4 // 3, n * 4 // 3, False)]       # U: 4 comps per 3 taps
    if rt.wino2d:
        # (the K-step padding of a channel count that is no multiple of 8 is never written)
        fs.append(_Form('wino2d', _lib.PACK_WINO2D, f32, Fn.wino2d_numel(s.cout, s.cin),
                        Fn.wino2d_numel(s.cin, s.cout), bool(s.cin % 8 or s.cout % 8)))
    return fs


class ConvRT:
    """nn.Conv2d used as a parameter container + cached packed weights.  fp32 activations run on
    the fp32 kernels (Winograd where eligible); 16-bit activations on conv_h.hip with the weights
    packed in the activations' dtype (the fp32 parameter stays the master copy)."""

    def __init__(self, conv):
        self.conv = conv
        self.spec = Fn.ConvSpec(conv.in_channels, conv.out_channels, tuple(conv.kernel_size),
                                tuple(conv.stride), tuple(conv.padding))
        # stride-1 3x1 / 1x3 convs run on the Winograd F(2,3) kernel (EMSA_WINO=0 disables it)
        self.wino = Fn.wino_enabled(self.spec)
        # dense 3x3 convs the per-shape rule sends to the 2-D Winograd F(2x2,3x3) kernel hold its
        # weights U2 as well; the row form stays (fallback for what that kernel refuses)
        self.wino2d = self.wino and Fn.wino2d_selected(self.spec)
        # stride-1 3x1 / 1x3 convs with 64..512 channels in 16-bit storage: the register-stationary
        # streaming kernel (conv_rs.hip) with fragment-ordered weights, where it takes the geometry
        self.rs = Fn.rs_eligible(self.spec)
        self.packs = _PackCache()     # the forms of `forms`
        self.plain_asked = 0      # times the [tap][n][k] 16-bit operand of an rs conv was read (PackPlan)

    def forms(self, dtype):
        """the forms this conv keeps for activations of `dtype`, the operand every kernel takes first:
        'gemm' [tap][n][k] (16-bit, and fp32 without the Winograd form) or 'wino' U (fp32); then
        'frag' fragment-ordered (16-bit, conv_rs) or 'wino2d' U2 (fp32, per-shape rule).  What
        `_operands` reads and PackPlan packs; decided per call (tests flip Fn.CONV_RS)"""
        n = self.conv.weight.numel()
        fs = _weight_forms(self, n, dtype)
        if dtype != torch.float32 and self.rs and Fn.CONV_RS:
            fs.append(_Form('frag', _lib.PACK_FRAG_16[Fn.DT[dtype]], dtype, n, n, False))
        return fs

    def spec_key(self):
        s = self.spec
        return (s.cin, s.cout, s.kh, s.kw, s.sh, s.sw, s.ph, s.pw)

    def key_now(self):
        w = self.conv.weight
        return (w._version, w.data_ptr())

    def _pack(self, form, dtype, fwd, dgrad):
        w = self.conv.weight.detach()
        if form == 'wino':
            return Fn.pack_wino(w, fwd=fwd, dgrad=dgrad)
        if form == 'wino2d':
            return Fn.pack_wino2d(w, fwd=fwd, dgrad=dgrad)
        if form == 'frag':
            return Fn.pack_weight_frag_t(w, dtype, fwd=fwd, dgrad=dgrad)
        if dtype != torch.float32:
            return Fn.pack_weight_t(w, dtype, fwd=fwd, dgrad=dgrad)
        if fwd and dgrad:
            # trainable: the data-gradient layout will be needed too -> one launch for both
            return Fn.pack_weight_pair(w)
        return (Fn.pack_weight(w, 'fwd'), None) if fwd else (None, Fn.pack_weight(w, 'dgrad'))

    def weights(self, form, side, dtype=torch.float32):
        """the forward (side 0) / data-gradient (side 1) operand of `form`: PackPlan's when fresh,
        else packed here -- both sides at a forward miss of a trainable weight"""
        w = self.conv.weight           # (one module attribute lookup per call: this is the hot path)
        return self.packs.get(form, dtype, side, (w._version, w.data_ptr()),
                              lambda fwd, dgrad: self._pack(form, dtype, fwd, dgrad), w.requires_grad)

    def _operands(self, side, dtype, wino2d=True):
        """(wp, keyword arguments) of Fn.conv_fwd (side 0) / Fn.conv_dgrad (side 1) that hand over
        this conv's operands for activations of `dtype`, best kernel first; wino2d=False: without U2"""
        if dtype != torch.float32:
            wf = self.frag(dtype, side)
            if wf is None:
                return self.packed(dtype, side), {}
            # the [tap][n][k] operand of a conv_rs-capable conv ON DEMAND: where conv_rs takes the
            # geometry (every NBt1D conv of a training step) nobody reads it, and PackPlan stops
            # packing it (`plain_asked` tells it when somebody did)
            return (lambda: self.packed(dtype, side)), {'wfrag': wf}
        if self.wino2d and wino2d:
            return None, {'wino2d_u': self.weights('wino2d', side),
                          'wino_u': lambda: self.weights('wino', side)}
        if self.wino:
            return None, {'wino_u': self.weights('wino', side)}
        return self.packed(side=side), {}

    def forward(self, x, **kw):
        """conv forward through the best kernel for this layer (fused-epilogue kwargs of conv_fwd)"""
        wp, operands = self._operands(0, x.dtype)
        return Fn.conv_fwd(x, wp, self.spec, **operands, **kw)

    def folds_input_bn(self, t):
        """this conv can take the BatchNorm + ReLU in front of it (input tensor `t`) into its
        loader: fp32 1-D Winograd form, forward and weight gradient; Fn.bn1_fold decides whether
        it pays at this size"""
        if t.dtype != torch.float32:
            return self.rs and Fn.bn1_fold16(t, self.spec)
        return self.wino and Fn.wino_rows(self.spec) == 1 and Fn.bn1_fold(t)

    def dgrad(self, dy, in_hw, mask_bits=None, **kw):
        """mask_bits: the ReLU mask of the producing layer as bits (conv_fwd(want_relu_bits));
        used by the 1-D Winograd kernel (U2 stays out then), otherwise the float `mask_src` applies"""
        wp, operands = self._operands(1, dy.dtype, wino2d=mask_bits is None)
        return Fn.conv_dgrad(dy, wp, self.spec, in_hw, mask_bits=mask_bits, **operands, **kw)

    def dgrad_takes_res_bits(self, dy, in_hw, residual):
        """this conv's data gradient can mask its residual operand by bits (Fn.conv_dgrad res_bits):
        the fp32 1-D Winograd launch, whole 64-channel tiles"""
        return self.wino and not self.wino2d and Fn.dgrad_takes_res_bits(self.spec, dy, in_hw, residual)

    def dgrad_bnb(self, dy, in_hw, t, affine, mean, invstd, residual=None, force=False):
        """data gradient + the backward reduction of the BatchNorm in front of this conv
        (Fn.conv_dgrad_bnb), or None when this conv's kernel has no such epilogue (fp32 without
        the Winograd form).  force: the caller has no other way (the forward folded the BatchNorm
        into this conv's loader: no ReLU bit mask exists)"""
        if affine is None or not (force or Fn.bn_fused_reduce(dy.dtype, self.spec.cin)):
            return None
        if dy.dtype == torch.float32 and not self.wino:
            return None
        scale, shift = affine
        wp, operands = self._operands(1, dy.dtype, wino2d=False)
        return Fn.conv_dgrad_bnb(dy, wp, self.spec, in_hw, t, scale, shift, mean, invstd,
                                 residual=residual, **operands)

    def frag(self, dtype, side=0):
        """fragment-ordered weights for conv_rs.hip (None: not that kind of conv)"""
        return self.weights('frag', side, dtype) if self.rs and Fn.CONV_RS else None

    def packed(self, dtype=torch.float32, side=0):
        if dtype != torch.float32:
            self.plain_asked += 1
        return self.weights('gemm', side, dtype)


# EMSA_PACK_LEAN=0: always pack both 16-bit operand forms of the conv_rs-capable convs (A/B runs)
PACK_LEAN = os.environ.get('EMSA_PACK_LEAN', '1') != '0'

# One job of PackPlan's table before it has addresses: `owner` (ConvRT / MultiConvRT) gets `form`
# (a _Form; None: the empty job a lean table keeps in a skipped operand's place) packed from the
# parameter `src` by a job of `kind` with dims = (cout, cin, kh, kw) and place = (cout_total, cout_off,
# cin_total, cin_off) inside a wider operand; elems = elements of the (forward, data-gradient) side, 0:
# no such side; persistent: into the owner's zero-initialised operand of that form, which all its
# placements share (merged heads), instead of into views carved from the arena
_PackEntry = collections.namedtuple('_PackEntry', 'owner form src kind dims place elems persistent')

# What one `PackPlan._build` made, and what a captured launch holds raw pointers into: the job table
# on the device, its launch arguments, the arena, views = {(owner, form): (fwd, dgrad)} -- arena views
# and the merged heads' operands -- and what it was built for: dtype, the parameters' addresses, and
# per conv whether its first form has a data-gradient side (None: skipped by a lean table)
_PackBuild = collections.namedtuple('_PackBuild', 'jobs n_jobs n_blocks arena views dtype ptrs two_sided')


class PackPlan:
    """All weight transforms of a model (packed implicit-GEMM layouts, Winograd U, or the 16-bit
    operands of the mixed-precision path) in ONE launch per optimizer step instead of one ~5 us
    kernel per layer (380 launches = 2.3 ms per step).  `refresh(dtype)` (called at the start of
    the model's forward) re-packs every form of `forms(dtype)` of every registered runtime when any
    weight changed and installs the results in the runtimes' own caches (`_PackCache.put`), so their
    per-layer fallback (`weights()`) finds fresh entries and launches nothing."""

    # forms whose jobs come after every conv's first form in the table
    _SECOND = ('frag', 'wino2d')

    def __init__(self, rts):
        self.rts = [rt for rt in rts if isinstance(rt, ConvRT)]
        # merged / channel-padded head convs (MultiConvRT: task heads, side heads, scene head): one
        # job per placed parameter (+ one per bias) into persistent zero-initialised operands --
        # they used to re-pack themselves every step with a zero-fill and 2-4 kernels each
        self.multi = [rt for rt in rts if isinstance(rt, MultiConvRT)]
        self._key = None
        self._built = None            # _PackBuild
        # lean: the conv_rs-capable convs get their fragment-ordered 16-bit operands only -- their
        # [tap][n][k] form (half of the 16-bit pack launch: 188 convs of the full model) is read only
        # where conv_rs refuses a geometry.  Decided from what the previous step asked for
        # (ConvRT.plain_asked): full table first, lean once a whole step went by without a reader,
        # full again as soon as one turns up (who meanwhile packs per layer, ConvRT.packed)
        self._lean = False
        self._asked_seen = None
        # a hipGraph that captured `emsa_pack_batch` holds RAW pointers to the job table, the arena
        # and the merged-head operands.  Once a refresh ran under capture the lean / full state is
        # frozen (the table a replay reads must stay the one it recorded) and whatever a later
        # rebuild supersedes (new dtype, moved parameters) is kept alive in `_retired` instead of
        # going back to the allocator, where a replay would scribble over someone else's memory
        # (ADVICE r5).  `thaw()` drops both when the graphs are gone.
        self._captured = False
        self._retired = []            # superseded _PackBuilds

    _jobs = property(lambda self: self._built and self._built.jobs)
    _arena = property(lambda self: self._built and self._built.arena)

    def thaw(self):
        """no captured graph replays this plan's pack launch any more: allow lean / full switches
        again and release the superseded tables"""
        self._captured = False
        self._retired.clear()

    def _asked(self):
        return sum(rt.plain_asked for rt in self.rts if rt.rs)

    def _src_ptrs(self):
        return tuple(rt.conv.weight.data_ptr() for rt in self.rts) + \
            tuple(q.weight.data_ptr() for m in self.multi for q, _, _ in m.placements)

    def _entries(self, dtype, lean):
        """the table in its order: every conv's first form, then the convs' second forms; then head by
        head the first form and the bias placement by placement, then the head's second form.  lean:
        a conv with fragment-ordered weights gets an empty job (one block) for its [tap][n][k] form"""
        ents = []
        for second in (False, True):
            for rt in self.rts:
                w, forms = rt.conv.weight, rt.forms(dtype)
                skip = lean and any(f.name == 'frag' for f in forms)
                for f in forms:
                    if (f.name in self._SECOND) != second:
                        continue
                    if skip and f.name == 'gemm':
                        ents.append(_PackEntry(rt, None, w, _lib.PACK_COPY, (0, 1, 1, 1), (0, 0, 0, 0),
                                               (0, 0), False))
                    else:
                        ents.append(_PackEntry(rt, f, w, f.kind, tuple(w.shape), (0, 0, 0, 0),
                                               (f.n_fwd, f.n_dgrad if w.requires_grad else 0), False))
        for m in self.multi:
            s = m.spec
            for second in (False, True):
                for q, co, ci in m.placements:
                    for f in m.forms(dtype):
                        if f.kind is None or (f.name in self._SECOND) != second:
                            continue
                        if f.name != 'bias':
                            ents.append(_PackEntry(m, f, q.weight, f.kind, tuple(m._w4(q).shape),
                                                   (s.cout, co, s.cin, ci), (f.n_fwd, f.n_dgrad), True))
                        elif q.bias is not None:
                            ents.append(_PackEntry(m, f, q.bias, f.kind, (q.bias.shape[0], 1, 1, 1),
                                                   (s.cout, co, 1, 0), (f.n_fwd, 0), True))
        return ents

    @staticmethod
    def _span(e):
        """(bytes of one side, sides) an entry takes of the arena: every pack starts 16-byte aligned,
        the data-gradient side one side's bytes behind the forward side"""
        if e.form is None or e.persistent:
            return 0, 0
        return (max(e.elems) * e.form.dtype.itemsize + 15) // 16 * 16, 2 if e.elems[1] else 1

    def _build(self, dev, dtype, lean=False):
        if self._captured and self._built is not None:
            self._retired.append(self._built)
        ents = self._entries(dtype, lean)
        self._lean = any(e.form is None for e in ents)
        arena = Fn._empty((sum(nb * sides for nb, sides in map(self._span, ents)),), dev, torch.uint8)
        jobs = (_lib.EmsaPackJob * len(ents))()
        views, off, blk = {}, 0, 0
        for j, e in enumerate(ents):
            key, (n_fwd, n_dgrad) = (e.owner, e.form), e.elems
            if e.form is None:
                # lean: no [tap][n][k] operand for this conv -- an empty job keeps the table's indexing
                fwd, dgrad = e.src, None
            elif e.persistent:
                if key not in views:
                    views[key] = (Fn._zeros((n_fwd,), dev, e.form.dtype),
                                  Fn._zeros((n_dgrad,), dev, e.form.dtype) if n_dgrad else None)
                fwd, dgrad = views[key]
            else:
                (nb, sides), dt = self._span(e), e.form.dtype
                if e.form.zero_pad:
                    arena[off:off + nb * sides].zero_()        # the K-step padding, never read by the kernel
                fwd = arena[off:off + n_fwd * dt.itemsize].view(dt)
                dgrad = arena[off + nb:off + nb + n_dgrad * dt.itemsize].view(dt) if n_dgrad else None
                off += nb * sides
                views[key] = (fwd, dgrad)
            jobs[j] = _lib.EmsaPackJob(e.src.data_ptr(), fwd.data_ptr(),
                                       dgrad.data_ptr() if dgrad is not None else None, *e.dims,
                                       e.kind, blk, *e.place)
            cout, cin, kh, kw = e.dims
            blk += max(1, min(64, (cout * cin * kh * kw + 2047) // 2048))
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        two_sided = tuple(None if e.form is None else e.elems[1] > 0 for e in ents[:len(self.rts)])
        self._built = _PackBuild(raw, len(ents), blk, arena, views, dtype, self._src_ptrs(), two_sided)

    def _install(self):
        """the install step of `refresh`: every view of the current table into its owner's cache (a
        lean table has none for a skipped operand: ConvRT.packed packs that one itself if asked)"""
        for (owner, form), (fwd, dgrad) in self._built.views.items():
            owner.packs.put(form.name, form.dtype, owner.key_now(), fwd, dgrad)

    def refresh(self, dtype=torch.float32):
        if not self.rts:
            return
        ws = [rt.conv.weight for rt in self.rts]
        key = (dtype,) + tuple((w._version, w.data_ptr(), w.requires_grad) for w in ws) + \
            tuple(m.key_now() for m in self.multi)
        if key == self._key:
            return
        if not ws[0].is_cuda:
            return                                   # host-side dry runs: per-layer path
        b = self._built
        if b is None or b.dtype != dtype or b.ptrs != self._src_ptrs() or \
                any(t is not None and t != w.requires_grad for t, w in zip(b.two_sided, ws)):
            self._build(ws[0].device, dtype, self._lean)
        # lean / full job table, from what the step behind us read (never switched inside a capture:
        # _build uploads the table)
        asked = self._asked()
        if torch.cuda.is_current_stream_capturing():
            self._captured = True
        if PACK_LEAN and dtype != torch.float32 and not self._captured:
            if self._lean and asked != self._asked_seen:
                self._build(ws[0].device, dtype, False)
            elif not self._lean and self._asked_seen is not None and asked == self._asked_seen:
                self._build(ws[0].device, dtype, True)
        self._asked_seen = asked
        b = self._built
        check(_lib.lib().emsa_pack_batch(b.jobs.data_ptr(), b.n_jobs, b.n_blocks, Fn._stream()),
              'emsa_pack_batch')
        self._install()
        self._key = key


# BatchNorm step counters (`num_batches_tracked`): nn.BatchNorm2d.forward is never called, so the
# engine counts training steps on the host -- ON THE MODULE (`bn._emsa_pending`), not in a global
# registry: a deep copy of the model (EMA twin) carries its own counts and hooks, and a
# sub-module's `state_dict()` flushes exactly like the whole model's.  The hooks are
# module-level functions (no closure over a runtime object), so `copy.deepcopy` keeps them valid.
def _bn_flush_hook(module, prefix=None, keep_vars=None):
    n = getattr(module, '_emsa_pending', 0)
    if n and module.num_batches_tracked is not None:
        module.num_batches_tracked += n
    module._emsa_pending = 0


def _bn_load_hook(module, state_dict, prefix, *unused):
    # counts gathered before a checkpoint is loaded belong to the state that is being replaced
    module._emsa_pending = 0


def mark_bn_stats_written(bn):
    """the running statistics of `bn` were (or are about to be) rewritten through raw pointers --
    `emsa_bn_finalize`, a replayed hipGraph -- which does not move their tensor version counters.
    Everything that caches a function of them keys on `_version` (BNRT._frozen_fold, the
    inference graph's `_weights_key`): bump it here, or the next eval silently runs on the folded
    statistics of an older state (eval -> train-mode forward under no_grad, frozen
    affine parameters -> eval)."""
    if bn.running_mean is not None:
        torch.autograd.graph.increment_version(bn.running_mean)
        torch.autograd.graph.increment_version(bn.running_var)


def flush_bn_counters(root):
    """add the host-side training-step counts of every BatchNorm below `root` to the
    `num_batches_tracked` buffers.  (`state_dict()` of the model or of any sub-module does this
    through the per-module pre-hook; a direct read of `bn.num_batches_tracked` during training
    needs this call first.)"""
    for m in root.modules():
        if hasattr(m, '_emsa_pending'):
            _bn_flush_hook(m)


class BNRT:
    """nn.BatchNorm2d used as a parameter/buffer container."""

    def __init__(self, bn):
        self.bn = bn
        if not hasattr(bn, '_emsa_pending'):
            bn._emsa_pending = 0
            bn.register_state_dict_pre_hook(_bn_flush_hook)
            bn.register_load_state_dict_pre_hook(_bn_load_hook)

    @property
    def pending_batches(self):
        return self.bn._emsa_pending

    @pending_batches.setter
    def pending_batches(self, value):
        self.bn._emsa_pending = value

    def batch_stats(self):
        # torch semantics: batch statistics in training mode or when no running stats exist
        return self.bn.training or self.bn.running_mean is None

    def running(self):
        bn = self.bn
        if bn.training and bn.track_running_stats and bn.running_mean is not None:
            return bn.running_mean, bn.running_var
        return None, None

    def forward_stats(self, stats, count):
        """-> scale, shift, mean, invstd for this call (updates running stats in train mode)."""
        bn = self.bn
        g, b = bn.weight.detach(), bn.bias.detach()
        if self.batch_stats():
            rm, rv = self.running()
            mom = bn.momentum if bn.momentum is not None else 0.1
            if rm is not None and bn.num_batches_tracked is not None:
                # nn.BatchNorm2d.forward is never called: keep its step counter like torch does
                # (checkpoints carry it); counted on the host, flushed by `flush_bn_counters`
                self.pending_batches += 1
            if rm is not None:
                mark_bn_stats_written(bn)
            return Fn.bn_finalize(stats, count, g, b, bn.eps, mom, rm, rv)
        scale, shift, invstd = self._frozen_fold()
        return scale, shift, bn.running_mean, invstd

    def _frozen_fold(self):
        """scale / shift / invstd of the frozen BatchNorm (running statistics), computed once per
        state of (weight, bias, running_mean, running_var) instead of once per forward pass: the
        bs=1 inference graph spent 127 of its ~440 launches re-deriving these constants (17 % of its
        GPU time, round 4).  Re-derived IN PLACE when a tensor changed, so that a captured graph's
        pointers stay valid."""
        bn = self.bn
        ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple((t._version, t.data_ptr()) for t in ts) + (bn.eps,)
        ent = getattr(self, '_fold_cache', None)
        if ent is None or ent[0] != key or ent[1].device != bn.weight.device:
            buf = ent[1] if ent is not None and ent[1].device == bn.weight.device else None
            s, t, inv = Fn.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                   bn.running_var, bn.eps, out=buf)
            self._fold_cache = ent = (key, s._base if s._base is not None else s, s, t, inv)
        return ent[2], ent[3], ent[4]

    def folded(self):
        s, t, _ = self._frozen_fold()
        return s, t


# _conv_bn_forward's result.  y: the conv's raw output; mask: bit mask of out > 0 for the backward
# pass (None without ReLU); affine: the BatchNorm as (scale, shift) with batch statistics, else None
# (a data gradient with the fused BatchNorm reduction recomputes the ReLU mask from it)
_ConvBN = collections.namedtuple('_ConvBN', 'out y mean invstd mask affine')


def _conv_bn_forward(x, crt, brt, act, drop=None, residual=None, wino_bits=False, res_affine=None):
    """conv (+bias) -> BN (batch or frozen statistics) -> *drop -> +residual -> act -> _ConvBN.
    wino_bits: the mask in the Winograd epilogue's layout (Fn.bn_act).  res_affine: the residual
    is `residual * scale + shift` (Fn.bn_act)"""
    bias = crt.conv.bias.detach() if crt.conv.bias is not None else None
    if brt.batch_stats():
        y, stats = crt.forward(x, bias=bias, want_stats=True)
        count = y.shape[0] * y.shape[2] * y.shape[3]
    else:
        y, stats, count = crt.forward(x, bias=bias), None, 0
    scale, shift, mean, invstd = brt.forward_stats(stats, count)
    out, mask = Fn.bn_act(y, scale, shift, drop, residual, act, want_mask=True, wino_bits=wino_bits,
                          res_affine=res_affine)
    return _ConvBN(out, y, mean, invstd, mask, (scale, shift) if brt.batch_stats() else None)


def _bn_targets(brt):
    """destinations of dgamma / dbeta inside the flat gradient buckets (or nothing)"""
    tg, tb = grad_target(brt.bn.weight), grad_target(brt.bn.bias)
    return {'dg_out': tg, 'db_out': tb} if tg is not None and tb is not None else {}


# EMSA_WGRAD_STREAM=1 / 2: the (deferred) weight gradients of the NBt1D blocks run on a side stream of
# LOW (1) / default (2) priority that joins the issuing stream when the backward pass ends.  The idea
# (round 5): the backward critical path alternates matrix-bound data gradients with HBM-bound
# BatchNorm passes; weight gradients are matrix-bound and nothing but the optimizer waits for them,
# so at low queue priority they can take the CU slots the HBM-bound passes leave idle instead of
# extending the critical path.  (Rounds 2 / 3 measured a plain second stream at default priority,
# joined per block, SLOWER: the weight gradients then displace their own block's data gradients.)
WGRAD_STREAM = int(os.environ.get('EMSA_WGRAD_STREAM', '0'))
_wgrad_sides = {}          # id of the issuing stream -> side stream
_wgrad_pending = []        # side streams with work of the current backward pass


def _wgrad_side(cur):
    key = (cur.device.index, cur.cuda_stream)
    side = _wgrad_sides.get(key)
    if side is None:
        lo, hi = 0, 0
        try:
            # (torch: smaller number = higher priority; ROCm exposes low = +1 where the runtime has it)
            side = torch.cuda.Stream(device=cur.device, priority=1 if WGRAD_STREAM == 1 else 0)
        except Exception:                       # noqa: BLE001
            side = torch.cuda.Stream(device=cur.device)
        _wgrad_sides[key] = side
        from .parallel import register_stream
        register_stream(side)
    return side


def _join_wgrad_streams():
    cur = torch.cuda.current_stream()
    while _wgrad_pending:
        cur.wait_stream(_wgrad_pending.pop())


class _Deferred:
    """placeholder of a weight / bias gradient whose launch was deferred (`_flush_wgrads`)"""

    def __init__(self, index, which):
        self.index, self.which = index, which


# a deferred weight gradient: conv input, output gradient, ConvRT, the flat-bucket views dw / dbias go
# to (or None), the BatchNorm + ReLU the forward folded into the conv's loader (or None)
_WgradJob = collections.namedtuple('_WgradJob', 'x dy crt tw tb in_affine')


def _bucket_view(dw, tw):
    """the gradient-bucket view `tw` itself when the kernel wrote `dw` into it"""
    return tw if tw is not None and dw.data_ptr() == tw.data_ptr() else dw


def _wgrad_now(x, dy, crt, tw, tb, in_affine=None):
    conv = crt.conv
    dw, db, packed = Fn.conv_wgrad(x, dy, crt.spec, conv.bias is not None, like=conv.weight,
                                   dw_out=tw, db_out=tb, in_affine=in_affine)
    if packed:
        return Fn.unpack_wgrad(dw, conv.weight, out=tw), db
    return _bucket_view(dw, tw), db


def _launch_wgrads(jobs):
    """the weight gradients of `jobs` -> [(dw, db), ...]: convs of equal channel counts together in
    one multi-job launch (Fn.conv_wgrad_multi; the four convs of an NBt1D block), the rest one by one"""
    res = [None] * len(jobs)
    groups = {}
    for i, job in enumerate(jobs):
        ok = (job.in_affine is None or job.x.dtype != torch.float32) and \
            Fn.wgrad_multi_eligible(job.x, job.crt.spec)
        groups.setdefault((job.crt.spec.cin, job.crt.spec.cout) if ok else ('single', i), []).append(i)
    for idx in groups.values():
        for k in range(0, len(idx), Fn.WGRAD_MULTI_MAX):
            part = idx[k:k + Fn.WGRAD_MULTI_MAX]
            out = None
            if len(part) >= 2:
                out = Fn.conv_wgrad_multi([(j.x, j.dy, j.crt.spec, j.crt.conv.weight, j.tw, j.tb,
                                            j.crt.conv.bias is not None, j.in_affine)
                                           for j in (jobs[i] for i in part)])
            if out is None:
                for i in part:
                    res[i] = _wgrad_now(*jobs[i])
            else:
                for i, (dw, db) in zip(part, out):
                    res[i] = (_bucket_view(dw, jobs[i].tw), db)
    return res


def _flush_wgrads(jobs, grads):
    """launch the deferred weight gradients (`_launch_wgrads`; with EMSA_WGRAD_STREAM on the side
    stream) and put the results in the places their `_Deferred` placeholders hold in `grads`"""
    if not jobs:
        return grads
    side = None
    if WGRAD_STREAM and jobs[0].x.is_cuda:
        cur = torch.cuda.current_stream()
        side = _wgrad_side(cur)
        side.wait_stream(cur)
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        res = _launch_wgrads(jobs)
    out = [res[g.index][g.which] if isinstance(g, _Deferred) else g for g in grads]
    if side is not None:
        for job in jobs:                        # (the caching allocator must not recycle them early)
            job.x.record_stream(side)
            job.dy.record_stream(side)
        # The join may wait for the end of the backward pass only where nobody reads these gradients
        # before: every one of them written into a bucket view of MANUAL buckets (no autograd hooks: the
        # caller reduces after backward).  Otherwise AccumulateGrad (adding into an existing .grad) or a
        # hook-driven bucket all-reduce would consume them while the side stream still writes (ADVICE
        # r5): join right here, and tell the allocator which stream the fresh tensors are used on.
        def _manual(job):
            slot = getattr(job.crt.conv.weight, '_emsa_grad_slot', None)
            bias = job.crt.conv.bias
            bslot = getattr(bias, '_emsa_grad_slot', None) if bias is not None else slot
            return (job.tw is not None and slot is not None and getattr(slot[1], 'manual', False) and
                    (bias is None or (job.tb is not None and bslot is not None)))
        if all(_manual(job) for job in jobs):
            if not _wgrad_pending:
                torch.autograd.Variable._execution_engine.queue_callback(_join_wgrad_streams)
            if side not in _wgrad_pending:
                _wgrad_pending.append(side)
        else:
            cur.wait_stream(side)
            for g in out:
                if torch.is_tensor(g):
                    g.record_stream(cur)
    return out


def _conv_backward(x, dy, crt, need_dx, mask_src=None, residual=None, mask_bits=None, bnb=None,
                   in_affine=None, defer=None, res_bits=None):
    """-> dx (or None), dw (OIHW), dbias (or None), bn_rows.  bnb = (t, (scale, shift), mean, invstd)
    of the BatchNorm+ReLU in front of the conv: bn_rows is (partial, rows) where the data gradient
    carries that BatchNorm's backward reduction -- dx then already has that ReLU's mask
    (ConvRT.dgrad_bnb) -- and None otherwise (always without bnb).  in_affine: the forward folded that
    BatchNorm + ReLU into the conv's loader (x = the BatchNorm's INPUT).  defer: a list -- the
    weight gradient is not launched here but queued as a _WgradJob (`_flush_wgrads`), dw / dbias
    are `_Deferred` placeholders.
    res_bits: `residual` is unmasked, its ReLU mask travels as bits (ConvRT.dgrad_takes_res_bits)"""
    conv = crt.conv
    _trace_grad(conv, dy)
    # the gradients go straight into their flat all-reduce / optimizer bucket views when
    # GradientBuckets manages the parameters (no gather copy later)
    tw = grad_target(conv.weight)
    tb = grad_target(conv.bias) if conv.bias is not None else None
    half = dy.dtype != torch.float32
    if defer is not None and (WGRAD_STREAM or ((in_affine is None or half) and
                                               Fn.wgrad_multi_eligible(x, crt.spec))):
        defer.append(_WgradJob(x, dy, crt, tw, tb, in_affine))
        dw, db = _Deferred(len(defer) - 1, 0), _Deferred(len(defer) - 1, 1)
    else:
        dw, db = _wgrad_now(x, dy, crt, tw, tb, in_affine)
    dx = None
    if bnb is not None and in_affine is not None and half:
        # 16-bit fold: plain data gradient; bn1's backward passes recompute the ReLU decisions from
        # the BatchNorm's input themselves (Fn.bn_bwd_aff)
        return crt.dgrad(dy, x.shape[2:], residual=residual), dw, db, None
    if bnb is not None:
        t, affine, mean, invstd = bnb
        r = crt.dgrad_bnb(dy, x.shape[2:], t, affine, mean, invstd, residual=residual,
                          force=in_affine is not None)
        if r is not None:
            return r[0], dw, db, (r[1], r[2])
        if in_affine is not None:
            raise _lib.EmsaError("folded BatchNorm: the data gradient has no fused reduction here")
        return crt.dgrad(dy, x.shape[2:], residual=residual), dw, db, None
    if need_dx and res_bits is not None:
        dx = crt.dgrad(dy, x.shape[2:], residual=residual, res_bits=res_bits)
    elif need_dx:
        dx = crt.dgrad(dy, x.shape[2:], mask_src=mask_src, residual=residual,
                       mask_bits=mask_bits)
    return dx, dw, db, None


# ---------------------------------------------------------------------------------------------
# NonBottleneck1D block
# ---------------------------------------------------------------------------------------------
class NBt1DRT:
    def __init__(self, block):
        self.c31_1, self.c13_1 = ConvRT(block.conv3x1_1), ConvRT(block.conv1x3_1)
        self.c31_2, self.c13_2 = ConvRT(block.conv3x1_2), ConvRT(block.conv1x3_2)
        self.bn1, self.bn2 = BNRT(block.bn1), BNRT(block.bn2)
        if block.downsample is not None:
            self.cds, self.bnds = ConvRT(block.downsample[0]), BNRT(block.downsample[1])
        else:
            self.cds = self.bnds = None

    def params(self):
        ps = []
        for c in (self.c31_1, self.c13_1):
            ps += [c.conv.weight, c.conv.bias]
        ps += [self.bn1.bn.weight, self.bn1.bn.bias]
        for c in (self.c31_2, self.c13_2):
            ps += [c.conv.weight, c.conv.bias]
        ps += [self.bn2.bn.weight, self.bn2.bn.bias]
        if self.cds is not None:
            ps += [self.cds.conv.weight, self.bnds.bn.weight, self.bnds.bn.bias]
        return ps


# what an NBt1D block keeps for its backward pass besides its input.  y1 .. y4: the four convs' raw
# outputs (y1, y3 after their ReLU); a2 = relu(bn1(y2)), None where bn1 is folded into conv3x1_2's
# loader; yd: the shortcut conv's output (or None); m* / is*: mean, invstd of bn1, bn2, the shortcut's
# BatchNorm; aff1: bn1 as (scale, shift) with batch statistics, else None; k1, k2: ReLU bit masks of
# the two BatchNorm outputs (the block output itself is not kept); q1, q3: those of y1, y3 (None when
# the layer does not run on the Winograd kernel)
_NBtSaved = collections.namedtuple(
    '_NBtSaved', 'y1 y2 a2 y3 y4 yd m1 is1 m2 is2 md isd k1 k2 q1 q3 aff1')


class NBt1DFunction(Function):
    """conv3x1+b,ReLU -> conv1x3+b,BN,ReLU -> conv3x1+b,ReLU -> conv1x3+b,BN -> Dropout2d
    -> + identity -> ReLU   (reference block: SURVEY.md §8 a3)."""

    @staticmethod
    def forward(ctx, x, rt, drop, *params):
        x = Fn.as_act(x, dense=True)
        b = lambda c: c.conv.bias.detach()   # noqa: E731
        y1, q1 = rt.c31_1.forward(x, bias=b(rt.c31_1), act=ACT_RELU, want_relu_bits=True)
        bn1_folded = rt.bn1.batch_stats() and rt.c31_2.folds_input_bn(y1)
        if bn1_folded:
            # bn1's normalise + ReLU happens in the loaders of conv3x1_2 (here) and of its weight
            # gradient; a2 = relu(bn1(y2)) is never written, no ReLU bit mask either (the data
            # gradient recomputes the decisions from y2)
            y2, stats = rt.c13_1.forward(y1, bias=b(rt.c13_1), want_stats=True)
            scale, shift, m1, is1 = rt.bn1.forward_stats(stats, y2.shape[0] * y2.shape[2] * y2.shape[3])
            aff1 = (scale, shift)
            a2 = k1 = None
            y3, q3 = rt.c31_2.forward(y2, bias=b(rt.c31_2), act=ACT_RELU, want_relu_bits=True,
                                      in_affine=aff1)
        else:
            a2, y2, m1, is1, k1, aff1 = _conv_bn_forward(y1, rt.c13_1, rt.bn1, ACT_RELU)
            y3, q3 = rt.c31_2.forward(a2, bias=b(rt.c31_2), act=ACT_RELU, want_relu_bits=True)
        aff_d = None
        if rt.cds is not None and rt.bnds.batch_stats() and rt.bn2.batch_stats() and Fn.idn_fold(y3):
            # the shortcut's normalise happens inside bn2's pass (Fn.idn_fold): idn is never written
            yd, stats = rt.cds.forward(x, want_stats=True)
            sd, td, md, isd = rt.bnds.forward_stats(stats, yd.shape[0] * yd.shape[2] * yd.shape[3])
            aff_d = (sd, td)
            idn = yd
        elif rt.cds is not None:
            idn, yd, md, isd, _, _ = _conv_bn_forward(x, rt.cds, rt.bnds, ACT_NONE)
        else:
            idn, yd, md, isd = x, None, None, None
        # k2 in the layout conv3x1_1's data gradient (bnds' backward in a down-sampling block) reads:
        # the masked skip gradient dres is then formed where it is consumed (Fn.dres_fold)
        wbits = False
        if y3.dtype == torch.float32 and rt.bn2.batch_stats() and Fn.dres_fold():
            wbits = Fn.wino_bits_ok(y3) and y3.shape[1] == rt.c13_2.spec.cout and \
                (rt.cds is not None or (rt.c31_1.wino and not rt.c31_1.wino2d))
            if not wbits:
                Fn._dres_fell_back()
        out, y4, m2, is2, k2, _ = _conv_bn_forward(y3, rt.c13_2, rt.bn2, ACT_RELU, drop=drop,
                                                   residual=idn, wino_bits=wbits, res_affine=aff_d)
        if MASK_TRACE is not None:
            a2t = a2 if a2 is not None else Fn.bn_act(y2, scale, shift, None, None, ACT_RELU)
            for tag, t in (('nbt.y1', y1), ('nbt.a2', a2t), ('nbt.y3', y3), ('nbt.out', out)):
                _trace_mask(tag, t)
        ctx.rt, ctx.drop = rt, drop
        ctx.save_for_backward(x)
        ctx.saved = _NBtSaved(y1, y2, a2, y3, y4, yd, m1, is1, m2, is2, md, isd, k1, k2, q1, q3, aff1)
        ctx.bn_train = (rt.bn1.batch_stats(), rt.bn2.batch_stats(),
                        rt.bnds.batch_stats() if rt.bnds is not None else False)
        return out

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dout):
        rt, drop = ctx.rt, ctx.drop
        (x,) = ctx.saved_tensors
        s = ctx.saved
        ctx.saved = None
        dout = Fn.as_act(dout, dense=True)
        t1, t2, tds = ctx.bn_train
        need_dx = ctx.needs_input_grad[0]
        defer = []           # the block's weight gradients: launched together at the end
        bn1_folded = s.a2 is None        # the forward folded bn1 into conv3x1_2's loader

        # out = relu(bn2(y4)*drop + idn)
        # (k2 in the Winograd layout: dres = dout * k2 is not stored, its one reader forms it)
        dres_folded = getattr(s.k2, '_emsa_wbits', False)
        if dres_folded and rt.cds is None and need_dx and \
                not rt.c31_1.dgrad_takes_res_bits(s.y1, x.shape[2:], dout):
            dres_folded = False
            Fn._dres_fell_back()
        dy4, dres, dg2, db2 = Fn.bn_bwd(dout, s.k2, s.y4, rt.bn2.bn.weight.detach(), s.m2, s.is2, drop,
                                        ACT_RELU, t2, want_dres=not dres_folded, **_bn_targets(rt.bn2))
        # conv1x3_2 (input y3 = relu(.)): ReLU mask fused into the dgrad epilogue
        dz3, dw4, dbias4, _ = _conv_backward(s.y3, dy4, rt.c13_2, True, mask_src=s.y3, mask_bits=s.q3,
                                             defer=defer)
        # conv3x1_2 (input a2 = relu(bn1(y2)))
        # the data gradient's epilogue applies bn1's ReLU mask and emits bn1's backward sums (one
        # pass over da2 and y2 less); falls back to the separate reduction pass
        bnb = (s.y2, s.aff1, s.m1, s.is1)
        if bn1_folded:                    # the conv's input is relu(bn1(y2))
            da2, dw3, dbias3, rows = _conv_backward(s.y2, dz3, rt.c31_2, True, bnb=bnb, in_affine=s.aff1,
                                                    defer=defer if s.y2.dtype != torch.float32 else None)
        else:
            da2, dw3, dbias3, rows = _conv_backward(s.a2, dz3, rt.c31_2, True, bnb=bnb, defer=defer)
        if rows is not None:
            dy2, dg1, db1 = Fn.bn_bwd_from_rows(da2, s.y2, rt.bn1.bn.weight.detach(), s.m1, s.is1,
                                                rows[0], rows[1], t1, **_bn_targets(rt.bn1))
        elif bn1_folded:
            # 16-bit fold: no a2, no bit mask -- the passes recompute the decisions from y2
            dy2, dg1, db1 = Fn.bn_bwd_aff(da2, s.y2, rt.bn1.bn.weight.detach(), s.m1, s.is1, s.aff1,
                                          **_bn_targets(rt.bn1))
        else:
            dy2, _, dg1, db1 = Fn.bn_bwd(da2, s.k1, s.y2, rt.bn1.bn.weight.detach(), s.m1, s.is1, None,
                                         ACT_RELU, t1, want_dres=False, **_bn_targets(rt.bn1))
        dz1, dw2, dbias2, _ = _conv_backward(s.y1, dy2, rt.c13_1, True, mask_src=s.y1, mask_bits=s.q1,
                                             defer=defer)
        if rt.cds is None:
            # identity skip: dx = dgrad(conv3x1_1) + dres, add fused into the epilogue
            if dres_folded:
                dx, dw1, dbias1, _ = _conv_backward(x, dz1, rt.c31_1, need_dx, residual=dout,
                                                    res_bits=s.k2, defer=defer)
            else:
                dx, dw1, dbias1, _ = _conv_backward(x, dz1, rt.c31_1, need_dx, residual=dres,
                                                    defer=defer)
        else:
            if dres_folded:    # the masked incoming gradient: dout with k2 as its ReLU mask
                dyd, _, dgd, dbd = Fn.bn_bwd(dout, s.k2, s.yd, rt.bnds.bn.weight.detach(), s.md, s.isd,
                                             None, ACT_RELU, tds, want_dres=False,
                                             **_bn_targets(rt.bnds))
            else:
                dyd, _, dgd, dbd = Fn.bn_bwd(dres, None, s.yd, rt.bnds.bn.weight.detach(), s.md, s.isd,
                                             None, ACT_NONE, tds, want_dres=False,
                                             **_bn_targets(rt.bnds))
            dxd, dwd, _, _ = _conv_backward(x, dyd, rt.cds, need_dx)
            dx, dw1, dbias1, _ = _conv_backward(x, dz1, rt.c31_1, need_dx, residual=dxd, defer=defer)
        grads = [dw1, dbias1, dw2, dbias2, dg1, db1, dw3, dbias3, dw4, dbias4, dg2, db2]
        if rt.cds is not None:
            grads += [dwd, dgd, dbd]
        grads = _flush_wgrads(defer, grads)
        return (dx, None, None) + tuple(grads)


def _half_block_specs(rt):
    """the block's two half-blocks are conv3x1 -> conv1x3 pairs the fused kernel takes (stride 1, equal
    channel counts); the first half of a down-sampling block is not"""
    def ok(ca, cb):
        sa, sb = ca.spec, cb.spec
        return (Fn.rs_eligible(sa) and Fn.rs_eligible(sb) and (sa.kh, sa.kw) == (3, 1) and
                (sb.kh, sb.kw) == (1, 3) and sa.cout == sb.cin)
    return ok(rt.c31_1, rt.c13_1), ok(rt.c31_2, rt.c13_2)


def _half(xs, cas, cbs, bns, residuals):
    """one fused half-block launch over 1 or 2 tensor sets (Fn.nbt_half_block)"""
    b = lambda c: c.conv.bias.detach() if c.conv.bias is not None else None   # noqa: E731
    folds = [bn.folded() for bn in bns]
    dtype = xs[0].dtype
    return Fn.nbt_half_block(xs, [c.frag(dtype) for c in cas], [b(c) for c in cas],
                             [c.frag(dtype) for c in cbs], [b(c) for c in cbs],
                             [f[0] for f in folds], [f[1] for f in folds], residuals, ACT_RELU)


def _convs(xs, crts, act=ACT_NONE, **kw):
    """the same conv layer of 1 or 2 (twin) modules on their inputs -> list of outputs.  Two: one
    twin launch -- of the register-stationary kernel where it takes the geometry (Fn.conv_fwd_pair),
    else of the implicit GEMM (Fn.conv_igemm_pair) -- or two launches (fp32 storage).
    kw: per-entry lists of operands (bias=, scale=, shift=, residual=)"""
    pr = {k: kw.get(k) or [None] * len(xs) for k in ('bias', 'scale', 'shift', 'residual')}
    if len(xs) == 2 and crts[0].spec_key() == crts[1].spec_key():
        (xa, xb), (ca, cb) = xs, crts
        r = Fn.conv_fwd_pair((xa, xb), (ca.frag(xa.dtype), cb.frag(xb.dtype)), ca.spec,
                             biases=pr['bias'], scales=pr['scale'], shifts=pr['shift'],
                             residuals=pr['residual'], act=act)
        if r is None and xa.dtype != torch.float32:
            r = Fn.conv_igemm_pair((xa, xb), (ca.packed(xa.dtype), cb.packed(xb.dtype)), ca.spec,
                                   biases=pr['bias'], scales=pr['scale'], shifts=pr['shift'],
                                   residuals=pr['residual'], act=act)
        if r is not None:
            return list(r)
    return [c.forward(x, act=act, **{k: v[i] for k, v in pr.items() if v[i] is not None})
            for i, (x, c) in enumerate(zip(xs, crts))]


def conv_bn_act_eval_pair(xa, xb, ma, mb):
    """conv_bn_act_eval of the same ConvNormAct layer of two twin modules (nn.ConvNormAct: `_crt`,
    `_brt`, `act`) as one twin launch; xa may be xb (the skip both decoders read)"""
    if ma.act != mb.act:
        raise _lib.EmsaError("twin ConvNormAct layers differ in their activation")
    (sa, ta), (sb, tb) = ma._brt.folded(), mb._brt.folded()
    return tuple(_convs([xa, xb], [ma._crt, mb._crt], scale=[sa, sb], shift=[ta, tb], act=ma.act))


def _nbt1d_eval(xs, rts):
    """the eval sequence of an NBt1D block over 1 tensor set, or over 2: the SAME block of two twin
    networks in lockstep, every conv both blocks share a geometry for as one twin launch (`_convs`).
    A fused half-block launch (`_half`) takes all tensor sets or none."""
    if any((r.cds is None) != (rts[0].cds is None) for r in rts):
        raise _lib.EmsaError("twin NBt1D blocks differ in their skip path")
    bias = lambda cs: [c.conv.bias.detach() for c in cs]   # noqa: E731
    same = lambda cs: all(c.spec_key() == cs[0].spec_key() for c in cs)   # noqa: E731
    halves = [_half_block_specs(r) for r in rts]
    c31_1, c13_1 = [r.c31_1 for r in rts], [r.c13_1 for r in rts]
    c31_2, c13_2 = [r.c31_2 for r in rts], [r.c13_2 for r in rts]
    if all(x.shape == xs[0].shape and x.dtype == xs[0].dtype for x in xs) and \
            all(h[0] for h in halves) and same(c31_1) and same(c13_1) and \
            all(Fn.half_block_ok(x, c.spec.cin) for x, c in zip(xs, c31_1)):
        # one launch for the first half-block (fused conv3x1 -> conv1x3, csrc/conv_hb.hip)
        a2s = _half(xs, c31_1, c13_1, [r.bn1 for r in rts], [None] * len(xs))
    else:
        y1s = _convs(xs, c31_1, bias=bias(c31_1), act=ACT_RELU)
        folds = [r.bn1.folded() for r in rts]
        a2s = _convs(y1s, c13_1, bias=bias(c13_1), scale=[f[0] for f in folds],
                     shift=[f[1] for f in folds], act=ACT_RELU)
    if rts[0].cds is not None:
        folds = [r.bnds.folded() for r in rts]
        idns = _convs(xs, [r.cds for r in rts], scale=[f[0] for f in folds], shift=[f[1] for f in folds])
    else:
        idns = xs
    if all(h[1] for h in halves) and same(c31_2) and same(c13_2) and \
            all(a2.shape == a2s[0].shape for a2 in a2s) and \
            all(Fn.half_block_ok(a2, c.spec.cin) for a2, c in zip(a2s, c31_2)) and \
            all(Fn.ld_of(idn) == idn.shape[1] for idn in idns):
        return _half(a2s, c31_2, c13_2, [r.bn2 for r in rts], idns)
    y3s = _convs(a2s, c31_2, bias=bias(c31_2), act=ACT_RELU)
    folds = [r.bn2.folded() for r in rts]
    return _convs(y3s, c13_2, bias=bias(c13_2), scale=[f[0] for f in folds],
                  shift=[f[1] for f in folds], residual=idns, act=ACT_RELU)


def nbt1d_eval(x, rt):
    """no-grad / eval fast path: both BatchNorms folded into the conv epilogues (4 launches; 2 where
    the fused half-block kernel takes the map: small-batch 16-bit inference at C = 64 / 128)."""
    return _nbt1d_eval([x], [rt])[0]


def nbt1d_eval_pair(xa, xb, ra, rb):
    """nbt1d_eval of the SAME block of two twin networks (rgb | depth encoder, semantic | instance
    decoder) in lockstep (4 instead of 8 launches per block pair; at batch 1 a launch is its fixed
    cost).  Results == nbt1d_eval."""
    return tuple(_nbt1d_eval([xa, xb], [ra, rb]))


# ---------------------------------------------------------------------------------------------
# conv + BN (+ReLU)
# ---------------------------------------------------------------------------------------------
class ConvBNActFunction(Function):
    @staticmethod
    def forward(ctx, x, crt, brt, act, weight, gamma, beta):
        x = Fn.as_act(x)
        out, y, mean, invstd, mask, _ = _conv_bn_forward(x, crt, brt, act)
        if act == ACT_RELU:
            _trace_mask('conv_bn_act', out)
        ctx.crt, ctx.brt, ctx.act = crt, brt, act
        ctx.save_for_backward(x)
        ctx.saved = (y, mean, invstd, mask)
        ctx.bn_train = brt.batch_stats()
        return out

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        y, mean, invstd, mask = ctx.saved
        ctx.saved = None
        dout = Fn.as_act(dout, dense=True)
        dy, _, dg, db = Fn.bn_bwd(dout, mask, y, ctx.brt.bn.weight.detach(), mean, invstd, None,
                                  ctx.act, ctx.bn_train, want_dres=False, **_bn_targets(ctx.brt))
        dx, dw, _, _ = _conv_backward(x, dy, ctx.crt, ctx.needs_input_grad[0])
        return dx, None, None, None, dw, dg, db


class ConvBNAddActFunction(Function):
    """act(bn(conv(x)) + residual): the closing conv of a basic / bottleneck ResNet block"""

    @staticmethod
    def forward(ctx, x, residual, crt, brt, act, weight, gamma, beta):
        x, residual = Fn.as_act(x), Fn.as_act(residual, dense=True)
        out, y, mean, invstd, mask, _ = _conv_bn_forward(x, crt, brt, act, residual=residual)
        if act == ACT_RELU:
            _trace_mask('conv_bn_add_act', out)
        ctx.crt, ctx.brt, ctx.act = crt, brt, act
        ctx.save_for_backward(x)
        ctx.saved = (y, mean, invstd, mask)
        ctx.bn_train = brt.batch_stats()
        return out

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        y, mean, invstd, mask = ctx.saved
        ctx.saved = None
        dout = Fn.as_act(dout, dense=True)
        dy, dres, dg, db = Fn.bn_bwd(dout, mask, y, ctx.brt.bn.weight.detach(), mean, invstd, None,
                                     ctx.act, ctx.bn_train, want_dres=ctx.needs_input_grad[1],
                                     **_bn_targets(ctx.brt))
        dx, dw, _, _ = _conv_backward(x, dy, ctx.crt, ctx.needs_input_grad[0])
        return dx, dres, None, None, None, dw, dg, db


def conv_bn_act_eval(x, crt, brt, act, residual=None):
    s, t = brt.folded()
    return crt.forward(x, scale=s, shift=t, act=act, residual=residual)


# ---------------------------------------------------------------------------------------------
# plain conv (+bias) whose packed weight may host several parameters (padding / block-diagonal)
# ---------------------------------------------------------------------------------------------
class MultiConvRT:
    """One GEMM-level convolution assembled from several nn.Conv2d / nn.Linear parameters.
    `placements` = [(module, cout_off, cin_off)], total (cout_total, cin_total) multiples of 4."""

    def __init__(self, placements, cout_total, cin_total, kernel, padding):
        self.placements = placements
        self.spec = Fn.ConvSpec(cin_total, cout_total, kernel, 1, padding)
        self.has_bias = any(m.bias is not None for m, _, _ in placements)
        # 3x3 stride-1 merged convs (the task heads) run on the Winograd kernel as well
        self.wino = Fn.wino_enabled(self.spec)
        # merged 3x3 heads the per-shape rule sends to the 2-D Winograd kernel: U2 beside the row form
        self.wino2d = self.wino and Fn.wino2d_selected(self.spec)
        self.packs = _PackCache()     # the forms of `forms`

    def forms(self, dtype):
        """the forms this conv keeps for activations of `dtype`: 'gemm' the assembled [tap][n][k]
        operands (16-bit, and fp32 without the Winograd form) or 'wino' U and, per-shape rule, 'wino2d'
        U2 (fp32); 'bias' the assembled fp32 bias vector (forward side only).  A Winograd head that
        packs by itself makes U and U2 from its fp32 'gemm' operands: a form no job of PackPlan makes"""
        s = self.spec
        n = s.kh * s.kw * s.cout * s.cin
        fs = _weight_forms(self, n, dtype)
        if fs[0].name == 'wino':
            fs.insert(0, _Form('gemm', None, torch.float32, n, n, False))
        if self.has_bias:
            fs.append(_Form('bias', _lib.PACK_COPY, torch.float32, s.cout, 0, False))
        return fs

    def _w4(self, m):
        w = m.weight
        return w if w.dim() == 4 else w[:, :, None, None]

    def key_now(self):
        return tuple((m.weight._version, m.weight.data_ptr(),
                      m.bias._version if m.bias is not None else 0) for m, _, _ in self.placements)

    def _bias_vec(self):
        bias = torch.zeros(self.spec.cout, device=self.placements[0][0].weight.device,
                           dtype=torch.float32)
        for m, co, _ in self.placements:
            if m.bias is not None:
                bias[co:co + m.bias.shape[0]].copy_(m.bias.detach())
        return bias

    def _assemble(self, side, dtype):
        """forward [tap][cout][cin] (side 0) / data-gradient [tap][cin][cout] (side 1) operand, fp32 or
        16-bit.  It starts as zeros: the padding channels and whatever lies between the placements
        belong to no parameter, and the kernels read them like any other weight"""
        s = self.spec
        wp = Fn._zeros((s.kh * s.kw * s.cout * s.cin,), self.placements[0][0].weight.device, dtype)
        for m, co, ci in self.placements:
            if dtype == torch.float32:
                Fn.pack_weight(self._w4(m).detach(), 'dgrad' if side else 'fwd', s.cout, co, s.cin, ci,
                               out=wp)
            else:
                Fn.pack_weight_t(self._w4(m).detach(), dtype, not side, bool(side), s.cout, co, s.cin, ci,
                                 out_fwd=None if side else wp, out_dgrad=wp if side else None)
        return wp

    def _pack(self, form, dtype, fwd, dgrad):
        s = self.spec
        if form == 'bias':
            return self._bias_vec(), None
        if form == 'gemm':
            return (self._assemble(0, dtype) if fwd else None,
                    self._assemble(1, dtype) if dgrad else None)
        # U / U2 from the CACHED assembled operands: one assembly serves both
        if form == 'wino':
            rows = Fn.wino_rows(s)
            return (Fn.pack_wino_packed(self.weights('gemm', 0), s.cout, s.cin, rows, flip=False)
                    if fwd else None,
                    Fn.pack_wino_packed(self.weights('gemm', 1), s.cin, s.cout, rows, flip=True)
                    if dgrad else None)
        return (Fn.pack_wino2d_packed(self.weights('gemm', 0), s.cout, s.cin, flip=False)
                if fwd else None,
                Fn.pack_wino2d_packed(self.weights('gemm', 1), s.cin, s.cout, flip=True)
                if dgrad else None)

    def weights(self, form, side, dtype=torch.float32):
        """the forward (side 0) / data-gradient (side 1) operand of `form`: PackPlan's when fresh,
        else re-packed -- the operands are rebuilt only when a parameter moved, and one side at a
        time (a zero-fill and 2-4 small kernels per head and side)"""
        return self.packs.get(form, dtype, side, self.key_now(),
                              lambda fwd, dgrad: self._pack(form, dtype, fwd, dgrad), False)

    def _operands(self, side, dtype):
        """(wp, keyword arguments) of Fn.conv_fwd (side 0) / Fn.conv_dgrad (side 1) that hand over
        this conv's operands for activations of `dtype`"""
        if dtype != torch.float32 or not self.wino:
            return self.weights('gemm', side, dtype), {}
        operands = {'wino_u': self.weights('wino', side)}
        if self.wino2d:
            operands['wino2d_u'] = self.weights('wino2d', side)
        return None, operands

    def forward(self, x):
        Fn.prof_flops(self.real_flops(x))
        bias = self.weights('bias', 0) if self.has_bias else None
        wp, operands = self._operands(0, x.dtype)
        return Fn.conv_fwd(x, wp, self.spec, bias=bias, **operands)

    def real_flops(self, x):
        """direct-convolution FLOPs of the REAL (un-padded, un-merged) convolutions on `x`"""
        n, _, h, w = x.shape
        return 2.0 * n * h * w * sum(m.weight.numel() for m, _, _ in self.placements)

    def dgrad(self, dy, in_hw):
        Fn.prof_flops(self.real_flops(dy))
        wp, operands = self._operands(1, dy.dtype)
        return Fn.conv_dgrad(dy, wp, self.spec, in_hw, **operands)

    def params(self):
        ps = []
        for m, _, _ in self.placements:
            ps.append(m.weight)
            if m.bias is not None:
                ps.append(m.bias)
        return ps


class MultiConvFunction(Function):
    @staticmethod
    def forward(ctx, x, rt, *params):
        x = Fn.as_act(x)
        y = rt.forward(x)
        ctx.rt = rt
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        rt = ctx.rt
        (x,) = ctx.saved_tensors
        dy = Fn.as_act(dy)
        s = rt.spec
        Fn.prof_flops(rt.real_flops(x))
        if GRAD_TRACE is not None:
            for m, co, _ in rt.placements:            # (merged convs: each module's own channels)
                _trace_grad(m, dy[:, co:co + m.weight.shape[0]])
        dwp, db, _ = Fn.conv_wgrad(x, dy, s, rt.has_bias)
        grads = []
        for m, co, ci in rt.placements:
            w4 = rt._w4(m)
            tw = grad_target(m.weight)
            dw = Fn.unpack_wgrad(dwp, w4, s.cout, co, s.cin, ci,
                                 out=tw.view(w4.shape) if tw is not None else None)
            grads.append(tw if tw is not None else dw.reshape(m.weight.shape))
            if m.bias is not None:
                grads.append(db[co:co + m.bias.shape[0]].clone())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = rt.dgrad(dy, x.shape[2:])
        return (dx, None) + tuple(grads)


# ---------------------------------------------------------------------------------------------
# stem: 7x7/2 conv + BN + ReLU on the NCHW network input
# ---------------------------------------------------------------------------------------------
class StemRT:
    def __init__(self, conv, bn):
        self.conv, self.brt = conv, BNRT(bn)
        self.spec = Fn.StemSpec(conv.in_channels, conv.out_channels)
        self._packs = {}             # dtype -> (key, packed weights)

    def packed(self, dtype=torch.float32):
        w = self.conv.weight
        key = (w._version, w.data_ptr())
        ent = self._packs.get(dtype)
        if ent is None or ent[0] != key:
            ent = (key, Fn.stem_pack_weight(w.detach(), dtype))
            self._packs[dtype] = ent
        return ent[1]


class StemFunction(Function):
    @staticmethod
    def forward(ctx, x_nchw, rt, weight, gamma, beta, bias=None, dtype=torch.float32):
        n, c, h, w = x_nchw.shape
        xp = Fn.stem_pack_input(x_nchw.detach().float(), dtype)
        brt = rt.brt
        b = bias.detach() if bias is not None else None      # [U] Spec.STEM_BIAS
        wpk = rt.packed(dtype)
        if brt.batch_stats():
            y, stats = Fn.stem_fwd(xp, wpk, rt.spec, n, h, w, want_stats=True, bias=b)
            count = y.shape[0] * y.shape[2] * y.shape[3]
        else:
            y, _ = Fn.stem_fwd(xp, wpk, rt.spec, n, h, w, want_stats=False, bias=b)
            stats, count = None, 0
        scale, shift, mean, invstd = brt.forward_stats(stats, count)
        out, mask = Fn.bn_act(y, scale, shift, None, None, ACT_RELU, want_mask=True)
        _trace_mask('stem', out)
        ctx.rt = rt
        ctx.hw = (n, h, w)
        ctx.saved = (xp, y, mean, invstd, mask)
        ctx.bn_train = brt.batch_stats()
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dout):
        rt = ctx.rt
        xp, y, mean, invstd, mask = ctx.saved
        ctx.saved = None
        n, h, w = ctx.hw
        dout = Fn.as_act(dout, dense=True)
        dy, _, dg, db = Fn.bn_bwd(dout, mask, y, rt.brt.bn.weight.detach(), mean, invstd, None,
                                  ACT_RELU, ctx.bn_train, want_dres=False, **_bn_targets(rt.brt))
        _trace_grad(rt.conv, dy)
        res = Fn.stem_wgrad(xp, dy, rt.spec, n, h, w, rt.conv.weight,
                            out=grad_target(rt.conv.weight), want_bias=ctx.has_bias)
        dw, dbias = res if ctx.has_bias else (res, None)
        # gradient w.r.t. the network input is not produced (the reference never needs it:
        # /root/reference/main.py:597-599 back-propagates into parameters only)
        return None, None, dw, dg, db, dbias, None


def stem_eval(x_nchw, rt, dtype=torch.float32):
    n, c, h, w = x_nchw.shape
    xp = Fn.stem_pack_input(x_nchw.float(), dtype)
    s, t = rt.brt.folded()
    b = rt.conv.bias.detach() if rt.conv.bias is not None else None
    return Fn.stem_fwd_folded(xp, rt.packed(dtype), rt.spec, n, h, w, s, t, bias=b)


# ---------------------------------------------------------------------------------------------
# the stage behind the two stems as four passes (csrc/stem_stage.hip; dispatch: nn.FusedEncoder)
# ---------------------------------------------------------------------------------------------
class StemConvFunction(Function):
    """the convolution half of StemFunction: y and its BatchNorm statistics rows forward, the weight
    gradient from dy backward.  One per stream, so the two stem convolutions and their weight
    gradients stay on their two HIP streams; everything between y and layer1 is StemStageFunction."""

    @staticmethod
    def forward(ctx, x_nchw, rt, weight, bias=None, dtype=torch.float32):
        n, c, h, w = x_nchw.shape
        xp = Fn.stem_pack_input(x_nchw.detach().float(), dtype)
        b = bias.detach() if bias is not None else None      # [U] Spec.STEM_BIAS
        y, stats = Fn.stem_fwd(xp, rt.packed(dtype), rt.spec, n, h, w, want_stats=True, bias=b)
        ctx.rt, ctx.hw, ctx.xp, ctx.has_bias = rt, (n, h, w), xp, bias is not None
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)      # (no zeros tensor for the statistics rows)
        return y, stats

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy, _dstats):
        rt, xp = ctx.rt, ctx.xp
        ctx.xp = None
        n, h, w = ctx.hw
        dy = Fn.as_act(dy, dense=True)
        _trace_grad(rt.conv, dy)
        res = Fn.stem_wgrad(xp, dy, rt.spec, n, h, w, rt.conv.weight,
                            out=grad_target(rt.conv.weight), want_bias=ctx.has_bias)
        dw, dbias = res if ctx.has_bias else (res, None)
        return None, None, dw, dbias, None


class StemStageFunction(Function):
    """(y_rgb, y_depth) -> (maxpool(a_rgb * SE_rgb + a_depth * SE_depth), maxpool(a_depth)) with
    a = relu(BatchNorm(y)), batch statistics: what StemFunction's BatchNorm half, SEAddFunction and
    two MaxPoolFunctions compute, in two passes over y forward and two backward.  Saved for the
    backward pass: y_rgb, y_depth, the two argmax maps and per-channel / per-image vectors."""

    @staticmethod
    def forward(ctx, y_rgb, stats_rgb, y_depth, stats_depth, rt_rgb, rt_depth, gamma_r, beta_r,
                gamma_d, beta_d, w1r, b1r, w2r, b2r, w1d, b1d, w2d, b2d):
        y_rgb, y_depth = Fn.as_act(y_rgb, dense=True), Fn.as_act(y_depth, dense=True)
        n, c, h, w = y_rgb.shape
        aff, st = [], []
        for rt, stats in ((rt_rgb, stats_rgb), (rt_depth, stats_depth)):
            scale, shift, mean, invstd = rt.brt.forward_stats(stats, n * h * w)
            aff.append((scale, shift))
            st.append((mean, invstd))
        if MASK_TRACE is not None:            # (tests: the activations exist for the trace only)
            for y, (scale, shift) in zip((y_rgb, y_depth), aff):
                _trace_mask('stem', Fn.bn_act(y, scale, shift, None, None, ACT_RELU))
        flat = lambda t: t.detach().reshape(t.shape[0], -1)   # noqa: E731
        gr, gd, hr, hd, sr, sd = Fn.stem_stage_se(
            y_rgb, y_depth, aff[0], aff[1], (flat(w1r), b1r.detach(), flat(w2r), b2r.detach()),
            (flat(w1d), b1d.detach(), flat(w2d), b2d.detach()))
        _trace_mask('se.rgb', hr)
        _trace_mask('se.depth', hd)
        pf, idx_f, pd, idx_d = Fn.stem_stage_fwd(y_rgb, y_depth, aff[0], aff[1], sr, sd)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y_rgb, y_depth)
        ctx.rts = (rt_rgb, rt_depth)
        ctx.saved = (idx_f, idx_d, aff, st, (gr, hr, sr, flat(w1r), flat(w2r)),
                     (gd, hd, sd, flat(w1d), flat(w2d)))
        ctx.shapes = (w1r.shape, w2r.shape)
        return pf, pd

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, g_f, g_d):
        y_rgb, y_depth = ctx.saved_tensors
        idx_f, idx_d, aff, st, se_r, se_d = ctx.saved
        ctx.saved = None
        rt_rgb, rt_depth = ctx.rts
        n, c, h, w = y_rgb.shape
        pooled = (n, (h + 1) // 2, (w + 1) // 2, c)

        def grad(g):                     # (an unused output arrives as None)
            if g is None:
                return torch.zeros(pooled, device=y_rgb.device).permute(0, 3, 1, 2)
            g = Fn.as_act(g, dense=True)
            return g if g.dtype == torch.float32 else Fn.cast(g, torch.float32)
        g_f, g_d = grad(g_f), grad(g_d)
        sums, ds_r, ds_d = Fn.stem_stage_bwd_reduce(g_f, idx_f, g_d, idx_d, y_rgb, y_depth, aff[0],
                                                    aff[1], st[0], st[1])
        s1, s2 = ctx.shapes
        se_grads, dgaps = [], []
        for (gap, hid, s, w1, w2), ds in ((se_r, ds_r), (se_d, ds_d)):
            dgap, dw1, db1, dw2, db2 = Fn.se_mlp_bwd(gap, w1, w2, hid, s, ds)
            dgaps.append(dgap)
            se_grads += [dw1.reshape(s1), db1, dw2.reshape(s2), db2]
        tr, td = _bn_targets(rt_rgb.brt), _bn_targets(rt_depth.brt)
        dgb = Fn.stem_stage_bwd_finalize(
            sums, h * w, se_r[2], se_d[2], dgaps[0], dgaps[1],
            (tr.get('dg_out'), tr.get('db_out')), (td.get('dg_out'), td.get('db_out')))
        dy_rgb, dy_depth = Fn.stem_stage_bwd_apply(
            g_f, idx_f, g_d, idx_d, y_rgb, y_depth, aff[0], aff[1], st[0], st[1],
            rt_rgb.brt.bn.weight.detach(), rt_depth.brt.bn.weight.detach(), se_r[2], se_d[2],
            dgaps[0], dgaps[1], dgb)
        return (dy_rgb, None, dy_depth, None, None, None, dgb[0], dgb[1], dgb[2], dgb[3], *se_grads)


# ---------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------
class MaxPoolFunction(Function):
    @staticmethod
    def forward(ctx, x):
        x = Fn.as_act(x, dense=True)
        y, idx = Fn.maxpool_fwd(x)
        ctx.idx, ctx.hw = idx, tuple(x.shape[2:])
        return y

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        return Fn.maxpool_bwd(Fn.as_act(dy, dense=True), ctx.idx, ctx.hw)


# ---------------------------------------------------------------------------------------------
# SE-add fusion
# ---------------------------------------------------------------------------------------------
# EMSA_SE_PAIR=0: the squeeze / excitation of the two inputs of an SE-add fusion as separate launches
SE_PAIR = os.environ.get('EMSA_SE_PAIR', '1') != '0'


def _se_params(se):
    f0, f2 = se.fc[0], se.fc[2]
    return [f0.weight, f0.bias, f2.weight, f2.bias]


class SEAddFunction(Function):
    """out = rgb * SE_rgb(rgb) + depth * SE_depth(depth)   ('se-add-uni-rgb'), and the depth stream
    handed on as a second output.  The depth stream has TWO consumers -- this fusion and the next
    depth stage -- so autograd used to add their two gradients with a torch kernel per stage (the
    largest one on the 629 MB stem output: 0.33 ms).  With the pass-through output this Function is
    the depth tensor's only consumer: the next stage's gradient arrives as `ddepth_next` and is
    added inside the SE backward kernel (`dx_extra` of emsa_se_scale_bwd_apply), one extra read
    instead of a read-read-write pass."""

    @staticmethod
    def forward(ctx, rgb, depth, w1r, b1r, w2r, b2r, w1d, b1d, w2d, b2d):
        rgb, depth = Fn.as_act(rgb, dense=True), Fn.as_act(depth, dense=True)
        flat = lambda w: w.detach().reshape(w.shape[0], -1)   # noqa: E731
        if SE_PAIR:
            # both squeezes in one launch, both excitation MLPs in one (7 launches -> 3 per fusion)
            gr, gd, hr, hd, sr, sd = Fn.se_pair_fwd(
                rgb, depth, (flat(w1r), b1r.detach(), flat(w2r), b2r.detach()),
                (flat(w1d), b1d.detach(), flat(w2d), b2d.detach()))
        else:
            gr, gd = Fn.channel_mean(rgb), Fn.channel_mean(depth)
            hr, sr = Fn.se_mlp_fwd(gr, flat(w1r), b1r.detach(), flat(w2r), b2r.detach())
            hd, sd = Fn.se_mlp_fwd(gd, flat(w1d), b1d.detach(), flat(w2d), b2d.detach())
        _trace_mask('se.rgb', hr)
        _trace_mask('se.depth', hd)
        out = Fn.se_scale_add(rgb, sr, depth, sd)
        # an unused pass-through depth output (last stage, cut boundaries) arrives as None in
        # backward instead of a materialised zeros tensor + one more read in the kernel
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(rgb, depth)
        ctx.saved = (gr, gd, hr, sr, hd, sd, flat(w1r), flat(w2r), flat(w1d), flat(w2d))
        ctx.shapes = (w1r.shape, w2r.shape)
        return out, depth[:]              # (an alias: same memory, this node as its grad_fn)

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dout, ddepth_next):
        rgb, depth = ctx.saved_tensors
        gr, gd, hr, sr, hd, sd, w1r, w2r, w1d, w2d = ctx.saved
        ctx.saved = None
        if dout is None:                     # (only the pass-through output was used downstream)
            dout = torch.zeros_like(rgb)
        dout = Fn.as_act(dout, dense=True)
        if ddepth_next is not None:
            ddepth_next = Fn.as_act(ddepth_next, dense=True)
            if ddepth_next.dtype != dout.dtype:
                ddepth_next = Fn.cast(ddepth_next, dout.dtype)
        s1, s2 = ctx.shapes
        res = []
        for x, g, h, s, w1, w2, extra in ((rgb, gr, hr, sr, w1r, w2r, None),
                                          (depth, gd, hd, sd, w1d, w2d, ddepth_next)):
            ds = Fn.se_scale_bwd_reduce(dout, x)
            dgap, dw1, db1, dw2, db2 = Fn.se_mlp_bwd(g, w1, w2, h, s, ds)
            dx = Fn.se_scale_bwd_apply(dout, s, dgap, extra)
            res.append((dx, dw1.reshape(s1), db1, dw2.reshape(s2), db2))
        (dr, a1, a2, a3, a4), (dd, e1, e2, e3, e4) = res
        return dr, dd, a1, a2, a3, a4, e1, e2, e3, e4


# ---------------------------------------------------------------------------------------------
# learned upsampling (nearest x2 + depth-wise 3x3) with optional fused skip add
# ---------------------------------------------------------------------------------------------
class UpsampleDWFunction(Function):
    """`wdw`/`bias` are the (possibly zero-padded) [c,1,3,3] / [c] tensors the kernel reads.
    out_f32: the result is written as fp32 from 16-bit features (the last up-sampling of a head
    produces the model's fp32 output directly; its cotangent arrives as fp32 too)."""

    @staticmethod
    def forward(ctx, x, wdw, bias, skip, out_f32=False):
        x = Fn.as_act(x, dense=True)
        if skip is not None:
            skip = Fn.as_act(skip, dense=True)
        w = wdw.detach().contiguous()
        y = Fn.up2x_dw_fwd(x, w, bias.detach() if bias is not None else None, skip,
                           out_f32=out_f32 and x.dtype != torch.float32)
        ctx.save_for_backward(x, w)
        ctx.has = (bias is not None, skip is not None)
        ctx.wshape = wdw.shape
        return y

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = Fn.as_act(dy, dense=True)
        dx, dw, db = Fn.up2x_dw_bwd(dy, x, w, need_dx=ctx.needs_input_grad[0])
        has_bias, has_skip = ctx.has
        dskip = None
        if has_skip:
            dskip = dy if dy.dtype == x.dtype else Fn.cast(dy, x.dtype)
        return dx, dw.reshape(ctx.wshape), (db if has_bias else None), dskip, None


class SkipUpsampleFunction(Function):
    """up2x(x) + relu(bn(conv1x1(skip))) of a decoder module with the skip path's BatchNorm + ReLU
    formed inside the up-sampler (Fn.skip_fold): what ConvBNActFunction followed by
    UpsampleDWFunction computes, bit for bit, without the activation and its ReLU bit mask in memory.
    Batch statistics, fp32.  Saved for the backward pass: x, skip, the conv output y and per-channel
    vectors."""

    @staticmethod
    def forward(ctx, x, skip, crt, brt, wdw, bias, weight, gamma, beta):
        x, skip = Fn.as_act(x, dense=True), Fn.as_act(skip)
        cb = crt.conv.bias.detach() if crt.conv.bias is not None else None
        y, stats = crt.forward(skip, bias=cb, want_stats=True)
        scale, shift, mean, invstd = brt.forward_stats(stats, y.shape[0] * y.shape[2] * y.shape[3])
        if MASK_TRACE is not None:            # (tests: the activation exists for the trace only)
            _trace_mask('conv_bn_act', Fn.bn_act(y, scale, shift, None, None, ACT_RELU))
        w = wdw.detach().contiguous()
        out = Fn.up2x_dw_fwd_skipbn(x, w, bias.detach() if bias is not None else None, y, scale, shift)
        ctx.crt, ctx.brt = crt, brt
        ctx.save_for_backward(x, w, skip)
        ctx.saved = (y, scale, shift, mean, invstd)
        ctx.has_bias, ctx.wshape = bias is not None, wdw.shape
        return out

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        x, w, skip = ctx.saved_tensors
        y, scale, shift, mean, invstd = ctx.saved
        ctx.saved = None
        dy = Fn.as_act(dy, dense=True)
        dx, dw, db = Fn.up2x_dw_bwd(dy, x, w, need_dx=ctx.needs_input_grad[0])
        # the up-sampler's cotangent is the skip activation's: bn backward with the ReLU decisions
        # recomputed from y, then the 1x1 conv's gradients
        dyk, dg, dbeta = Fn.bn_bwd_aff(dy, y, ctx.brt.bn.weight.detach(), mean, invstd,
                                       (scale, shift), **_bn_targets(ctx.brt))
        dskip, dwc, _, _ = _conv_backward(skip, dyk, ctx.crt, ctx.needs_input_grad[1])
        return (dx, dskip, None, None, dw.reshape(ctx.wshape), db if ctx.has_bias else None, dwc,
                dg, dbeta)


class PlainUpsampleFunction(Function):
    """x2 up-sampling without weights -- 'nearest' / 'bilinear' (align_corners=False) of
    `--{semantic,instance,normal}-decoder-upsampling` / `--upsampling-prediction`
    (/root/reference/emsanet/args.py:280-298,363-372) -- plus the optional skip add; out_f32 as in
    UpsampleDWFunction (16-bit features -> the model's fp32 output)."""

    @staticmethod
    def forward(ctx, x, mode, skip, out_f32=False):
        if mode not in ('bilinear', 'nearest'):
            raise NotImplementedError(f"upsampling '{mode}'")
        x = Fn.as_act(x, dense=True)
        ctx.mode, ctx.x_dtype, ctx.hw = mode, x.dtype, tuple(x.shape[2:])
        if out_f32 and x.dtype != torch.float32:
            x = Fn.cast(x, torch.float32)
        n, c, h, w = x.shape
        y = Fn.act_empty(n, c, 2 * h, 2 * w, x.device, dtype=x.dtype)
        (Fn.bilinear_fwd if mode == 'bilinear' else Fn.nearest_fwd)(x, y)
        ctx.has_skip = skip is not None
        if skip is not None:
            skip = Fn.as_act(skip, dense=True)
            y = Fn.add(y, skip if skip.dtype == y.dtype else Fn.cast(skip, y.dtype))
        return y

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        dy = Fn.as_act(dy, dense=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (Fn.bilinear_bwd if ctx.mode == 'bilinear' else Fn.nearest_bwd)(dy, ctx.hw)
            if dx.dtype != ctx.x_dtype:
                dx = Fn.cast(dx, ctx.x_dtype)
        dskip = None
        if ctx.has_skip:
            dskip = dy if dy.dtype == ctx.x_dtype else Fn.cast(dy, ctx.x_dtype)
        return dx, None, dskip, None


# ---------------------------------------------------------------------------------------------
# pyramid pooling pieces
# ---------------------------------------------------------------------------------------------
class AdaptiveAvgPoolFunction(Function):
    @staticmethod
    def forward(ctx, x, bins):
        x = Fn.as_act(x, dense=True)
        ctx.bins, ctx.shape = bins, tuple(x.shape)
        return Fn.adaptive_avgpool_fwd(x, bins)

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dy):
        n, c, h, w = ctx.shape
        dy = Fn.as_act(dy, dense=True)
        dx = Fn.act_empty(n, c, h, w, dy.device, dtype=dy.dtype)
        Fn.adaptive_avgpool_bwd(dy, dx, ctx.bins, accumulate=False)
        return dx, None


class PPMConcatFunction(Function):
    """cat([x, up(y_i) ...], dim=1) written straight into one NHWC buffer; up = bilinear
    (align_corners=False) or -- a trailing 'nearest' argument -- nearest, the two choices of
    `--upsampling-context-module` (/root/reference/emsanet/args.py:250-256)."""

    @staticmethod
    def forward(ctx, x, *ys):
        mode = 'bilinear'
        if ys and isinstance(ys[-1], str):
            mode, ys = ys[-1], ys[:-1]
            ctx.has_mode = True
        else:
            ctx.has_mode = False
        if mode not in ('bilinear', 'nearest'):
            raise NotImplementedError(f"upsampling_context_module='{mode}'")
        up = Fn.bilinear_fwd if mode == 'bilinear' else Fn.nearest_fwd
        x = Fn.as_act(x)
        ys = [Fn.as_act(y, dense=True) for y in ys]
        n, c, h, w = x.shape
        total = c + sum(y.shape[1] for y in ys)
        buf = Fn.act_empty(n, total, h, w, x.device, dtype=x.dtype)
        Fn.copy_channels(x, buf[:, :c])
        off = c
        for y in ys:
            up(y, buf[:, off:off + y.shape[1]])
            off += y.shape[1]
        ctx.meta = (c, [tuple(y.shape) for y in ys], mode)
        return buf

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, dbuf):
        dbuf = Fn.as_act(dbuf)
        c, yshapes, mode = ctx.meta
        down = Fn.bilinear_bwd if mode == 'bilinear' else Fn.nearest_bwd
        n, _, h, w = dbuf.shape
        dx = Fn.act_empty(n, c, h, w, dbuf.device, dtype=dbuf.dtype)
        Fn.copy_channels(dbuf[:, :c], dx)
        off, dys = c, []
        for ys in yshapes:
            dys.append(down(dbuf[:, off:off + ys[1]], ys[2:]))
            off += ys[1]
        return (dx,) + tuple(dys) + ((None,) if ctx.has_mode else ())


# ---------------------------------------------------------------------------------------------
# head activations
# ---------------------------------------------------------------------------------------------
class HeadActFunction(Function):
    """sigmoid / tanh (/ L2 normalisation of the orientation pair) on the leading channels of the
    (channel-padded) instance head output and the split into the task tensors.  The outputs are
    channel-slice VIEWS of one activated tensor; backward gathers their gradients into one padded
    tensor with strided channel copies -- slicing outside (autograd's SliceBackward) materialised
    a zero-filled full-size tensor per task and added them up: three fills, three copies and two
    adds of the 315 MB full-resolution tensor."""

    @staticmethod
    def forward(ctx, x, n_sig, n_tanh, sizes, n_norm=0):
        x = Fn.as_act(x, dense=True)
        y = Fn.head_act_fwd(x, n_sig, n_tanh, n_norm)
        ctx.save_for_backward(y, x if n_norm else None)
        ctx.cfg = (n_sig, n_tanh, n_norm)
        ctx.dtype = x.dtype
        ctx.sizes = tuple(sizes)
        outs, o = [], 0
        for sz in sizes:
            outs.append(y[:, o:o + sz])
            o += sz
        return tuple(outs)

    @staticmethod
    @once_differentiable
    @_traced
    def backward(ctx, *dys):
        y, x = ctx.saved_tensors
        n, c, h, w = y.shape
        # the three task gradients are gathered INSIDE the backward kernel (round 5: the padded
        # 8-channel gradient tensor -- 315 MB at bs 32 -- is no longer written and read again)
        dx = Fn.head_act_bwd_gather(dys, ctx.sizes, y, *ctx.cfg, x=x, dtype=ctx.dtype)
        if dx is not None:
            return dx, None, None, None, None
        dy = Fn.act_empty(n, c, h, w, y.device)
        o = 0
        for sz, g in zip(ctx.sizes, dys):
            Fn.copy_channels(Fn.as_act(g.float()), dy[:, o:o + sz])
            o += sz
        if o < c:
            dy[:, o:].zero_()                      # padding channels carry no gradient
        return Fn.head_act_bwd(dy, y, *ctx.cfg, x=x, dtype=ctx.dtype), None, None, None, None


# ---------------------------------------------------------------------------------------------
# storage-type boundary: small 16-bit tensors leave the engine as fp32 (side outputs, scene logits)
# ---------------------------------------------------------------------------------------------
class CastFunction(Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return Fn.cast(x, dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return Fn.cast(dy, ctx.src), None


def to_float(x):
    """fp32 view of an engine tensor (identity for the fp32 engine)"""
    return x if x.dtype == torch.float32 else CastFunction.apply(x, torch.float32)
