# -*- coding: utf-8 -*-
"""
ORACLE -- TEST INFRASTRUCTURE ONLY.  PARITY PINNED for the loss weighting and the optimizer /
schedule (both restated from the reference's own sources); the per-scale reduction of the
multi-scale losses is [U].

One training step of the reference (`RunHelper.training_step`, /root/reference/main.py:121-152)
in plain PyTorch, any dtype, on the raw output list of `EMSANetOracle.forward` in train mode:

* every task helper's losses, composed from the existing oracle pieces: `semantic_ce` /
  `smoothed_ce` for the semantic decoder (class weights, `--semantic-loss-label-smoothing`),
  `smoothed_ce` for the scene head (`--scene-loss-label-smoothing`, no class weights), and
  `instance_losses` for the centre / offset / orientation outputs;
* multi-scale supervision (`--semantic-no-multiscale-supervision` / `--instance-no-multiscale-
  supervision`, emsanet/args.py:731,757): the side outputs /32, /16, /8 are supervised like the
  full-resolution output, each against the target of its own size;     [Spec.SCALE_REDUCTION]
* the fixed loss weighting of emsanet/loss_weighting.py:15-49, restated in `loss_weights`:
  orientation keeps its own task weight; the instance task weight is multiplied into the
  (centre, offset) pair of `--instance-weighting`; every other task keeps its weight;
* `FixedLossWeighting.reduce_losses`: total = sum of weight x loss over the weighted losses.

`make_optimizer` is the reference's optimizer and schedule: torch.optim.SGD(nesterov=True)
(emsanet/optimizer.py:29-36) under torch.optim.lr_scheduler.OneCycleLR configured as in
emsanet/lr_scheduler.py:23-31 (momentum cycling left on, as the reference leaves it).

`synthetic_targets` makes deterministic targets of every supervised size from the INPUTS (a
fixed random projection of each RGB-D pixel, bucketed), so that a training loop has something
to learn; `OracleTrainer` runs the oracle's side of a training loop.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from oracle.instance_loss_oracle import instance_losses, smoothed_ce
from oracle.semantic_loss_oracle import semantic_ce


class Spec:
    # [U] a multi-scale task loss is the SUM of its per-scale losses (the task helpers live in
    # the un-vendored nicr_mt_scene_analysis library); 'mean' would divide by the scale count
    SCALE_REDUCTION = 'sum'
    SIDE_DOWNSCALES = (32, 16, 8)      # order of the side outputs (decoder module order)


def loss_weights(args):
    """flat per-loss weights from the task weights (emsanet/loss_weighting.py:15-49)"""
    assert len(args.tasks) == len(args.tasks_weighting)              # loss_weighting.py:17
    task_w = dict(zip(args.tasks, args.tasks_weighting))             # :18-21
    w = {}
    if 'orientation' in args.tasks:                                  # :28-30
        w['instance_orientation'] = task_w.pop('orientation')
    if 'instance' in args.tasks:                                     # :33-42
        w_instance = task_w.pop('instance')
        w_center, w_offset = args.instance_weighting
        w['instance_center'] = w_instance * w_center
        w['instance_offset'] = w_instance * w_offset
    w.update(task_w)                                                 # :45-48
    return w


def _reduce_scales(values):
    s = torch.stack(list(values)).sum()
    return s if Spec.SCALE_REDUCTION == 'sum' else s / len(values)


def training_losses(outputs, targets, args, semantic_class_weights, n_scene_classes):
    """outputs: the list `EMSANetOracle.forward(batch)` returns in train mode (decoder order
    semantic, instance, scene; each (full, side outputs) with side outputs /32, /16, /8).
    targets: {'semantic': [full, /32, /16, /8] (N,H,W) int 0 = void, 'instance': [dict(center,
    offset, foreground, orientation, orientation_foreground)] per scale alike, 'scene': (N,) int
    0 = void}.  -> (total, {loss name: unweighted loss summed over the supervised scales})"""
    tasks = tuple(args.tasks)
    it = iter(outputs)
    losses = {}
    if 'semantic' in tasks:
        full, side = next(it)
        xs = [full] + (list(side) if not args.semantic_no_multiscale_supervision else [])
        eps = args.semantic_loss_label_smoothing
        w = torch.as_tensor(semantic_class_weights, dtype=full.dtype)
        per_scale = [semantic_ce(x, t, w) if eps == 0.0 else smoothed_ce(x, t, w, eps)
                     for x, t in zip(xs, targets['semantic'])]
        assert len(per_scale) == len(xs)
        losses['semantic'] = _reduce_scales(per_scale)
    if 'instance' in tasks:
        full, side = next(it)
        preds = [full] + (list(side) if not args.instance_no_multiscale_supervision else [])
        per_scale = {}
        for pred, tgt in zip(preds, targets['instance']):
            orient = pred[2] if 'orientation' in tasks else None
            r = instance_losses(pred[0], pred[1], orient, tgt['center'], tgt['offset'],
                                tgt['foreground'], tgt.get('orientation'),
                                tgt.get('orientation_foreground'), tgt.get('center_mask'),
                                kappa=args.orientation_kappa)
            for k, v in r.items():
                per_scale.setdefault(k, []).append(v)
        for k, v in per_scale.items():
            assert len(v) == len(preds)
            losses[k] = _reduce_scales(v)
    if 'scene' in tasks:
        logits = next(it)[0]
        ones = torch.ones(n_scene_classes, dtype=logits.dtype)
        losses['scene'] = smoothed_ce(logits, targets['scene'], ones,
                                      args.scene_loss_label_smoothing)
    weights = loss_weights(args)
    assert set(weights) == set(losses), (sorted(weights), sorted(losses))
    total = sum(weights[k] * losses[k] for k in weights)            # FixedLossWeighting
    return total, losses


def synthetic_targets(batch, n_classes, n_scene, scales=(1,) + Spec.SIDE_DOWNSCALES, seed=7):
    """Deterministic targets of every supervised size, derived from the inputs (dict of 'rgb'
    (N,3,H,W) and 'depth' (N,1,H,W), CPU float): each scale's targets come from the inputs
    average-pooled to that size through the same fixed projections.
      * semantic: one projection bucketed into `n_classes` equally populated classes (edges from
        the full resolution), 0 = void where a second projection is in its lowest 10 %;
      * instance foreground = non-void pixels of the upper half of the classes, EMPTY for sample 1;
        centre heatmap in [0, 1], offsets in (-1, 1) on the foreground (0 elsewhere), orientation
        in (-pi, pi] labelled on part of the foreground;
      * scene: the mean projection of each image bucketed into 1..n_scene, 0 (void) for sample 0.
    -> {'semantic': [...], 'instance': [...], 'scene': (N,)} with float tensors float32"""
    x = torch.cat([batch['rgb'], batch['depth']], 1).double()
    n, c = x.shape[:2]
    assert n >= 2, "needs two samples (void scene label, empty instance foreground)"
    rng = np.random.default_rng(seed)
    proj = torch.from_numpy(rng.standard_normal((7, c)))
    off = torch.from_numpy(rng.standard_normal(7)) * 0.1

    def project(xs):
        return torch.einsum('kc,nchw->nkhw', proj, xs - 0.5) + off.view(1, -1, 1, 1)

    z = project(x)
    edges = torch.quantile(z[:, 0].flatten()[::7], torch.linspace(0, 1, n_classes + 1,
                                                                   dtype=torch.float64)[1:-1])
    void_edge = torch.quantile(z[:, 1].flatten()[::7], 0.1)
    sem, inst = [], []
    for s in scales:
        zs = project(F.avg_pool2d(x, s)) if s > 1 else z
        cls = torch.bucketize(zs[:, 0].contiguous(), edges) + 1            # 1..n_classes
        void = zs[:, 1] < void_edge
        cls = torch.where(void, torch.zeros_like(cls), cls)
        fg = (cls > n_classes // 2)
        fg[1] = False                                                       # no instance at all
        center = torch.exp(-zs[:, 2:3] ** 2)
        offset = torch.tanh(zs[:, 3:5]) * fg.unsqueeze(1)
        orient = torch.atan2(zs[:, 5], zs[:, 6])
        ofg = fg & (zs[:, 5] > -0.3)
        sem.append(cls)
        inst.append({'center': center.float(), 'offset': offset.float(), 'foreground': fg,
                     'orientation': orient.float(), 'orientation_foreground': ofg})
    m = z[:, 0].mean((1, 2))
    scene = (torch.argsort(torch.argsort(m)) % n_scene) + 1
    scene[0] = 0                                                            # void scene label
    return {'semantic': sem, 'instance': inst, 'scene': scene}


def targets_to(targets, device=None, dtype=None):
    """copy of `targets` with every tensor on `device` and every FLOAT tensor in `dtype`"""
    def cv(t):
        t = t.to(device) if device is not None else t
        return t.to(dtype) if (dtype is not None and t.is_floating_point()) else t
    return {'semantic': [cv(t) for t in targets['semantic']],
            'instance': [{k: cv(v) for k, v in d.items()} for d in targets['instance']],
            'scene': cv(targets['scene'])}


def make_optimizer(params, args, total_steps, nesterov=True):
    """(SGD, OneCycleLR) as the reference builds them (emsanet/optimizer.py:29-36,
    emsanet/lr_scheduler.py:23-31) with `total_steps` scheduler steps.  `params` may be a list of
    parameter groups (torch.optim convention)."""
    opt = torch.optim.SGD(params, lr=args.learning_rate, weight_decay=args.weight_decay,
                          momentum=args.momentum, nesterov=nesterov)
    sched = torch.optim.lr_scheduler.OneCycleLR(
        opt, max_lr=[g['lr'] for g in opt.param_groups], total_steps=total_steps, div_factor=25,
        pct_start=0.1, anneal_strategy='cos', final_div_factor=1e4)
    return opt, sched


class OracleTrainer:
    """the oracle's side of a training loop: forward (train mode), `training_losses`, backward,
    SGD step, then ONE scheduler step -- one step stands in for one of the reference's epochs, so
    that learning rate and momentum move within a short run.

    Deviations for the tests that show the gates have teeth: nesterov=False (plain momentum),
    decay_1d=False (no weight decay on 1-D tensors), advance_dropout=False (the Dropout2d masks of
    step 0 every step); loss / BatchNorm settings are changed on `args` / the model by the caller."""

    def __init__(self, model, args, semantic_class_weights, n_scene_classes, total_steps,
                 nesterov=True, decay_1d=True, advance_dropout=True):
        self.model, self.args = model, copy.copy(args)
        self.class_weights = semantic_class_weights
        self.n_scene = n_scene_classes
        self.advance_dropout = advance_dropout
        params = [p for p in model.parameters() if p.requires_grad]
        if decay_1d:
            groups = params
        else:
            groups = [{'params': [p for p in params if p.dim() > 1]},
                      {'params': [p for p in params if p.dim() <= 1], 'weight_decay': 0.0}]
        self.opt, self.sched = make_optimizer(groups, self.args, total_steps, nesterov=nesterov)

    def step(self, batch, targets, relu=None):
        """one training step; `relu`: replacement of torch.nn.functional.relu for the forward
        pass (mask pinning).  -> (total, per-loss dict), detached"""
        m = self.model
        m.train()
        self.opt.zero_grad(set_to_none=True)
        dropout_step = m.dropout_step
        saved = F.relu
        if relu is not None:
            F.relu = relu
        try:
            out = m(batch)
        finally:
            F.relu = saved
        if not self.advance_dropout:
            m.dropout_step = dropout_step
        total, losses = training_losses(out, targets, self.args, self.class_weights, self.n_scene)
        total.backward()
        self.opt.step()
        self.sched.step()
        return total.detach(), {k: v.detach() for k, v in losses.items()}
