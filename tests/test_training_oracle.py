"""CPU checks of the oracle side of a training step (oracle/training_oracle.py), which
tests/test_training_trajectory_gpu.py runs beside the engine's training loop:

* `training_losses` against values computed by hand on a tiny case: the weight of every task,
  the sum over the supervised scales, void pixels / void scene labels ignored, the multi-scale
  flags honoured;
* at label smoothing 0 its semantic term is `semantic_ce_multiscale`, which is pinned to the
  reference's own class through tests/golden/semantic_ce.npz;
* `synthetic_targets`: every supervised size, void pixels, one sample without instances, one void
  scene label, deterministic;
* the trajectory gates have teeth: the fp64 oracle's trajectory is run once as is and once per
  deliberate deviation (plain momentum, BatchNorm momentum 0.12, Dropout2d masks not advanced, no
  weight decay on 1-D tensors, instance weighting (1, 2), no scene label smoothing), and each
  deviation moves the quantity the GPU test gates by at least 10x that gate -- except the missing
  weight decay on 1-D tensors, which four steps of lr <= 1e-3 move by 6x (see DEVIATIONS).
"""
import copy
import math
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'semantic_ce.npz')
TASKS_WEIGHTING = (1.0, 0.25, 3.0, 0.5)


def _tiny_case():
    """two images of 2x3 pixels with one side output of 1x2; 3 semantic and 4 scene classes"""
    from emsanet_amd import full_args
    from oracle.training_oracle import targets_to
    g = torch.Generator().manual_seed(5)
    args = full_args(tasks_weighting=TASKS_WEIGHTING, instance_weighting=(2, 1),
                     scene_loss_label_smoothing=0.1)
    sizes = [(2, 3), (1, 2)]
    sem_out = [torch.randn(2, 3, h, w, generator=g, dtype=torch.float64) for h, w in sizes]
    inst_out = [(torch.rand(2, 1, h, w, generator=g, dtype=torch.float64),
                 torch.rand(2, 2, h, w, generator=g, dtype=torch.float64) * 2 - 1,
                 torch.randn(2, 2, h, w, generator=g, dtype=torch.float64)) for h, w in sizes]
    scene_out = torch.randn(2, 4, generator=g, dtype=torch.float64)
    outputs = [(sem_out[0], (sem_out[1],)), (inst_out[0], (inst_out[1],)), (scene_out, ())]
    sem_t = [torch.tensor([[[0, 1, 2], [3, 3, 0]], [[2, 2, 1], [0, 3, 1]]]),
             torch.tensor([[[2, 0]], [[0, 0]]])]
    inst_t = []
    for h, w in sizes:
        fg = torch.rand(2, h, w, generator=g) > 0.4
        fg[0, 0, 0] = True
        inst_t.append({'center': torch.rand(2, 1, h, w, generator=g),
                       'offset': torch.rand(2, 2, h, w, generator=g) * 2 - 1,
                       'foreground': fg,
                       'orientation': (torch.rand(2, h, w, generator=g) * 2 - 1) * 3.1,
                       'orientation_foreground': fg & (torch.rand(2, h, w, generator=g) > 0.3)})
    targets = targets_to({'semantic': sem_t, 'instance': inst_t, 'scene': torch.tensor([3, 0])},
                         dtype=torch.float64)
    return args, outputs, targets, (0.5, 2.0, 1.5)


def _hand_losses(args, outputs, targets, class_w, n_scales):
    """the same losses with explicit per-pixel loops (numpy, fp64)"""
    sem = 0.0
    for s in range(n_scales):
        x = outputs[0][0] if s == 0 else outputs[0][1][s - 1]
        x, t = x.numpy(), targets['semantic'][s].numpy()
        num = den = 0.0
        for n, i, j in np.ndindex(*t.shape):
            if t[n, i, j] == 0:
                continue
            c = t[n, i, j] - 1
            z = x[n, :, i, j]
            lse = math.log(np.exp(z - z.max()).sum()) + z.max()
            num += class_w[c] * (lse - z[c])
            den += class_w[c]
        sem += num / den
    center = offset = orient = 0.0
    for s in range(n_scales):
        c_p, o_p, r_p = [a.numpy() for a in (outputs[1][0] if s == 0 else outputs[1][1][s - 1])]
        tg = {k: v.double().numpy() for k, v in targets['instance'][s].items()}
        center += ((c_p - tg['center']) ** 2).mean()
        fg = tg['foreground'].astype(bool)
        l1 = np.abs(o_p - tg['offset']).transpose(0, 2, 3, 1)           # (N, H, W, 2)
        offset += l1[fg].sum() / (2 * fg.sum())
        fo = tg['orientation_foreground'].astype(bool)
        acc = 0.0
        for n, i, j in zip(*np.nonzero(fo)):
            sn, cs = r_p[n, 0, i, j], r_p[n, 1, i, j]
            norm = math.hypot(sn, cs)
            cosd = (sn * math.sin(tg['orientation'][n, i, j])
                    + cs * math.cos(tg['orientation'][n, i, j])) / norm
            acc += 1.0 - math.exp(args.orientation_kappa * (cosd - 1.0))
        orient += acc / fo.sum()
    eps = args.scene_loss_label_smoothing
    z = outputs[2][0].numpy()
    scene, cnt = 0.0, 0
    for n, t in enumerate(targets['scene'].tolist()):
        if t == 0:
            continue
        logp = z[n] - (math.log(np.exp(z[n] - z[n].max()).sum()) + z[n].max())
        scene += (1 - eps) * -logp[t - 1] + eps * -logp.mean()
        cnt += 1
    scene /= cnt
    losses = {'semantic': sem, 'instance_center': center, 'instance_offset': offset,
              'instance_orientation': orient, 'scene': scene}
    total = (1.0 * sem + 0.25 * scene + 3.0 * 2 * center + 3.0 * 1 * offset + 0.5 * orient)
    return total, losses


@pytest.mark.parametrize('multiscale', [True, False])
def test_training_losses_by_hand(multiscale):
    from oracle.training_oracle import loss_weights, training_losses
    args, outputs, targets, class_w = _tiny_case()
    args.semantic_no_multiscale_supervision = not multiscale
    args.instance_no_multiscale_supervision = not multiscale
    assert loss_weights(args) == {'instance_orientation': 0.5, 'instance_center': 6.0,
                                  'instance_offset': 3.0, 'semantic': 1.0, 'scene': 0.25}
    total, losses = training_losses(outputs, targets, args, class_w, 4)
    ref_total, ref = _hand_losses(args, outputs, targets, class_w, 2 if multiscale else 1)
    assert set(losses) == set(ref)
    for k in ref:
        assert abs(float(losses[k]) - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, float(losses[k]), ref[k])
    assert abs(float(total) - ref_total) <= 1e-12 * abs(ref_total)
    # void pixels and the void scene label contribute nothing: change the predictions there
    o2 = copy.deepcopy(outputs)
    o2[0][0][targets['semantic'][0].unsqueeze(1).expand_as(o2[0][0]) == 0] = 123.0
    o2[2][0][1] = torch.tensor([9.0, -9.0, 3.0, 1.0], dtype=torch.float64)
    total2, _ = training_losses(o2, targets, args, class_w, 4)
    assert float(total2) == float(total)


def test_semantic_term_is_the_pinned_multiscale_loss():
    """label smoothing 0: the semantic term of `training_losses` == the sum of
    `semantic_ce_multiscale`, which reproduces the reference class's golden losses"""
    from emsanet_amd import default_args
    from oracle.semantic_loss_oracle import NYUV2_TEST_CLASS_WEIGHTS, semantic_ce_multiscale
    from oracle.training_oracle import training_losses
    g = np.load(GOLD)
    preds = [torch.from_numpy(g[f'pred{i}']).double() for i in range(3)]
    tgts = [torch.from_numpy(g[f'target{i}']).long() for i in range(3)]
    args = default_args(tasks=('semantic',), semantic_loss_label_smoothing=0.0)
    total, losses = training_losses([(preds[0], tuple(preds[1:]))], {'semantic': tgts}, args,
                                    NYUV2_TEST_CLASS_WEIGHTS, 10)
    ms = semantic_ce_multiscale(preds, tgts, NYUV2_TEST_CLASS_WEIGHTS)
    assert float(losses['semantic']) == float(torch.stack(ms).sum()) == float(total)
    ref = float(np.sum(g['loss'][:3]))
    assert abs(float(total) - ref) <= 1e-5 * ref


def test_synthetic_targets():
    from oracle.emsanet_oracle import synthetic_batch
    from oracle.training_oracle import synthetic_targets
    b = synthetic_batch(4, 64, 96, seed=3)
    t = synthetic_targets(b, 40, 10)
    assert [tuple(s.shape) for s in t['semantic']] == [(4, 64, 96), (4, 2, 3), (4, 4, 6), (4, 8, 12)]
    full = t['semantic'][0]
    assert 0.05 < (full == 0).double().mean() < 0.2                 # void pixels
    assert full.max() == 40 and len(full.unique()) == 41            # every class is used
    for s, d in zip(t['semantic'], t['instance']):
        assert tuple(d['center'].shape) == (4, 1) + tuple(s.shape[1:])
        assert tuple(d['offset'].shape) == (4, 2) + tuple(s.shape[1:])
        assert not d['foreground'][1].any() and d['foreground'][0].any()    # one empty sample
        assert not (d['foreground'] & (s == 0)).any()
        assert (d['offset'] * ~d['foreground'].unsqueeze(1) == 0).all()
        assert not (d['orientation_foreground'] & ~d['foreground']).any()
        assert 0 <= d['center'].min() and d['center'].max() <= 1
    assert t['scene'][0] == 0 and (t['scene'][1:] >= 1).all() and (t['scene'] <= 10).all()
    t2 = synthetic_targets(b, 40, 10)
    assert all(torch.equal(a, c) for a, c in zip(t['semantic'], t2['semantic']))


# ---------------------------------------------------------------------------------------------
# the gates of the GPU trajectory test have teeth
# ---------------------------------------------------------------------------------------------
H, W, BS, K = 64, 96, 2, 4


def _trajectory(model, args, batches, targets, cw, **kw):
    from oracle.training_oracle import OracleTrainer
    tr = OracleTrainer(model, args, cw, 10, K, **kw)
    losses = []
    for i in range(K):
        total, l = tr.step(batches[i % len(batches)], targets[i % len(batches)])
        l = {k: float(v) for k, v in l.items()}
        l['total'] = float(total)
        losses.append(l)
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    mom = {k: tr.opt.state[p]['momentum_buffer'].clone() for k, p in model.named_parameters()}
    run = {k: b.clone() for k, b in model.named_buffers() if 'running' in k}
    return losses, params, mom, run


def _gated(base, dev, p_init, r_init):
    """the GPU test's gated quantities with the deviated run in the engine's place, each as a
    multiple of its gate"""
    from test_training_trajectory_gpu import (EPS_32, LOSS_TOL_32, MOM_TOL_32, MOVE_TOL_32,
                                              RUN_TOL_32, ZERO_GRAD, ZERO_MOVE_TOL_32)
    (lb, pb, mb, rb), (ld, pd, md, rd) = base, dev
    loss = max(abs(d[k] - b[k]) / abs(b[k]) for b, d in zip(lb, ld) for k in b)
    move = max((pd[k] - pb[k]).norm().item()
               / (MOVE_TOL_32 * (pb[k] - p_init[k]).norm().item() + EPS_32 * pb[k].norm().item())
               for k in pb if not k.endswith(ZERO_GRAD))
    move_zero = max((pd[k] - pb[k]).norm().item() / (pb[k] - p_init[k]).norm().item()
                    for k in pb if k.endswith(ZERO_GRAD))
    mom = max((md[k] - mb[k]).norm().item() / mb[k].norm().item()
              for k in mb if not k.endswith(ZERO_GRAD))
    run = max((rd[k] - rb[k]).norm().item() / (rb[k] - r_init[k]).norm().item() for k in rb)
    return {'loss': loss / LOSS_TOL_32, 'param': move, 'param_zero_grad': move_zero / ZERO_MOVE_TOL_32,
            'momentum': mom / MOM_TOL_32, 'running': run / RUN_TOL_32}


DEVIATIONS = {
    # name: (trainer keyword arguments, args overrides, BatchNorm momentum, gated quantity,
    #        required multiple of its gate)
    'plain momentum': ({'nesterov': False}, {}, None, 'param', 10),
    'BatchNorm momentum 0.12': ({}, {}, 0.12, 'running', 10),
    'dropout step not advanced': ({'advance_dropout': False}, {}, None, 'loss', 10),
    # weight decay 1e-4 x lr is ~1e-7 of a 1-D tensor per step: measured 6.3x the running-statistics
    # gate, 2.6x the loss gate, 2.0x the gate of the biases that weight decay alone moves (their
    # movement is all decay; the fp32 roundoff gradient the engine adds costs 0.18 of it)
    'no weight decay on 1-D tensors': ({'decay_1d': False}, {}, None, 'running', 3),
    'instance weighting (1, 2)': ({}, {'instance_weighting': (1, 2)}, None, 'param', 10),
    'scene label smoothing 0': ({}, {'scene_loss_label_smoothing': 0.0}, None, 'loss', 10),
}


def test_each_deviation_exceeds_its_gate_tenfold():
    from emsanet_amd import full_args, nyuv2_config
    from oracle.emsanet_oracle import EMSANetOracle, deterministic_state_dict, synthetic_batch
    from oracle.semantic_loss_oracle import NYUV2_TEST_CLASS_WEIGHTS
    from oracle.training_oracle import synthetic_targets, targets_to
    from test_training_trajectory_gpu import DROPOUT_SEED, MAX_LR
    args = full_args(input_height=H, input_width=W, tasks_weighting=TASKS_WEIGHTING,
                     learning_rate=MAX_LR)
    model = EMSANetOracle(args, nyuv2_config())
    model.load_state_dict(deterministic_state_dict(model, 0))
    model = model.double()
    model.dropout_seed = DROPOUT_SEED
    raw = [synthetic_batch(BS, H, W, seed=100 + s) for s in range(2)]
    batches = [{k: v.double() for k, v in b.items()} for b in raw]
    targets = [targets_to(synthetic_targets(b, 40, 10), dtype=torch.float64) for b in raw]
    cw = torch.tensor(NYUV2_TEST_CLASS_WEIGHTS)
    p_init = {k: p.detach().clone() for k, p in model.named_parameters()}
    r_init = {k: b.clone() for k, b in model.named_buffers() if 'running' in k}
    base = _trajectory(copy.deepcopy(model), args, batches, targets, cw)
    report, short = [], []
    for name, (kw, over, bn_mom, what, need) in DEVIATIONS.items():
        m = copy.deepcopy(model)
        if bn_mom is not None:
            for bn in m.modules():
                if isinstance(bn, torch.nn.BatchNorm2d):
                    bn.momentum = bn_mom
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        q = _gated(base, _trajectory(m, a, batches, targets, cw, **kw), p_init, r_init)
        report.append(f"{name}: {what} {q[what]:.0f}x gate (" +
                      ', '.join(f'{k} {v:.1f}x' for k, v in q.items()) + ')')
        if q[what] < need:
            short.append(name)
    print('\n'.join(report))
    assert not short, report
