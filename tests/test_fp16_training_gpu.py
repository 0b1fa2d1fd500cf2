"""Training in float16 storage under the device-side loss scaler (emsanet_amd.optim.LossScaler): full
RGB-D model, all four heads, the real training losses.

* the refusal of scaler-less fp16 training is kept; with a scaler attached a step runs;
* overflow reached through an ordinary (absurdly large) scale: every step is skipped, nothing the
  optimizer owns moves, what the forward pass owns (BatchNorm statistics, Dropout2d step) does;
* the captured step (`GraphedTrainStep(loss_scaler=...)`) grows the scale and takes the decision to
  skip on the device, at replay time -- a host-side scaler cannot pass this;
* the K = 4 trajectory of tests/test_training_trajectory_gpu.py in fp16 storage against the fp64
  oracle emulating fp16 storage, both under the same fixed power-of-two loss scale.

Trajectory gates (LOSS_TOL_F16 ...): worst of three runs on MI355X times three to four, the ratio the
fp32 gates of test_training_trajectory_gpu.py carry over their measurements, and never looser than
the bf16 twin (0.5, 0.3, (0.6, 2.5), 0.5).  Measured values stand beside the constants."""
import copy

import pytest
import torch
import torch.nn.functional as F

import test_training_trajectory_gpu as TT
from util import DEV, deterministic_state_dict

pytestmark = pytest.mark.gpu

F16 = torch.float16
SH, SW, SBS = 64, 96, 2                 # everything but the trajectory

# fixed loss scale of the trajectory test: 2^10 as asked, no halving was needed (skipped == 0 in every
# measured run; 2^14 and 2^6 did not overflow either)
TRAJ_SCALE = 2.0 ** 10
# fp16 trajectory gates against the fp16-emulating oracle.  Measured on MI355X, three runs at 2^10
# (plain fp64 trajectory on the same masks against the emulating one in brackets):
#   per-step worst loss error  1.3e-3, 5.7e-2, 0.21..0.22, 0.28..0.34   (6.2e-3, 2.0e-2, 0.10..0.12, 6.1e-2..0.23)
#   whole-model movement cosine 0.7526..0.7532 (0.8207..0.8211)
#   per tensor >= 1024 el.: cosine min 0.6533..0.6548, median 0.753..0.754 (0.717..0.720, 0.818)
#   norm ratio 1.016 .. 1.267, median 1.18 (0.980 .. 1.149)
# THE FINDING: only step 0 is tighter than bf16 by the eight-fold the three extra mantissa bits
# promise (1.3e-3 against bf16's 9.9e-3).  From step 1 on fp16 sits where bf16 sits (bf16: 0.18,
# 0.23, 0.29; cosine 0.713, min 0.571): what separates engine and oracle after the first update is
# the trajectory's own sensitivity (§3 of DESIGN.md: the fp32 and fp64 oracles drift apart likewise),
# not the storage format -- fp16 storage ITSELF moves the fp64 trajectory as far as bf16 storage does
# (cosine 0.82 both).  The loss scale matters more than the format: at 2^6 the same run gives cosine
# 0.863 / min 0.785 / losses <= 0.22, at 2^14 0.754 / 0.634 / 0.29.
# Worst run times three to four (the margin of the fp32 gates), capped by the bf16 twin:
#   loss 0.34 x 3 = 1.0 -> the cap 0.5;  1 - cosine 0.247 x 3 and 0.347 x 3 -> the caps 0.5 and 0.3;
#   ratio: |r - 1| <= 0.267, x 3.75 -> 2.0 above (tighter than bf16's 2.5); nothing below 1 was
#   measured, the mirror image 1 / 2.0 is looser than the cap 0.6.
LOSS_TOL_F16 = 0.5
MOVE_COS_F16, MOVE_RATIO_F16, MOVE_COS_ALL_F16 = 0.3, (0.6, 2.0), 0.5


def _bits(t):
    """the tensor's bit patterns (fp32 parameters / moments, Adam's fp64 device state)"""
    return t.detach().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _small(optimizer='sgd', lr=1e-3, seed_batches=(1, 2)):
    """fp16 model at 64x96, its buckets / optimizer / criterion, device batches and targets"""
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.loss import TrainingLosses
    from emsanet_amd.model import EMSANet
    from emsanet_amd.optim import get_optimizer
    from emsanet_amd.parallel import GradientBuckets
    from oracle.emsanet_oracle import synthetic_batch
    from oracle.semantic_loss_oracle import NYUV2_TEST_CLASS_WEIGHTS
    from oracle.training_oracle import synthetic_targets, targets_to
    args = full_args(input_height=SH, input_width=SW, tasks_weighting=TT.TASKS_WEIGHTING,
                     learning_rate=lr, optimizer=optimizer)
    cfg = nyuv2_config()
    model = EMSANet(args, cfg)
    model.load_state_dict(deterministic_state_dict(model, 0))
    model.to(DEV).train()
    model.dropout_seed = TT.DROPOUT_SEED
    model.set_compute_dtype(F16)
    n_scene = len(cfg.scene_label_list_without_void)
    crit = TrainingLosses(args, torch.tensor(NYUV2_TEST_CLASS_WEIGHTS), n_scene).to(DEV)
    buckets = GradientBuckets([p for p in model.parameters() if p.requires_grad])
    opt = get_optimizer(args, buckets)
    cpu = [synthetic_batch(SBS, SH, SW, seed=s) for s in seed_batches]
    batches = [{k: v.to(DEV) for k, v in b.items()} for b in cpu]
    targets = [targets_to(synthetic_targets(b, 40, n_scene, seed=7), DEV) for b in cpu]
    return model, buckets, opt, crit, batches, targets


def _eager_step(model, buckets, scaler, crit, batch, targets):
    buckets.reset()
    out = model(batch)
    total, _ = crit(out, targets)
    scaler.backward(total)
    buckets.finish()
    scaler.step()
    return out, total


def test_refusal_kept_and_one_scaled_step_runs():
    from emsanet_amd import _lib
    from emsanet_amd.optim import LossScaler
    from test_model_gpu import _flatten
    model, buckets, opt, crit, batches, targets = _small()
    with pytest.raises(_lib.EmsaError, match='float16 storage is an inference mode'):
        model(batches[0])
    assert model.dropout_step == 0
    scaler = LossScaler(opt, init_scale=TRAJ_SCALE).attach(model)
    assert model.loss_scaler is scaler
    before = [fp.clone() for fp in opt.flat_params]
    out, total = _eager_step(model, buckets, scaler, crit, batches[0], targets[0])
    torch.cuda.synchronize()
    flat = _flatten(out)
    assert flat and all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in flat)
    assert total.dtype == torch.float32 and bool(torch.isfinite(total))
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert bool(torch.isfinite(p.grad).all()), f"non-finite gradient of {k}"
    assert scaler.state() == {'scale': TRAJ_SCALE, 'growth_tracker': 1, 'steps': 1, 'skipped': 0}
    assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(opt.flat_params, before))
    # detached again, the refusal is back
    model.loss_scaler = None
    with pytest.raises(_lib.EmsaError):
        model(batches[0])


@pytest.mark.parametrize('optimizer', ['sgd', 'adamw'])
def test_overflow_skips_the_update_and_nothing_else(optimizer):
    """init_scale 2^60: the scaled gradients leave fp16 (and fp32), three eager steps are skipped"""
    from emsanet_amd.optim import LossScaler
    model, buckets, opt, crit, batches, targets = _small(optimizer)
    scaler = LossScaler(opt, init_scale=2.0 ** 60).attach(model)
    params0 = [fp.clone() for fp in opt.flat_params]
    mom0 = [m.clone() for m in opt.flat_momentum]
    nbt0 = {k: int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    run0 = {k: v.clone() for k, v in model.named_buffers() if k.endswith('running_mean')}
    for i in range(3):
        _eager_step(model, buckets, scaler, crit, batches[i % 2], targets[i % 2])
    st = scaler.state()
    assert st == {'scale': 2.0 ** 57, 'growth_tracker': 0, 'steps': 3, 'skipped': 3}, st
    for a, b in zip(opt.flat_params + opt.flat_momentum, params0 + mom0):
        assert torch.equal(_bits(a), _bits(b))
    if optimizer != 'sgd':
        assert opt.step_count == 0
    # the forward pass ran three times: Dropout2d step and BatchNorm statistics have advanced
    assert model.dropout_step == 3
    nbt = {k: int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')}
    assert nbt0 and all(nbt[k] == nbt0[k] + 3 for k in nbt0)
    assert any(not torch.equal(v, run0[k]) for k, v in model.named_buffers() if k in run0)


def test_graphed_step_scales_and_skips_on_the_device():
    from emsanet_amd.graph import GraphedTrainStep
    from emsanet_amd.optim import LossScaler
    model, buckets, opt, crit, batches, targets = _small()
    scaler = LossScaler(opt, init_scale=2.0 ** 8, growth_interval=2).attach(model)
    params0 = [fp.clone() for fp in opt.flat_params]
    step = GraphedTrainStep(model, batches[0], buckets, opt, loss_fn=lambda out: crit(out, targets[0])[0],
                            warmup=3, loss_scaler=scaler)
    # the warm-up ran three real steps (the scale grew once); all of it is taken back
    assert scaler.state() == {'scale': 2.0 ** 8, 'growth_tracker': 0, 'steps': 0, 'skipped': 0}
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(opt.flat_params, params0))
    for _ in range(4):
        loss, _ = step.replay()
    assert scaler.state() == {'scale': 2.0 ** 10, 'growth_tracker': 0, 'steps': 4, 'skipped': 0}
    assert bool(torch.isfinite(loss))
    assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(opt.flat_params, params0))
    params4 = [fp.clone() for fp in opt.flat_params]
    mom4 = [m.clone() for m in opt.flat_momentum]
    # the host learns nothing of this: the replayed graph reads the scale, overflows, and skips
    scaler.device_state[0] = 2.0 ** 60
    step.replay()
    assert scaler.state() == {'scale': 2.0 ** 59, 'growth_tracker': 0, 'steps': 5, 'skipped': 1}
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(opt.flat_params + opt.flat_momentum,
                                                               params4 + mom4))
    assert model.dropout_step == 5


class _ScaledEngineLoop(TT._EngineLoop):
    """the engine's eager step of the trajectory tests under a LossScaler"""

    def __init__(self, model, args, class_weights, n_scene, total_steps, scale):
        from emsanet_amd.optim import LossScaler
        super().__init__(model, args, class_weights, n_scene, total_steps)
        self.scaler = LossScaler(self.opt, init_scale=scale, growth_interval=total_steps + 1).attach(model)

    def step(self, batch, targets):
        from emsanet_amd import ops
        from emsanet_amd.optim import one_cycle
        from oracle.training_oracle import targets_to
        lr, mom = one_cycle(self.i, self.total_steps, self.args.learning_rate)
        self.opt.set_schedule(lr, mom)
        self.buckets.reset()
        ops.MASK_TRACE = []
        try:
            out = self.model({k: v.to(DEV) for k, v in batch.items()})
            trace = ops.MASK_TRACE
        finally:
            ops.MASK_TRACE = None
        total, losses = self.crit(out, targets_to(targets, DEV))
        self.scaler.backward(total)
        self.buckets.finish()
        self.scaler.step()
        self.i += 1
        return (lr, mom), trace, float(total.detach()), {k: float(v.detach()) for k, v in losses.items()}


def _scaled_oracle_trainer(model, args, cw, n_scene, total_steps, scale):
    """OracleTrainer whose step runs under the loss scale: (total * S).backward(), gradients divided
    by S (exact: a power of two) in front of opt.step().  In storage-emulation mode the oracle then
    rounds the SAME scaled gradients the engine stores."""
    from oracle.training_oracle import OracleTrainer, training_losses

    class Scaled(OracleTrainer):
        def step(self, batch, targets, relu=None):
            m = self.model
            m.train()
            self.opt.zero_grad(set_to_none=True)
            saved = F.relu
            if relu is not None:
                F.relu = relu
            try:
                out = m(batch)
            finally:
                F.relu = saved
            total, losses = training_losses(out, targets, self.args, self.class_weights, self.n_scene)
            (total * scale).backward()
            for group in self.opt.param_groups:
                for p in group['params']:
                    if p.grad is not None:
                        p.grad.div_(scale)
            self.opt.step()
            self.sched.step()
            return total.detach(), {k: v.detach() for k, v in losses.items()}

    return Scaled(model, args, cw, n_scene, total_steps)


def test_fp16_trajectory_matches_storage_emulating_oracle():
    """protocol of test_bf16_trajectory_matches_storage_emulating_oracle (128x160, bs 4, K = 4, dropout
    seed 77, the reference's task weighting, max lr 1e-3, ReLU decisions pinned) with Spec.STORAGE =
    float16 and the fixed loss scale TRAJ_SCALE on both sides; the plain fp64 oracle runs beside it."""
    from oracle.training_oracle import targets_to
    K = TT.K16
    args, model, emu, batches, targets, cw, n_scene = TT._setup()
    plain = copy.deepcopy(emu)
    model.set_compute_dtype(F16)
    eng = _ScaledEngineLoop(model, args, cw, n_scene, K, TRAJ_SCALE)
    t_emu = _scaled_oracle_trainer(emu, args, cw, n_scene, K, TRAJ_SCALE)
    t_plain = _scaled_oracle_trainer(plain, args, cw, n_scene, K, TRAJ_SCALE)
    b64 = [{k: v.double() for k, v in b.items()} for b in batches]
    t64 = [targets_to(t, dtype=torch.float64) for t in targets]
    p_init = {k: p.detach().clone() for k, p in emu.named_parameters()}
    loss_err, loss_err_plain = [], []
    for i in range(K):
        _, trace, tot_e, l_e = eng.step(batches[i % 4], targets[i % 4])
        tot_q, l_q, pin_q = TT._oracle_step(t_emu, b64[i % 4], t64[i % 4], trace, F16)
        tot_p, l_p, _ = TT._oracle_step(t_plain, b64[i % 4], t64[i % 4], trace, None)
        e = {k: TT._rel(l_e[k], l_q[k]) for k in l_q}
        e['total'] = TT._rel(tot_e, tot_q)
        ep = {k: TT._rel(l_p[k], l_q[k]) for k in l_q}
        ep['total'] = TT._rel(tot_p, tot_q)
        kw = max(e, key=e.get)
        loss_err.append((e[kw], kw))
        loss_err_plain.append(max(ep.values()))
        print(f"fp16 step {i}: total emulating {tot_q:.5f} engine {tot_e:.5f} plain fp64 {tot_p:.5f}; "
              f"worst loss rel err engine {e[kw]:.2e} ({kw}), plain-vs-emulating "
              f"{loss_err_plain[-1]:.2e}; {pin_q.flips} of {pin_q.total} ReLU decisions differ")
    st = eng.scaler.state()
    print(f"fp16 loss scale {TRAJ_SCALE:g}: {st}")

    def movement(params):
        return {k: p.detach().cpu().double() - p_init[k] for k, p in params}

    m_e, m_q, m_p = movement(model.named_parameters()), movement(emu.named_parameters()), \
        movement(plain.named_parameters())
    mp = dict(model.named_parameters())

    def compare(a, b):
        names = [k for k in b if not k.endswith(TT.ZERO_GRAD)]
        cos = torch.tensor([F.cosine_similarity(a[k].flatten(), b[k].flatten(), dim=0).item()
                            for k in names])
        ratio = torch.tensor([a[k].norm().item() / b[k].norm().item() for k in names])
        cos_all = F.cosine_similarity(torch.cat([a[k].flatten() for k in names]),
                                      torch.cat([b[k].flatten() for k in names]), dim=0).item()
        big = torch.tensor([mp[k].numel() >= 1024 and '.se_' not in k for k in names])
        return names, cos, ratio, cos_all, big

    names, cos, ratio, cos_all, big = compare(m_e, m_q)
    _, cos_p, ratio_p, cos_all_p, _ = compare(m_p, m_q)
    nb = [k for k, b_ in zip(names, big.tolist()) if b_]
    cb, rb = cos[big], ratio[big]
    print(f"fp16 after {K} steps, movement engine vs emulating oracle: whole-model cosine "
          f"{cos_all:.4f}; per tensor (>= 1024 el.) cosine min {cb.min():.4f} ({nb[int(cb.argmin())]}) "
          f"median {cb.median():.4f}; norm ratio {rb.min():.3f} ({nb[int(rb.argmin())]}) .. "
          f"{rb.max():.3f} ({nb[int(rb.argmax())]}), median {rb.median():.4f}; all tensors cosine min "
          f"{cos.min():.4f} ratio {ratio.min():.3f} .. {ratio.max():.3f}")
    print(f"fp16 storage itself (plain fp64 vs emulating, same masks): whole-model cosine "
          f"{cos_all_p:.4f}; per tensor cosine min {cos_p[big].min():.4f} median "
          f"{cos_p[big].median():.4f}; norm ratio {ratio_p[big].min():.3f} .. {ratio_p[big].max():.3f}"
          f" median {ratio_p[big].median():.4f}; losses {' '.join(f'{e:.1e}' for e in loss_err_plain)}")
    print(f"fp16 per-step worst loss error engine vs emulating: "
          f"{' '.join(f'{e:.1e}' for e, _ in loss_err)}")
    assert st['skipped'] == 0 and st['steps'] == K and st['scale'] == TRAJ_SCALE, st
    assert model.dropout_step == emu.dropout_step == K
    assert max(e for e, _ in loss_err) <= LOSS_TOL_F16, loss_err
    assert cos_all >= MOVE_COS_ALL_F16
    assert cb.min().item() >= MOVE_COS_F16, (nb[int(cb.argmin())], cb.min().item())
    assert MOVE_RATIO_F16[0] <= rb.min().item() and rb.max().item() <= MOVE_RATIO_F16[1], \
        (nb[int(rb.argmin())], rb.min().item(), nb[int(rb.argmax())], rb.max().item())
