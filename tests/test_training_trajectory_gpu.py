"""The real training loop over several steps against an independent fp64 reference.

Every other parity gate covers ONE forward / backward pass.  Here the engine runs its eager
training step -- `TrainingLosses` -> backward -> `GradientBuckets` -> `FusedSGD` under
`set_schedule(one_cycle(...))`, Dropout2d on, BatchNorm running statistics updating -- for K steps
on four cycled batches, and the fp64 oracle runs the reference's step beside it
(oracle/training_oracle.py: the reference's loss weighting, torch.optim.SGD(nesterov=True) under
torch's OneCycleLR), with its ReLU decisions pinned to the engine's every step (`_PinnedRelu`:
without pinning one fp32-flipped ReLU moves the gradients by ~1e-2 and the comparison measures
chaos, see tests/test_model_gpu.py).  What only shows across steps: momentum (incl. the nesterov
first step, momentum cycled by the schedule), BatchNorm running mean / unbiased variance /
`num_batches_tracked`, the Dropout2d masks advancing per step, the packed / Winograd weight caches
refreshing after every update, weight decay on every tensor, the sparse loss gradient (zero at
void pixels, four supervised scales).

Configuration: full RGB-D model, all four heads, the reference's published weighting
(tasks_weighting (1, 0.25, 3, 0.5), instance weighting (2, 1)), 128x160, bs 4 (the /32 BatchNorms
see 80 samples), dropout seed 77, NYUv2 class weights of the reference's semantic-loss test,
one-cycle schedule over K = 4 steps with max lr 1e-3 (lr 5.9e-4 .. 4e-9, momentum 0.87 .. 0.95).

Why K = 4 at max lr 1e-3 and not 12 steps at the default 1e-2: the same experiment WITHOUT the
engine -- the fp32 oracle on its own ReLU decisions against the fp64 oracle pinned to them, same
batches and targets -- drifts apart on its own.  Measured (CPU, 128x160 bs 4), worst per-task loss
error by step: lr 1e-2, K 12: 3e-7, 2e-4, 1e-2, 0.49; lr 1e-3, K 12: ... 2.6e-4 (step 3), 8.8e-4,
3.3e-2; lr 1e-4, K 12: <= 1.4e-5 up to step 5, then a jump to 2.2e-3 (an unpinned discrete choice,
e.g. a max-pool selection, flipping); lr 3e-4, K 6: the same jump at step 2.  lr 1e-3, K 4: 3e-7,
1.3e-5, 8.6e-5, 1.5e-4, parameters within 1.0e-3 of their movement -- the trajectory the engine
can be held to at a tight tolerance.

Gates (measured on MI355X, three runs; DESIGN.md section 3 keeps the step-by-step values):
  * fp32, against the fp64 oracle:
      - every unweighted per-task loss and the total, every step: rel. error <= LOSS_TOL_32
      - ReLU decisions the oracle would have taken differently: <= FLIPS_REL of all, every step
      - every parameter after K steps: |p_eng - p_64| <= MOVE_TOL_32 |p_64 - p_init| + EPS_32 |p_64|
        (against the MOVEMENT: a wrong momentum, schedule or weight decay changes that); the conv
        biases in front of a batch-statistics BatchNorm, whose gradient is mathematically zero and
        which weight decay alone moves: <= ZERO_MOVE_TOL_32 of that movement
      - momentum buffers (FusedSGD's flat buffers unflattened through the bucket layout) against
        torch.optim.SGD's: rel-L2 <= MOM_TOL_32 (buffers of the mathematically zero gradients --
        conv biases in front of a batch-statistics BatchNorm -- against the largest buffer)
      - BatchNorm running mean / var: error <= RUN_TOL_32 of their movement from the initial values
      - num_batches_tracked and dropout_step equal
      - eval forward (running statistics, no pinning) of the trained engine against the oracle
        loaded with the engine's trained state: the existing eval gate, 1e-3 and `_argmax_check`;
        against the oracle's own trained model: <= EVAL_TRAJ_TOL (the trajectories' drift shows:
        the tanh offset map differs by 9e-4 .. 1.5e-3 from run to run of the engine's atomics)
  * bf16 (`set_compute_dtype(torch.bfloat16)`), against the fp64 oracle in storage-emulation
    mode (Spec.STORAGE = bf16) on the engine's ReLU branch; the plain fp64 oracle pinned to the same
    masks is run beside it and reports how far bf16 storage ITSELF moves the trajectory:
      - per-step losses: rel. error <= LOSS_TOL_16
      - parameter movement per tensor: cosine >= MOVE_COS_16, norm ratio inside MOVE_RATIO_16
        (tensors of >= 1024 elements outside the squeeze-excite MLPs; see the loose class in
        tests/test_model16_gpu.py), whole-model movement cosine >= MOVE_COS_ALL_16
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from util import DEV

pytestmark = pytest.mark.gpu

H, W, BS = 128, 160, 4
K32 = K16 = 4
DROPOUT_SEED = 77
TASKS_WEIGHTING = (1.0, 0.25, 3.0, 0.5)
MAX_LR = 1e-3

# fp32 gates
LOSS_TOL_32 = 1e-3             # measured 6.1e-7, 9.3e-6, 7.7e-5, 2.4e-4 (steps 0..3)
FLIPS_REL = 1e-3               # measured 1.9e-6, 1.3e-5, 7.3e-5, 1.7e-4
MOVE_TOL_32, EPS_32 = 1e-2, 1e-7        # measured worst 3.2e-3, median 2.6e-4
ZERO_MOVE_TOL_32 = 0.5         # measured worst 0.18, median 0.13 (fp32 roundoff gradient vs decay)
MOM_TOL_32 = 0.3               # measured worst 0.117, median 4.1e-2: see below
RUN_TOL_32 = 1e-3              # measured worst 2.1e-4, median 1.6e-5
EVAL_TOL = 1e-3                # the eval gate of tests/test_model_gpu.py, on the engine's trained state
EVAL_TRAJ_TOL = 5e-3           # against the oracle's own trained model: measured 7.4e-4 .. 1.5e-3
# bf16 gates against the storage-emulating oracle (measured: per-step losses 9.9e-3, 0.18, 0.23, 0.29 --
# the plain fp64 trajectory on the same masks is 1.4e-2 .. 9.1e-2 away from the emulating one; movement
# cosine whole model 0.713 (plain vs emulating 0.823), per tensor >= 1024 el. min 0.571 median 0.699,
# norm ratio 1.003 .. 1.725 median 1.196 (plain vs emulating 0.860 .. 1.284))
LOSS_TOL_16 = 0.5
MOVE_COS_16, MOVE_RATIO_16, MOVE_COS_ALL_16 = 0.3, (0.6, 2.5), 0.5

ZERO_GRAD = ('conv1x3_1.bias', 'conv1x3_2.bias')     # biases in front of a train-mode BatchNorm


def _setup():
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.model import EMSANet
    from oracle.emsanet_oracle import EMSANetOracle, deterministic_state_dict, synthetic_batch
    from oracle.semantic_loss_oracle import NYUV2_TEST_CLASS_WEIGHTS
    from oracle.training_oracle import synthetic_targets
    args = full_args(input_height=H, input_width=W, tasks_weighting=TASKS_WEIGHTING,
                     learning_rate=MAX_LR)
    assert tuple(args.instance_weighting) == (2, 1)
    cfg = nyuv2_config()
    oracle = EMSANetOracle(args, cfg)
    sd = deterministic_state_dict(oracle, 0)
    oracle.load_state_dict(sd)
    oracle = oracle.double()
    model = EMSANet(args, cfg)
    model.load_state_dict(sd)
    model.to(DEV)
    for m in (model, oracle):
        m.train()
        m.dropout_seed = DROPOUT_SEED
    batches = [synthetic_batch(BS, H, W, seed=100 + s) for s in range(4)]
    n_scene = len(cfg.scene_label_list_without_void)
    targets = [synthetic_targets(b, 40, n_scene, seed=7) for b in batches]
    return args, model, oracle, batches, targets, torch.tensor(NYUV2_TEST_CLASS_WEIGHTS), n_scene


class _EngineLoop:
    """the engine's eager training step with the ReLU decisions recorded"""

    def __init__(self, model, args, class_weights, n_scene, total_steps):
        from emsanet_amd.loss import TrainingLosses
        from emsanet_amd.optim import FusedSGD
        from emsanet_amd.parallel import GradientBuckets
        self.model, self.args, self.total_steps = model, args, total_steps
        self.crit = TrainingLosses(args, class_weights, n_scene).to(DEV)
        self.buckets = GradientBuckets([p for p in model.parameters() if p.requires_grad])
        self.opt = FusedSGD(self.buckets, lr=args.learning_rate, momentum=args.momentum,
                            weight_decay=args.weight_decay)
        self.i = 0

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
        total.backward()
        self.buckets.finish()
        self.opt.step()
        self.i += 1
        return (lr, mom), trace, float(total), {k: float(v) for k, v in losses.items()}

    def momentum_buffers(self):
        """{parameter: momentum buffer} from FusedSGD.state_dict() through the bucket layout"""
        bufs = self.opt.state_dict()['momentum_buffers']
        out = {}
        for (flat_g, ps, views), fm in zip(self.buckets.buckets, bufs):
            for p, v in zip(ps, views):
                off = v.storage_offset() - flat_g.storage_offset()
                out[p] = fm[off:off + p.numel()].view(p.shape)
        return out


def _oracle_step(trainer, batch, targets, trace, storage=None):
    from oracle import emsanet_oracle as O
    from test_model_gpu import _PinnedRelu
    pinned = _PinnedRelu(trace)
    saved = O.Spec.STORAGE
    O.Spec.STORAGE = storage
    try:
        total, losses = trainer.step(batch, targets, relu=pinned)
    finally:
        O.Spec.STORAGE = saved
    assert pinned.i == len(trace), f"oracle made {pinned.i} ReLU calls, engine {len(trace)}"
    return float(total), {k: float(v) for k, v in losses.items()}, pinned


def _rel(a, b):
    return abs(a - b) / max(1e-30, abs(b))


def test_fp32_trajectory_matches_fp64_oracle():
    from oracle.training_oracle import OracleTrainer, targets_to
    from test_model_gpu import _argmax_check, _flatten
    args, model, oracle, batches, targets, cw, n_scene = _setup()
    eng = _EngineLoop(model, args, cw, n_scene, K32)
    orc = OracleTrainer(oracle, args, cw, n_scene, K32)
    b64 = [{k: v.double() for k, v in b.items()} for b in batches]
    t64 = [targets_to(t, dtype=torch.float64) for t in targets]
    p_init = {k: p.detach().clone() for k, p in oracle.named_parameters()}
    r_init = {k: b.detach().clone() for k, b in oracle.named_buffers() if 'running' in k}
    worst_loss, worst_flips, sched_err = [], [], 0.0
    for i in range(K32):
        g = orc.opt.param_groups[0]
        (lr, mom), trace, tot_e, l_e = eng.step(batches[i % 4], targets[i % 4])
        sched_err = max(sched_err, _rel(lr, g['lr']), _rel(mom, g['momentum']))
        tot_o, l_o, pinned = _oracle_step(orc, b64[i % 4], t64[i % 4], trace)
        errs = {k: _rel(l_e[k], l_o[k]) for k in l_o}
        errs['total'] = _rel(tot_e, tot_o)
        k_w = max(errs, key=errs.get)
        worst_loss.append((errs[k_w], k_w))
        worst_flips.append(pinned.flips / pinned.total)
        print(f"fp32 step {i:2d}: lr {lr:.3e} momentum {mom:.4f} total {tot_o:.6f} "
              f"(engine {tot_e:.6f}); worst loss rel err {errs[k_w]:.2e} ({k_w}); "
              f"{pinned.flips} of {pinned.total} ReLU decisions differ")
    # parameters against their movement
    mp, op = dict(model.named_parameters()), dict(oracle.named_parameters())
    move, move_zero = [], []
    for k, p64 in op.items():
        p64 = p64.detach()
        d = (mp[k].detach().cpu().double() - p64).norm().item()
        mv = (p64 - p_init[k]).norm().item()
        if k.endswith(ZERO_GRAD):
            # the oracle moves these by weight decay alone; the engine adds its roundoff gradient
            move_zero.append((d / max(mv, 1e-30), k))
        else:
            move.append((d / (mv + EPS_32 / MOVE_TOL_32 * p64.norm().item()), d / max(mv, 1e-30), k))
    move.sort()
    move_zero.sort()
    # momentum buffers
    bufs = eng.momentum_buffers()
    bmax = max(orc.opt.state[p]['momentum_buffer'].abs().max().item() for p in op.values())
    mom_err, mom_zero = [], []
    for k, p in mp.items():
        r = orc.opt.state[op[k]]['momentum_buffer']
        e = bufs[p].detach().cpu().double()
        if k.endswith(ZERO_GRAD):
            mom_zero.append(((e - r).abs().max().item() / bmax, k))
        else:
            mom_err.append(((e - r).norm().item() / r.norm().item(), k))
    mom_err.sort()
    mom_zero.sort()
    # running statistics against their movement
    mb, ob = dict(model.named_buffers()), dict(oracle.named_buffers())
    run_err = sorted(((mb[k].detach().cpu().double() - ob[k]).norm().item()
                      / max(1e-30, (ob[k] - r_init[k]).norm().item()), k) for k in r_init)
    print(f"fp32 after {K32} steps: schedule vs torch OneCycleLR {sched_err:.1e}; parameters "
          f"|p_eng - p_64| / (|movement| + eps|p|): worst {move[-1][0]:.2e} ({move[-1][2]}), "
          f"median {move[len(move) // 2][0]:.2e}; /|movement| alone worst {max(m[1] for m in move):.2e}; "
          f"biases with a zero gradient (weight decay only) worst {move_zero[-1][0]:.2e} "
          f"({move_zero[-1][1]}), median {move_zero[len(move_zero) // 2][0]:.2e}")
    print(f"fp32 momentum buffers rel-L2: worst {mom_err[-1][0]:.2e} ({mom_err[-1][1]}), median "
          f"{mom_err[len(mom_err) // 2][0]:.2e}; zero-gradient biases {mom_zero[-1][0]:.2e} of the "
          f"largest buffer; running stats / movement: worst {run_err[-1][0]:.2e} ({run_err[-1][1]}),"
          f" median {run_err[len(run_err) // 2][0]:.2e}")
    print(f"fp32 per-step worst loss error: {' '.join(f'{e:.1e}' for e, _ in worst_loss)}; "
          f"flips: {' '.join(f'{f:.1e}' for f in worst_flips)}")
    # counters
    msd, osd = model.state_dict(), oracle.state_dict()
    n_bt = [k for k in osd if k.endswith('num_batches_tracked')]
    assert n_bt and all(int(msd[k]) == int(osd[k]) == K32 for k in n_bt), \
        [(k, int(msd[k]), int(osd[k])) for k in n_bt if int(msd[k]) != int(osd[k])][:5]
    assert model.dropout_step == oracle.dropout_step == K32
    # eval forward of both trained models; and of the oracle holding the ENGINE's trained state (what
    # the eval kernels owe on updated weights and running statistics, stale packed caches included)
    model.eval(), oracle.eval()
    twin = copy.deepcopy(oracle)
    twin.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        fo = _flatten(model({k: v.to(DEV) for k, v in batches[0].items()}))
        fr = _flatten(oracle(b64[0]))
        ft = _flatten(twin(b64[0]))

    def max_err(got, ref):
        return [(a.detach().cpu().double() - b).abs().max().item() / max(1.0, b.abs().max().item())
                for a, b in zip(got, ref)]
    ev, ev_twin = max_err(fo, fr), max_err(fo, ft)
    print(f"fp32 eval after training, max err per output vs the trained oracle "
          f"{' '.join(f'{e:.1e}' for e in ev)}; vs the oracle on the engine's trained state "
          f"{' '.join(f'{e:.1e}' for e in ev_twin)}")
    assert sched_err <= 1e-9
    assert max(e for e, _ in worst_loss) <= LOSS_TOL_32, worst_loss
    assert max(worst_flips) <= FLIPS_REL, worst_flips
    assert move[-1][0] <= MOVE_TOL_32, move[-3:]
    # the buffers after the last step hold mostly that step's gradient (whose lr, 4e-9, no longer
    # moves the parameters): gradients taken on parameters that already differ by 3e-3 of their
    # movement, through ~100 batch-statistics BatchNorms -- hence the wider band than the parameters'
    assert mom_err[-1][0] <= MOM_TOL_32, mom_err[-3:]
    assert move_zero[-1][0] <= ZERO_MOVE_TOL_32, move_zero[-3:]
    assert mom_zero[-1][0] <= 1e-4, mom_zero[-3:]
    assert run_err[-1][0] <= RUN_TOL_32, run_err[-3:]
    assert max(ev_twin) <= EVAL_TOL, ev_twin
    _argmax_check(fo[0], ft[0], 'semantic (eval on the trained state)')
    assert max(ev) <= EVAL_TRAJ_TOL, ev


def test_bf16_trajectory_matches_storage_emulating_oracle():
    from oracle.training_oracle import OracleTrainer, targets_to
    args, model, emu, batches, targets, cw, n_scene = _setup()
    plain = copy.deepcopy(emu)
    model.set_compute_dtype(torch.bfloat16)
    eng = _EngineLoop(model, args, cw, n_scene, K16)
    t_emu = OracleTrainer(emu, args, cw, n_scene, K16)
    t_plain = OracleTrainer(plain, args, cw, n_scene, K16)
    b64 = [{k: v.double() for k, v in b.items()} for b in batches]
    t64 = [targets_to(t, dtype=torch.float64) for t in targets]
    p_init = {k: p.detach().clone() for k, p in emu.named_parameters()}
    loss_err, loss_err_plain = [], []
    for i in range(K16):
        _, trace, tot_e, l_e = eng.step(batches[i % 4], targets[i % 4])
        tot_q, l_q, pin_q = _oracle_step(t_emu, b64[i % 4], t64[i % 4], trace, torch.bfloat16)
        tot_p, l_p, _ = _oracle_step(t_plain, b64[i % 4], t64[i % 4], trace, None)
        e = {k: _rel(l_e[k], l_q[k]) for k in l_q}
        e['total'] = _rel(tot_e, tot_q)
        ep = {k: _rel(l_p[k], l_q[k]) for k in l_q}
        ep['total'] = _rel(tot_p, tot_q)
        kw = max(e, key=e.get)
        loss_err.append((e[kw], kw))
        loss_err_plain.append(max(ep.values()))
        print(f"bf16 step {i}: total emulating {tot_q:.5f} engine {tot_e:.5f} plain fp64 {tot_p:.5f}; "
              f"worst loss rel err engine {e[kw]:.2e} ({kw}), plain-vs-emulating "
              f"{loss_err_plain[-1]:.2e}; {pin_q.flips} of {pin_q.total} ReLU decisions differ")

    def movement(params):
        return {k: p.detach().cpu().double() - p_init[k] for k, p in params}

    m_e, m_q, m_p = movement(model.named_parameters()), movement(emu.named_parameters()), \
        movement(plain.named_parameters())
    mp = dict(model.named_parameters())

    def compare(a, b):
        names = [k for k in b if not k.endswith(ZERO_GRAD)]
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
    print(f"bf16 after {K16} steps, movement engine vs emulating oracle: whole-model cosine "
          f"{cos_all:.4f}; per tensor (>= 1024 el.) cosine min {cb.min():.4f} ({nb[int(cb.argmin())]}) "
          f"median {cb.median():.4f}; norm ratio {rb.min():.3f} ({nb[int(rb.argmin())]}) .. "
          f"{rb.max():.3f} ({nb[int(rb.argmax())]}), median {rb.median():.4f}; all tensors cosine min "
          f"{cos.min():.4f} ratio {ratio.min():.3f} .. {ratio.max():.3f}")
    print(f"bf16 storage itself (plain fp64 vs emulating, same masks): whole-model cosine "
          f"{cos_all_p:.4f}; per tensor cosine min {cos_p[big].min():.4f} median "
          f"{cos_p[big].median():.4f}; norm ratio {ratio_p[big].min():.3f} .. {ratio_p[big].max():.3f}"
          f" median {ratio_p[big].median():.4f}; losses {' '.join(f'{e:.1e}' for e in loss_err_plain)}")
    print(f"bf16 per-step worst loss error engine vs emulating: "
          f"{' '.join(f'{e:.1e}' for e, _ in loss_err)}")
    assert model.dropout_step == emu.dropout_step == K16
    assert max(e for e, _ in loss_err) <= LOSS_TOL_16, loss_err
    assert cos_all >= MOVE_COS_ALL_16
    assert cb.min().item() >= MOVE_COS_16, (nb[int(cb.argmin())], cb.min().item())
    assert MOVE_RATIO_16[0] <= rb.min().item() and rb.max().item() <= MOVE_RATIO_16[1], \
        (nb[int(rb.argmin())], rb.min().item(), nb[int(rb.argmax())], rb.max().item())
