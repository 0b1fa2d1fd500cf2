#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Times the graphed training step in bf16 and in fp16 storage at the same shape on one GPU.

Three configurations are built once and then timed in turn, `--reps` times over (alternating, so
that clock and thermal drift hit all of them alike):

    bf16          GraphedTrainStep, FusedSGD                       (the existing mixed-precision step)
    bf16+scaler   the same with a LossScaler attached              (cost of scan + state update)
    fp16+scaler   float16 storage under the LossScaler             (the unfused weight-gradient routes)

The step is bench.py's: full RGB-D model, all four heads, fixed output cotangents, lr 0 (every step
starts from the same weights), the whole step one hipGraph replay; `--losses` runs the device-side
task losses instead (there the scaler adds no multiply kernel).  Prints one JSON line.

    python tools/fp16_train_bench.py --batch-size 32 --height 480 --width 640 --steps 20 --reps 3
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def flatten(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        return [t for v in out.values() for t in flatten(v)]
    if isinstance(out, (list, tuple)):
        return [t for v in out for t in flatten(v)]
    return []


def build(dtype, with_scaler, args, batch, dev):
    from emsanet_amd import full_args, nyuv2_config
    from emsanet_amd.graph import GraphedTrainStep
    from emsanet_amd.model import EMSANet
    from emsanet_amd.optim import FusedSGD, LossScaler
    from emsanet_amd.parallel import GradientBuckets
    torch.manual_seed(0)
    a = full_args(input_height=args.height, input_width=args.width)
    model = EMSANet(a, nyuv2_config()).to(dev).train()
    model.dropout_seed = 1234
    model.set_compute_dtype(dtype)
    buckets = GradientBuckets([p for p in model.parameters() if p.requires_grad])
    opt = FusedSGD(buckets, lr=0.0, momentum=0.9, weight_decay=1e-4)
    scaler = LossScaler(opt, init_scale=args.init_scale).attach(model) if with_scaler else None
    flat0 = flatten(model(batch))
    g = torch.Generator(device='cpu').manual_seed(4321)
    cots = [(torch.randn(t.shape, generator=g) * 1e-3).to(dev).contiguous(
        memory_format=torch.channels_last if t.dim() == 4 else torch.contiguous_format) for t in flat0]
    del flat0
    model.dropout_step = 0
    if args.losses:
        # the complete training step: all task losses on the device (bench.py --losses); the scaler
        # then seeds the backward pass with its scale and adds no kernel in front of the scan
        from bench import training_losses_and_targets
        crit, targets = training_losses_and_targets(a, args.batch_size, args.height, args.width, dev)
        step = GraphedTrainStep(model, batch, buckets, opt, loss_fn=lambda out: crit(out, targets)[0],
                                loss_scaler=scaler)
    else:
        # fixed output cotangents: with a scaler every cotangent is multiplied by the scale inside
        # the step (LossScaler.scale_cotangents: one read + write of every output per step)
        step = GraphedTrainStep(model, batch, buckets, opt, cotangents=cots, loss_scaler=scaler)
    return step, scaler, buckets


def time_replays(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    step.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        step.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--steps', type=int, default=20, help='replays per timed block')
    ap.add_argument('--reps', type=int, default=3, help='timed blocks per configuration, alternating')
    ap.add_argument('--init-scale', type=float, default=2.0 ** 10)
    ap.add_argument('--losses', action='store_true',
                    help='loss.backward() on the device-side task losses instead of fixed output cotangents')
    args = ap.parse_args()
    from oracle.emsanet_oracle import synthetic_batch
    dev = torch.device('cuda:0')
    batch = {k: v.to(dev) for k, v in synthetic_batch(args.batch_size, args.height, args.width, seed=1).items()}
    configs = [('bf16', torch.bfloat16, False), ('bf16+scaler', torch.bfloat16, True),
               ('fp16+scaler', torch.float16, True)]
    built = {name: build(dtype, sc, args, batch, dev) for name, dtype, sc in configs}
    ms = {name: [] for name in built}
    for _ in range(args.reps):
        for name, (step, _, _) in built.items():
            ms[name].append(round(time_replays(step, args.steps), 4))
    res = {'tool': 'fp16_train_bench', 'mode': 'losses' if args.losses else 'cotangents', 'batch_size': args.batch_size, 'height': args.height,
           'width': args.width, 'steps_per_block': args.steps, 'init_scale': args.init_scale,
           'device': torch.cuda.get_device_name(0), 'ms_per_step': ms,
           'median_ms': {k: round(statistics.median(v), 4) for k, v in ms.items()},
           'gradient_bytes': built['bf16'][2].n_bytes(),
           'scaler_state': {k: s.state() for k, (_, s, _) in built.items() if s is not None}}
    m = res['median_ms']
    res['scaler_cost_pct_bf16'] = round(100.0 * (m['bf16+scaler'] / m['bf16'] - 1.0), 3)
    res['fp16_vs_bf16_pct'] = round(100.0 * (m['fp16+scaler'] / m['bf16'] - 1.0), 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
