#!/usr/bin/env python
"""A/B of the deterministic training mode against the default mode, one process.

For each precision (bf16_all, fp32): two FusedSteps on identical networks, one per mode, fed the same
1,024-ray batches; after a warm-up, ROUNDS rounds alternate 50 default-mode steps and 50 deterministic
steps (each round timed wall-clock between device synchronisations), so both modes see the same clocks
and neighbours. Prints, per precision and mode, the per-step median / minimum / maximum over the rounds
and the deterministic : default ratio of the medians, then one JSON line.

    python tools/train_det_ab.py [--rounds 10] [--steps 50] [--rays 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import config  # noqa: E402
from animatable_nerf_amd.trainer import FusedStep  # noqa: E402
from tests.quality import frame, make_net, sub  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--precisions', default='bf16_all,fp32')
    args = ap.parse_args()
    if os.environ.get('ANR_TRAIN_DETERMINISTIC') is not None:
        sys.exit('unset ANR_TRAIN_DETERMINISTIC: it overrides the per-step mode this script alternates')
    dev = torch.device('cuda:0')
    batch, gt = frame(dev, frame_rays=64 * 1024)
    R = int(batch['ray_o'].shape[1])
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    # a fixed pool of batches, reused by both modes (device tensors: the steps read them in place)
    pool = []
    for _ in range(8):
        idx = torch.randint(0, R, (args.rays,), device=dev, generator=g)
        pool.append((sub(batch, idx, gt[idx]), torch.rand((args.rays, 64), device=dev, generator=g)))
    result = {'rays': args.rays, 'rounds': args.rounds, 'steps': args.steps, 'modes': {}}
    for prec in args.precisions.split(','):
        cfg = config.subject('aninerf_313', perturb=1, train_precision=prec)
        steps = {}
        for mode in ('default', 'deterministic'):
            net = make_net(cfg, 1234, dev)
            net.train()
            steps[mode] = FusedStep(net, cfg, deterministic=(mode == 'deterministic'))
        times = {'default': [], 'deterministic': []}

        def run(mode, n):
            st = steps[mode]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(n):
                b, tr = pool[i % len(pool)]
                st.step(b, t_rand=tr)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / n * 1e3

        for mode in times:
            run(mode, args.warmup)
        for r in range(args.rounds):
            for mode in (('default', 'deterministic') if r % 2 == 0 else ('deterministic', 'default')):
                times[mode].append(run(mode, args.steps))
        med = {m: statistics.median(v) for m, v in times.items()}
        for m, v in times.items():
            print(f'{prec:9s} {m:14s} ms/step: median {med[m]:.4f}  min {min(v):.4f}  max {max(v):.4f}  '
                  f'rounds {" ".join(f"{x:.4f}" for x in v)}')
        ratio = med['deterministic'] / med['default']
        print(f'{prec:9s} deterministic / default (medians): {ratio:.4f}')
        result['modes'][prec] = {m: {'median_ms': med[m], 'min_ms': min(v), 'max_ms': max(v), 'rounds_ms': v}
                                 for m, v in times.items()}
        result['modes'][prec]['ratio'] = ratio
        del steps
    print(json.dumps(result))


if __name__ == '__main__':
    main()
