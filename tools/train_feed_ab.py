#!/usr/bin/env python
"""A/B of what a training iteration costs with its rays drawn three ways, one process, one synthetic
view of SIDE x SIDE pixels (512) on the benchmark's training scene, 1,024 rays per iteration:

  (a) ``data.sample_ray_h36m(split='train')`` (np.random draws on the host, a device round per
      resampling round, image and masks uploaded every call), then ``FusedStep.step``;
  (b) ``data.ResidentViews.sample`` (one launch, nothing from the host), then ``FusedStep.step``;
  (c) ``FusedStep.step`` on one fixed batch: the number ``bench.py --mode train`` reports.

The bound mask is the projected box dilated by --dilate pixels, so that some drawn rays miss the box
and both samplers run several rounds (the dataset's masks do the same at the box's silhouette).

After a warm-up, ROUNDS rounds run ITERS iterations of each leg, the order rotated every round, each
leg timed on the host clock between device synchronisations. Prints the per-iteration median / minimum
/ maximum over the rounds per leg, the sampler launch alone from device events (measured apart from
the timed rounds, sample() calls back to back), the rounds a batch took, the launch's time on masks that
need more and more rounds (what a round costs inside the single workgroup), and one JSON line.

    python tools/train_feed_ab.py [--rounds 10] [--iters 50] [--side 512] [--dilate 8] [--precision bf16_all]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import config, data, network, synthetic  # noqa: E402
from animatable_nerf_amd.trainer import FusedStep  # noqa: E402
from tests.philox_ref import PhiloxDraws  # noqa: E402


class CountingRNG:
    """np.random.RandomState that counts the sampling rounds (randint calls / calls per round)."""

    def __init__(self, seed, calls_per_round):
        self.rs, self.calls, self.per = np.random.RandomState(seed), 0, calls_per_round

    def randint(self, lo, hi, n):
        self.calls += 1
        return self.rs.randint(lo, hi, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--side', type=int, default=512)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--dilate', type=int, default=8)
    ap.add_argument('--precision', choices=('fp32', 'bf16', 'bf16_all'), default='bf16_all')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('train_feed_ab.py needs a GPU: there is nothing to time without one')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    H = W = args.side
    sc = synthetic.Scene(vsize=0.025)
    f = 300.0 * args.side / 256.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], dtype=np.float32)
    R = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]], dtype=np.float32)
    T = np.array([[0.0], [0.0], [3.0]], dtype=np.float32)
    bm0 = data.get_bound_2d_mask(sc.bounds, K, np.concatenate([R, T], axis=1), H, W)
    msk = bm0.copy()  # every pixel of the projected box a body pixel

    def dilated(px):
        d = np.zeros_like(bm0)
        for dy in range(-px, px + 1):
            for dx in range(-px, px + 1):
                d |= np.roll(np.roll(bm0, dy, 0), dx, 1)
        return d
    bm = dilated(args.dilate)
    img = np.random.Generator(np.random.PCG64(9)).random((H, W, 3), dtype=np.float32)

    z = np.zeros((1, 3), np.float32)
    frame = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
             for k, v in sc.batch_arrays(z, z, np.zeros(1, np.float32), np.zeros(1, np.float32)).items()
             if k not in ('ray_o', 'ray_d', 'near', 'far', 'rgb', 'mask_at_box', 'occupancy')}
    cfg = config.subject('aninerf_313', perturb=1, train_precision=args.precision)
    net = network.Network(cfg)
    network.load_numpy_state(net, synthetic.init_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    net = net.to(dev)
    net.train()
    step = FusedStep(net, cfg)
    rv = data.ResidentViews(dev, nrays=args.rays, seed=1)
    rv.add('v', img, msk, K, R, T, sc.bounds, bound_mask=bm)
    rng = CountingRNG(0, 2)
    it = [0]

    def batch_a():
        rgb, ro, rd, near, far, coord, mab = data.sample_ray_h36m(img, msk, K, R, T, sc.bounds, args.rays, 'train',
                                                                  bound_mask=bm, rng=rng, device=dev)
        b = dict(frame)
        b.update(rgb=rgb[None], ray_o=ro[None], ray_d=rd[None], near=near[None], far=far[None],
                 mask_at_box=mab[None], coord=coord[None])
        return b

    def batch_b():
        it[0] += 1
        b = dict(frame)
        b.update(rv.sample('v', it[0]))
        return b

    fixed = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch_b().items() if k != 'anr_volatile'}
    feeds = {'a': batch_a, 'b': batch_b, 'c': lambda: fixed}

    def leg(k, iters):
        feed = feeds[k]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            step.step(feed())
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / iters * 1e3

    for k in feeds:
        leg(k, args.warmup)
    calls0, n_a = rng.calls, 0
    times = {k: [] for k in feeds}
    order = ['a', 'b', 'c']
    for r in range(args.rounds):
        for k in order[r % 3:] + order[:r % 3]:
            times[k].append(leg(k, args.iters))
            n_a += args.iters if k == 'a' else 0
    rounds_a = (rng.calls - calls0) / rng.per / max(n_a, 1)

    # the sampler launch alone, from device events: sample() back to back
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 200
    for _ in range(10):
        batch_b()
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        batch_b()
    e1.record()
    torch.cuda.synchronize(dev)
    sample_ms = e0.elapsed_time(e1) / reps
    # the same calls on the host clock: what sample() costs the issuing thread
    t0 = time.perf_counter()
    for _ in range(reps):
        batch_b()
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    torch.cuda.synchronize(dev)
    short = rv.shortfall()

    # what a round costs inside the single workgroup: the launch by device events on masks that need more
    # and more rounds; the rounds of a (seed, step) are counted by replaying its draws through
    # sample_ray_h36m (tests/philox_ref.py; the two paths take the same rounds, tests/test_gpu_resident_views.py)
    per_round = []
    for px in (0, args.dilate, 4 * args.dilate, 8 * args.dilate):
        bmx = dilated(px)
        rv.add(('d', px), img, msk, K, R, T, sc.bounds, bound_mask=bmx)
        nr = []
        for s in range(1, 9):
            pr = PhiloxDraws(1, s, 2)
            data.sample_ray_h36m(img, msk, K, R, T, sc.bounds, args.rays, 'train', bound_mask=bmx, rng=pr, device=dev)
            nr.append(pr.rounds)
        for _ in range(10):
            rv.sample(('d', px), 1)
        torch.cuda.synchronize(dev)
        e0.record()
        for i in range(reps):
            rv.sample(('d', px), 1 + i % 8)
        e1.record()
        torch.cuda.synchronize(dev)
        per_round.append((px, statistics.mean(nr), e0.elapsed_time(e1) / reps * 1e3))
    short_all = rv.shortfall()

    names = {'a': 'sample_ray_h36m + FusedStep.step', 'b': 'ResidentViews.sample + FusedStep.step',
             'c': 'FusedStep.step, fixed batch'}
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'view {H}x{W}, {args.rays} rays, {args.precision}, bound mask dilated {args.dilate} px, '
          f'{args.rounds} rounds x {args.iters} iterations per leg')
    for k, v in times.items():
        print(f'({k}) {names[k]:38s} ms/iteration: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}  '
              f'rounds {" ".join(f"{x:.2f}" for x in v)}')
    print(f'(a) - (c) = {med["a"] - med["c"]:.3f} ms   (b) - (c) = {med["b"] - med["c"]:.3f} ms   '
          f'(a) / (b) = {med["a"] / med["b"]:.2f}')
    print(f'sampler launch alone (device events, {reps} calls back to back): {sample_ms * 1e3:.1f} us; '
          f'host time of sample(): {host_ms * 1e3:.1f} us')
    print(f'sampling rounds per batch in leg (a): {rounds_a:.2f}; rays missing from all of leg (b)\'s batches: {short}')
    for px, nr, us in per_round:
        print(f'sampler launch, mask dilated {px:3d} px: {nr:5.2f} rounds per batch (steps 1..8), {us:6.1f} us per launch')
    (_, r0, u0), (_, r1, u1) = per_round[0], per_round[-1]
    print(f'slope between the first and the last row: {(u1 - u0) / max(r1 - r0, 1e-9):.2f} us per round; '
          f'rays missing in these launches: {short_all - short}')
    print(json.dumps({'side': args.side, 'rays': args.rays, 'precision': args.precision, 'dilate': args.dilate,
                      'rounds': args.rounds, 'iters': args.iters,
                      **{f'{k}_ms': {'median': med[k], 'min': min(v), 'max': max(v), 'rounds': v}
                         for k, v in times.items()},
                      'sampler_us': sample_ms * 1e3, 'sample_host_us': host_ms * 1e3, 'rounds_per_batch_a': rounds_a,
                      'shortfall_b': short, 'sampler_by_dilation': [list(t) for t in per_round]}))


if __name__ == '__main__':
    main()
