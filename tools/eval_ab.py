#!/usr/bin/env python
"""A/B of the evaluation loop's per-frame cost, one process, on one 512x512 config-2 synthetic frame.

  (a) the way evaluation runs with the stock host evaluator: ``Renderer.render`` (outputs copied to the
      host), float64 PSNR on the host, SSIM by the scipy ``uniform_filter`` restatement of the reference's
      ``structural_similarity`` call (tests/ssim_ref.py);
  (b) ``Renderer.render_device`` + ``Evaluator.evaluate`` (anr_eval_frame on the device), with one
      ``summarize()`` per round inside the timed span.

After a warm-up, ROUNDS rounds alternate FRAMES frames of each leg (order swapped every round, each leg
timed wall-clock between device synchronisations). Prints the per-frame median / minimum / maximum over
the rounds per leg, leg (b)'s evaluator cost per frame from device events (measured apart from the timed
rounds, evaluate() calls back to back on a rendered frame), the difference of the two legs' numbers, and
one JSON line.

    python tools/eval_ab.py [--rounds 10] [--frames 10] [--side 512]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import config, network, synthetic  # noqa: E402
from animatable_nerf_amd.evaluator import Evaluator  # noqa: E402
from animatable_nerf_amd.renderer import Renderer, near_far  # noqa: E402
from tests import ssim_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--side', type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_ab.py needs a GPU: there is nothing to time without one')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    H = W = args.side
    # the benchmark's frame (bench.py render mode): side^2 box rays, the hit mask as the frame's mask_at_box
    sc = synthetic.Scene(vsize=0.025)
    ro, rd = sc.box_rays(H * W, seed=2)
    nr, fr, m = near_far(torch.from_numpy(sc.bounds).to(dev), torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev))
    m_np = m.cpu().numpy()
    n = int(m_np.sum())
    gt = np.random.Generator(np.random.PCG64(9)).uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    b = sc.batch_arrays(ro[m_np], rd[m_np], nr.cpu().numpy(), fr.cpu().numpy(), rgb=gt)
    b.update(mask_at_box=m_np.reshape(1, -1), H=np.array([H]), W=np.array([W]))
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    batch['H'], batch['W'] = torch.tensor([H]), torch.tensor([W])  # host integers: no per-frame copy
    net = network.Network()
    network.load_numpy_state(net, synthetic.init_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    net = net.to(dev)
    net.train()  # run.py evaluates in train() mode with perturb = 0
    cfg = config.defaults()
    cfg.perturb = 0
    cfg.result_dir = tempfile.mkdtemp(prefix='eval_ab_')
    renderer = Renderer(net, cfg)
    ev = Evaluator()
    ev.cfg = cfg
    last = {}

    def leg_a(frames):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(frames):
            with torch.no_grad():
                out = renderer.render(batch)
            pred = out['rgb_map'][0].numpy()
            mse = ssim_ref.mse_f64(pred, gt)
            last['a'] = (mse, float(ssim_ref.psnr(mse)), ssim_ref.frame_ssim(pred, gt, m_np, H, W))
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / frames * 1e3

    def leg_b(frames):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(frames):
            with torch.no_grad():
                ev.evaluate(renderer.render_device(batch), batch)
        got = ev.summarize()
        torch.cuda.synchronize(dev)
        last['b'] = (got['mse'][-1], got['psnr'][-1], got['ssim'][-1])
        return (time.perf_counter() - t0) / frames * 1e3

    legs = {'a': leg_a, 'b': leg_b}
    for f in legs.values():
        f(args.warmup)
    times = {'a': [], 'b': []}
    for r in range(args.rounds):
        for k in (('a', 'b') if r % 2 == 0 else ('b', 'a')):
            times[k].append(legs[k](args.frames))

    # the evaluator alone, from device events: evaluate() back to back on one rendered frame
    with torch.no_grad():
        out = renderer.render_device(batch)
    for _ in range(3):
        ev.evaluate(out, batch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        ev.evaluate(out, batch)
    e1.record()
    torch.cuda.synchronize(dev)
    eval_ms = e0.elapsed_time(e1) / reps
    ev.summarize()

    names = {'a': 'render + host psnr/ssim (scipy)', 'b': 'render_device + Evaluator'}
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'frame {H}x{W}, {n} in-box rays, {args.rounds} rounds x {args.frames} frames per leg')
    for k, v in times.items():
        print(f'({k}) {names[k]:34s} ms/frame: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}  '
              f'rounds {" ".join(f"{x:.2f}" for x in v)}')
    print(f'(b) evaluator alone (device events, {reps} calls): {eval_ms:.4f} ms/frame = '
          f'{100.0 * eval_ms / med["b"]:.3f} % of leg (b)\'s frame')
    for i, q in enumerate(('mse', 'psnr', 'ssim')):
        print(f'{q}: (a) {last["a"][i]!r}  (b) {last["b"][i]!r}  |diff| {abs(last["a"][i] - last["b"][i]):.3e}')
    print(json.dumps({'side': args.side, 'rays': n, 'rounds': args.rounds, 'frames': args.frames,
                      'a_ms': {'median': med['a'], 'min': min(times['a']), 'max': max(times['a']), 'rounds': times['a']},
                      'b_ms': {'median': med['b'], 'min': min(times['b']), 'max': max(times['b']), 'rounds': times['b']},
                      'evaluator_ms': eval_ms, 'a': last['a'], 'b': last['b']}))


if __name__ == '__main__':
    main()
