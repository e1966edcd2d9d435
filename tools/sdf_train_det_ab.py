#!/usr/bin/env python
"""A/B of the deterministic training mode against the default mode on the sdf_pdf step, one process.

For each precision (fp32, bf16x3): two SdfSteps on identical networks, one per mode, fed the same 1,024-ray
batches (bench.py --mode sdf-train's scene and batch recipe); after a warm-up, ROUNDS rounds alternate STEPS
default-mode steps and STEPS deterministic steps (each round timed wall-clock between device
synchronisations), so both modes see the same clocks and neighbours. Prints, per precision and mode, the
per-step median / minimum / maximum over the rounds and the deterministic : default ratio of the medians,
the two workspace sizes, then one JSON line.

    python tools/sdf_train_det_ab.py [--rounds 10] [--steps 20] [--rays 1024]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import _lib, config, network, network_sdf, synthetic  # noqa: E402
from animatable_nerf_amd.renderer import near_far  # noqa: E402
from animatable_nerf_amd.trainer_sdf import SdfStep  # noqa: E402


def batches(dev, rays, n=4):
    sc = synthetic.PdfScene(vsize=0.05)
    out = []
    for j in range(n):
        ro, rd = sc.box_rays(rays * 2, seed=2000 + j)
        nr, fr, m = near_far(torch.from_numpy(sc.pbounds).to(dev), torch.from_numpy(ro).to(dev),
                             torch.from_numpy(rd).to(dev))
        m_np = m.cpu().numpy()
        rgb = np.random.default_rng(j).random((len(ro), 3)).astype(np.float32)
        b = sc.batch_arrays(ro[m_np][:rays], rd[m_np][:rays], nr.cpu().numpy()[:rays], fr.cpu().numpy()[:rays],
                            latent_index=7, rgb=rgb[m_np][:rays])
        bt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
        bt['iter_step'] = 12000
        out.append(bt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--precisions', default='fp32,bf16x3')
    args = ap.parse_args()
    if os.environ.get('ANR_TRAIN_DETERMINISTIC') is not None:
        sys.exit('unset ANR_TRAIN_DETERMINISTIC: it overrides the per-step mode this script alternates')
    dev = torch.device('cuda:0')
    pool = batches(dev, args.rays)
    tb0 = [b['tbounds'].clone() for b in pool]
    o = _lib.RenderOpts()
    o.n_samples, o.chunk = 64, int(config.subject('anisdf_pdf_s9p').get('chunk', 2048))
    ws_bytes = int(_lib.load().anr_sdf_train_workspace_bytes(args.rays, ctypes.byref(o)))
    print(f'anr_sdf_train_workspace_bytes({args.rays}, chunk {o.chunk}) = {ws_bytes}')
    result = {'rays': args.rays, 'rounds': args.rounds, 'steps': args.steps, 'workspace_bytes': ws_bytes, 'modes': {}}
    for prec in args.precisions.split(','):
        cfg = config.subject('anisdf_pdf_s9p', perturb=1, sdf_train_precision=prec)
        steps = {}
        for mode in ('default', 'deterministic'):
            net = network_sdf.Network(cfg)
            sd = synthetic.init_state_dict_sdf({k: tuple(v.shape) for k, v in net.state_dict().items()})
            network.load_numpy_state(net, sd)
            net = net.to(dev)
            net.train()
            steps[mode] = SdfStep(net, cfg, deterministic=(mode == 'deterministic'))
        times = {'default': [], 'deterministic': []}

        def run(mode, n):
            st = steps[mode]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(n):
                k = i % len(pool)
                pool[k]['tbounds'].copy_(tb0[k])
                st.step(pool[k])
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / n * 1e3

        for mode in times:
            run(mode, args.warmup)
        for r in range(args.rounds):
            for mode in (('default', 'deterministic') if r % 2 == 0 else ('deterministic', 'default')):
                times[mode].append(run(mode, args.steps))
        med = {m: statistics.median(v) for m, v in times.items()}
        for m, v in times.items():
            print(f'{prec:7s} {m:14s} ms/step: median {med[m]:.4f}  min {min(v):.4f}  max {max(v):.4f}  '
                  f'rounds {" ".join(f"{x:.4f}" for x in v)}')
        ratio = med['deterministic'] / med['default']
        print(f'{prec:7s} deterministic / default (medians): {ratio:.4f}')
        result['modes'][prec] = {m: {'median_ms': med[m], 'min_ms': min(v), 'max_ms': max(v), 'rounds_ms': v}
                                 for m, v in times.items()}
        result['modes'][prec]['ratio'] = ratio
        del steps
    print(json.dumps(result))


if __name__ == '__main__':
    main()
