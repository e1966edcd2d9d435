#!/usr/bin/env python
"""A/B of the full render program against the image-only one (cfg render_image_only), one process, on the
512x512 config-2 synthetic frame of bench.py, in each render precision.

  (full)  ``Renderer.render_device(batch)``: anr_render_fwd, the pbw / tbw alpha_ind rows gathered;
  (image) ``Renderer.render_device(batch, image_only=True)``: anr_render_image_fwd, the four image outputs.

Per precision, after a warm-up:
* ROUNDS rounds alternate the two legs (order swapped every round), each leg FRAMES frames between two device
  events: per-frame median / min / max over the rounds. The image leg passes when its median is below the full
  leg's by more than the full leg's own min-max spread;
* the fused network kernel alone (k_mlp* against k_mlp_img*): the library's event pair around the launch and the
  shader clock from the in-kernel stamps (anr_profile_read_clock), again alternating, outside the timed rounds;
  kernel-time ratio and cycle ratio (ms x MHz) beside the ratio of executed MFMAs (16,168 / 23,976 = 0.674);
* ``Renderer.render(batch)`` (outputs on the host) with and without the key, wall clock between device
  synchronisations: the host leg of both;
* the four image outputs of both legs compared bit for bit.
Prints a table and one JSON line.

    python tools/render_image_ab.py [--rounds 7] [--frames 5] [--side 512] [--precisions fp32,bf16x3,bf16x6]
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

from animatable_nerf_amd import config, network, synthetic  # noqa: E402
from animatable_nerf_amd.renderer import Renderer, near_far  # noqa: E402

MFMA_RATIO = 16168 / 23976  # fp32 MFMAs per tile and wave, image program / render program (anr_mlp_body.h)
KEYS = ('rgb_map', 'acc_map', 'depth_map', 'raw')


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'rounds': v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--side', type=int, default=512)
    ap.add_argument('--precisions', default='fp32,bf16x3,bf16x6')
    args = ap.parse_args()
    if args.rounds < 7:
        sys.exit('render_image_ab.py: at least 7 alternating rounds')
    if not torch.cuda.is_available():
        sys.exit('render_image_ab.py needs a GPU: there is nothing to time without one')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device('cuda:0')
    H = W = args.side
    sc = synthetic.Scene(vsize=0.025)
    ro, rd = sc.box_rays(H * W, seed=2)
    nr, fr, m = near_far(torch.from_numpy(sc.bounds).to(dev), torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev))
    m_np = m.cpu().numpy()
    n = int(m_np.sum())
    b = sc.batch_arrays(ro[m_np], rd[m_np], nr.cpu().numpy(), fr.cpu().numpy())
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    net = network.Network()
    network.load_numpy_state(net, synthetic.init_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    net = net.to(dev)
    net.train()  # run.py evaluates in train() mode with perturb = 0
    print(f'frame {H}x{W}, {n} in-box rays, {args.rounds} rounds x {args.frames} frames per leg; '
          f'executed-MFMA ratio image / full {MFMA_RATIO:.4f}')
    result = {'side': args.side, 'rays': n, 'rounds': args.rounds, 'frames': args.frames, 'mfma_ratio': MFMA_RATIO,
              'precisions': {}}
    ok = True
    for prec in args.precisions.split(','):
        cfg = config.defaults()
        cfg.perturb = 0
        cfg.render_precision = prec
        r = Renderer(net, cfg)
        kcfg = config.defaults()
        kcfg.perturb = 0
        kcfg.render_precision = prec
        kcfg.render_image_only = True
        rk = Renderer(net, kcfg)
        lib = r.lib

        def device_leg(image_only, frames):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(frames):
                with torch.no_grad():
                    r.render_device(batch, image_only=image_only)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) / frames

        def kernel_leg(image_only, frames):
            """-> (fused kernel ms per launch, in-kernel shader clock MHz)"""
            lib.anr_profile_enable(1)
            lib.anr_profile_read(None, None)
            for _ in range(frames):
                with torch.no_grad():
                    r.render_device(batch, image_only=image_only)
            torch.cuda.synchronize(dev)
            ms, cnt, mhz = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0)
            rc = lib.anr_profile_read_clock(ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(mhz))
            lib.anr_profile_enable(0)
            if rc != 0 or cnt.value != frames:
                sys.exit(f'anr_profile_read_clock: code {rc}, {cnt.value} launches for {frames} frames')
            return ms.value / cnt.value, mhz.value

        def host_leg(renderer, frames):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(frames):
                with torch.no_grad():
                    renderer.render(batch)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / frames * 1e3

        for io in (False, True):
            device_leg(io, args.warmup)
        t = {False: [], True: []}
        for k in range(args.rounds):
            for io in ((False, True) if k % 2 == 0 else (True, False)):
                t[io].append(device_leg(io, args.frames))
        kt = {False: [], True: []}
        for k in range(args.rounds):
            for io in ((False, True) if k % 2 == 0 else (True, False)):
                kt[io].append(kernel_leg(io, args.frames))
        for rr in (r, rk):
            host_leg(rr, 1)
        ht = {False: [], True: []}
        for k in range(args.rounds):
            for io in ((False, True) if k % 2 == 0 else (True, False)):
                ht[io].append(host_leg(rk if io else r, 2))
        with torch.no_grad():
            full = r.render_device(batch, bw_rows=False, image_only=False)
            img = r.render_device(batch, image_only=True)
        equal = {k: bool(torch.equal(full[k], img[k])) for k in KEYS}

        full_s, img_s = stats(t[False]), stats(t[True])
        spread = full_s['max'] - full_s['min']
        passed = img_s['median'] < full_s['median'] - spread
        ok = ok and passed
        kms = {io: statistics.median(x[0] for x in kt[io]) for io in kt}
        kmhz = {io: statistics.median(x[1] for x in kt[io]) for io in kt}
        kratio = kms[True] / kms[False]
        cratio = (kms[True] * kmhz[True]) / (kms[False] * kmhz[False]) if kmhz[False] > 0 and kmhz[True] > 0 else 0.0
        hfull, himg = stats(ht[False]), stats(ht[True])
        print(f'--- {prec}')
        for name, s in (('full  render_device', full_s), ('image render_device', img_s)):
            print(f'{name} ms/frame: median {s["median"]:.3f}  min {s["min"]:.3f}  max {s["max"]:.3f}  '
                  f'rounds {" ".join(f"{x:.2f}" for x in s["rounds"])}')
        print(f'frame ratio image / full {img_s["median"] / full_s["median"]:.4f}; full spread {spread:.3f} ms; '
              f'image below full by {full_s["median"] - img_s["median"]:.3f} ms: {"PASS" if passed else "FAIL"}')
        print(f'fused kernel ms: full {kms[False]:.3f} @ {kmhz[False]:.0f} MHz, image {kms[True]:.3f} @ '
              f'{kmhz[True]:.0f} MHz; kernel-time ratio {kratio:.4f}, cycle ratio {cratio:.4f}, '
              f'executed-MFMA ratio {MFMA_RATIO:.4f} (kernel - MFMA {kratio - MFMA_RATIO:+.4f})')
        for name, s in (('full  render() host', hfull), ('image render() host', himg)):
            print(f'{name} ms/frame: median {s["median"]:.3f}  min {s["min"]:.3f}  max {s["max"]:.3f}')
        print(f'host leg (render() - render_device): full {hfull["median"] - full_s["median"]:.3f} ms, '
              f'image {himg["median"] - img_s["median"]:.3f} ms')
        print('outputs equal bit for bit: ' + ' '.join(f'{k}={v}' for k, v in equal.items()))
        result['precisions'][prec] = {
            'full_ms': full_s, 'image_ms': img_s, 'spread_ms': spread, 'pass': passed,
            'kernel_ms': {'full': kms[False], 'image': kms[True]}, 'clock_mhz': {'full': kmhz[False], 'image': kmhz[True]},
            'kernel_ratio': kratio, 'cycle_ratio': cratio, 'host_full_ms': hfull, 'host_image_ms': himg,
            'bit_equal': equal}
    print(json.dumps(result))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
