"""Frame time of the aligned_aninerf_lbw render (renderer_lbw.Renderer.render_device) in one process: config-2
geometry (512 x 512 box rays over synthetic.PdfScene), device events around each call, 7 rounds rotating over
{fp32, bf16x3, bf16x6} x {full, image-only}, medians with min-max; for the fused precisions also the summed time of
the fused launches and the shader clock from their in-kernel stamps (anr_profile_read_clock).

``--sibling``: every round also renders the sdf_pdf network (seeded weights, the same rays, its KNN threshold set to
this variant's 0.05 so that both keep the same samples) in bf16x3 and bf16x6, so that a kernel trace of this process
holds k_sdfnet_* and k_lbw_density_* over the same row count. The per-kernel split, the share of the two searches
(k_sdf_front: a full call runs both, an image-only call the first alone) and that comparison come from such a trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lbw_render_ab.py --sibling --rounds 3 --precisions bf16x6

Run:  python tools/lbw_render_ab.py [--rays 262144] [--rounds 7] > profiles/lbw_render_ab.log
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=512 * 512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--precisions', default='fp32,bf16x3,bf16x6')
    ap.add_argument('--sibling', action='store_true')
    args = ap.parse_args()
    from animatable_nerf_amd import _lib, config, network, network_lbw, network_sdf, renderer_sdf, synthetic
    from animatable_nerf_amd.renderer_lbw import Renderer
    from oracle import restate
    lib = _lib.load()
    dev = torch.device('cuda:0')
    sc = synthetic.PdfScene(vsize=0.05)
    ro, rd = sc.box_rays(args.rays, seed=5)
    near, far, mask = restate.near_far(sc.pbounds, ro, rd)
    b = sc.batch_arrays(ro[mask], rd[mask], near.astype(np.float32), far.astype(np.float32), latent_index=7)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    tb0 = batch['tbounds'].clone()
    precs = args.precisions.split(',')
    cases = [(p, img) for p in precs for img in (False, True)]
    rs = {}
    for prec, img in cases:
        cfg = config.subject('aligned_aninerf_lbw_s9p', perturb=0, render_precision=prec)
        net = network_lbw.Network(cfg)
        sd = synthetic.init_state_dict_lbw({k: tuple(v.shape) for k, v in net.state_dict().items()})
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        rs[(prec, img)] = Renderer(net.to(dev), cfg)
    sib = {}
    if args.sibling:
        renderer_sdf.NORM_TH = 0.05  # the same keep mask as this variant's front-end
        for prec in ('bf16x3', 'bf16x6'):
            cfg = config.subject('anisdf_pdf_s9p', perturb=0, render_precision=prec)
            net = network_sdf.Network(cfg)
            sd = synthetic.init_state_dict_sdf({k: tuple(v.shape) for k, v in net.state_dict().items()})
            network.load_numpy_state(net, sd)
            sib[prec] = renderer_sdf.Renderer(net.to(dev), cfg)
    lib.anr_profile_enable(1)
    ms, n, clk = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    times = {c: [] for c in cases}
    fused = {c: [] for c in cases}
    clocks = {c: [] for c in cases}
    kept = sib_kept = None
    for rnd in range(args.rounds + 1):  # round 0 warms up (workspace allocation, code load)
        for i in range(len(cases)):
            c = cases[(i + rnd) % len(cases)]
            batch['tbounds'].copy_(tb0)
            lib.anr_profile_read_clock(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(clk))  # reset
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rs[c].render_device(batch, image_only=c[1])
            e1.record()
            torch.cuda.synchronize()
            lib.anr_profile_read_clock(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(clk))
            if rnd > 0:
                times[c].append(e0.elapsed_time(e1))
                fused[c].append(ms.value)
                clocks[c].append(clk.value)
            if not c[1]:
                kept = rs[c].last_counts
        for prec, r in sib.items():
            batch['tbounds'].copy_(tb0)
            r.render_device(batch)
            torch.cuda.synchronize()
            sib_kept = r.last_counts[0]
    lib.anr_profile_enable(0)
    print(f'device {torch.cuda.get_device_name(0)}; {int(mask.sum())} rays, kept samples / alpha_ind rows {kept}; '
          f'{args.rounds} rounds after one warm-up round' + (f'; sdf_pdf sibling kept {sib_kept}' if sib else ''))
    for c in cases:
        t = times[c]
        line = (f'{c[0]:7s} {"image-only" if c[1] else "full      "}  median {statistics.median(t):9.2f} ms  '
                f'min {min(t):9.2f}  max {max(t):9.2f}')
        if c[0] != 'fp32':
            line += (f'   fused launches {statistics.median(fused[c]):8.2f} ms at {statistics.median(clocks[c]):6.0f} MHz '
                     '(in-kernel stamps)')
        print(line)
    for prec in precs:
        f, i = statistics.median(times[(prec, False)]), statistics.median(times[(prec, True)])
        print(f'{prec}: image-only / full = {i / f:.3f}')
        if prec != 'fp32':
            # what a full call adds to an image-only one is the second search, the T-pose blend-weight launches, the
            # two small tbw kernels, the alpha_ind stage and the row copies; the fused launches' difference is the
            # T-pose blend-weight program, so the rest bounds the second search from above
            t = statistics.median(fused[(prec, False)]) - statistics.median(fused[(prec, True)])
            print(f'{prec}: full - image-only = {f - i:.2f} ms, of which the T-pose blend-weight launches {t:.2f} ms; second '
                  f'search + tbw kernels + alpha_ind stage + row copies = {f - i - t:.2f} ms = {100 * (f - i - t) / f:.1f} % of '
                  'the full frame')


if __name__ == '__main__':
    main()
