"""Frame time of the aligned_aninerf_pdf render (renderer_pdf.Renderer.render_device) in one process: config-2
geometry (512 x 512 box rays over synthetic.PdfScene), device events around each call, 7 rounds rotating over
{fp32, bf16x3, bf16x6} x {with the resd rows, image-only}, medians with min-max, and the kept-sample count.

``--sibling``: every round also renders the sdf_pdf network (seeded weights, the same rays; both networks keep
``pnorm < 0.1``, so k_resd_* and k_pdf_resd_* see the same rows) in bf16x3 and bf16x6, so that a kernel trace of
this process holds both displacement programs over the same rows:

    rocprofv3 --kernel-trace --stats -d <dir> -o pdf -- python tools/pdf_render_ab.py --sibling --rounds 3

``--analyze <kernel_trace.csv>`` reads such a trace instead of rendering and prints (a) the displacement program with
its epilogue against k_resd_* (per-launch ratio of the full batches, with the sibling's own launch-to-launch spread)
and (b) the time between the end of the displacement program and the start of the density program per batch on the
fused path against k_pdf_mid's time on the exact-fp32 path; ``--stats-out`` writes the per-kernel split as csv.

Run:  python tools/pdf_render_ab.py [--rays 262144] [--rounds 7] > profiles/pdf_render_ab.log
"""
import argparse
import csv
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def short(name):
    """kernel name without namespace, arguments and the .kd suffix"""
    n = name.split('(')[0].replace('.kd', '')
    return n.split('::')[-1].split(' ')[-1]


def analyze(path, stats_out):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])))
    rows.sort()
    per = {}
    for s, e, k in rows:
        per.setdefault(k, []).append((e - s) / 1e6)
    total = sum(sum(v) for v in per.values())
    if stats_out:
        with open(stats_out, 'w') as f:
            f.write('kernel,calls,total_ms,mean_ms,min_ms,max_ms,percent\n')
            for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
                f.write(f'{k},{len(v)},{sum(v):.3f},{sum(v) / len(v):.4f},{min(v):.4f},{max(v):.4f},{100 * sum(v) / total:.2f}\n')
    print(f'{len(rows)} dispatches, {total:.1f} ms of kernel time')

    def full(v):  # the full batches: a frame's partial last batch (under half the median launch) drops out
        m = statistics.median(v)
        return [x for x in v if x >= 0.5 * m]
    for new, sib in (('k_pdf_resd_b16', 'k_resd_b16'), ('k_pdf_resd_x6', 'k_resd_x6')):
        if new in per and sib in per:
            a, b = full(per[new]), full(per[sib])
            ma, mb = statistics.median(a), statistics.median(b)
            print(f'(a) {new}: {len(a)} full-batch launches, median {ma:.3f} ms ({min(a):.3f}-{max(a):.3f}); {sib} (2^19-row '
                  f'batches of the same rows): {len(b)} launches, median {mb:.3f} ms ({min(b):.3f}-{max(b):.3f}), spread '
                  f'{100 * (max(b) - min(b)) / mb:.1f} % of its median; per 2^18 rows {ma:.3f} against {mb / 2:.3f} ms = ratio '
                  f'{2 * ma / mb:.3f}; in total {sum(per[new]):.2f} ms over {len(per[new])} launches against '
                  f'{sum(per[sib]):.2f} ms over {len(per[sib])}')
    # (b) per batch: end of the displacement program -> start of the next density program
    for x6, resd, dens in ((False, 'k_pdf_resd_b16', 'k_lbw_density_b16'), (True, 'k_pdf_resd_x6', 'k_lbw_density_x6')):
        gaps = []
        for i, (s, e, k) in enumerate(rows[:-1]):
            if k == resd and rows[i + 1][2] == dens:
                gaps.append((rows[i + 1][0] - e) / 1e3)
        if gaps:
            print(f'(b) {resd} end -> {dens} start: {len(gaps)} batches, median {statistics.median(gaps):.1f} us '
                  f'({min(gaps):.1f}-{max(gaps):.1f}); no kernel runs in between')
    if 'k_pdf_mid' in per:
        v = full(per['k_pdf_mid'])
        print(f'(b) exact-fp32 path: k_pdf_mid {len(per["k_pdf_mid"])} launches, full batches median '
              f'{statistics.median(v) * 1e3:.1f} us ({min(v) * 1e3:.1f}-{max(v) * 1e3:.1f}), '
              f'{sum(per["k_pdf_mid"]):.3f} ms in total over the run')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=512 * 512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--precisions', default='fp32,bf16x3,bf16x6')
    ap.add_argument('--sibling', action='store_true')
    ap.add_argument('--analyze')
    ap.add_argument('--stats-out')
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze, args.stats_out)
    import torch
    from animatable_nerf_amd import config, network, network_pdf, network_sdf, renderer_sdf, synthetic
    from animatable_nerf_amd.renderer_pdf import Renderer
    from oracle import restate
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
        cfg = config.subject('aligned_aninerf_pdf_s9p', perturb=0, render_precision=prec)
        net = network_pdf.Network(cfg)
        sd = synthetic.init_state_dict_pdf({k: tuple(v.shape) for k, v in net.state_dict().items()})
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        rs[(prec, img)] = Renderer(net.to(dev), cfg)
    sib = {}
    if args.sibling:
        for prec in ('bf16x3', 'bf16x6'):
            cfg = config.subject('anisdf_pdf_s9p', perturb=0, render_precision=prec)
            net = network_sdf.Network(cfg)
            sd = synthetic.init_state_dict_sdf({k: tuple(v.shape) for k, v in net.state_dict().items()})
            network.load_numpy_state(net, sd)
            sib[prec] = renderer_sdf.Renderer(net.to(dev), cfg)
    times = {c: [] for c in cases}
    kept = sib_kept = None
    for rnd in range(args.rounds + 1):  # round 0 warms up (workspace allocation, code load)
        for i in range(len(cases)):
            c = cases[(i + rnd) % len(cases)]
            batch['tbounds'].copy_(tb0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rs[c].render_device(batch, image_only=c[1])
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                times[c].append(e0.elapsed_time(e1))
            if not c[1]:
                kept = rs[c].last_counts[0]
        for prec, r in sib.items():
            batch['tbounds'].copy_(tb0)
            r.render_device(batch)
            torch.cuda.synchronize()
            sib_kept = r.last_counts[0]
    print(f'device {torch.cuda.get_device_name(0)}; {int(mask.sum())} rays, {kept} kept samples; '
          f'{args.rounds} rounds after one warm-up round' + (f'; sdf_pdf sibling kept {sib_kept}' if sib else ''))
    for c in cases:
        t = times[c]
        print(f'{c[0]:7s} {"image-only     " if c[1] else "with resd rows "}  median {statistics.median(t):9.2f} ms  '
              f'min {min(t):9.2f}  max {max(t):9.2f}')
    for prec in precs:
        f, i = statistics.median(times[(prec, False)]), statistics.median(times[(prec, True)])
        print(f'{prec}: image-only / with rows = {i / f:.3f} ({f - i:.2f} ms for the resd rows, their count read and copies)')


if __name__ == '__main__':
    main()
