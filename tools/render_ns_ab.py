#!/usr/bin/env python
"""A/B of the 64-sample render programs (anr_render_fwd / anr_render_image_fwd) against the programs of
anr_render_ns_fwd at 64, 128 and 256 samples per ray, one process, on the 512x512 config-2 synthetic frame of
bench.py, full and image-only, in each render precision.

Legs per precision and program: ``old64`` (the 64-sample entry), ``ns64``, ``ns128``, ``ns256`` (the new entry).
After a warm-up, ROUNDS rounds run the legs in an order rotated every round; each leg is FRAMES entry calls
between two device events (the entry alone: no row gather, no count read), with the library's event pair around
the fused network launch (anr_profile_read) in the same frames. Reported per leg: frame ms and fused-kernel ms
(median, min - max over the rounds) and the fused kernel's ns per kept sample (kernel ms / kept samples, the kept
count read once outside the timed frames). The comparison is the old 64-sample program in the same run: a new leg
whose median ns per kept sample lies outside old64's min - max spread is marked ``OUTSIDE``.
Also prints the workspace sizes at each count, and checks that ns64's outputs equal old64's bit for bit.
Prints a table and one JSON line.

    python tools/render_ns_ab.py [--rounds 7] [--frames 2] [--side 512] [--precisions fp32,bf16x3,bf16x6]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import _lib, config, network, synthetic  # noqa: E402
from animatable_nerf_amd.renderer import Renderer, _Call, near_far  # noqa: E402

LEGS = (('old64', 64, False), ('ns64', 64, True), ('ns128', 128, True), ('ns256', 256, True))
KEYS = ('rgb', 'acc', 'depth', 'raw')


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}


def fmt(s, nd=3):
    return f'{s["median"]:.{nd}f} ({s["min"]:.{nd}f} - {s["max"]:.{nd}f})'


class Leg:
    """one entry at one sample count and program: its call structs, outputs and workspace"""

    def __init__(self, net, batch, prec, ns, use_ns, image):
        cfg = config.defaults()
        cfg.perturb = 0
        cfg.render_precision = prec
        cfg.N_samples = ns
        self.r = r = Renderer(net, cfg)
        self.lib, self.image, self.use_ns = r.lib, image, use_ns
        self.p = r.params()
        self.R = batch['ray_o'].shape[1]
        self.c = c = _Call(r, batch, None)
        c.opts.precision = c.render_precision
        io = 1 if image else 0
        if use_ns:
            self.nbytes = self.lib.anr_render_ns_workspace_bytes(self.R, ctypes.byref(c.opts), ctypes.byref(c.frame), io)
        else:
            size = self.lib.anr_render_image_workspace_bytes if image else self.lib.anr_render_workspace_bytes
            self.nbytes = size(self.R, ctypes.byref(c.opts), ctypes.byref(c.frame))
        self.ws = None

    def run(self, ws):
        c, lib = self.c, self.lib
        args = (ctypes.byref(self.p), ctypes.byref(c.frame), *c.ray_ptrs(), self.R, ctypes.byref(c.opts),
                ctypes.byref(c.out))
        tail = (_lib.ptr(ws), self.nbytes, _lib.stream_ptr(c.dev))
        if self.use_ns:
            _lib.check(lib.anr_render_ns_fwd(*args, 1 if self.image else 0, *tail), 'anr_render_ns_fwd')
        else:
            fwd = lib.anr_render_image_fwd if self.image else lib.anr_render_fwd
            _lib.check(fwd(*args, *tail), 'anr_render_fwd')

    def kept(self, ws):
        return self.r._counts(ws, self.R)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--side', type=int, default=512)
    ap.add_argument('--precisions', default='fp32,bf16x3,bf16x6')
    args = ap.parse_args()
    if args.rounds < 7:
        sys.exit('render_ns_ab.py: at least 7 alternating rounds')
    if not torch.cuda.is_available():
        sys.exit('render_ns_ab.py needs a GPU: there is nothing to time without one')
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
    print(f'frame {H}x{W}, {n} in-box rays, {args.rounds} rounds x {args.frames} frames per leg')
    result = {'side': args.side, 'rays': n, 'rounds': args.rounds, 'frames': args.frames, 'precisions': {}}
    lib = _lib.load()
    for pi, prec in enumerate(args.precisions.split(',')):
        result['precisions'][prec] = {}
        for image in (False, True):
            prog = 'image' if image else 'full'
            legs = [(name, Leg(net, batch, prec, ns, use_ns, image)) for name, ns, use_ns in LEGS]
            ws = torch.empty(max(L.nbytes for _, L in legs), dtype=torch.uint8, device=dev)  # one workspace, by turns
            if pi == 0:
                print(f'workspace bytes, {prog}: ' + ', '.join(f'{name} {L.nbytes / 2 ** 30:.3f} GiB' for name, L in legs))
                result.setdefault('workspace_bytes', {})[prog] = {name: int(L.nbytes) for name, L in legs}
            kept, outs = {}, {}
            for name, L in legs:
                for _ in range(args.warmup):
                    L.run(ws)
                kept[name] = L.kept(ws)
                if name in ('old64', 'ns64'):
                    outs[name] = {k: getattr(L.c, k).clone() for k in KEYS}
            equal = all(torch.equal(outs['old64'][k], outs['ns64'][k]) for k in KEYS)
            frame_ms = {name: [] for name, _ in legs}
            kern_ms = {name: [] for name, _ in legs}
            for k in range(args.rounds):
                order = legs[k % len(legs):] + legs[:k % len(legs)]
                for name, L in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    lib.anr_profile_enable(1)
                    lib.anr_profile_read(None, None)
                    torch.cuda.synchronize(dev)
                    e0.record()
                    for _ in range(args.frames):
                        L.run(ws)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    ms, cnt = ctypes.c_double(0), ctypes.c_int(0)
                    rc = lib.anr_profile_read(ctypes.byref(ms), ctypes.byref(cnt))
                    lib.anr_profile_enable(0)
                    if rc != 0 or cnt.value != args.frames:
                        sys.exit(f'anr_profile_read: code {rc}, {cnt.value} launches for {args.frames} frames')
                    frame_ms[name].append(e0.elapsed_time(e1) / args.frames)
                    kern_ms[name].append(ms.value / cnt.value)
            print(f'--- {prec} {prog}: ns64 outputs equal old64 bit for bit: {equal}')
            print(f'{"leg":6s} {"kept":>10s} {"frame ms":>28s} {"fused kernel ms":>28s} {"ns / kept sample":>28s}')
            ref = None
            res = {}
            for name, L in legs:
                per = [x * 1e6 / kept[name] for x in kern_ms[name]]
                fs, ks, ps = stats(frame_ms[name]), stats(kern_ms[name]), stats(per)
                if name == 'old64':
                    ref = ps
                inside = ref['min'] <= ps['median'] <= ref['max']
                mark = '' if name == 'old64' else ('  inside old64 spread' if inside else
                                                   f'  OUTSIDE ({ps["median"] / ref["median"] - 1:+.2%} of old64 median)')
                print(f'{name:6s} {kept[name]:10d} {fmt(fs):>28s} {fmt(ks):>28s} {fmt(ps, 4):>28s}{mark}')
                res[name] = {'kept': kept[name], 'frame_ms': fs, 'kernel_ms': ks, 'ns_per_kept': ps,
                             'inside_old64_spread': bool(inside)}
            res['ns64_bit_equal'] = bool(equal)
            result['precisions'][prec][prog] = res
            del legs, ws, outs
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
