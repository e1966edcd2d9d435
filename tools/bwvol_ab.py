#!/usr/bin/env python
"""A/B of building one blend-weight volume, one process, on a lat-long ellipsoid of SMPL size (6,890
vertices, 13,776 faces) and the reference's grids: (63, 75, 38) for a frame's ``pbw`` and (76, 75, 19)
for ``tbw`` (``tpose_dataset.py:158, 216``), 25 channels.

  (a) anr_bw_volume, vertex mode, pruned (a_ex: exhaustive), on the pbw grid   device events
  (b) anr_bw_volume, surface mode, exhaustive, on the tbw grid device events
  (c) anr_bw_volume, surface mode, pruned, on the tbw grid     device events
  (d) the host ``synthetic.blend_weight_volume`` on the pbw mesh, over the grid it forms itself (numpy,
      the BLAS thread count of the environment)                 wall clock
  (e) ``np.load`` of a pbw-sized volume from local disk + its H2D copy (what the reference pays per
      frame, ``data.ResidentFrames`` once)                      wall clock between synchronisations

After a warm-up, ROUNDS rounds run the legs in an order that alternates every round; the device legs
time REPS calls per round between two events. Prints median / min / max per leg, the exhaustive
search's pair rate against the float32 vector peak, and one JSON line.

Per (voxel, triangle) pair the search kernel's tri_d2 + update issue 74 vector instructions, 32 of them
fused multiply-adds = 106 flop (counted from csrc/anr_bwvol.hip: 3 sub for p - a; 2 dot products 2 mul +
4 fma; per edge a parameter (3 to 6 ops) and a squared residual (1 mul + 5 or 8 fma) and a min; the plane's
s, r (6), its residual (1 mul + 8 fma), the inside test (6), select + min (2); the lexicographic update (6)).
A vertex-mode pair is 3 sub, 1 mul, 2 fma and the update (6): 12 instructions, 14 flop.

    python tools/bwvol_ab.py [--rounds 9] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from animatable_nerf_amd import _lib, synthetic  # noqa: E402
from tests import bwvol_ref  # noqa: E402

VSIZE = 0.025
PEAK_TFLOPS = 157.3   # float32 vector peak (MI355X)
TRI_INSTR, TRI_FLOP = 74, 106
VERT_INSTR, VERT_FLOP = 12, 14


def subject(dims, seed):
    """An 83 x 84 lat-long ellipsoid (6,890 vertices, 13,776 faces) whose padded bounds give `dims`."""
    ext = (np.array(dims) - 1) * VSIZE
    semi = (ext - 0.1 - 0.5 * VSIZE) / 2.0 / 1.25  # the 6 % radial jitter stays inside (4 sigma)
    v, f = bwvol_ref.ellipsoid(83, 84, seed=seed, semi=semi, centre=(0.0, 0.0, 0.0))
    return v, f, -ext / 2.0


class Call:
    """One prepared anr_bw_volume call: inputs uploaded, outputs and workspace allocated."""

    def __init__(self, lib, dev, verts, faces, skin, origin, dims, mode, search):
        self.lib, self.dev, self.dims = lib, dev, dims
        self.nv, self.nb = skin.shape
        self.nf = 0 if faces is None else len(faces)
        self.v = torch.from_numpy(verts).to(dev)
        self.f = torch.from_numpy(faces).to(dev) if faces is not None else None
        self.s = torch.from_numpy(skin).to(dev)
        self.vol = torch.empty(tuple(dims) + (self.nb + 1,), dtype=torch.float32, device=dev)
        self.idx = torch.empty(tuple(dims), dtype=torch.int32, device=dev)
        self.nbytes = lib.anr_bw_volume_workspace_bytes(self.nv, self.nf, *dims)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.opts = _lib.BwvOpts(mode, search)
        self.org = (ctypes.c_double * 3)(*[float(x) for x in origin])

    def __call__(self):
        _lib.check(self.lib.anr_bw_volume(_lib.ptr(self.v), self.nv, _lib.ptr(self.f), self.nf, _lib.ptr(self.s), self.nb,
                                          self.org, VSIZE, self.dims[0], self.dims[1], self.dims[2],
                                          ctypes.byref(self.opts), _lib.ptr(self.vol), _lib.ptr(self.idx),
                                          _lib.ptr(self.ws), self.nbytes, _lib.stream_ptr(self.dev)), 'anr_bw_volume')

    def timed(self, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(self.dev)
        e0.record()
        for _ in range(reps):
            self()
        e1.record()
        torch.cuda.synchronize(self.dev)
        return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3, help='rounds that also run the slow host leg (d)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bwvol_ab.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    pdims, tdims = (63, 75, 38), (76, 75, 19)
    pv, pf, porg = subject(pdims, 5)
    tv, tf, torg = subject(tdims, 6)
    skin = bwvol_ref.skin_weights(len(pv), 24)
    a = Call(lib, dev, pv, None, skin, porg, pdims, _lib.BWV_VERTEX, _lib.BWV_PRUNED)
    a_ex = Call(lib, dev, pv, None, skin, porg, pdims, _lib.BWV_VERTEX, _lib.BWV_EXHAUSTIVE)
    b = Call(lib, dev, tv, tf, skin, torg, tdims, _lib.BWV_SURFACE, _lib.BWV_EXHAUSTIVE)
    c = Call(lib, dev, tv, tf, skin, torg, tdims, _lib.BWV_SURFACE, _lib.BWV_PRUNED)
    # the legs agree before they are timed
    b(), c(), a(), a_ex()
    torch.cuda.synchronize(dev)
    same_surface = bool(torch.equal(b.idx, c.idx) and torch.equal(b.vol.view(torch.int32), c.vol.view(torch.int32)))
    same_vertex = bool(torch.equal(a.idx, a_ex.idx) and torch.equal(a.vol.view(torch.int32), a_ex.vol.view(torch.int32)))

    tmp = tempfile.mkdtemp(prefix='bwvol_ab_')
    path = os.path.join(tmp, 'pbw.npy')
    np.save(path, a.vol.cpu().numpy())

    def leg_d():
        t0 = time.perf_counter()
        synthetic.blend_weight_volume(pv.astype(np.float64), skin, VSIZE)
        return (time.perf_counter() - t0) * 1e3

    def leg_e():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = torch.from_numpy(np.load(path)).to(dev)
        torch.cuda.synchronize(dev)
        del t
        return (time.perf_counter() - t0) * 1e3

    legs = {'a': lambda: a.timed(args.reps), 'a_ex': lambda: a_ex.timed(args.reps), 'b': lambda: b.timed(args.reps),
            'c': lambda: c.timed(args.reps), 'e': leg_e}
    for f in legs.values():
        f()
    times = {k: [] for k in ('a', 'a_ex', 'b', 'c', 'd', 'e')}
    order = list(legs)
    for r in range(args.rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(legs[k]())
        if r < args.host_rounds:
            times['d'].append(leg_d())

    names = {'a': f'vertex mode, pruned, pbw grid {pdims}', 'a_ex': 'vertex mode, exhaustive, pbw grid',
             'b': f'surface mode, exhaustive, tbw grid {tdims}', 'c': 'surface mode, pruned, tbw grid',
             'd': 'host synthetic.blend_weight_volume, pbw grid', 'e': 'np.load + H2D of a pbw-sized volume'}
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'{len(pv)} vertices, {len(pf)} faces, nb 24, vsize {VSIZE}; {args.rounds} rounds x {args.reps} calls '
          f'per device leg; BLAS threads {torch.get_num_threads()}')
    print(f'pruned == exhaustive bits: surface {same_surface}, vertex {same_vertex}')
    for k in ('a', 'a_ex', 'b', 'c', 'd', 'e'):
        v = times[k]
        print(f'({k:4s}) {names[k]:52s} ms: median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}  '
              f'rounds {" ".join(f"{x:.3f}" for x in v)}')
    # pair rates of the exhaustive legs: every lane of every 4x4x4 brick visits every primitive (the other
    # launches of the call are inside the span, so the search kernel's own rate is at least this)
    lanes = lambda d: 64 * int(np.prod([(x + 3) // 4 for x in d]))  # noqa: E731
    tri_pairs = lanes(tdims) * len(tf)
    vert_pairs = lanes(pdims) * len(pv)
    tri_rate, vert_rate = tri_pairs / (med['b'] * 1e-3), vert_pairs / (med['a_ex'] * 1e-3)
    print(f'(b) {tri_pairs:.4g} voxel-triangle pairs: {tri_rate:.4g} pairs/s = {tri_rate * TRI_FLOP / 1e12:.2f} TFLOP/s '
          f'({100 * tri_rate * TRI_FLOP / 1e12 / PEAK_TFLOPS:.1f} % of the {PEAK_TFLOPS} TFLOP/s float32 vector peak; '
          f'{tri_rate * TRI_INSTR / 1e12:.2f} T lane-instructions/s of {PEAK_TFLOPS / 2:.2f})')
    print(f'(a_ex) {vert_pairs:.4g} voxel-vertex pairs: {vert_rate:.4g} pairs/s = {vert_rate * VERT_FLOP / 1e12:.2f} TFLOP/s '
          f'({100 * vert_rate * VERT_FLOP / 1e12 / PEAK_TFLOPS:.1f} % of peak; '
          f'{vert_rate * VERT_INSTR / 1e12:.2f} T lane-instructions/s of {PEAK_TFLOPS / 2:.2f})')
    print(f'pruned / exhaustive: surface {med["c"] / med["b"]:.3f}, vertex {med["a"] / med["a_ex"]:.3f} '
          f'(the default search stays pruned only where this is below 1)')
    print(json.dumps({'rounds': args.rounds, 'reps': args.reps, 'same_surface': same_surface, 'same_vertex': same_vertex,
                      'ms': {k: {'median': med[k], 'min': min(v), 'max': max(v), 'rounds': v} for k, v in times.items()},
                      'tri_pairs': tri_pairs, 'vert_pairs': vert_pairs, 'tri_pairs_per_s': tri_rate,
                      'vert_pairs_per_s': vert_rate}))


if __name__ == '__main__':
    main()
