#!/usr/bin/env python
"""A/B of the device mesh evaluator (anr_mesh_metrics), one process, on the two meshes of tools/mesh_cc_ab.py:

  large  the device marching cubes of ``synthetic.mesh_scene``'s alpha cube at the reference's 5 mm grid,
         about 3.1 M triangles
  small  the marching cubes of two spheres in an 80^3 volume, 19,712 triangles

Each mesh is evaluated against a copy of itself scaled by 1.01 and shifted by 3 mm (a "scan" of as many faces),
with the reference's 1,000 + 1,000 Chamfer and 10,000 P2S samples from one seeded set of uniforms.

  (a) the composite, pruned by both levels of boxes (cells of 64 faces, groups of 64 cells)   device events
  (p) the composite, pruned by the cell boxes alone: every wave reads every cell's box    device events
  (b) the composite, exhaustive search                                            device events
  (n) the composite with 1 + 1 + 1 samples: everything but the search (areas and their scan, the box, the
      Morton codes, the radix sort, the records) — the part that has to stay linear   device events
  (c) the ordering alone (anr_mesh_order) against a k_bwv_rank-style count: anr_bw_volume in surface mode over a
      4 x 4 x 4 grid, i.e. its code + rank + prep and a one-brick search. The count compares every pair of
      keys, so it runs on the small mesh only                                      device events
  (d) the float64 host restatement of the metrics (tests/meshdist_ref.py: numpy sampling, brute-force torch
      distances on 16 threads). A restatement of this project, NOT trimesh (which is not installed). It
      visits every (sample, face) pair, so it runs on the small mesh only            wall clock

After a warm-up, ROUNDS rounds run the device legs in an order that alternates every round; each leg times REPS
calls between two events. Prints median / min / max per leg, checks pruned == exhaustive bit for bit and the
device metrics against the host restatement, and ends with one JSON line. The fastest of (a) / (p) / (b) is what
MD_DEFAULT_SEARCH in csrc/anr_meshdist.hip should select.

    python tools/mesh_eval_ab.py [--rounds 7] [--reps 3] [--voxel 0.005]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from animatable_nerf_amd import _lib  # noqa: E402
from animatable_nerf_amd.renderer_mesh import marching_cubes  # noqa: E402

N_CHAMFER, N_P2S = 1000, 10000
HOST_BUDGET = 1e9  # (sample, face) pairs the host leg may visit


def _mesh_cc_ab():
    spec = importlib.util.spec_from_file_location('mesh_cc_ab', os.path.join(ROOT, 'tools', 'mesh_cc_ab.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Case:
    """A mesh and its scaled copy on the device, with the workspace and outputs prepared."""

    def __init__(self, lib, dev, verts64, tris64, u):
        self.lib, self.dev = lib, dev
        self.sv = verts64.to(torch.float32).contiguous()
        self.sf = tris64.to(torch.int32).contiguous()
        ctr = verts64.mean(dim=0)
        self.tv = ((verts64 - ctr) * 1.01 + ctr + 0.003).to(torch.float32).contiguous()
        self.tf = self.sf
        self.nv, self.nf = int(self.sv.shape[0]), int(self.sf.shape[0])
        self.u = torch.from_numpy(u).to(dev)
        self.u3 = torch.from_numpy(np.ascontiguousarray(u[[0, N_CHAMFER, 2 * N_CHAMFER]])).to(dev)
        self.nbytes = lib.anr_mesh_dist_workspace_bytes(self.nf, 2 * N_CHAMFER + N_P2S)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.row = torch.zeros(_lib.MESHM_NOUT, dtype=torch.float64, device=dev)
        self.perm = torch.empty(self.nf, dtype=torch.int32, device=dev)

    def composite(self, search, n_c=N_CHAMFER, n_p=N_P2S, u=None):
        opts = _lib.MeshDistOpts(search, n_c, n_p)
        _lib.check(self.lib.anr_mesh_metrics(_lib.ptr(self.sv), self.nv, _lib.ptr(self.sf), self.nf, _lib.ptr(self.tv),
                                             self.nv, _lib.ptr(self.tf), self.nf, _lib.ptr(self.u if u is None else u),
                                             ctypes.byref(opts), _lib.ptr(self.row), _lib.ptr(self.ws), self.nbytes,
                                             _lib.stream_ptr(self.dev)), 'anr_mesh_metrics')

    def order(self):
        _lib.check(self.lib.anr_mesh_order(_lib.ptr(self.sv), self.nv, _lib.ptr(self.sf), self.nf, _lib.ptr(self.perm),
                                           _lib.ptr(self.ws), self.nbytes, _lib.stream_ptr(self.dev)), 'anr_mesh_order')

    def prepare_rank(self):
        """anr_bw_volume, surface mode, over one 4 x 4 x 4 brick at the mesh: code + rank + prep dominate"""
        self.skin = torch.ones((self.nv, 1), dtype=torch.float32, device=self.dev)
        self.vol = torch.empty((4, 4, 4, 2), dtype=torch.float32, device=self.dev)
        self.rbytes = self.lib.anr_bw_volume_workspace_bytes(self.nv, self.nf, 4, 4, 4)
        self.rws = torch.empty(self.rbytes, dtype=torch.uint8, device=self.dev)
        lo = self.sv.min(dim=0).values.cpu().numpy().astype(np.float64)
        self.org = (ctypes.c_double * 3)(*[float(x) for x in lo])

    def rank(self):
        opts = _lib.BwvOpts(_lib.BWV_SURFACE, _lib.BWV_PRUNED)
        _lib.check(self.lib.anr_bw_volume(_lib.ptr(self.sv), self.nv, _lib.ptr(self.sf), self.nf, _lib.ptr(self.skin), 1,
                                          self.org, 0.01, 4, 4, 4, ctypes.byref(opts), _lib.ptr(self.vol), None,
                                          _lib.ptr(self.rws), self.rbytes, _lib.stream_ptr(self.dev)), 'anr_bw_volume')

    def events(self, f, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(self.dev)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize(self.dev)
        return e0.elapsed_time(e1) / reps


def host_leg(case, u):
    from tests import meshdist_ref as M
    torch.set_num_threads(16)
    src = (case.sv.cpu().numpy(), case.sf.cpu().numpy())
    tgt = (case.tv.cpu().numpy(), case.tf.cpu().numpy())
    t0 = time.perf_counter()
    ref = M.metrics(src, tgt, u)
    return (time.perf_counter() - t0) * 1e3, ref


def run(name, c, u, rounds, reps, with_rank):
    legs = {'a': lambda: c.events(lambda: c.composite(_lib.BWV_PRUNED), reps),
            'p': lambda: c.events(lambda: c.composite(_lib.MESHDIST_PRUNED_CELLS), reps),
            'b': lambda: c.events(lambda: c.composite(_lib.BWV_EXHAUSTIVE), max(1, reps // 3)),
            'n': lambda: c.events(lambda: c.composite(_lib.BWV_PRUNED, 1, 1, c.u3), reps),
            'c': lambda: c.events(c.order, reps)}
    if with_rank:
        c.prepare_rank()
        legs['r'] = lambda: c.events(c.rank, reps)
    for f in legs.values():
        f()
    times = {k: [] for k in legs}
    order = list(legs)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(legs[k]())
    c.composite(_lib.BWV_PRUNED)
    pruned = c.row.cpu().numpy().copy()
    c.composite(_lib.BWV_EXHAUSTIVE)
    exhaustive = c.row.cpu().numpy().copy()
    c.composite(_lib.MESHDIST_PRUNED_CELLS)
    cells = c.row.cpu().numpy().copy()
    same = bool(np.array_equal(pruned.view(np.int64), exhaustive.view(np.int64))
                and np.array_equal(cells.view(np.int64), exhaustive.view(np.int64)))
    names = {'a': 'composite, pruned by two levels of boxes', 'p': 'composite, pruned by the cell boxes alone',
             'b': 'composite, exhaustive search',
             'n': 'composite with 1 + 1 + 1 samples (no search)', 'c': 'ordering alone: anr_mesh_order (radix sort)',
             'r': 'k_bwv_rank-style count: anr_bw_volume, one brick'}
    print(f'[{name}] {c.nv} vertices, {c.nf} triangles per mesh; workspace {c.nbytes / 2 ** 20:.1f} MiB; '
          f'chamfer {pruned[0]:.9g} m, p2s {pruned[1]:.9g} m, status {int(pruned[4])}; both pruned searches == exhaustive: {same}')
    med = {}
    for k in legs:
        v = times[k]
        med[k] = statistics.median(v)
        print(f'[{name}] ({k}) {names[k]:50s} ms: median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}  '
              f'rounds {" ".join(f"{x:.3f}" for x in v)}')
    out = {'nv': c.nv, 'nf': c.nf, 'row': pruned.tolist(), 'pruned_equals_exhaustive': same, 'workspace_bytes': c.nbytes,
           'ms': {k: {'median': med[k], 'min': min(times[k]), 'max': max(times[k]), 'rounds': times[k]} for k in med}}
    pairs = (2 * N_CHAMFER + N_P2S) * c.nf
    if pairs <= HOST_BUDGET:
        ms, ref = host_leg(c, u)
        err = {k: abs(ref[k] - pruned[i]) for i, k in enumerate(('chamfer', 'p2s', 'src_tgt', 'tgt_src'))}
        print(f'[{name}] (d) float64 host RESTATEMENT (numpy + torch, 16 threads; not trimesh)        ms: {ms:.1f}; '
              f'device - restatement: chamfer {err["chamfer"]:.3g} m, p2s {err["p2s"]:.3g} m; '
              f'restatement / composite: {ms / med["a"]:.0f}x')
        out['host_restatement_ms'] = ms
        out['host_restatement_err'] = err
    else:
        print(f'[{name}] (d) host restatement skipped: {pairs:.2e} (sample, face) pairs is beyond {HOST_BUDGET:.0e}')
    return out


def shader_clock():
    """the device's current shader clock in MHz as the driver reports it, None where torch cannot read it"""
    try:
        return int(torch.cuda.clock_rate())
    except Exception:  # noqa: BLE001  (no amdsmi binding in this environment)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--voxel', type=float, default=0.005, help='voxel size of the large mesh (the reference: 5 mm)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mesh_eval_ab.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    cc = _mesh_cc_ab()
    u = np.random.Generator(np.random.PCG64(11)).random((2 * N_CHAMFER + N_P2S, 3))
    clk = [shader_clock()]
    out = {'rounds': args.rounds, 'reps': args.reps, 'voxel': args.voxel}
    v, t = marching_cubes(cc.spheres_cube(dev), 0.0, 0)
    small = Case(lib, dev, v, t, u)
    out['small'] = run('small', small, u, args.rounds, args.reps, with_rank=True)
    del small
    v, t = marching_cubes(cc.alpha_cube(dev, args.voxel), 2.95, 10)
    large = Case(lib, dev, v * args.voxel, t, u)
    del v, t
    out['large'] = run('large', large, u, args.rounds, args.reps, with_rank=False)
    clk.append(shader_clock())
    out['shader_clock_mhz'] = clk
    print(f'shader clock (torch.cuda.clock_rate) before / after the legs: {clk[0]} / {clk[1]} MHz')
    s, l = out['small'], out['large']
    ratio = l['nf'] / s['nf']
    for k, what in (('n', 'composite without the search'), ('c', 'ordering alone'), ('a', 'composite, two levels'),
                    ('p', 'composite, cell boxes alone')):
        g = l['ms'][k]['median'] / s['ms'][k]['median']
        print(f'large / small: faces {ratio:.1f}x, {what} {g:.1f}x')
    out['growth'] = {k: l['ms'][k]['median'] / s['ms'][k]['median'] for k in ('a', 'p', 'b', 'n', 'c')}
    out['faces_ratio'] = ratio
    print(json.dumps(out))


if __name__ == '__main__':
    main()
