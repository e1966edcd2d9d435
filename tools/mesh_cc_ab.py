#!/usr/bin/env python
"""A/B of keeping the largest watertight mesh component, one process, on two meshes:

  large  the device marching cubes of ``synthetic.mesh_scene``'s alpha cube at the reference's 5 mm grid
         (``bench.py --mode mesh``: inside = all voxels, iso 2.95), about 3.1 M triangles
  small  the marching cubes of two spheres in an 80^3 volume, about 20 k triangles

  (a) anr_mesh_cc_count + anr_mesh_cc_emit into preallocated outputs            device events
  (b) ``largest_component_device`` end to end: workspace and output allocation, the host read of the
      counts between the two calls                                              wall clock between synchronisations
  (c) the host ``largest_component`` with the D2H copy of the whole mesh it needs   wall clock
  (m) the device marching cubes that produced the mesh, for scale                wall clock between synchronisations

After a warm-up, ROUNDS rounds run the device legs in an order that alternates every round; leg (a) times
REPS calls per round between two events. The host leg takes seconds on the large mesh and runs in the
first HOST_ROUNDS rounds only (``--host-rounds-large`` for the large mesh). Prints median / min / max per
leg, whether the device and host results are equal, and one JSON line. Where the host pass cannot run (it
visits every face once per component) the device result is still compared with a vectorised restatement of it.

    python tools/mesh_cc_ab.py [--rounds 9] [--reps 5] [--voxel 0.005]
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

from animatable_nerf_amd import _lib, config, network, synthetic  # noqa: E402
from animatable_nerf_amd.renderer_mesh import Renderer, largest_component_device, marching_cubes  # noqa: E402
from animatable_nerf_amd.renderer_sdf_mesh import largest_component  # noqa: E402


HOST_BUDGET = 3e10


def alpha_cube(dev, voxel):
    """the cube bench.py --mode mesh hands to marching cubes"""
    b = synthetic.mesh_scene(voxel=voxel, inside_frac=1.01)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    net = network.Network()
    network.load_numpy_state(net, synthetic.init_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}))
    r = Renderer(net.to(dev), config.load_cfg(opts=['vis_posed_mesh', 'True', 'render_precision', 'bf16x3']))
    inside = batch['inside'][0].bool()
    cube = torch.zeros(tuple(inside.shape), device=dev)
    cube[inside] = r.alpha_points(batch['pts'][0][inside].contiguous(), batch)
    return cube


def spheres_cube(dev):
    x = np.arange(80, dtype=np.float64)
    g = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1)
    d = lambda c, r: r - np.linalg.norm(g - np.array(c), axis=-1)  # noqa: E731
    return torch.from_numpy(np.maximum(d((22.3, 22.1, 24.2), 17.2), d((56.2, 55.9, 52.4), 15.1)).astype(np.float32)).to(dev)


def vectorised_reference(v, t):
    """The host pass's result without its per-component Python loops (scipy's connected components over the
    face graph, numpy for the rest): a second host restatement, used to check the device result on a mesh
    with too many components for ``largest_component``; checked against it on the small mesh."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nt, nv = len(t), len(v)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    key = e[:, 0] * nv + e[:, 1]
    order = np.argsort(key, kind='stable')
    ks, fs = key[order], np.tile(np.arange(nt), 3)[order]
    same = np.nonzero(ks[1:] == ks[:-1])[0]
    g = coo_matrix((np.ones(len(same), np.int8), (fs[same], fs[same + 1])), shape=(nt, nt))
    ncomp, comp = connected_components(g, directed=False)
    root = np.full(ncomp, nt, np.int64)
    np.minimum.at(root, comp, np.arange(nt))  # a component's label: its lowest face
    _, first, cnt = np.unique(ks, return_index=True, return_counts=True)
    bad = np.zeros(ncomp, bool)
    bad[comp[fs[first[cnt != 2]]]] = True
    pairs = np.unique(np.repeat(comp, 3).astype(np.int64) * nv + t.ravel())
    nverts = np.bincount(pairs // nv, minlength=ncomp)
    if bad.all():
        return v, t
    cand = np.nonzero(~bad)[0]
    top = cand[nverts[cand] == nverts[cand].max()]
    best = top[np.argmin(root[top])]
    uv, inv = np.unique(t[comp == best], return_inverse=True)
    return v[uv], inv.reshape(-1, 3).astype(np.int64)


class Mesh:
    """One mesh on the device with the workspace and outputs of leg (a) prepared."""

    def __init__(self, lib, dev, cube, iso, pad):
        self.lib, self.dev, self.cube, self.iso, self.pad = lib, dev, cube, iso, pad
        self.v, self.t = marching_cubes(cube, iso, pad)
        self.nv, self.nt = int(self.v.shape[0]), int(self.t.shape[0])
        self.nbytes = lib.anr_mesh_cc_workspace_bytes(self.nv, self.nt)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(_lib.MESHCC_NCOUNT, dtype=torch.int32, device=dev)
        self.ov, self.ot = torch.empty_like(self.v), torch.empty_like(self.t)

    def device_pass(self):
        st = _lib.stream_ptr(self.dev)
        _lib.check(self.lib.anr_mesh_cc_count(_lib.ptr(self.t), self.nt, self.nv, _lib.ptr(self.counts), None,
                                              _lib.ptr(self.ws), self.nbytes, st), 'anr_mesh_cc_count')
        _lib.check(self.lib.anr_mesh_cc_emit(_lib.ptr(self.v), _lib.ptr(self.t), self.nt, self.nv, _lib.ptr(self.ov),
                                             _lib.ptr(self.ot), _lib.ptr(self.ws), self.nbytes, st), 'anr_mesh_cc_emit')

    def leg_a(self, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(self.dev)
        e0.record()
        for _ in range(reps):
            self.device_pass()
        e1.record()
        torch.cuda.synchronize(self.dev)
        return e0.elapsed_time(e1) / reps

    def wall(self, f):
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize(self.dev)
        return (time.perf_counter() - t0) * 1e3, out

    def leg_b(self):
        return self.wall(lambda: largest_component_device(self.v, self.t))

    def leg_c(self):
        return self.wall(lambda: largest_component(self.v.cpu().numpy(), self.t.cpu().numpy()))

    def leg_m(self):
        return self.wall(lambda: marching_cubes(self.cube, self.iso, self.pad))[0]


def run(name, m, rounds, reps, host_rounds):
    legs = {'a': lambda: m.leg_a(reps), 'b': lambda: m.leg_b()[0], 'm': m.leg_m}
    for f in legs.values():
        f()
    times = {k: [] for k in ('a', 'b', 'c', 'm')}
    order = list(legs)
    same = None
    # the host pass scans all faces once per component (t[root == r]): with very many components it takes
    # hours, so the host leg is skipped beyond HOST_BUDGET face visits
    ncomp = int(m.counts.cpu()[_lib.MESHCC_NCOMP])
    skipped = ncomp * m.nt > HOST_BUDGET
    if skipped:
        print(f'[{name}] host leg skipped: {ncomp} components x {m.nt} faces is beyond {HOST_BUDGET:.0e} face visits')
        host_rounds = 0
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(legs[k]())
        if r < host_rounds:
            ms, (hv, ht) = m.leg_c()
            times['c'].append(ms)
            if same is None:
                kv, kt = m.leg_b()[1]
                same = bool(np.array_equal(kv.cpu().numpy(), hv) and np.array_equal(kt.cpu().numpy(), ht))
    # the vectorised restatement: against the device result always, against the host pass where that ran
    t0 = time.perf_counter()
    rv, rt = vectorised_reference(m.v.cpu().numpy(), m.t.cpu().numpy())
    ref_ms = (time.perf_counter() - t0) * 1e3
    kv, kt = m.leg_b()[1]
    same_ref = bool(np.array_equal(kv.cpu().numpy(), rv) and np.array_equal(kt.cpu().numpy(), rt))
    print(f'[{name}] device == vectorised host restatement (scipy connected components, {ref_ms:.0f} ms): {same_ref}'
          + ('' if skipped or not host_rounds else f'; restatement == host pass: {bool(np.array_equal(rv, hv) and np.array_equal(rt, ht))}'))
    c = m.counts.cpu().tolist()
    names = {'a': 'device pass, count + emit (events)', 'b': 'largest_component_device end to end',
             'c': 'host largest_component + D2H of the mesh', 'm': 'device marching cubes (for scale)'}
    print(f'[{name}] {m.nv} vertices, {m.nt} triangles; counts (V\', T\', components, watertight, kept, status) {c}; '
          f'workspace {m.nbytes / 2 ** 20:.1f} MiB; device == host: {same}')
    med = {}
    for k in ('a', 'b', 'c', 'm'):
        v = times[k]
        if not v:
            continue
        med[k] = statistics.median(v)
        print(f'[{name}] ({k}) {names[k]:44s} ms: median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}  '
              f'rounds {" ".join(f"{x:.3f}" for x in v)}')
    if 'c' in med:
        print(f'[{name}] host / device end to end: {med["c"] / med["b"]:.1f}x; host per triangle '
              f'{1e3 * med["c"] / max(m.nt, 1):.2f} us; device pass per triangle {1e6 * med["a"] / max(m.nt, 1):.2f} ns')
    return {'nv': m.nv, 'nt': m.nt, 'counts': c, 'same': same, 'same_vectorised': same_ref, 'workspace_bytes': m.nbytes,
            'ms': {k: {'median': med[k], 'min': min(times[k]), 'max': max(times[k]), 'rounds': times[k]} for k in med}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3, help='rounds that also run the host leg (c), small mesh')
    ap.add_argument('--host-rounds-large', type=int, default=1, help='the same for the large mesh (it takes seconds)')
    ap.add_argument('--voxel', type=float, default=0.005, help='voxel size of the large mesh (the reference: 5 mm)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mesh_cc_ab.py needs a GPU: there is nothing to time without one')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    out = {'rounds': args.rounds, 'reps': args.reps, 'voxel': args.voxel}
    small = Mesh(lib, dev, spheres_cube(dev), 0.0, 0)
    out['small'] = run('small', small, args.rounds, args.reps, args.host_rounds)
    del small
    large = Mesh(lib, dev, alpha_cube(dev, args.voxel), 2.95, 10)
    out['large'] = run('large', large, args.rounds, args.reps, args.host_rounds_large)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
