"""Meshes for the component pass (anr_mesh_cc_count / anr_mesh_cc_emit) and its host yardstick.

``case(name)`` -> (vertices (V,3) float64, triangles (T,3) int64), built once per name.
``host(name)`` -> the host ``renderer_sdf_mesh.largest_component`` of that mesh, computed once.
``host_labels(triangles)`` restates the host pass's union-find alone (its ``root`` array, which the host
function does not return): a face's label is the lowest face index of its edge-connected component.
tests/test_mesh_cc_api.py checks, on the CPU, that the cases have the properties the GPU tests rely on."""
import functools

import numpy as np

from animatable_nerf_amd.renderer_sdf_mesh import largest_component

TET = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int64)  # a closed tetrahedron
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)


def box(offset, scale=1.0):
    v = (np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64) * scale) + offset
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [(a, b, c) for a, b, c, d in q] + [(a, c, d) for a, b, c, d in q]
    return v, np.array(t, np.int64)


def host_labels(triangles):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    parent = np.arange(len(t))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    first = {}
    for f, tri in enumerate(t.tolist()):
        for k in range(3):
            e = (min(tri[k], tri[(k + 1) % 3]), max(tri[k], tri[(k + 1) % 3]))
            g = first.setdefault(e, f)
            ra, rb = find(f), find(g)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(f) for f in range(len(t))], np.int64)


def edge_multiplicities(triangles):
    """-> (unique undirected edges (E,2), their side counts (E,), the face of each edge's first side)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    face = np.tile(np.arange(len(t)), 3)
    u, first, cnt = np.unique(e, axis=0, return_index=True, return_counts=True)
    return u, cnt, face[first]


def components(triangles):
    """-> {label: (watertight, number of distinct vertices)} under the host semantics"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    root = host_labels(t)
    _, cnt, f = edge_multiplicities(t)
    bad = set(root[f[cnt != 2]].tolist())
    return {int(r): (int(r) not in bad, len(np.unique(t[root == r]))) for r in np.unique(root)}


def tets(n, seed, open_triangle=False):
    """n disjoint tetrahedra (every one watertight, 4 vertices: all tie), faces shuffled; optionally one
    open triangle appended (3 more vertices), which shifts nt off a multiple of 4"""
    rng = np.random.default_rng(seed)
    v = (TET_V[None] + 3.0 * np.arange(n)[:, None, None]).reshape(-1, 3)
    t = (TET[None] + 4 * np.arange(n)[:, None, None]).reshape(-1, 3)
    if open_triangle:
        v = np.concatenate([v, TET_V[:3] - 5.0])
        t = np.concatenate([t, [[4 * n, 4 * n + 1, 4 * n + 2]]])
    return v, t[rng.permutation(len(t))]


def mc(vol, iso=0.0):
    from oracle import mcubes
    return mcubes.marching_cubes(np.asarray(vol, np.float32).astype(np.float64), iso)


def tube_volume():
    """a thin long box of 4 x 4 x 200 inside voxels: its surface is one closed tube, whose union chains
    run the length of the face list"""
    vol = -np.ones((8, 8, 204), np.float32)
    vol[2:6, 2:6, 2:202] = 1.0
    return vol


def pieces_volume():
    """48^3: two closed spheres of different radius, a small closed floater, and a sphere cut open by the
    volume's border (the largest piece, not watertight)"""
    x = np.arange(48, dtype=np.float64)
    g = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1)
    d = lambda c, r: r - np.linalg.norm(g - np.array(c, np.float64), axis=-1)  # noqa: E731
    vol = np.maximum.reduce([d((14.3, 14.1, 14.2), 9.4), d((34.2, 33.9, 14.4), 6.3), d((10.1, 38.2, 36.3), 2.2),
                             d((36.0, 30.0, 47.0), 15.7)])
    return vol.astype(np.float32)


def bipyramid(n):
    """closed: n rim vertices, two apexes of valence n"""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.cos(a), np.sin(a), 0 * a], 1), [[0, 0, 1.0], [0, 0, -1.0]]])
    i = np.arange(n)
    j = (i + 1) % n
    t = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)])
    return v, t.astype(np.int64)


def _join(parts):
    """concatenate (v, t) pieces, offsetting the indices"""
    vs, ts, o = [], [], 0
    for v, t in parts:
        vs.append(v)
        ts.append(t + o)
        o += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def _build(name):
    rng = np.random.default_rng(7)
    if name == 'boxes3':
        # two closed boxes that tie on vertices and an open one (a face missing, beside 4 vertices no face uses);
        # vertices permuted, so the kept
        # piece's vertex order must be preserved
        v3 = np.concatenate([box(-9.0)[0], box(-9.0)[0][:4] + 0.5])
        v, t = _join([box(0.0), box(5.0, 2.0), (v3, box(-9.0)[1][:-1])])
        perm = np.random.default_rng(0).permutation(len(v))
        return v[perm], np.argsort(perm)[t]
    if name == 'glued':
        # an extra face on an edge of box 2 (multiplicity 3) that touches box 3 in one vertex only: box 2 is
        # not watertight, boxes 1 and 3 tie and box 1 is kept
        v1, t1 = box(0.0)
        v4, t4 = box(20.0)
        return np.concatenate([v1, v4, v4 + 100.0]), np.concatenate([t1, t4 + 8, t4 + 16, np.array([[8, 9, 16]])])
    if name == 'open':
        v, t = box(0.0)
        return v, t[:-1]
    if name == 'empty':
        return TET_V.copy(), np.zeros((0, 3), np.int64)
    if name.startswith('tets'):  # tets63, tets64o, ...
        n = int(name[4:].rstrip('o'))
        return tets(n, n, name.endswith('o'))
    if name.startswith('tube'):
        v, t = mc(tube_volume())
        if name == 'tube_reversed':
            t = t[::-1].copy()
        elif name == 'tube_random':
            t = t[rng.permutation(len(t))]
        return v, t
    if name == 'bipyramid':
        return bipyramid(300)
    if name == 'shared_vertex':
        # two tetrahedra with exactly one vertex in common: two components, the vertex counted in both
        return np.concatenate([TET_V, TET_V[1:] + 4.0]), np.concatenate([TET, np.array([0, 4, 5, 6])[TET]])
    if name == 'dup_degenerate':
        # a closed box; a tetrahedron with every face twice (edges of multiplicity 4); a tetrahedron plus
        # the degenerate face (0, 0, 1) (edge (0, 1) of multiplicity 4, edge (0, 0) of multiplicity 1);
        # a two-triangle pillow (closed, 3 vertices)
        pillow = (TET_V[:3] + 30.0, np.array([[0, 1, 2], [0, 2, 1]], np.int64))
        v, t = _join([(TET_V + 10.0, np.concatenate([TET, TET])),
                      (TET_V + 20.0, np.concatenate([TET, [[0, 0, 1]]])), pillow, box(0.0)])
        return v, t
    if name == 'unreferenced':
        v, t = box(0.0)
        ids = np.sort(rng.choice(40, 8, replace=False))
        vv = rng.normal(size=(40, 3))
        vv[ids] = v
        return vv, ids[t]
    if name == 'interleaved':
        # a tetrahedron on the even vertex ids below 8 and a box on the other ids: the box is kept and its
        # vertices are not contiguous in the input
        tid = np.array([0, 2, 4, 6])
        bid = np.array([1, 3, 5, 7, 8, 9, 10, 11])
        vv = np.zeros((12, 3))
        vv[tid], vv[bid] = TET_V + 50.0, box(0.0)[0]
        return vv, np.concatenate([tid[TET], bid[box(0.0)[1]]])
    if name == 'many_vertices':
        # 263,000 vertices (more than 1,024 scan blocks of 256) with three tetrahedra and a box spread over
        # them: the vertex scans carry across the tiles of the block-sum scan
        nv = 263_000
        vv = rng.normal(size=(nv, 3))
        ts = []
        for base, (pv, pt) in zip((5, 131_070, 262_140, 262_990), ((TET_V, TET), (TET_V, TET), box(0.0), (TET_V, TET))):
            ids = base + 2 * np.arange(len(pv))
            vv[ids] = pv
            ts.append(ids[pt])
        return vv, np.concatenate(ts)
    if name == 'pieces':
        return mc(pieces_volume())
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    v, t = _build(name)
    v, t = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(t, np.int64)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def case(name):
    return _case(name)


@functools.lru_cache(maxsize=None)
def host(name):
    v, t = case(name)
    kv, kt = largest_component(v, t)
    return np.asarray(kv), np.asarray(kt)


@functools.lru_cache(maxsize=None)
def labels(name):
    return host_labels(case(name)[1])


TET_COUNTS = (63, 64, 65, 1025)
CASES = (['boxes3', 'glued', 'open', 'empty'] + [f'tets{n}' for n in TET_COUNTS] + [f'tets{n}o' for n in TET_COUNTS] +
         ['tube', 'tube_reversed', 'tube_random', 'bipyramid', 'shared_vertex', 'dup_degenerate', 'unreferenced',
          'interleaved', 'many_vertices', 'pieces'])
