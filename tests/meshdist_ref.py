"""Helpers for the mesh-evaluator tests (no test in here): the float64 numpy restatement of the surface
sampling rule, brute-force closest-face distances through ``bwvol_ref.tri_distance_matrix``, the Chamfer /
P2S metrics, the float32 restatement of the search's selection with the builder's centring, and the seeded
meshes, uniforms and query sets the CPU and GPU tests share (csrc/anr_meshdist.hip)."""
import functools

import numpy as np

from . import bwvol_ref as R

N_CHAMFER, N_P2S = 1000, 10000
SHIFT = np.array([3.0, -2.0, 5.0])
DELTA = 1e-6  # the project's selection bar (tests/test_gpu_bwvol.py)


# ---- sampling ---------------------------------------------------------------------------------------------
def face_areas(verts, faces):
    """0.5 |e0 x e1| in float64 from the float32 vertices, e0 = b - a, e1 = c - a (the kernel's expression)."""
    V = np.asarray(verts, dtype=np.float32).astype(np.float64)
    a, b, c = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    e0, e1 = b - a, c - a
    cx = e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1]
    cy = e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2]
    cz = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def sample_surface(verts, faces, u):
    """The sampling rule: face = searchsorted(cumsum(area), u0 cum[-1], 'left'); (u1, u2) -> |u - 1| when
    u1 + u2 > 1; point = a + (e0 u1 + e1 u2). -> points (n,3) float64, face (n,) int64."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    cum = np.cumsum(face_areas(verts, faces))
    k = np.searchsorted(cum, u[:, 0] * cum[-1], side='left')
    V = np.asarray(verts, dtype=np.float32).astype(np.float64)
    a, b, c = V[faces[k, 0]], V[faces[k, 1]], V[faces[k, 2]]
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    flip = u1 + u2 > 1.0
    u1[flip] = np.abs(u1[flip] - 1.0)
    u2[flip] = np.abs(u2[flip] - 1.0)
    e0, e1 = b - a, c - a
    return a + (e0 * u1[:, None] + e1 * u2[:, None]), k


def cum_margin(verts, faces, u0):
    """The smallest distance of any u0 cum[-1] to an entry of cumsum(area), in units of
    tau = nf 2^-52 cum[-1] (the bound on the difference of two summation orders)."""
    cum = np.cumsum(face_areas(verts, faces))
    x = np.asarray(u0, dtype=np.float64) * cum[-1]
    i = np.clip(np.searchsorted(cum, x, side='left'), 0, len(cum) - 1)
    gap = np.minimum(np.abs(cum[i] - x), np.abs(x - cum[np.maximum(i - 1, 0)]))
    return gap.min() / (len(faces) * 2.0 ** -52 * cum[-1])


# ---- distances ---------------------------------------------------------------------------------------------
def brute_force(P, verts, faces, chunk=1024):
    """Per point the float64 distance to the closest face and that face (lowest index on a tie), through
    bwvol_ref.tri_distance_matrix in row chunks (the whole matrix is never held)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    d, k = np.empty(len(P)), np.empty(len(P), np.int64)
    for s in range(0, len(P), chunk):
        D = R.tri_distance_matrix(P[s:s + chunk], verts, faces)
        k[s:s + chunk] = D.argmin(axis=1)
        d[s:s + chunk] = D[np.arange(len(D)), k[s:s + chunk]]
    return d, k


def nan0_mean(d):
    d = np.asarray(d, dtype=np.float64)
    return np.where(np.isnan(d), 0.0, d).mean()


def metrics(src, tgt, u, n_chamfer=N_CHAMFER, n_p2s=N_P2S):
    """{'chamfer', 'p2s', 'src_tgt', 'tgt_src'} of (verts, faces) pairs from the (2 n_chamfer + n_p2s, 3)
    uniforms in the reference's draw order: Chamfer source, Chamfer target, P2S source."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    ps, _ = sample_surface(*src, u[:n_chamfer])
    pt, _ = sample_surface(*tgt, u[n_chamfer:2 * n_chamfer])
    pp, _ = sample_surface(*src, u[2 * n_chamfer:2 * n_chamfer + n_p2s])
    st = nan0_mean(brute_force(ps, *tgt)[0])
    ts = nan0_mean(brute_force(pt, *src)[0])
    p2s = nan0_mean(brute_force(pp, *tgt)[0])
    return {'chamfer': (st + ts) / 2, 'p2s': p2s, 'src_tgt': st, 'tgt_src': ts}


# ---- the float32 selection, with the builder's centring ----------------------------------------------------
def centre(verts, faces):
    """The builder's centre: the midpoint, in float64, of the float32 box of the vertices the faces use."""
    used = np.asarray(verts, dtype=np.float32)[np.clip(faces, 0, len(verts) - 1).reshape(-1)]
    return 0.5 * (used.min(axis=0).astype(np.float64) + used.max(axis=0).astype(np.float64))


def select_f32(P, verts, faces, chunk=512):
    """The face the float32 search selects: records and queries about ``centre`` (subtracted in float64, then
    cast), lexicographic (float32 d^2 of bwvol_ref.tri_d2_f32, face index) minimum over every face."""
    ctr = centre(verts, faces)
    t = R.tri_records(np.asarray(verts, dtype=np.float32).astype(np.float64) - ctr, faces)
    p = (np.asarray(P, dtype=np.float64) - ctr).astype(np.float32)
    k = np.empty(len(p), np.int64)
    for s in range(0, len(p), chunk):
        k[s:s + chunk] = R.tri_d2_f32(p[s:s + chunk], t, slice(None)).argmin(axis=1)  # first minimum: lowest index
    return k


# ---- the shared cases ---------------------------------------------------------------------------------------
def uniforms(n, seed=11):
    return np.random.Generator(np.random.PCG64(seed)).random((n, 3))


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts float32, faces int32) of a named test mesh."""
    if name == 'A':
        return R.mesh_a()
    if name == 'B':
        return R.mesh_b()
    if name == 'A_degenerate':  # as tests/test_gpu_bwvol.py: the first face again, an edge face, a point face
        v, f = R.mesh_a()
        return v, np.concatenate([f, f[:1], [[f[0, 0], f[0, 0], f[0, 1]], [5, 5, 5]]]).astype(np.int32)
    if name == 'zero_face':     # a single zero-area face
        v, _ = R.mesh_a()
        return v, np.array([[3, 3, 40]], np.int32)
    if name == 'big':           # 70,312 faces, just above 2^16
        return R.ellipsoid(188, 188)
    if name == 'B_shifted':     # world space: metres from the origin
        v, f = R.mesh_b()
        return (v.astype(np.float64) + SHIFT).astype(np.float32), f
    if name == 'B_scaled':      # the end-to-end target: B scaled by 1.02 and shifted
        v, f = R.mesh_b()
        return (v.astype(np.float64) * 1.02 + np.array([0.004, -0.003, 0.002])).astype(np.float32), f
    raise KeyError(name)


DIST_CASES = ('A', 'B', 'A_degenerate', 'zero_face', 'big', 'B_shifted')


@functools.lru_cache(maxsize=None)
def queries(name):
    """The float64 query points of a distance case: samples of a scaled, shifted copy of the mesh, points
    exactly on vertices and on edge midpoints, points far outside the box, one point 130 times; 875 in all
    (no multiple of 64). 'big' takes a seeded subset of 256 of them; 'B_shifted' B's, translated."""
    if name == 'B_shifted':
        return queries('B') + SHIFT
    base = 'A' if name in ('A_degenerate', 'zero_face') else name
    v, f = mesh(base)
    V = v.astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(23))
    ctr = V.mean(axis=0)
    copy = ((V - ctr) * 1.03 + ctr + np.array([0.006, -0.004, 0.005])).astype(np.float32)
    near, _ = sample_surface(copy, f, rng.random((601, 3)))
    on_v = V[rng.choice(len(V), 64, replace=False)]
    fe = f[rng.choice(len(f), 64, replace=False)]
    mid = 0.5 * (V[fe[:, 0]] + V[fe[:, 1]])
    far = ctr + rng.standard_normal((16, 3)) * 40.0
    rep = np.repeat(near[7:8], 130, axis=0)
    P = np.concatenate([near, on_v, mid, far, rep])
    assert len(P) == 875
    if name == 'big':
        P = P[np.sort(rng.choice(len(P), 256, replace=False))]
    return P


@functools.lru_cache(maxsize=None)
def distance_reference(name):
    """(d_min, k_min) of the case's queries by brute force, computed once."""
    return brute_force(queries(name), *mesh(name))


def face_distance(P, verts, faces, k):
    """float64 distance of point i to face k[i], by bwvol_ref._tri_dist2 (the matrix's own entries)."""
    import torch
    V = torch.from_numpy(np.asarray(verts, dtype=np.float32).astype(np.float64))
    F = torch.from_numpy(np.asarray(faces)[np.asarray(k)].astype(np.int64))
    Pt = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64))
    return R._tri_dist2(Pt, V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]).sqrt().numpy()
