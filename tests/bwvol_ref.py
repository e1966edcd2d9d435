"""Helpers for the blend-weight-volume tests (no test in here): a float64 numpy restatement of the
point-triangle distance, the seeded test meshes, and a float32 restatement of the kernel's search with
its cell-pruning rule (csrc/anr_bwvol.hip)."""
import numpy as np
import torch

SEMI = np.array([0.25, 0.15, 0.45])
CENTRE = np.array([0.013, -0.007, 0.021])


def ellipsoid(nlat, nlon, seed=5, jitter=0.06, semi=None, centre=None):
    """Closed lat-long ellipsoid (semi-axes SEMI about CENTRE unless given), every vertex radius scaled by
    1 + jitter N(0,1) (PCG64(seed)): poles first and last, rings in between; (V,3) float32 vertices and
    (F,3) int32 faces."""
    semi = SEMI if semi is None else np.asarray(semi, dtype=np.float64)
    centre = CENTRE if centre is None else np.asarray(centre, dtype=np.float64)
    rng = np.random.Generator(np.random.PCG64(seed))
    dirs = [np.array([0.0, 0.0, 1.0])]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2.0 * np.pi * j / nlon
            dirs.append(np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    dirs.append(np.array([0.0, 0.0, -1.0]))
    dirs = np.stack(dirs)
    scale = 1.0 + jitter * rng.standard_normal(len(dirs))
    verts = (dirs * semi * scale[:, None] + centre).astype(np.float32)
    ring = lambda i, j: 1 + (i - 1) * nlon + (j % nlon)  # noqa: E731
    south = len(dirs) - 1
    faces = []
    for j in range(nlon):
        faces.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            faces.append((a, c, d))
            faces.append((a, d, b))
    for j in range(nlon):
        faces.append((south, ring(nlat - 1, j + 1), ring(nlat - 1, j)))
    return verts, np.array(faces, dtype=np.int32)


def mesh_a():
    return ellipsoid(12, 16)


def mesh_b():
    return ellipsoid(36, 48)


def skin_weights(nv, nb, seed=6):
    """Seeded per-vertex weights (nv, nb) float32, positive, rows normalised in float64 before the cast."""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.random((nv, nb)) ** 4
    return (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


def grid_points(origin, dims, vsize):
    """float64 voxel positions (N,3) in C order of (X,Y,Z): origin + index * vsize."""
    ax = [origin[c] + np.arange(dims[c], dtype=np.float64) * vsize for c in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1).reshape(-1, 3)


def _seg_bary(ap, e):
    ee = np.sum(e * e, axis=-1)
    t = np.where(ee > 0.0, np.sum(ap * e, axis=-1) / np.where(ee > 0.0, ee, 1.0), 0.0)
    return np.clip(t, 0.0, 1.0)


def closest_bary(P, a, b, c):
    """Barycentrics (..., 3) of the closest point of triangles (a, b, c) to points P (broadcast against
    each other, float64): the projection when it lies inside the triangle, else the closest of the three
    edge segments; and the distance."""
    e0, e1, e2 = b - a, c - a, c - b
    ap, bp = P - a, P - b
    d00, d01, d11 = np.sum(e0 * e0, -1), np.sum(e0 * e1, -1), np.sum(e1 * e1, -1)
    d1, d2 = np.sum(ap * e0, -1), np.sum(ap * e1, -1)
    det = d00 * d11 - d01 * d01
    ok = det > 1e-10 * d00 * d11
    sd = np.where(ok, det, 1.0)
    s = (d11 * d1 - d01 * d2) / sd
    r = (d00 * d2 - d01 * d1) / sd
    inside = ok & (s >= 0.0) & (r >= 0.0) & (s + r <= 1.0)
    t0, t1, t2 = _seg_bary(ap, e0), _seg_bary(ap, e1), _seg_bary(bp, e2)
    z = np.zeros_like(t0)
    cands = [np.stack([1.0 - t0, t0, z], -1), np.stack([1.0 - t1, z, t1], -1), np.stack([z, 1.0 - t2, t2], -1)]
    best_w, best_d = None, None
    for w in cands:
        q = w[..., 0:1] * a + w[..., 1:2] * b + w[..., 2:3] * c
        d = np.sum((P - q) ** 2, -1)
        if best_d is None:
            best_w, best_d = w, d
        else:
            m = d < best_d
            best_w = np.where(m[..., None], w, best_w)
            best_d = np.where(m, d, best_d)
    wi = np.stack([1.0 - s - r, s, r], -1)
    qi = wi[..., 0:1] * a + wi[..., 1:2] * b + wi[..., 2:3] * c
    di = np.sum((P - qi) ** 2, -1)
    best_w = np.where(inside[..., None], wi, best_w)
    best_d = np.where(inside, di, best_d)
    return best_w, np.sqrt(best_d)


def _tri_dist2(P, a, b, c):
    """Squared distances only, float64 torch tensors (multi-threaded; the matrix of mesh B has 2e7
    entries): the same definition as closest_bary."""
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    e0, e1, e2 = b - a, c - a, c - b
    ap, bp = P - a, P - b
    d00, d01, d11, d22 = dot(e0, e0), dot(e0, e1), dot(e1, e1), dot(e2, e2)
    d1, d2, d3 = dot(ap, e0), dot(ap, e1), dot(bp, e2)
    det = d00 * d11 - d01 * d01
    ok = det > 1e-10 * d00 * d11
    sd = torch.where(ok, det, torch.ones_like(det))
    s = (d11 * d1 - d01 * d2) / sd
    r = (d00 * d2 - d01 * d1) / sd
    inside = ok & (s >= 0.0) & (r >= 0.0) & (s + r <= 1.0)

    def seg(x, ee):
        return torch.where(ee > 0.0, x / torch.where(ee > 0.0, ee, torch.ones_like(ee)), torch.zeros_like(x)).clamp(0.0, 1.0)

    t0, t1, t2 = seg(d1, d00), seg(d2, d11), seg(d3, d22)
    out = ((ap - t0[..., None] * e0) ** 2).sum(-1)
    out = torch.minimum(out, ((ap - t1[..., None] * e1) ** 2).sum(-1))
    out = torch.minimum(out, ((bp - t2[..., None] * e2) ** 2).sum(-1))
    di = ((ap - s[..., None] * e0 - r[..., None] * e1) ** 2).sum(-1)
    return torch.where(inside, di, out)


def tri_distance_matrix(P, verts, faces, chunk=1024):
    """(N, F) float64 distances from points P (N,3) to every triangle."""
    V = torch.from_numpy(verts.astype(np.float64))
    F = torch.from_numpy(faces.astype(np.int64))
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    Pt = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64))
    out = torch.empty((len(P), len(faces)), dtype=torch.float64)
    for s in range(0, len(P), chunk):
        out[s:s + chunk] = _tri_dist2(Pt[s:s + chunk, None, :], a, b, c).sqrt()
    return out.numpy()


def tri_weights(P, verts, faces, skin, k):
    """float64 interpolated weights (N, nb) and distance (N,) of point n on its face k[n]."""
    V = verts.astype(np.float64)
    f = faces[k]
    w, d = closest_bary(P, V[f[:, 0]], V[f[:, 1]], V[f[:, 2]])
    S = skin.astype(np.float64)
    return w[:, 0:1] * S[f[:, 0]] + w[:, 1:2] * S[f[:, 1]] + w[:, 2:3] * S[f[:, 2]], d


def vert_distance_matrix(P, verts, chunk=2048):
    V = verts.astype(np.float64)
    out = np.empty((len(P), len(V)))
    for s in range(0, len(P), chunk):
        out[s:s + chunk] = np.sqrt(np.sum((P[s:s + chunk, None, :] - V[None]) ** 2, -1))
    return out


# ---- float32 restatement of the kernel's search (k_bwv_search) ---------------------------------------
F32 = np.float32
CELL = 64
REL = F32(1e-5)
EPS = F32(5.9604644775390625e-08)


def _sq3(x, y, z):
    return (x * x + y * y) + z * z


def tri_records(verts, faces):
    V = verts.astype(np.float64)
    a, b, c = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    e0, e1 = b - a, c - a
    d00, d01, d11 = np.sum(e0 * e0, -1), np.sum(e0 * e1, -1), np.sum(e1 * e1, -1)
    d22, det = d00 - 2.0 * d01 + d11, d00 * d11 - d01 * d01
    inv = lambda x, ok: np.where(ok, 1.0 / np.where(ok, x, 1.0), 0.0).astype(F32)  # noqa: E731
    return dict(a=a.astype(F32), e0=e0.astype(F32), e1=e1.astype(F32), d00=d00.astype(F32), d01=d01.astype(F32),
                d11=d11.astype(F32), r00=inv(d00, d00 > 0), r11=inv(d11, d11 > 0), r22=inv(d22, d22 > 0),
                rdet=inv(det, det > 1e-10 * d00 * d11))


def tri_d2_f32(p, t, sl):
    """float32 squared distances (n, m) from points p (n,3) float32 to the records t[sl] (m of them)."""
    a, e0, e1 = t['a'][sl][None], t['e0'][sl][None], t['e1'][sl][None]
    ap = p[:, None, :] - a
    ax, ay, az = ap[..., 0], ap[..., 1], ap[..., 2]
    d1 = (ax * e0[..., 0] + ay * e0[..., 1]) + az * e0[..., 2]
    d2 = (ax * e1[..., 0] + ay * e1[..., 1]) + az * e1[..., 2]
    one, zero = F32(1), F32(0)
    t0 = np.clip(d1 * t['r00'][sl][None], zero, one)
    best = _sq3(ax - t0 * e0[..., 0], ay - t0 * e0[..., 1], az - t0 * e0[..., 2])
    t1 = np.clip(d2 * t['r11'][sl][None], zero, one)
    best = np.minimum(best, _sq3(ax - t1 * e1[..., 0], ay - t1 * e1[..., 1], az - t1 * e1[..., 2]))
    t2 = np.clip(((d2 - d1) + (t['d00'][sl] - t['d01'][sl])[None]) * t['r22'][sl][None], zero, one)
    u = one - t2
    best = np.minimum(best, _sq3((ax - u * e0[..., 0]) - t2 * e1[..., 0], (ay - u * e0[..., 1]) - t2 * e1[..., 1],
                                 (az - u * e0[..., 2]) - t2 * e1[..., 2]))
    rdet = t['rdet'][sl][None]
    s = (t['d11'][sl][None] * d1 - t['d01'][sl][None] * d2) * rdet
    r = (t['d00'][sl][None] * d2 - t['d01'][sl][None] * d1) * rdet
    dp = _sq3((ax - s * e0[..., 0]) - r * e1[..., 0], (ay - s * e0[..., 1]) - r * e1[..., 1],
              (az - s * e0[..., 2]) - r * e1[..., 2])
    inside = (s >= 0) & (r >= 0) & (s + r <= 1) & (rdet != 0)
    out = np.minimum(best, np.where(inside, dp, F32(np.inf)))
    assert out.dtype == F32
    return out


def morton_order(verts, faces, lo, hi):
    """Faces sorted by (30-bit Morton code of the centroid over [lo, hi], index)."""
    cen = verts[faces].astype(np.float64).mean(axis=1)
    ext = np.where(hi > lo, hi - lo, 1.0)
    q = np.clip(((cen - lo) * (1023.0 / ext)).astype(np.int64), 0, 1023)
    code = np.zeros(len(faces), np.int64)
    for b in range(10):
        for c in range(3):
            code |= ((q[:, c] >> b) & 1) << (3 * b + c)
    return np.argsort((code << 32) | np.arange(len(faces)), kind='stable')


def cell_boxes(verts, faces):
    """Per cell of 64 consecutive faces: float32 lo, hi, the absolute margin 32 eps diag^2 and the
    representative point (first vertex of the cell's first face)."""
    tv = verts[faces]  # (F,3,3)
    lo, hi, rep = [], [], []
    for s in range(0, len(faces), CELL):
        lo.append(tv[s:s + CELL].reshape(-1, 3).min(0))
        hi.append(tv[s:s + CELL].reshape(-1, 3).max(0))
        rep.append(tv[s, 0])
    lo, hi = np.array(lo, F32), np.array(hi, F32)
    e = hi - lo
    return lo, hi, F32(32) * EPS * _sq3(e[:, 0], e[:, 1], e[:, 2]), np.array(rep, F32)


def box_d2_f32(p, lo, hi):
    d = np.maximum(np.maximum(lo - p, p - hi), F32(0))
    return _sq3(d[..., 0], d[..., 1], d[..., 2])


def search_f32(p, verts, faces, prune, glo, ghi):
    """One 'wave' (the rows of p, float32) over Morton-ordered cells of 64 faces: lexicographic
    (d2, original index) update; pruned, a cell is skipped when its box bound exceeds
    thr (1 + REL) + 32 eps diag^2 for every row, thr = min(best, ub) and ub the smallest
    |p - rep|^2 (1 + REL) + 32 eps diag^2 over the cells. Returns (best d2, index, cells visited)."""
    order = morton_order(verts, faces, glo, ghi)
    sf = faces[order]
    t = tri_records(verts, sf)
    lo, hi, mabs, rep = cell_boxes(verts, sf)
    best = np.full(len(p), np.inf, F32)
    besti = np.full(len(p), np.iinfo(np.int64).max, np.int64)
    ub = np.full(len(p), np.inf, F32)
    if prune:
        for c in range(len(lo)):
            d = p - rep[c]
            u = _sq3(d[:, 0], d[:, 1], d[:, 2])
            ub = np.minimum(ub, (u * REL + u) + mabs[c])
    visited = 0
    for c in range(len(lo)):
        thr = np.minimum(best, ub)
        if prune and np.all(box_d2_f32(p, lo[c], hi[c]) > (thr * REL + thr) + mabs[c]):
            continue
        visited += 1
        sl = slice(c * CELL, min((c + 1) * CELL, len(sf)))
        d = tri_d2_f32(p, t, sl)
        o = order[sl]
        for k in range(d.shape[1]):
            m = (d[:, k] < best) | ((d[:, k] == best) & (o[k] < besti))
            best = np.where(m, d[:, k], best)
            besti = np.where(m, o[k], besti)
    return best, besti, visited
