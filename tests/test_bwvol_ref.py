"""CPU: the blend-weight-volume oracle helpers (tests/bwvol_ref.py), ``volumes.grid`` and the
cell-pruning rule of k_bwv_search (csrc/anr_bwvol.hip) restated in float32 numpy.

The pruning claim under test: over Morton-ordered cells of 64 faces, skipping a cell when its float32
box bound exceeds thr * (1 + 1e-5) + 32 eps diag^2 for every voxel of the brick (thr: the smaller of the
voxel's best so far and its upper bound from the cells' representative points) gives exactly the
lexicographic minimum (d^2, index) of the exhaustive visit (DESIGN.md §2 'Blend-weight volumes')."""
import numpy as np

from animatable_nerf_amd import synthetic, volumes
from tests import bwvol_ref as R


def test_mesh_sizes_and_grids():
    va, fa = R.mesh_a()
    vb, fb = R.mesh_b()
    assert va.shape == (178, 3) and fa.shape == (352, 3)
    assert fb.shape == (3360, 3)
    # closed and consistently wound: every directed edge appears once, its reverse once
    for f in (fa, fb):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
        key = e[:, 0] * 100000 + e[:, 1]
        rev = e[:, 1] * 100000 + e[:, 0]
        assert len(np.unique(key)) == len(key)
        assert set(key) == set(rev)


def test_surface_samples_have_zero_distance_and_their_weights():
    v, f = R.mesh_a()
    skin = R.skin_weights(len(v), 24)
    rng = np.random.Generator(np.random.PCG64(1))
    k = rng.integers(0, len(f), 400)
    b = rng.dirichlet([1.0, 1.0, 1.0], 400)
    V = v.astype(np.float64)
    P = b[:, 0:1] * V[f[k, 0]] + b[:, 1:2] * V[f[k, 1]] + b[:, 2:3] * V[f[k, 2]]
    w, d = R.tri_weights(P, v, f, skin, k)
    assert d.max() <= 1e-12
    S = skin.astype(np.float64)
    want = b[:, 0:1] * S[f[k, 0]] + b[:, 1:2] * S[f[k, 1]] + b[:, 2:3] * S[f[k, 2]]
    assert np.abs(w - want).max() <= 1e-9
    assert R.tri_distance_matrix(P, v, f).min(axis=1).max() <= 1e-12
    # the distance-only routine and the barycentric one are the same definition
    Q = P + rng.normal(0.0, 0.1, P.shape)
    D = R.tri_distance_matrix(Q, v, f)
    _, d = R.tri_weights(Q, v, f, skin, k)
    assert np.abs(D[np.arange(len(Q)), k] - d).max() <= 1e-14


def test_distance_is_sandwiched():
    v, f = R.mesh_a()
    origin, dims = volumes.grid(v, 0.05)
    P = R.grid_points(origin, dims, 0.05)[::7]
    D = R.tri_distance_matrix(P, v, f)
    dmin = D.min(axis=1)
    # never above the nearest vertex
    assert np.all(dmin <= R.vert_distance_matrix(P, v).min(axis=1) + 1e-15)
    # a dense barycentric sampling (step h) bounds it from above within h * (longest edge)
    h = 1.0 / 24
    i, j = np.meshgrid(np.arange(25), np.arange(25), indexing='ij')
    m = i + j <= 24
    b = np.stack([i[m], j[m], 24 - i[m] - j[m]], -1) * h
    V = v.astype(np.float64)
    S = np.einsum('sb,fbc->fsc', b, V[f])  # (F, samples, 3)
    longest = max(np.linalg.norm(V[f[:, a]] - V[f[:, c]], axis=1).max() for a, c in ((0, 1), (1, 2), (2, 0)))
    for n in range(0, len(P), 40):
        ds = np.sqrt(((S - P[n]) ** 2).sum(-1)).min()
        assert dmin[n] <= ds + 1e-15
        assert ds <= dmin[n] + h * longest


def test_degenerate_triangles_are_finite():
    v, f = R.mesh_a()
    f2 = np.concatenate([f, [[f[0, 0], f[0, 0], f[0, 1]], [5, 5, 5]]]).astype(np.int32)
    origin, dims = volumes.grid(v, 0.05)
    P = R.grid_points(origin, dims, 0.05)[::11]
    D = R.tri_distance_matrix(P, v, f2)
    assert np.all(np.isfinite(D))
    V = v.astype(np.float64)
    assert np.allclose(D[:, -1], np.linalg.norm(P - V[5], axis=1), rtol=0, atol=1e-15)
    w, d = R.tri_weights(P, v, f2, R.skin_weights(len(v), 24), np.full(len(P), len(f2) - 2))
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(d))
    # the float32 restatement too
    t = R.tri_records(v, f2)
    assert np.all(np.isfinite(R.tri_d2_f32(P.astype(np.float32), t, slice(len(f2) - 2, len(f2)))))


def test_grid_dims_are_numpys():
    for vs in (0.05, 0.025):
        sc = synthetic.Scene(vsize=vs)
        origin, dims = volumes.grid(sc.verts, vs)
        assert dims == sc.volume.shape[:3]
        assert origin.dtype == np.float64
        assert np.array_equal(origin, sc.verts.astype(np.float64).min(0) - 0.05)
    # bounds where (hi + vsize - lo) / vsize lands within 1e-12 of an integer
    vs = 0.025
    hits = 0
    for n in range(3, 60):
        for lo in (-0.3, 0.1, 0.123):
            hi = lo + 0.1 + n * vs  # extent after the padding: (n + 4) voxels, nearly
            xyz = np.array([[lo, lo, lo], [hi, hi, hi]])
            o, dims = volumes.grid(xyz, vs)
            q = ((hi + 0.05) + vs - (lo - 0.05)) / vs
            hits += abs(q - round(q)) < 1e-12
            want = synthetic.blend_weight_volume(xyz, np.zeros((2, 24), np.float32), vs).shape[:3]
            assert dims == want
    assert hits > 20


def test_pruned_search_equals_exhaustive_in_float32():
    v, f = R.mesh_b()
    f = np.concatenate([f, f[:1], [[7, 7, 9]]]).astype(np.int32)  # a duplicate face and a zero-area one
    origin, dims = volumes.grid(v, 0.04)
    P = R.grid_points(origin, dims, 0.04).reshape(dims + (3,))
    glo, ghi = origin, origin + (np.array(dims) - 1) * 0.04
    rng = np.random.Generator(np.random.PCG64(2))
    visited = total = 0
    worst_err = worst_excess = 0.0
    for _ in range(12):
        b = [int(rng.integers(0, (d + 3) // 4)) * 4 for d in dims]
        p64 = P[b[0]:b[0] + 4, b[1]:b[1] + 4, b[2]:b[2] + 4].reshape(-1, 3)
        p = p64.astype(np.float32)
        d_ex, i_ex, n_ex = R.search_f32(p, v, f, False, glo, ghi)
        d_pr, i_pr, n_pr = R.search_f32(p, v, f, True, glo, ghi)
        assert np.array_equal(i_ex, i_pr)
        assert np.array_equal(d_ex, d_pr)
        assert not np.any(i_ex == len(f) - 2)  # the duplicate never wins
        visited += n_pr
        total += n_ex
        D = R.tri_distance_matrix(p64, v, f)
        worst_err = max(worst_err, np.abs(np.sqrt(d_ex.astype(np.float64)) - D[np.arange(len(p)), i_ex]).max())
        worst_excess = max(worst_excess, (D[np.arange(len(p)), i_ex] - D.min(axis=1)).max())
    print(f'cells visited {visited} of {total}; float32 distance error {worst_err:.3g} m, '
          f'selection excess {worst_excess:.3g} m')
    assert visited < total // 2  # the bound prunes (bricks of 16 cm on a 0.9 m mesh: no more is to be had)
    # the two figures the GPU test's delta = 1e-6 m has to cover
    assert worst_err <= 1e-6 and worst_excess <= 1e-6


def test_float32_search_figures_on_mesh_a():
    """The two figures DELTA = 1e-6 m of tests/test_gpu_bwvol.py has to cover, for the kernel's formula
    restated in float32 numpy (no fused multiply-adds), every voxel of mesh A's grids."""
    v, f = R.mesh_a()
    t = R.tri_records(v, f)
    for vs in (0.05, 0.04):
        origin, dims = volumes.grid(v, vs)
        P = R.grid_points(origin, dims, vs)
        d2 = R.tri_d2_f32(P.astype(np.float32), t, slice(0, len(f)))
        k = np.argmin(d2, axis=1)
        D = R.tri_distance_matrix(P, v, f)
        n = np.arange(len(P))
        err = np.abs(np.sqrt(d2[n, k].astype(np.float64)) - D[n, k]).max()
        excess = (D[n, k] - D.min(axis=1)).max()
        print(f'vsize {vs}: float32 distance error {err:.3g} m, selection excess {excess:.3g} m')
        assert err <= 2.5e-7 and excess <= 2.5e-7  # a quarter of DELTA
