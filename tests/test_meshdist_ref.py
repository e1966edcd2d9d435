"""CPU: the restatements the mesh-evaluator GPU tests stand on (tests/meshdist_ref.py), the .obj parser and
the PLY writer.

Figures measured here (printed by the tests below), PCG64(11) uniforms, PCG64(23) query sets:
  * sampling: the smallest distance of any u0 cum[-1] to an entry of cumsum(area), in units of
    tau = nf 2^-52 cum[-1]: A 2.9e7, B 3.0e4 (1,000 draws), the 70,312-face mesh 109 (1,000 draws),
    A_degenerate 6.2e7, the end-to-end pairs 1.5e4 (B, 11,000 draws) and 2.4e5 (B scaled). All far above the
    2 tau that two summation orders can differ by, so the GPU test demands exact face indices.
  * selection: the worst excess of the float32-selected face (bwvol_ref.tri_d2_f32 about the builder's
    centre) over the true minimum: A 4.1e-17 m, B 6.7e-18 m, A_degenerate 4.1e-17 m, zero_face 0, the
    70,312-face mesh 1.7e-18 m, B translated by (3, -2, 5) m 1.8e-8 m. DELTA = 1e-6 m keeps more than 50x.
"""
import numpy as np
import pytest

from animatable_nerf_amd import evaluator_mesh

from . import bwvol_ref as R
from . import meshdist_ref as M


def test_sampled_points_lie_on_their_face():
    for name in ('A', 'B', 'A_degenerate'):
        v, f = M.mesh(name)
        pts, k = M.sample_surface(v, f, M.uniforms(1000))
        assert k.min() >= 0 and k.max() < len(f)
        V = v.astype(np.float64)
        w, d = R.closest_bary(pts, V[f[k, 0]], V[f[k, 1]], V[f[k, 2]])
        print(f'{name}: worst distance of a sample to its own face {d.max():.3g} m')
        assert d.max() <= 1e-15  # a convex combination of the corners, rounded in float64 at ~0.5 m
        assert np.all(M.face_areas(v, f)[k] > 0.0)  # a zero-area face is never drawn


def test_sampling_is_area_weighted():
    v, f = M.mesh('A')
    area = M.face_areas(v, f)
    _, k = M.sample_surface(v, f, M.uniforms(10000))
    top = np.argsort(area)[-40:]
    got, want = np.isin(k, top).mean(), area[top].sum() / area.sum()
    assert abs(got - want) < 4 * np.sqrt(want * (1 - want) / 10000)


def sampling_pairs():
    """every (mesh, u0) pair the GPU tests sample with"""
    u = M.uniforms(2 * M.N_CHAMFER + M.N_P2S)
    yield 'A', u[:1000, 0]
    yield 'B', u[:1000, 0]
    yield 'big', u[:1000, 0]
    yield 'A_degenerate', u[:1000, 0]
    yield 'B', np.concatenate([u[:1000, 0], u[2000:, 0]])  # end to end: the source's Chamfer and P2S draws
    yield 'B_scaled', u[1000:2000, 0]                       # end to end: the target's


def test_no_draw_within_two_tau_of_a_cumulative_area():
    for name, u0 in sampling_pairs():
        m = M.cum_margin(*M.mesh(name), u0)
        print(f'{name}: {len(u0)} draws keep {m:.3g} tau')
        assert m > 2.0


def test_float32_selection_excess():
    for name in M.DIST_CASES:
        v, f = M.mesh(name)
        P = M.queries(name)
        d, _ = M.distance_reference(name)
        k = M.select_f32(P, v, f)
        excess = (M.face_distance(P, v, f, k) - d).max()
        print(f'{name}: {len(P)} queries, worst selection excess {excess:.3g} m')
        assert 3.0 * excess <= M.DELTA


def test_float64_distance_formulas_agree():
    """closest_bary (the finish kernel's formula) against _tri_dist2 (the matrix's) on every case's queries and
    winners: the largest difference, 1.42e-14 m (far points and the translated mesh), sets the GPU test's
    distance bound at 100x."""
    worst = 0.0
    for name in M.DIST_CASES:
        v, f = M.mesh(name)
        P = M.queries(name)
        d, k = M.distance_reference(name)
        V = v.astype(np.float64)
        _, db = R.closest_bary(P, V[f[k, 0]], V[f[k, 1]], V[f[k, 2]])
        worst = max(worst, np.abs(db - d).max())
    print(f'closest_bary against _tri_dist2: {worst:.17g} m')
    assert worst <= 1.4210854715202004e-14


def test_metrics_definition():
    src, tgt = M.mesh('A'), M.mesh('A')
    u = M.uniforms(2 * 50 + 70, seed=3)
    m = M.metrics(src, tgt, u, n_chamfer=50, n_p2s=70)
    assert m['chamfer'] == (m['src_tgt'] + m['tgt_src']) / 2
    assert max(m.values()) <= 1e-15  # a mesh against itself
    assert M.nan0_mean([1.0, np.nan, 3.0]) == 4.0 / 3.0


def test_draw_order_is_the_references():
    rng = np.random.Generator(np.random.PCG64(4))
    u = evaluator_mesh.draw_uniforms(rng)
    ref = np.random.Generator(np.random.PCG64(4))
    assert u.shape == (12000, 3)
    for lo, n in ((0, 1000), (1000, 1000), (2000, 10000)):
        assert np.array_equal(u[lo:lo + n, 0], ref.random(n))
        assert np.array_equal(u[lo:lo + n, 1:], ref.random((n, 2)))
    state = np.random.get_state()
    try:
        np.random.seed(9)
        a = evaluator_mesh.draw_uniforms()
        np.random.seed(9)
        assert np.array_equal(a[:1000, 0], np.random.random(1000))
    finally:
        np.random.set_state(state)


# ---- files -------------------------------------------------------------------------------------------------
def read_ply_ascii(path):
    with open(path) as f:
        lines = f.read().split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format ascii 1.0'
    nv = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith('element face')][0].split()[-1])
    body = lines[lines.index('end_header') + 1:]
    v = np.array([[float(x) for x in ln.split()] for ln in body[:nv]]).reshape(-1, 3)
    t = np.array([[int(x) for x in ln.split()] for ln in body[nv:nv + nf]]).reshape(-1, 4)
    assert np.all(t[:, 0] == 3)
    return v, t[:, 1:]


def test_obj_parser_and_ply_writer_round_trip(tmp_path):
    v, f = M.mesh('A')
    path = tmp_path / 'm.obj'
    with open(path, 'w') as o:
        o.write('# a comment\nmtllib none.mtl\n')
        for p in v:
            o.write(f'v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n')
        o.write('vn 0 0 1\nvt 0.5 0.5\n')
        for i, t in enumerate(f):
            a, b, c = (int(x) + 1 for x in t)
            if i % 3 == 0:
                o.write(f'f {a} {b} {c}\n')
            elif i % 3 == 1:
                o.write(f'f {a}/1/1 {b}//1 {c}/1\n')
            else:
                o.write(f'f {a - len(v) - 1} {b - len(v) - 1} {c - len(v) - 1}\n')  # relative indices
    gv, gf = evaluator_mesh.read_obj(path)
    assert gv.dtype == np.float64 and gf.dtype == np.int32
    assert np.array_equal(gv, v.astype(np.float64)) and np.array_equal(gf, f)
    ply = tmp_path / 'm.ply'
    evaluator_mesh.write_ply(ply, gv * (1.0 / 3.0), gf)
    pv, pf = read_ply_ascii(ply)
    assert np.array_equal(pv, gv * (1.0 / 3.0)) and np.array_equal(pf, f)  # repr round-trips a float64


def test_obj_parser_rejects_what_it_does_not_read(tmp_path):
    quad = tmp_path / 'q.obj'
    quad.write_text('v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n')
    with pytest.raises(ValueError, match='triangles'):
        evaluator_mesh.read_obj(quad)
    bad = tmp_path / 'b.obj'
    bad.write_text('v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1 2 7\n')
    with pytest.raises(ValueError, match='outside'):
        evaluator_mesh.read_obj(bad)
