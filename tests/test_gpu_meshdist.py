"""GPU: the device mesh evaluator (anr_mesh_sample, anr_mesh_point_dist, anr_mesh_metrics,
animatable_nerf_amd.evaluator_mesh) against the float64 restatements of tests/meshdist_ref.py.

Sampling: faces equal np.searchsorted(np.cumsum(area), u0 cum[-1]) exactly and points equal the restatement
bit for bit; tests/test_meshdist_ref.py shows that no draw of these (mesh, u) pairs lies within 2 tau of a
cumulative area, tau bounding what two summation orders differ by.

Distances, with D the float64 distances of bwvol_ref (its _tri_dist2) and k the returned face:
  D[i, k] <= min_j D[i, j] + DELTA, DELTA = 1e-6 m (the project's bar; the float32 selection measured on the
  CPU exceeds the minimum by at most 1.8e-8 m, on the mesh translated by (3, -2, 5) m);
  |dist - D[i, k]| <= DIST_TOL = 100 x 1.4210854715202004e-14 m: the largest difference between
  bwvol_ref.closest_bary (the finish kernel's formula) and _tri_dist2 on these cases, measured on the CPU
  (tests/test_meshdist_ref.py::test_float64_distance_formulas_agree; it comes from the points 40 m away
  and the translated mesh, where one ulp of a coordinate is 1.4e-14 m and 8.9e-16 m).
"""
import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib, config, evaluator_mesh

from . import meshdist_ref as M

pytestmark = pytest.mark.gpu

DELTA = M.DELTA
DIST_TOL = 100 * 1.4210854715202004e-14


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


# ---- 1: sampling --------------------------------------------------------------------------------------------
def check_sampling(dev, name, u):
    v, f = M.mesh(name)
    pts, face = evaluator_mesh.mesh_sample(v, f, u, device=dev)
    ref_p, ref_k = M.sample_surface(v, f, u)
    assert pts.dtype == torch.float64 and face.dtype == torch.int32 and pts.shape == (len(u), 3)
    assert np.array_equal(face.cpu().numpy(), ref_k)
    assert np.array_equal(bits(pts), bits(ref_p))
    return face.cpu().numpy()


@pytest.mark.parametrize('name', ['A', 'B', 'big'])
def test_sampling(dev, name):
    check_sampling(dev, name, M.uniforms(12000)[:1000])


@pytest.mark.parametrize('n', [1, 63, 65])
def test_sampling_small_counts(dev, n):
    check_sampling(dev, 'A', M.uniforms(12000)[:n])


def test_sampling_never_draws_a_zero_area_face(dev):
    k = check_sampling(dev, 'A_degenerate', M.uniforms(12000)[:1000])
    v, f = M.mesh('A_degenerate')
    assert np.all(M.face_areas(v, f)[k] > 0.0) and k.max() <= 352  # 353 and 354 are the zero-area faces
    # the first draws at the edges of the range: u0 = 0 takes the first face with area, u0 -> 1 the last
    u = np.array([[0.0, 0.25, 0.25], [1.0 - 2.0 ** -53, 0.9, 0.8]])
    check_sampling(dev, 'A_degenerate', u)


def test_sampling_reports_a_mesh_without_area(dev):
    v, f = M.mesh('zero_face')
    u = M.uniforms(12000)[:65]
    pts, face = evaluator_mesh.mesh_sample(v, f, u, device=dev, check=False)
    assert not pts.any() and bool((face == -1).all())  # nothing is drawn, no NaN
    with pytest.raises(ValueError, match='area'):
        evaluator_mesh.mesh_sample(v, f, u, device=dev)
    with pytest.raises(ValueError, match='no face'):
        evaluator_mesh.mesh_sample(v, np.zeros((0, 3), np.int32), u, device=dev)


# ---- 2: distances ---------------------------------------------------------------------------------------------
def check_distances(name, dist, face):
    v, f = M.mesh(name)
    P = M.queries(name)
    d_min, _ = M.distance_reference(name)
    k = face.cpu().numpy().astype(np.int64)
    assert k.shape == (len(P),) and k.min() >= 0 and k.max() < len(f)
    Dk = M.face_distance(P, v, f, k)
    excess = (Dk - d_min).max()
    derr = np.abs(dist.cpu().numpy() - Dk).max()
    print(f'{name}: {len(P)} queries, selection excess {excess:.3g} m, distance error {derr:.3g} m')
    assert excess <= DELTA
    assert derr <= DIST_TOL


@pytest.mark.parametrize('name', M.DIST_CASES)
def test_distances(dev, name):
    v, f = M.mesh(name)
    P = M.queries(name)
    assert len(P) % 64 != 0 or name == 'big'
    dist, face = evaluator_mesh.mesh_point_distance(v, f, P, device=dev)
    assert dist.dtype == torch.float64 and face.dtype == torch.int32
    assert bool(torch.isfinite(dist).all())
    check_distances(name, dist, face)
    if name == 'A_degenerate':
        assert not bool((face == 352).any())  # the copy of face 0 never wins: the lowest index does
    if name not in ('big',):
        rep = dist[-130:]  # one point 130 times: one answer
        assert bool((rep == rep[0]).all()) and bool((face[-130:] == face[-1]).all())


# ---- 3: search variants ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A_degenerate', 'B_shifted', 'big'])
def test_pruned_and_exhaustive_write_the_same_bits(dev, name):
    v, f = M.mesh(name)
    P = M.queries(name)
    outs = [evaluator_mesh.mesh_point_distance(v, f, P, exhaustive=e, device=dev)
            for e in (False, True, _lib.BWV_PRUNED, _lib.MESHDIST_PRUNED_CELLS)]
    for dist, face in outs[1:]:
        assert torch.equal(face, outs[0][1])
        assert torch.equal(dist.view(torch.int64), outs[0][0].view(torch.int64))


# ---- 4: query order -------------------------------------------------------------------------------------------
def test_shuffled_queries_give_the_same_bits(dev):
    v, f = M.mesh('B')
    P = M.queries('B')
    perm = np.random.Generator(np.random.PCG64(31)).permutation(len(P))
    d0, k0 = evaluator_mesh.mesh_point_distance(v, f, P, device=dev)
    d1, k1 = evaluator_mesh.mesh_point_distance(v, f, P[perm], device=dev)
    back = torch.from_numpy(np.argsort(perm)).to(dev)
    assert torch.equal(k1[back], k0)
    assert torch.equal(d1[back].view(torch.int64), d0.view(torch.int64))


# ---- 5: streams -------------------------------------------------------------------------------------------------
def test_two_streams_same_bits(dev):
    v, f = M.mesh('B')
    P = M.queries('B')
    u = M.uniforms(12000)[:1000]
    d0, k0, m0 = evaluator_mesh.mesh_point_distance(v, f, P, device=dev, return_mean=True)
    p0, f0 = evaluator_mesh.mesh_sample(v, f, u, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        d1, k1, m1 = evaluator_mesh.mesh_point_distance(v, f, P, device=dev, return_mean=True)
        p1, f1 = evaluator_mesh.mesh_sample(v, f, u, device=dev)
    side.synchronize()
    assert torch.equal(k0, k1) and torch.equal(f0, f1)
    for a, b in ((d0, d1), (m0, m1), (p0, p1)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---- 6: the NaN rule ------------------------------------------------------------------------------------------
def test_a_nan_query_counts_as_zero(dev):
    v, f = M.mesh('A')
    P = M.queries('A').copy()
    P[5] = v[17].astype(np.float64)  # exactly on a vertex: its distance is exactly 0
    d0, _, m0 = evaluator_mesh.mesh_point_distance(v, f, P, device=dev, return_mean=True)
    assert float(d0[5]) == 0.0
    P[5, 1] = np.nan
    d1, k1, m1 = evaluator_mesh.mesh_point_distance(v, f, P, device=dev, return_mean=True)
    assert bool(torch.isnan(d1[5])) and 0 <= int(k1[5]) < len(f)
    keep = torch.arange(len(P), device=dev) != 5
    assert torch.equal(d1[keep].view(torch.int64), d0[keep].view(torch.int64))
    assert torch.equal(m1.view(torch.int64), m0.view(torch.int64))
    want = M.nan0_mean(d1.cpu().numpy())
    assert abs(float(m1) - want) <= len(P) * 2.0 ** -52 * want


# ---- 7: end to end ------------------------------------------------------------------------------------------------
def test_evaluator_end_to_end(dev, tmp_path):
    src, tgt = M.mesh('B'), M.mesh('B_scaled')
    u = M.uniforms(2 * M.N_CHAMFER + M.N_P2S)
    ref = M.metrics(src, tgt, u)
    obj = tmp_path / 'data' / 'object'
    obj.mkdir(parents=True)
    with open(obj / '000007.obj', 'w') as o:
        for p in tgt[0]:
            o.write(f'v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n')
        for t in tgt[1]:
            o.write(f'f {t[0] + 1}/{t[0] + 1} {t[1] + 1}/{t[1] + 1} {t[2] + 1}/{t[2] + 1}\n')
    cfg = config.defaults()
    cfg.result_dir = str(tmp_path / 'result')
    cfg.test_dataset = config.CfgNode({'human': 'CoreView_313', 'data_root': str(tmp_path / 'data')})
    ev = evaluator_mesh.Evaluator()
    ev.cfg = cfg
    out_np = {'posed_vertex': src[0].astype(np.float64), 'triangle': src[1].astype(np.int64)}
    out_dev = {'posed_vertex': torch.from_numpy(src[0]).to(dev), 'triangle': torch.from_numpy(src[1]).to(dev)}
    # frame 1: numpy mesh, the target by its .obj path; frame 2: device tensors, the target given as tensors
    ev.evaluate(out_np, {'frame_index': torch.tensor([7])}, u=u)
    ev.evaluate(out_dev, {'frame_index': torch.tensor([8]), 'tgt_vertex': torch.from_numpy(tgt[0]).to(dev),
                          'tgt_triangle': tgt[1]}, u=u)
    rows = ev._table[:2].cpu().numpy()
    assert np.array_equal(bits(rows[0]), bits(rows[1]))  # the two ways to give a target agree bit for bit
    assert rows[0, _lib.MESHM_STATUS] == 0
    got = ev.summarize()
    for key, n in (('chamfer', M.N_CHAMFER), ('p2s', M.N_P2S)):
        err = abs(got[key][0] - ref[key])
        print(f'{key}: device {got[key][0]:.17g}, restatement {ref[key]:.17g}, difference {err:.3g}')
        assert err <= DELTA + n * 2.0 ** -52 * ref[key]
    for i, key in ((_lib.MESHM_SRC_TGT, 'src_tgt'), (_lib.MESHM_TGT_SRC, 'tgt_src')):
        assert abs(rows[0, i] - ref[key]) <= DELTA + M.N_CHAMFER * 2.0 ** -52 * ref[key]
    saved = np.load(tmp_path / 'result' / 'mesh_metrics.npy', allow_pickle=True).item()
    assert sorted(saved) == ['chamfer', 'p2s'] and len(saved['p2s']) == 2 and len(saved['chamfer']) == 2
    assert saved['chamfer'] == got['chamfer'] and saved['p2s'] == got['p2s']
    assert ev.p2ss == [] and ev.chamfers == [] and ev._n == 0


def test_evaluator_axis_swap_mesh_file_and_bad_mesh(dev, tmp_path, monkeypatch):
    src, tgt = M.mesh('A'), M.mesh('A')
    u = M.uniforms(2 * M.N_CHAMFER + M.N_P2S)
    cfg = config.defaults()
    cfg.result_dir = str(tmp_path / 'result')
    cfg.exp_name = 'meshdist_test'
    cfg.eval_write_meshes = True
    cfg.test_dataset = config.CfgNode({'human': 'rp_subject', 'data_root': str(tmp_path)})
    monkeypatch.chdir(tmp_path)
    ev = evaluator_mesh.Evaluator()
    ev.cfg = cfg
    # 'rp' in human (mesh_evaluator.py:22-27): (x, y, z) -> (x, z, -y); undo it on the way in
    v = src[0].astype(np.float64)
    pre = np.stack([v[:, 0], -v[:, 2], v[:, 1]], axis=1)
    batch = {'frame_index': torch.tensor([3]), 'tgt_vertex': tgt[0], 'tgt_triangle': tgt[1]}
    ev.evaluate({'posed_vertex': pre, 'triangle': src[1]}, batch, u=u)
    row = ev._table[0].cpu().numpy()
    assert row[_lib.MESHM_STATUS] == 0 and 0.0 <= row[_lib.MESHM_CHAMFER] <= 1e-7  # the mesh against itself
    lines = (tmp_path / 'data/animation/meshdist_test/posed_mesh/0003.ply').read_text().split('\n')
    assert lines[0] == 'ply' and f'element vertex {len(v)}' in lines and f'element face {len(src[1])}' in lines
    ev.summarize()
    cfg.eval_write_meshes = False
    ev.evaluate({'posed_vertex': src[0], 'triangle': np.zeros((0, 3), np.int64)}, batch, u=u)
    with pytest.raises(ValueError, match='extracted mesh has no face'):
        ev.summarize()
    assert ev._n == 0


# ---- 8: the device render path ------------------------------------------------------------------------------------
def test_render_device_equals_render(dev):
    from animatable_nerf_amd import synthetic
    from animatable_nerf_amd.renderer_sdf_mesh import Renderer

    from ._common import make_net_sdf
    net = make_net_sdf(dev)
    net.train()
    cfg = config.subject('anisdf_pdf_s9p', perturb=0)
    cfg.voxel_size = [0.02, 0.02, 0.02]
    b = synthetic.sdf_mesh_scene(voxel=0.02)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    r = Renderer(net, cfg)
    host = r.render(batch)
    on_dev = r.render_device(batch)
    assert sorted(on_dev) == sorted(host)
    for k in host:
        assert torch.is_tensor(on_dev[k]) and on_dev[k].is_cuda, k
        got = on_dev[k].cpu().numpy()
        assert got.dtype == host[k].dtype and np.array_equal(got, host[k]), k
    # and the loop render -> evaluate takes the tensors as they are
    ev = evaluator_mesh.Evaluator()
    ev.cfg = config.defaults()
    ev.evaluate(on_dev, {'frame_index': 0, 'tgt_vertex': on_dev['posed_vertex'], 'tgt_triangle': on_dev['triangle']},
                u=M.uniforms(2 * M.N_CHAMFER + M.N_P2S))
    row = ev._table[0].cpu().numpy()
    assert row[_lib.MESHM_STATUS] == 0 and 0.0 <= row[_lib.MESHM_P2S] <= 1e-6


# ---- 9: the ordering --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'big'])
def test_order_is_the_morton_order(dev, name):
    """anr_mesh_order: a permutation, sorted by (code, face); the codes are float32 on the device, so against
    the float64 restatement a centroid on a quantisation border may sit one step over: nearly every position
    agrees, and 'big' takes 69 waves and 18 blocks of the radix passes."""
    from . import bwvol_ref as R
    lib = _lib.load()
    v, f = M.mesh(name)
    dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    perm = torch.full((len(f),), -1, dtype=torch.int32, device=dev)
    nbytes = lib.anr_mesh_dist_workspace_bytes(len(f), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.anr_mesh_order(_lib.ptr(dv), len(v), _lib.ptr(df), len(f), _lib.ptr(perm), _lib.ptr(ws), nbytes,
                                  _lib.stream_ptr(dev)), 'anr_mesh_order')
    got = perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(got), np.arange(len(f)))
    used = v[f.reshape(-1)].astype(np.float64)
    want = R.morton_order(v, f, used.min(axis=0), used.max(axis=0))
    same = (got == want).mean()
    print(f'{name}: {same:.4f} of the positions equal the float64 Morton order')
    assert same > 0.9
