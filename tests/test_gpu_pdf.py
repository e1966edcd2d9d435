"""GPU: the aligned_aninerf_pdf render (renderer_pdf.Renderer / anr_pdf_render_fwd) against the reference's
fixtures G18 / G19 (tools/gen_golden_pdf.py) and the restatement tests/pdf_ref.py (pinned to them on the CPU by
tests/test_pdf_ref.py). Keep mask and tbounds are compared bit for bit, values within 1e-4 (the project's fp32
tolerance, tests/test_gpu_sdf.py TOL), in the three render precisions: exact fp32 layer GEMMs, and the fused
programs in bf16x3 and bf16x6."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pdf_ref
from tests._common import golden

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ('fp32', 'bf16x3', 'bf16x6')
MAPS = ('raw', 'rgb_map', 'acc_map', 'depth_map')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def _renderer(P, dev, prec='fp32', mmsk=False, **cfg_kw):
    from animatable_nerf_amd import renderer_pdf, renderer_pdf_mmsk
    cfg = pdf_ref.pdf_cfg(render_precision=prec, **cfg_kw)
    net = pdf_ref.make_net(P, dev, cfg)
    net.train()  # run.py evaluates in train() mode with perturb = 0
    return (renderer_pdf_mmsk if mmsk else renderer_pdf).Renderer(net, cfg)


def _clone(batch, dev=None):
    return {k: (v.clone() if dev is None else v.to(dev).clone()) for k, v in batch.items()}


def _close(a, b, tol, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a.astype(np.float64) - b).max()) if a.size else 0.0
    print(f'{what}: max |err| {err:.3e}')
    assert err <= tol, (what, err)


@pytest.fixture(scope='module')
def g18():
    g = golden('g18_pdf_tiny')
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    pn = g['pnorm'][0, :, 0]
    keep = pn < pdf_ref.NORM_TH
    keep[int(pn.argmin())] = True
    return g, batch, P, keep


@pytest.fixture(scope='module')
def g19():
    g = golden('g19_pdf_chunks')
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    batch['tbounds'] = torch.from_numpy(g['tbounds_before'].copy())
    return g, batch, P


@pytest.mark.parametrize('prec', PRECISIONS)
def test_g18_matches_reference(dev, g18, prec):
    g, batch, P, keep = g18
    r = _renderer(P, dev, prec)
    b = _clone(batch)
    ret = r.render_device(b)
    kept = r.kept_ids().cpu().numpy()
    assert np.array_equal(kept, np.nonzero(keep)[0])                      # kept ids, bit for bit
    assert np.array_equal(b['tbounds'].numpy(), g['tbounds_after'])       # tbounds, bit for bit
    assert np.array_equal(r.last_row_ids.cpu().numpy(), kept)
    # the front-end's KNN records against the reference's blend: weights x skin rows = pbw, and the weighted
    # distance pnorm from the recorded indices
    rec = r.knn_records().cpu().numpy()
    w = rec[:, :5].copy().view(np.float32)
    u = rec[:, 5:].copy().view(np.uint32)
    idx = np.stack([u[:, 0] & 0xffff, u[:, 0] >> 16, u[:, 1] & 0xffff, u[:, 1] >> 16, u[:, 2]], 1).astype(np.int64)
    skin = batch['weights'][0].numpy()
    pbw = np.einsum('nkl,nk->nl', skin[idx[kept]], w[kept])
    _close(pbw, g['pbw'][0], 1e-6, 'pbw from the KNN records')
    pts, _ = pdf_ref.restate.sample_points(batch['ray_o'], batch['ray_d'], batch['near'], batch['far'])
    pose = pdf_ref.restate.world_to_pose(pts.view(1, -1, 3), batch['R'], batch['Th'])[0].numpy()
    d = np.linalg.norm(pose[:, None] - batch['pvertices'][0].numpy()[idx], axis=2)
    _close((d * w).sum(1), g['pnorm'][0, :, 0], 1e-6, 'pnorm from the KNN records')
    # values
    big, tpose, tdirs = r.warped(kept.shape[0])
    _close(big, g['init_bigpose'][0], TOL, 'init_bigpose')
    _close(tpose, g['tpose'][0], TOL, 'tpose')
    _close(tdirs, g['tpose_dirs'][0], TOL, 'tpose_dirs')
    assert r.last_counts == (int(keep.sum()),)
    _close(ret['resd'], g['resd'], TOL, 'resd rows')
    for k in MAPS + ('resd',):
        _close(ret[k], g['out_' + k], TOL, k)


@pytest.mark.parametrize('prec', PRECISIONS)
def test_g19_chunks_match_reference(dev, g19, prec):
    """4,136 rays in chunks of 2048 / 2048 / 40: forced argmin in the last chunk, per-chunk tbounds widening. A
    kept sample whose box decision differs from the reference's must be one the float64 restatement puts within
    pdf_ref.EDGE_MARGIN of a box face (G19 edge_pid); at most 0.1 % of the kept samples may be exempt so."""
    g, batch, P = g19
    r = _renderer(P, dev, prec)
    b = _clone(batch)
    ret = r.render_device(b)
    R = batch['ray_o'].shape[1]
    keep = np.unpackbits(g['keep_bits'])[:R * 64].astype(bool)
    kept = r.kept_ids().cpu().numpy()
    assert np.array_equal(kept, np.nonzero(keep)[0])
    assert np.array_equal(b['tbounds'].numpy(), g['tbounds_after'])
    assert ret['resd'].shape == (1, kept.shape[0], 3)
    ref_out = np.unpackbits(g['outside_bits'])[:kept.shape[0]].astype(bool)
    raw_k = ret['raw'][0, torch.from_numpy(kept).to(dev)].cpu().numpy()
    out = (raw_k == 0).all(axis=1)  # rgb is a sigmoid: a kept sample inside the box never has an all-zero raw
    differ = kept[out != ref_out]
    print(f'{prec}: {kept.shape[0]} kept, {differ.shape[0]} box decisions differ')
    assert np.isin(differ, g['edge_pid']).all(), differ
    assert differ.shape[0] <= 0.001 * kept.shape[0]
    ok = ~np.isin(kept, differ)
    ev = np.arange(0, kept.shape[0], 2)  # G19 stores every second kept sample's alpha
    _close(raw_k[ev][ok[ev], 3], g['kept_alpha_even'][ok[ev]], TOL, 'kept alpha')
    bad = np.unique(differ // 64)   # rays holding an excluded sample
    sel = np.setdiff1d(np.arange(R), bad)
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        _close(ret[k][0, torch.from_numpy(sel).to(dev)], g['out_' + k][0, sel], TOL, k)
    # sampled rows (compact, kept order)
    rows = g['row_sample_idx']
    assert np.array_equal(kept[rows], g['row_sample_pid'])
    _close(ret['resd'][0, torch.from_numpy(rows).to(dev)], g['resd_sample'], TOL, 'resd rows (sampled)')
    oks = ok[rows] & ~ref_out[rows]
    _close(raw_k[rows][oks, :3], g['rgb_sample'][oks], TOL, 'rgb (sampled, inside the box)')


def test_stratified_z(dev, g19):
    """A given t_rand, 300 rays in one chunk plus a 7-ray second chunk, against the float32 restatement."""
    g, _, _ = g19
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=3, rays=slice(100, 407))
    t_rand = torch.rand((307, 64), generator=torch.Generator().manual_seed(5))
    trace = {}
    ref = pdf_ref.render(P, _clone(batch), t_rand=t_rand, chunk=300, trace=trace)
    r = _renderer(P, dev, 'fp32', chunk=300)
    b = _clone(batch)
    ret = r.render_device(b, t_rand=t_rand)
    keep = torch.cat([c['pind'][0] for c in trace['chunks']]).numpy()
    assert len(trace['chunks']) == 2 and trace['chunks'][1]['pind'].shape[1] == 7 * 64
    assert np.array_equal(r.kept_ids().cpu().numpy(), np.nonzero(keep)[0])  # keep mask exact
    assert np.array_equal(b['tbounds'].numpy(), trace['chunks'][1]['tbounds'].numpy().reshape(b['tbounds'].shape[1:])[None])
    for k in MAPS + ('resd',):
        _close(ret[k], ref[k], TOL, k)


@pytest.mark.parametrize('prec', PRECISIONS)
def test_image_only_equals_full_bit_for_bit(dev, g18, prec):
    _, batch, P, _ = g18
    r = _renderer(P, dev, prec)
    b_full, b_img = _clone(batch), _clone(batch)
    full = r.render_device(b_full)
    assert 'resd' in full
    img = _renderer(P, dev, prec).render_device(b_img, image_only=True)
    assert sorted(img) == sorted(MAPS)
    for k in MAPS:
        assert torch.equal(img[k], full[k]), k
    assert torch.equal(b_img['tbounds'], b_full['tbounds'])
    # cfg.render_image_only routes Renderer.render there
    with torch.no_grad():  # run.py renders under no_grad
        out = _renderer(P, dev, prec, render_image_only=True).render(_clone(batch))
    assert sorted(out) == sorted(MAPS) and torch.equal(out['raw'], full['raw'].cpu())


@pytest.mark.parametrize('prec', PRECISIONS)
def test_two_calls_are_bit_identical(dev, g18, prec):
    _, batch, P, _ = g18
    r = _renderer(P, dev, prec)
    a = {k: v.clone() for k, v in r.render_device(_clone(batch)).items()}
    b = r.render_device(_clone(batch))
    assert sorted(a) == sorted(MAPS + ('resd',))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_split_precisions_are_fp32_level(dev, g18):
    """On G18's rays, against a float64 evaluation of the same network (pdf_ref on the GPU with PyTorch): every output
    of the bf16x6 render is within 1.5x (the factor of test_sdf_split_precisions_are_fp32_level) the exact fp32
    render's own error. The keep mask agrees across the three precisions."""
    _, batch, P, keep = g18
    P64, b64 = pdf_ref.to_dtype({k: v.to(dev) for k, v in P.items()}, {k: v.to(dev) for k, v in batch.items()},
                                torch.float64)
    r64 = pdf_ref.render(P64, b64)
    keys = MAPS + ('resd',)
    err = {}
    for prec in PRECISIONS:
        r = _renderer(P, dev, prec)
        ret = r.render_device(_clone(batch))
        assert np.array_equal(r.kept_ids().cpu().numpy(), np.nonzero(keep)[0])
        err[prec] = {k: float((ret[k].double() - r64[k]).abs().max()) for k in keys}
        print(prec, err[prec])
    for k in keys:
        assert err['bf16x6'][k] <= 1.5 * err['fp32'][k], (k, err['bf16x6'][k], err['fp32'][k])


def test_batches_of_256_are_bit_identical_to_one_batch(dev, g18, tmp_path):
    """G18 with the test-only capacity ANR_PDF_BATCH = 256 in a fresh child process (tests/_pdf_child.py): several
    batches with a partial last one. raw, the maps and the compact resd rows (kept order across the batch
    boundaries) equal this process's single-batch result bit for bit, in each precision."""
    _, batch, P, keep = g18
    n = int(keep.sum())
    assert n > 2 * 256 and n % 256 != 0, n  # at least three batches, the last one partial
    out = tmp_path / 'child.npz'
    env = dict(os.environ, ANR_PDF_BATCH='256')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, '-m', 'tests._pdf_child', str(out)], cwd=root, env=env, capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    child = np.load(out)
    for prec in PRECISIONS:
        r = _renderer(P, dev, prec)
        ret = r.render_device(_clone(batch))
        assert np.array_equal(child[prec + '_ids'], r.last_row_ids.cpu().numpy())
        for k in MAPS + ('resd',):
            assert np.array_equal(child[prec + '_' + k], ret[k].cpu().numpy()), (prec, k)


MMSK_CHUNK = 512


def _mmsk_batch():
    """The batch recipe of tests/test_gpu_sdf_mmsk.py: 3 chunks of box rays, then a partial chunk of rays along the
    box's top-back edge whose samples all project outside a training view's mask (a chunk without a network call)."""
    from animatable_nerf_amd import synthetic
    from tests._common import pdf_batch_np, pdf_scene
    sc = pdf_scene()
    ro, rd = sc.box_rays(3 * MMSK_CHUNK, seed=41)
    rng = np.random.Generator(np.random.PCG64(3))
    b = sc.pbounds.astype(np.float64)
    o2 = np.stack([np.full(200, b[0, 0] - 0.5), b[1, 1] - rng.uniform(0.001, 0.01, 200),
                   b[0, 2] + rng.uniform(0.001, 0.01, 200)], 1)
    d2 = np.broadcast_to(np.array([1.0, 0.0, 0.0]), (200, 3))
    ro = np.concatenate([ro, o2.astype(np.float32)])
    rd = np.concatenate([rd, d2.astype(np.float32)])
    bb, mask = pdf_batch_np(sc, ro, rd)
    Ks, RTs, msks, H, W = synthetic.training_views(sc.pvertices, n_views=3, dilate=0)
    bb.update(Ks=Ks[None], RT=RTs[None], msks=msks[None], H=np.array([H]), W=np.array([W]))
    return bb, int(mask[3 * MMSK_CHUNK:].sum())


@pytest.mark.parametrize('prec', PRECISIONS)
def test_mmsk_visibility_filter(dev, g18, prec):
    """renderer_pdf_mmsk against oracle.restate.render_mmsk around pdf_ref's network: maps within 1e-4, and
    batch['tbounds'] widened exactly three times (the chunk with no visible sample makes no network call)."""
    from oracle import restate
    from tests._common import to_torch
    _, _, P, _ = g18
    b, n_corner = _mmsk_batch()
    R = b['ray_o'].shape[1]
    assert R > 3 * MMSK_CHUNK and n_corner > 0
    bt = to_torch(b, dev)  # before the oracle call: bc shares b's arrays and is widened in place
    bc = to_torch(b)
    tb0 = bc['tbounds'].clone()
    calls = []

    def net_fwd(P_, wpts, viewdir, dists, batch):
        calls.append(len(wpts))
        return pdf_ref.network_forward(P_, wpts, viewdir, dists, batch)
    with torch.no_grad():
        ref = restate.render_mmsk(P, bc, chunk=MMSK_CHUNK, net_forward=net_fwd)
    assert len(calls) == 3
    out = _renderer(P, dev, prec, mmsk=True, chunk=MMSK_CHUNK).render(bt)
    assert set(out) == {'rgb_map', 'acc_map', 'depth_map'}
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        _close(out[k], ref[k], TOL, k)
    want = tb0.clone()
    for _ in range(3):  # widened exactly three times, in fp32 as the reference does
        want[0, 0] -= 0.05
        want[0, 1] += 0.05
    assert torch.equal(bc['tbounds'], want)
    assert torch.equal(bt['tbounds'].cpu(), want)


# ---- get_alpha / mesh ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g20(g18):
    g = golden('g20_pdf_alpha')
    _, batch, P, _ = g18
    keep = np.unpackbits(g['keep_bits'])[:g['pts'].shape[0]].astype(bool)
    return g, batch, P, keep


@pytest.mark.parametrize('prec', PRECISIONS)
def test_g20_get_alpha_matches_reference(dev, g20, prec):
    """Network.get_alpha over G20's grid points in one call: within 1e-4 of the reference, the keep mask exact
    (exactly 0 where the reference dropped a point, and no kept point dropped: every kept alpha of G20 is non-zero)."""
    g, batch, P, keep = g20
    net = pdf_ref.make_net(P, dev, pdf_ref.pdf_cfg(render_precision=prec))
    alpha = net.get_alpha(torch.from_numpy(g['pts']), batch).cpu().numpy()
    assert alpha.shape == g['alpha'].shape
    assert (g['alpha'][keep] != 0).all() and int(keep.sum()) == int(g['n_kept'])
    assert (alpha[~keep] == 0).all() and (alpha[keep] != 0).all()
    _close(alpha, g['alpha'], TOL, 'alpha')


@pytest.mark.parametrize('prec', PRECISIONS)
def test_alpha_points_in_three_chunks(dev, g20, prec):
    """2,500 points in chunks of 1,024: three network calls, the last partial, each with its own forced argmin,
    against the restatement's batchify."""
    g, batch, P, _ = g20
    pts = torch.from_numpy(g['pts'][::-1][:2500].copy())  # the grid's far end first: chunks with few kept points
    trace = {}
    ref = pdf_ref.alpha_points(P, pts, batch, 1024, trace=trace)
    keep = torch.cat(trace['keep']).numpy()
    assert len(trace['keep']) == 3 and trace['keep'][2].shape[0] == 2500 - 2048
    r = _renderer(P, dev, prec)
    alpha = r.alpha_points(pts, batch, chunk_pts=1024).cpu().numpy()
    assert (alpha[~keep] == 0).all() and (alpha[keep] != 0).all()
    _close(alpha, ref, TOL, 'alpha')


def test_mesh_renderer_counts_match_marching_cubes_over_the_restatement(dev, g20):
    """renderer_pdf_mesh.Renderer.render on G20's coarse grid: the vertex / triangle counts of marching cubes over
    pdf_ref's cube (renderer_mesh.marching_cubes on the restatement's alpha volume)."""
    from animatable_nerf_amd import renderer_mesh, renderer_pdf_mesh
    from tests._common import pdf_scene
    g, batch, P, _ = g20
    voxel = float(g['voxel'])
    sc = pdf_scene()
    grid = renderer_mesh.grid_points(sc.pbounds, [voxel] * 3)
    assert np.array_equal(grid.reshape(-1, 3), g['pts'])
    mb = dict(batch, pts=torch.from_numpy(grid)[None], inside=torch.ones(grid.shape[:3], dtype=torch.bool)[None],
              wbounds=torch.from_numpy(sc.pbounds)[None])
    iso = 0.2
    cfg = pdf_ref.pdf_cfg(mesh_th=iso, voxel_size=[voxel] * 3)
    net = pdf_ref.make_net(P, dev, cfg)
    out = renderer_pdf_mesh.Renderer(net, cfg).render(mb)
    cube = pdf_ref.alpha_points(P, torch.from_numpy(g['pts']), batch, renderer_mesh.MESH_CHUNK).view(grid.shape[:3])
    # the device's alpha is within TOL of the restatement's (the tests above): with no grid value within TOL of the
    # iso level every corner falls on the same side in both cubes, so both have the same crossing edges and cases
    assert float((cube - iso).abs().min()) > TOL
    v, t = renderer_mesh.marching_cubes(cube.to(dev), iso)
    assert v.shape[0] > 100 and t.shape[0] > 100
    assert out['vertex'].shape == (v.shape[0], 3) and out['triangle'].shape == (t.shape[0], 3)
    assert out['posed_vertex'] is out['vertex'] or np.array_equal(out['posed_vertex'], out['vertex'])
