"""GPU: the aligned_aninerf_lbw render (renderer_lbw.Renderer / anr_lbw_render_fwd) against the reference's
fixtures G16 / G17 (tools/gen_golden_lbw.py) and the restatement tests/lbw_ref.py (pinned to them on the CPU by
tests/test_lbw_ref.py). Keep mask, tbounds and the alpha_ind decisions are compared bit for bit, values within 1e-4
(the project's fp32 tolerance, tests/test_gpu_sdf.py TOL), in the three render precisions: exact fp32 layer GEMMs,
and the fused programs in bf16x3 and bf16x6."""
import numpy as np
import pytest
import torch

from tests import lbw_ref
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


def _renderer(P, dev, prec='fp32', **cfg_kw):
    from animatable_nerf_amd.renderer_lbw import Renderer
    cfg = lbw_ref.lbw_cfg(render_precision=prec, **cfg_kw)
    net = lbw_ref.make_net(P, dev, cfg)
    net.train()  # run.py evaluates in train() mode with perturb = 0
    return Renderer(net, cfg)


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
def g16():
    g = golden('g16_lbw_tiny')
    batch, P = lbw_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    pn = g['pnorm'][0, :, 0]
    keep = pn < lbw_ref.NORM_TH
    keep[int(pn.argmin())] = True
    return g, batch, P, keep


@pytest.fixture(scope='module')
def g17():
    g = golden('g17_lbw_chunks')
    batch, P = lbw_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    batch['tbounds'] = torch.from_numpy(g['tbounds_before'].copy())
    return g, batch, P


@pytest.mark.parametrize('prec', PRECISIONS)
def test_g16_matches_reference(dev, g16, prec):
    g, batch, P, keep = g16
    r = _renderer(P, dev, prec)
    b = _clone(batch)
    ret = r.render_device(b)
    kept = r.kept_ids().cpu().numpy()
    assert np.array_equal(kept, np.nonzero(keep)[0])                      # keep mask, bit for bit
    assert np.array_equal(b['tbounds'].numpy(), g['tbounds_after'])       # tbounds, bit for bit
    # the front-end's KNN records against the reference's blend: weights x skin rows = init_pbw, and the weighted
    # distance pnorm from the recorded indices
    rec = r.knn_records().cpu().numpy()
    w = rec[:, :5].copy().view(np.float32)
    u = rec[:, 5:].copy().view(np.uint32)
    idx = np.stack([u[:, 0] & 0xffff, u[:, 0] >> 16, u[:, 1] & 0xffff, u[:, 1] >> 16, u[:, 2]], 1).astype(np.int64)
    skin = batch['weights'][0].numpy()
    init = np.einsum('nkl,nk->nl', skin[idx[kept]], w[kept])
    _close(init, g['init_pbw'][0], 1e-6, 'init_pbw from the KNN records')
    pts, _ = lbw_ref.restate.sample_points(batch['ray_o'], batch['ray_d'], batch['near'], batch['far'])
    pose = lbw_ref.restate.world_to_pose(pts.view(1, -1, 3), batch['R'], batch['Th'])[0].numpy()
    d = np.linalg.norm(pose[:, None] - batch['pvertices'][0].numpy()[idx], axis=2)
    _close((d * w).sum(1), g['pnorm'][0, :, 0], 1e-6, 'pnorm from the KNN records')
    # values
    tpose, tdirs = r.warped(kept.shape[0])
    _close(tpose, g['tpose'], TOL, 'tpose')
    _close(tdirs, g['tpose_dirs'], TOL, 'tpose_dirs')
    assert r.last_counts == (int(keep.sum()), g['out_pbw'].shape[1])
    for k in MAPS + ('pbw', 'tbw'):
        _close(ret[k], g['out_' + k], TOL, k)
    ai = np.isin(kept, r.last_row_ids.cpu().numpy())
    _close(ret['pbw'][0], g['pbw'][0].T[ai], TOL, 'pbw rows by sample id')
    _close(ret['tbw'][0], g['tbw'][0].T[ai], TOL, 'tbw rows by sample id')


@pytest.mark.parametrize('prec', PRECISIONS)
def test_g17_chunks_match_reference(dev, g17, prec):
    """4,136 rays in chunks of 2048 / 2048 / 40: forced argmin in the last chunk, per-chunk tbounds widening.
    alpha_ind decisions equal the reference's bit for bit, except that a sample decided differently must be one
    the float64 restatement puts within lbw_ref.EDGE_MARGIN of the decision (G17 edge_pid), and at most 0.1 % of
    the rows may differ so."""
    g, batch, P = g17
    r = _renderer(P, dev, prec)
    b = _clone(batch)
    ret = r.render_device(b)
    R = batch['ray_o'].shape[1]
    keep = np.unpackbits(g['keep_bits'])[:R * 64].astype(bool)
    kept = r.kept_ids().cpu().numpy()
    assert np.array_equal(kept, np.nonzero(keep)[0])
    assert np.array_equal(b['tbounds'].numpy(), g['tbounds_after'])
    ref_ai = np.unpackbits(g['bw_row_bits'])[:kept.shape[0]].astype(bool)
    ids = r.last_row_ids.cpu().numpy().astype(np.int64)
    ai = np.isin(kept, ids)
    differ = kept[ai != ref_ai]
    print(f'{prec}: {ids.shape[0]} rows, {differ.shape[0]} decided differently')
    assert np.isin(differ, g['edge_pid']).all(), differ
    assert differ.shape[0] <= 0.001 * int(g['bw_rows'])
    assert ids.shape[0] - int(ai[~ref_ai].sum()) + int(ref_ai[~ai].sum()) == int(g['bw_rows'])
    if differ.shape[0] == 0:
        assert r.last_counts[1] == int(g['bw_rows'])
    ok = ~np.isin(kept, differ)
    _close(ret['raw'][0, torch.from_numpy(kept[ok]).to(dev), 3], g['kept_alpha'][ok], TOL, 'kept alpha')
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        bad = np.unique(differ // 64)   # rays holding an excluded sample
        sel = np.setdiff1d(np.arange(R), bad)
        _close(ret[k][0, torch.from_numpy(sel).to(dev)], g['out_' + k][0, sel], TOL, k)
    # sampled rows, matched by sample id
    pos = {int(p): i for i, p in enumerate(ids)}
    n_matched = 0
    for j, pid in enumerate(g['bw_sample_pid']):
        if int(pid) in pos:
            i = pos[int(pid)]
            assert float((ret['pbw'][0, i].cpu() - torch.from_numpy(g['pbw_sample'][j])).abs().max()) <= TOL, pid
            assert float((ret['tbw'][0, i].cpu() - torch.from_numpy(g['tbw_sample'][j])).abs().max()) <= TOL, pid
            n_matched += 1
        else:
            assert pid in differ, pid
    assert n_matched >= g['bw_sample_pid'].shape[0] - differ.shape[0]


def test_stratified_z(dev, g17):
    """A given t_rand, 300 rays in one chunk plus a 7-ray second chunk, against the float32 restatement."""
    g, _, _ = g17
    batch, P = lbw_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=3, rays=slice(100, 407))
    t_rand = torch.rand((307, 64), generator=torch.Generator().manual_seed(5))
    trace = {}
    ref = lbw_ref.render(P, _clone(batch), t_rand=t_rand, chunk=300, trace=trace)
    r = _renderer(P, dev, 'fp32', chunk=300)
    b = _clone(batch)
    ret = r.render_device(b, t_rand=t_rand)
    keep = torch.cat([c['pind'][0] for c in trace['chunks']]).numpy()
    assert len(trace['chunks']) == 2 and trace['chunks'][1]['pind'].shape[1] == 7 * 64
    assert np.array_equal(r.kept_ids().cpu().numpy(), np.nonzero(keep)[0])
    assert np.array_equal(b['tbounds'].numpy(), trace['chunks'][1]['tbounds'].numpy().reshape(b['tbounds'].shape[1:])[None])
    for k in MAPS + ('pbw', 'tbw'):
        _close(ret[k], ref[k], TOL, k)


@pytest.mark.parametrize('prec', PRECISIONS)
def test_image_only_equals_full_bit_for_bit(dev, g16, prec):
    _, batch, P, _ = g16
    r = _renderer(P, dev, prec)
    b_full, b_img = _clone(batch), _clone(batch)
    full = r.render_device(b_full)
    img = _renderer(P, dev, prec).render_device(b_img, image_only=True)
    assert sorted(img) == sorted(MAPS)
    for k in MAPS:
        assert torch.equal(img[k], full[k]), k
    assert torch.equal(b_img['tbounds'], b_full['tbounds'])
    # cfg.render_image_only routes Renderer.render there
    with torch.no_grad():  # run.py renders under no_grad
        out = _renderer(P, dev, prec, render_image_only=True).render(_clone(batch))
    assert sorted(out) == sorted(MAPS) and torch.equal(out['raw'], full['raw'].cpu())


def test_split_precisions_are_fp32_level(dev, g16):
    """On G16's rays, against a float64 evaluation of the same network (lbw_ref on the GPU with PyTorch): every output
    of the bf16x6 render is within 1.5x (the factor of test_sdf_split_precisions_are_fp32_level) the exact fp32
    render's own error; bf16x3 stays within 1e-4. Keep mask and row set agree across the three."""
    _, batch, P, keep = g16
    P64, b64 = lbw_ref.to_dtype({k: v.to(dev) for k, v in P.items()}, {k: v.to(dev) for k, v in batch.items()},
                                torch.float64)
    r64 = lbw_ref.render(P64, b64)
    keys = MAPS + ('pbw', 'tbw')
    err = {}
    for prec in PRECISIONS:
        r = _renderer(P, dev, prec)
        ret = r.render_device(_clone(batch))
        assert np.array_equal(r.kept_ids().cpu().numpy(), np.nonzero(keep)[0])
        assert ret['pbw'].shape == r64['pbw'].shape
        err[prec] = {k: float((ret[k].double() - r64[k]).abs().max()) for k in keys}
        print(prec, err[prec])
    for k in keys:
        assert err['bf16x6'][k] <= 1.5 * err['fp32'][k], (k, err['bf16x6'][k], err['fp32'][k])
        assert err['bf16x3'][k] <= TOL, (k, err['bf16x3'][k])


def _subset_with_kept(per_ray, total):
    """Indices of rays whose kept counts (all > 0) sum to exactly ``total`` (subset sum by dynamic programming)."""
    reach = {0: []}
    for i, c in enumerate(per_ray):
        if c <= 0:
            continue
        for s, sel in list(reach.items()):
            if s + c <= total and s + c not in reach:
                reach[s + c] = sel + [i]
        if total in reach:
            return reach[total]
    raise AssertionError('no ray subset keeps exactly %d samples' % total)


@pytest.mark.parametrize('prec', PRECISIONS)
@pytest.mark.parametrize('case', ['one_ray', 'seventeen_rays', 'batch_plus_one'])
def test_edge_row_counts(dev, g16, case, prec, monkeypatch):
    """1 ray; 17 rays (one partial 128-sample tile of kept rows); kept samples = the per-batch capacity + 1 with the
    test-only capacity ANR_LBW_BATCH = 256 (two batches, the second of one row: the fused programs and the second
    search at a batch offset > 0), against the restatement, in each precision."""
    g, batch, P, keep = g16
    per_ray = keep.reshape(-1, 64).sum(1)
    if case == 'one_ray':
        sel = [int(np.argmax(per_ray > 0))]
    elif case == 'seventeen_rays':
        sel = list(range(17))
    else:
        sel = _subset_with_kept(per_ray, 257)
        monkeypatch.setenv('ANR_LBW_BATCH', '256')
    b = _clone(batch)
    for k in ('ray_o', 'ray_d', 'near', 'far', 'occupancy', 'mask_at_box', 'rgb'):
        b[k] = batch[k][:, sel].clone()
    trace = {}
    ref = lbw_ref.render(P, _clone(b), trace=trace)
    r = _renderer(P, dev, prec)
    ret = r.render_device(b)
    kref = np.nonzero(trace['chunks'][0]['pind'][0].numpy())[0]
    if case == 'batch_plus_one':
        assert kref.shape[0] == 257
    assert np.array_equal(r.kept_ids().cpu().numpy(), kref)
    assert r.last_counts == (kref.shape[0], ref['pbw'].shape[1])
    for k in MAPS + ('pbw', 'tbw'):
        _close(ret[k], ref[k], TOL, k)


def test_same_workspace_repeats_bit_for_bit(dev, g16, g17):
    """G16, then a larger frame, a smaller one, and G16 again on the same renderer / workspace: the last result
    equals the first bit for bit (nothing stale is read)."""
    _, batch, P, _ = g16
    _, big, _ = g17
    r = _renderer(P, dev, 'fp32')
    large = _clone(big)
    for k in ('ray_o', 'ray_d', 'near', 'far', 'occupancy', 'mask_at_box', 'rgb'):
        large[k] = big[k][:, :300].clone()
    r.render_device(_clone(large))  # sizes the workspace every later call reuses
    ws = r._ws
    first = r.render_device(_clone(batch))
    first = {k: v.clone() for k, v in first.items()}
    ids = r.last_row_ids.clone()
    r.render_device(large)
    small = _clone(batch)
    for k in ('ray_o', 'ray_d', 'near', 'far', 'occupancy', 'mask_at_box', 'rgb'):
        small[k] = batch[k][:, :5].clone()
    r.render_device(small)
    again = r.render_device(_clone(batch))
    assert r._ws is ws
    for k in first:
        assert torch.equal(first[k], again[k]), k
    assert torch.equal(ids, r.last_row_ids)
