"""GPU: the exact-fp32 MFMA stream of the fused kernels (k_mlp, k_alpha; anr_mlp_body.h mode 0).

The A fragments of every k-step are read one k-step ahead, across slice, layer and tile boundaries,
from the ring slot the slice stream certified. What that can break, and what is checked here:

* a workgroup's second tile starts from fragments prefetched during the first tile's last k-step
  (the wrap to program entry 0): a render in which every workgroup runs at least two tiles, against
  the CPU oracle, every output at the render parity tolerance (tests/test_gpu_render.py);
* a read from a ring slot that is not certified yet or is being refilled depends on timing: the
  same batch rendered three times must give the same bits;
* a last tile that is not full (n_kept % 128 != 0);
* k_alpha runs the same layer code on its own program: ~70 k mesh points against the oracle's
  get_alpha at the mesh test's tolerance, twice for equal bits.
"""
import numpy as np
import pytest
import torch

from oracle import restate

from ._common import batch_np, golden, make_net, oracle_params, scene, to_torch
from .test_gpu_render import TOL, _keep, _match_rows, _RowTrace

pytestmark = pytest.mark.gpu

KEYS = ('rgb_map', 'acc_map', 'depth_map', 'raw')
MULTI_RAYS = 4096  # ~97 k kept samples on the bench's scene: > 2 tiles for each of 256 workgroups
TAIL_RAYS = 300


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def renderer(dev):
    from animatable_nerf_amd import config
    from animatable_nerf_amd.renderer import Renderer
    net = make_net(dev)
    net.train()
    cfg = config.defaults()
    cfg.perturb = 0
    cfg.render_precision = 'fp32'
    return Renderer(net, cfg)


def _oracle_render(n_rays, seed):
    """the batch, the CPU oracle's outputs and its row trace (sample ids of the alpha_ind rows, sigma')"""
    torch.set_num_threads(16)
    sc = scene(0.025)  # the bench's scene
    ro, rd = sc.box_rays(n_rays, seed=seed)
    b, _ = batch_np(sc, ro, rd)
    bt = to_torch(b)
    fwd = restate.network_forward
    trace = _RowTrace(fwd, int(bt['ray_o'].shape[1]) * 64)
    restate.network_forward = trace
    try:
        with torch.no_grad():
            ref = restate.render(oracle_params(), bt)
    finally:
        restate.network_forward = fwd
    return b, ref, trace


@pytest.fixture(scope='module')
def multi():
    return _oracle_render(MULTI_RAYS, 31)


@pytest.fixture(scope='module')
def tail():
    return _oracle_render(TAIL_RAYS, 33)


def _check_against_oracle(renderer, dev, case):
    b, ref, trace = case
    ref_ids = trace.row_ids()
    bt = to_torch(b, dev)
    ret = renderer.render_device(bt)
    assert torch.equal(_keep(ret['raw']).cpu(), _keep(ref['raw']))
    for k in KEYS:
        err = (ret[k].cpu() - ref[k]).abs().max().item()
        print(k, err)
        assert err <= TOL, (k, err)
    ids = renderer.row_ids(int(bt['ray_o'].shape[1])).cpu()
    assert ids.numel() == ret['pbw'].shape[1] and ref_ids.numel() == ref['pbw'].shape[1]
    ia, ib, only = _match_rows(ids, ref_ids)
    # the row set is the oracle's; it may differ only where sigma' ties with train_th (tests/test_gpu_render.py)
    assert only.numel() <= max(8, ref_ids.numel() // 10000), only.numel()
    assert bool((trace.sig[only].abs() <= 1e-4).all()), (only, trace.sig[only])
    for k in ('pbw', 'tbw'):
        err = (ret[k][0].cpu()[ia] - ref[k][0][ib]).abs().max().item()
        print(k, err)
        assert err <= TOL, (k, err)
    return ret


def test_multi_tile_render_matches_oracle(renderer, dev, multi):
    ret = _check_against_oracle(renderer, dev, multi)
    n_kept, m = renderer.last_counts
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert n_kept > 2 * 128 * cus, (n_kept, cus)  # every workgroup wraps from its first tile to a second
    assert m == ret['pbw'].shape[1]


def test_render_is_repeatable(renderer, dev, multi):
    bt = to_torch(multi[0], dev)
    first = {k: v.clone() for k, v in renderer.render_device(bt).items()}
    for _ in range(2):
        again = renderer.render_device(bt)
        for k in first:
            assert torch.equal(first[k], again[k]), k


def test_tail_tile_render_matches_oracle(renderer, dev, tail):
    _check_against_oracle(renderer, dev, tail)
    n_kept, _ = renderer.last_counts
    assert n_kept % 128 != 0, n_kept  # the last tile is partly filled


def test_alpha_points_match_oracle_and_repeat(dev):
    """k_alpha on the 69,662 points of golden G10's chunked set (17 chunks of 4096 and one of 30)"""
    from animatable_nerf_amd import config, synthetic
    from animatable_nerf_amd.renderer_mesh import Renderer
    torch.set_num_threads(16)
    g = golden('g10_mesh')
    b = synthetic.mesh_scene(voxel=0.02)
    pts = torch.from_numpy(g['pts_b'])
    chunk = int(g['chunk_b'])
    assert pts.shape[0] > 65536
    keys = ('A', 'pbw', 'tbw', 'pbounds', 'wbounds', 'tbounds', 'R', 'Th', 'latent_index')
    with torch.no_grad():
        ref = restate.mesh_alpha(oracle_params(), pts, {k: torch.from_numpy(np.ascontiguousarray(b[k])) for k in keys},
                                 chunk=chunk)
    cfg = config.load_cfg(opts=['vis_posed_mesh', 'True', 'render_precision', 'fp32'])
    r = Renderer(make_net(dev), cfg)
    batch = to_torch(b, dev)
    a1 = r.alpha_points(pts.to(dev), batch, chunk_pts=chunk).clone()
    a2 = r.alpha_points(pts.to(dev), batch, chunk_pts=chunk)
    assert torch.equal(a1, a2)
    got = a1.cpu()
    assert torch.equal(got != 0, ref != 0)
    err = (got - ref).abs().max().item()
    print('alpha', err)
    assert err <= 1e-4, err
