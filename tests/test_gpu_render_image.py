"""GPU: the image-only render (anr_render_image_fwd; k_mlp_img, k_mlp_img_b16, k_mlp_img_x6; anr_mlp_body.h
programs 9 / 19), the render program without its T-pose blend-weight pass.

The full program (anr_render_fwd) is pinned to the reference by tests/test_gpu_render.py and is the yardstick
here: every layer the image program keeps sees the operands it sees in the full program, in the same order, so
raw / rgb_map / acc_map / depth_map are expected to be equal bit for bit in the three render precisions.

Shapes (the bench's scene, tests/test_gpu_mlp_fp32_stream.py):
* 2 rays: one workgroup, one partly filled tile;
* 300 rays: a last tile that is not full;
* 4,096 rays: more than two tiles for every workgroup, so each wraps from program entry 18 to entry 0 of its next
  tile with fragments (fp32) / slices (all) prefetched across the wrap, which only this program's own tables
  describe.
The kept count is read through anr_render_counts here in the test; the renderer itself reads nothing back.
"""
import ctypes

import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib
from oracle import restate

from ._common import batch_np, golden, make_net, oracle_params, scene, to_torch
from .test_gpu_render import TOL, _keep

pytestmark = pytest.mark.gpu

KEYS = ('rgb_map', 'acc_map', 'depth_map', 'raw')
PRECISIONS = ('fp32', 'bf16x3', 'bf16x6')
SHAPES = {'one_tile': (2, 35), 'tail': (300, 33), 'multi': (4096, 31)}  # rays, seed
BAND = 4096


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def _renderer(dev, precision, cls=None, net=None, cfg=None, **keys):
    from animatable_nerf_amd import config
    from animatable_nerf_amd.renderer import Renderer
    if net is None:
        net = make_net(dev)
        net.train()  # run.py evaluates in train() mode with perturb = 0
    if cfg is None:
        cfg = config.defaults()
        cfg.perturb = 0
    cfg.render_precision = precision
    for k, v in keys.items():
        cfg[k] = v
    return (cls or Renderer)(net, cfg)


@pytest.fixture(scope='module')
def renderers(dev):
    return {p: _renderer(dev, p) for p in PRECISIONS}


@pytest.fixture(scope='module')
def batches():
    sc = scene(0.025)  # the bench's scene
    out = {}
    for name, (n, seed) in SHAPES.items():
        ro, rd = sc.box_rays(n, seed=seed)
        out[name], _ = batch_np(sc, ro, rd)
    return out


def _counts(r, ws, R):
    addr = r.lib.anr_render_counts(_lib.ptr(ws), R)
    off = addr - ws.data_ptr()
    c = ws[off:off + 8].view(torch.int32).cpu()
    return int(c[0]), int(c[1])


def _run(r, bt, image_only, **kw):
    """one device render -> (the four image outputs, (kept, rows) read from the workspace right after it)"""
    ret = r.render_device(bt, bw_rows=False, image_only=image_only, **kw)
    assert set(ret) == set(KEYS)
    return ret, _counts(r, r._ws, int(bt['ray_o'].shape[1]))


def _assert_equal_bits(a, b, what=''):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


@pytest.fixture(scope='module')
def pairs(dev, renderers, batches):
    """(shape, precision) -> (full outputs, image outputs, kept count), computed once and left unchanged"""
    cache = {}

    def get(shape, precision):
        if (shape, precision) not in cache:
            r = renderers[precision]
            bt = to_torch(batches[shape], dev)
            full, (kf, _) = _run(r, bt, False)
            img, (ki, mi) = _run(r, bt, True)
            assert r.last_counts is None
            assert ki == kf, (ki, kf)
            assert mi == 0, mi  # entry 1 of an image workspace's counts is written as 0
            cache[shape, precision] = (full, img, ki)
        return cache[shape, precision]
    return get


# ---- 1. bit comparison with the full program --------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_image_render_equals_full_render_bit_for_bit(dev, pairs, shape, precision):
    full, img, n_kept = pairs(shape, precision)
    print(shape, precision, 'n_kept', n_kept)
    if shape == 'one_tile':
        assert 0 < n_kept < 128, n_kept  # one workgroup, one partly filled tile
    elif shape == 'tail':
        assert n_kept % 128 != 0, n_kept
    else:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert n_kept > 2 * 128 * cus, (n_kept, cus)  # every workgroup wraps from entry 18 to entry 0
    assert int(_keep(img['raw']).sum().item()) == n_kept
    _assert_equal_bits(img, full, (shape, precision))


# ---- 2. independent of the full program -------------------------------------------------------------------
@pytest.fixture(scope='module')
def tail_oracle(batches):
    torch.set_num_threads(16)
    with torch.no_grad():
        return restate.render(oracle_params(), to_torch(batches['tail']))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_tail_case_matches_oracle(pairs, tail_oracle, precision):
    _, img, _ = pairs('tail', precision)
    assert torch.equal(_keep(img['raw']).cpu(), _keep(tail_oracle['raw']))
    for k in KEYS:
        err = (img[k].cpu() - tail_oracle[k]).abs().max().item()
        print(precision, k, err)
        assert err <= TOL, (k, err)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_goldens_g1_g2(dev, renderers, precision):
    r = renderers[precision]
    sc = scene(0.05)
    g = golden('g1_tiny')
    ro, rd = sc.box_rays(64, seed=2)
    b, _ = batch_np(sc, ro, rd)
    ret = {k: v.cpu() for k, v in r.render_device(to_torch(b, dev), image_only=True).items()}
    assert set(ret) == set(KEYS)
    assert torch.equal(_keep(ret['raw']), torch.from_numpy(g['out_raw'][0, :, :3].sum(-1) != 0))
    for k in KEYS:
        err = (ret[k] - torch.from_numpy(g['out_' + k])).abs().max().item()
        assert err <= TOL, (k, err)
    g = golden('g2_chunks')
    b, _ = batch_np(sc, g['ray_o'], g['ray_d'])
    ret = r.render_device(to_torch(b, dev), image_only=True)
    keep = _keep(ret['raw']).cpu().numpy()
    assert np.array_equal(np.packbits(keep), g['keep_bits'])
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        err = np.abs(ret[k].cpu().numpy() - g['out_' + k]).max()
        assert err <= TOL, (k, err)
    kept_alpha = ret['raw'][0, :, 3].cpu().numpy()[keep]
    assert np.abs(kept_alpha - g['kept_alpha']).max() <= TOL
    assert keep.reshape(-1, 64)[4096:].sum() == 1  # forced per-chunk argmin in the grazing chunk


# ---- 3. repeatability -------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_image_render_is_repeatable(dev, renderers, batches, pairs, precision):
    """a read from a ring slot that is not certified yet, or is being refilled, depends on timing"""
    _, first, _ = pairs('multi', precision)
    bt = to_torch(batches['multi'], dev)
    for i in range(3):
        again, _ = _run(renderers[precision], bt, True)
        _assert_equal_bits(again, first, (precision, i))


# ---- 4. the T-pose volume is not read ---------------------------------------------------------------------
def _direct_call(r, bt, drop_tbw=False, bands=False):
    """anr_render_image_fwd called directly, its workspace exactly anr_render_image_workspace_bytes.
    bands: the workspace and every output sit inside larger 0xA5-filled buffers, BAND bytes on either side.
    -> (outputs, [(buffer, payload bytes)])"""
    from animatable_nerf_amd.renderer import _Call
    p = r.params()
    dev = r.device()
    R = int(bt['ray_o'].shape[1])
    c = _Call(r, bt, None)
    c.opts.precision = c.render_precision
    if drop_tbw:
        c.frame.tbw = None
        for i in range(3):
            c.frame.tbw_dims[i] = 0
    ws_bytes = r.lib.anr_render_image_workspace_bytes(R, ctypes.byref(c.opts), ctypes.byref(c.frame))
    assert ws_bytes > 0
    pad = BAND if bands else 0
    sizes = {'ws': ws_bytes, 'rgb_map': R * 3 * 4, 'acc_map': R * 4, 'depth_map': R * 4, 'raw': R * 64 * 16}
    bufs = {k: torch.full((n + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    ptr = {k: ctypes.c_void_p(v.data_ptr() + pad) for k, v in bufs.items()}
    out = _lib.RenderOut(ptr['rgb_map'], ptr['acc_map'], ptr['depth_map'], ptr['raw'])
    _lib.check(r.lib.anr_render_image_fwd(ctypes.byref(p), ctypes.byref(c.frame), *c.ray_ptrs(), R,
                                          ctypes.byref(c.opts), ctypes.byref(out), ptr['ws'], ws_bytes,
                                          _lib.stream_ptr(dev)), 'anr_render_image_fwd')
    torch.cuda.synchronize(dev)
    shapes = {'rgb_map': (1, R, 3), 'acc_map': (1, R), 'depth_map': (1, R), 'raw': (1, R * 64, 4)}
    ret = {k: bufs[k][pad:pad + sizes[k]].view(torch.float32).reshape(shapes[k]) for k in KEYS}
    return ret, [(bufs[k], sizes[k]) for k in sizes]


@pytest.mark.parametrize('precision', PRECISIONS)
def test_tbw_volume_is_not_read(dev, renderers, batches, pairs, precision):
    _, img, _ = pairs('tail', precision)
    r = renderers[precision]
    b = dict(batches['tail'])
    b['tbw'] = np.full_like(b['tbw'], np.nan)
    poisoned, _ = _run(r, to_torch(b, dev), True)
    _assert_equal_bits(poisoned, img, 'tbw = NaN')
    absent, _ = _direct_call(r, to_torch(batches['tail'], dev), drop_tbw=True)
    _assert_equal_bits(absent, img, 'tbw NULL, dims 0')


# ---- 5. options, against the full program bit for bit -----------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_novel_pose(dev, precision):
    from ._common import make_net_novel, novel_batch_np, novel_cfg
    g = golden('g5_novel_pose')
    net = make_net_novel(dev)
    net.train()
    r = _renderer(dev, precision, net=net, cfg=novel_cfg())
    bt = to_torch(novel_batch_np(), dev)
    full, (kf, _) = _run(r, bt, False)
    img, (ki, _) = _run(r, bt, True)
    assert ki == kf and ki > 0
    _assert_equal_bits(img, full, 'novel_pose')
    # and it is the novel-pose render (golden G5), not the training-pose one
    for k in KEYS:
        err = (img[k].cpu() - torch.from_numpy(g['out_' + k])).abs().max().item()
        assert err <= TOL, (k, err)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_given_t_rand_in_training_mode(dev, batches, precision):
    r = _renderer(dev, precision, perturb=1)
    assert r.net.training and r.cfg.perturb == 1
    bt = to_torch(batches['tail'], dev)
    R = int(bt['ray_o'].shape[1])
    t_rand = torch.rand((R, 64), generator=torch.Generator().manual_seed(5)).to(dev)
    full, (kf, _) = _run(r, bt, False, t_rand=t_rand)
    img, (ki, _) = _run(r, bt, True, t_rand=t_rand)
    assert ki == kf and ki > 0
    _assert_equal_bits(img, full, 't_rand')
    plain, _ = _run(_renderer(dev, precision), bt, True)
    assert not torch.equal(plain['depth_map'], img['depth_map'])  # the draws moved the samples


@pytest.mark.parametrize('precision', PRECISIONS)
def test_mmsk_renderer_and_empty_render(dev, renderers, precision):
    from animatable_nerf_amd.renderer_mmsk import Renderer as MRenderer
    from ._common import mmsk_batch_np
    g = golden('g9_mmsk')
    r = MRenderer(renderers[precision].net, renderers[precision].cfg)
    assert r.cfg.get('render_image_only', None) is False  # the plugin keeps the key's default
    b, _ = mmsk_batch_np(g['chunks_ray_o'], g['chunks_ray_d'])
    bt = to_torch(b, dev)
    full, (kf, _) = _run(r, bt, False)
    img, (ki, _) = _run(r, bt, True)
    assert ki == kf and ki > 0
    _assert_equal_bits(img, full, 'mmsk')
    keep = _keep(img['raw']).cpu().numpy()
    vis = np.unpackbits(g['chunks_inside_bits'])[:keep.size].astype(bool)
    assert not keep[~vis].any()  # the visibility filter ran: kept samples are visible ones
    # no view sees anything: nothing is kept, no tile runs
    b0 = dict(b)
    b0['msks'] = np.zeros_like(b['msks'])
    bt0 = to_torch(b0, dev)
    full0, (kf0, _) = _run(r, bt0, False)
    img0, (ki0, _) = _run(r, bt0, True)
    assert kf0 == 0 and ki0 == 0
    _assert_equal_bits(img0, full0, 'n_kept == 0')
    assert not bool(_keep(img0['raw']).any())


# ---- 6. guard bands ---------------------------------------------------------------------------------------
def test_guard_bands(dev, renderers, batches, pairs):
    _, img, _ = pairs('tail', 'fp32')
    ret, regions = _direct_call(renderers['fp32'], to_torch(batches['tail'], dev), bands=True)
    _assert_equal_bits(ret, img, 'exact-size workspace')
    for buf, n in regions:
        assert buf.numel() == n + 2 * BAND
        assert bool((buf[:BAND] == 0xA5).all()), n
        assert bool((buf[BAND + n:] == 0xA5).all()), n


# ---- 7. host render() under the key -----------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('n_rays', [300, 8192])
def test_host_render_under_the_key(dev, renderers, n_rays, precision):
    sc = scene(0.025)
    ro, rd = sc.box_rays(n_rays, seed=37)
    b, _ = batch_np(sc, ro, rd)
    bt = to_torch(b, dev)
    R = int(bt['ray_o'].shape[1])
    plain = renderers[precision]
    keyed = _renderer(dev, precision, net=plain.net, render_image_only=True)
    parts = min(keyed.HOST_PARTS, ((R + 2047) // 2048) // 2)
    assert (parts >= 2) == (n_rays == 8192), (R, parts)  # 300: the single copy; 8,192: _render_overlapped
    with torch.no_grad():
        ref = plain.render(bt)
        got = keyed.render(bt)
    assert set(ref) == set(KEYS) | {'pbw', 'tbw'}
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert not got[k].is_cuda, k
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), k
    assert keyed.last_counts is None
    with pytest.raises(RuntimeError):
        keyed.row_ids(R)
    # the device render of the keyed renderer: image-only by the key, rows refused
    dret = keyed.render_device(bt)
    assert set(dret) == set(KEYS)
    for k in KEYS:
        assert torch.equal(dret[k].cpu(), ref[k]), k
    with pytest.raises(RuntimeError):
        keyed.row_ids(R)
    with pytest.raises(ValueError):
        keyed.render_device(bt, bw_rows=True)
