"""GPU parity of the render at 128, 192 and 256 samples per ray (anr_render_ns_fwd) against the oracle and
golden G15, in the three render precisions: sample keep mask bit-exact; rgb / acc / depth / raw and the blend-weight
rows within 1e-4 absolute (the tolerances of tests/test_gpu_render.py). The batches are a few dozen rays with
cfg.chunk = 8, so every chunk shape is met: full box chunks, a grazing chunk that keeps only its forced sample
(in segment 0 at 128 samples, in segment 1 at 192 and 256), a partial last chunk. tests/test_oracle_ns.py checks
on the CPU that these batches have those properties."""
import ctypes

import numpy as np
import pytest
import torch

from ._common import batch_np, golden, make_net, scene, to_torch
from ._ns_common import (CHUNK, g15_batch, keep_of, mmsk_small_batch, oracle_mmsk, oracle_small, small_batch,
                         small_t_rand)

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ['fp32', 'bf16x3', 'bf16x6']
COUNTS = [128, 192, 256]
IMAGE_KEYS = ('rgb_map', 'acc_map', 'depth_map', 'raw')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def net(dev):
    n = make_net(dev)
    n.train()  # run.py evaluates in train() mode with perturb = 0
    return n


def make_renderer(net, precision, n, chunk=CHUNK, cls=None, **kw):
    from animatable_nerf_amd import config
    from animatable_nerf_amd.renderer import Renderer
    cfg = config.defaults()
    cfg.perturb = 0
    cfg.render_precision = precision
    cfg.N_samples = n
    cfg.chunk = chunk
    for k, v in kw.items():
        cfg[k] = v
    return (cls or Renderer)(net, cfg)


def check_against(ret, ref, keys):
    for k in keys:
        assert ret[k].shape == ref[k].shape, (k, ret[k].shape, ref[k].shape)
        err = (ret[k].cpu() - ref[k]).abs().max().item()
        print(k, err)
        assert err <= TOL, (k, err)


@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_small_chunks_match_oracle(net, dev, precision, n):
    ref, ref_ids = oracle_small(n)
    r = make_renderer(net, precision, n)
    ret = r.render_device(to_torch(small_batch(), dev))
    assert ret['raw'].shape == (1, 29 * n, 4)
    keep, ref_keep = keep_of(ret['raw']).cpu(), keep_of(ref['raw'])
    per_chunk = [int(ref_keep.view(29, n)[i:i + CHUNK].sum()) for i in range(0, 29, CHUNK)]
    print('oracle kept per chunk', per_chunk)
    assert per_chunk[2] == 1  # the grazing chunk: its forced argmin sample alone
    assert int((ref_keep.view(29, n // 64, 64).any(-1).sum(-1) > 1).sum()) >= 15  # rays spanning segments
    assert torch.equal(keep, ref_keep)
    assert r.last_counts == (int(ref_keep.sum()), ref['pbw'].shape[1])
    check_against(ret, ref, IMAGE_KEYS + ('pbw', 'tbw'))
    assert torch.equal(r.row_ids(29).cpu(), ref_ids)


@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_stratified_z_matches_oracle(net, dev, precision, n):
    ref, ref_ids = oracle_small(n, True)
    r = make_renderer(net, precision, n)
    ret = r.render_device(to_torch(small_batch(), dev), t_rand=small_t_rand(n).to(dev))
    assert torch.equal(keep_of(ret['raw']).cpu(), keep_of(ref['raw']))
    check_against(ret, ref, IMAGE_KEYS + ('pbw', 'tbw'))
    assert torch.equal(r.row_ids(29).cpu(), ref_ids)


@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_image_only_equals_full_program(net, dev, precision, n):
    bt = to_torch(small_batch(), dev)
    full = make_renderer(net, precision, n).render_device(bt)
    r = make_renderer(net, precision, n)
    img = r.render_device(bt, image_only=True)
    assert set(img) == set(IMAGE_KEYS)
    for k in IMAGE_KEYS:
        assert torch.equal(img[k], full[k]), k
    assert r.last_counts is None
    with pytest.raises(ValueError):
        r.render_device(bt, image_only=True, bw_rows=True)
    # the cfg key selects it too
    key = make_renderer(net, precision, n, render_image_only=True).render_device(bt)
    assert set(key) == set(IMAGE_KEYS) and torch.equal(key['raw'], full['raw'])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_visibility_filter_matches_oracle(net, dev, precision):
    from animatable_nerf_amd.renderer_mmsk import Renderer as MRenderer
    b, _ = mmsk_small_batch()
    ref, ref_raw, inside = oracle_mmsk(128)
    r = make_renderer(net, precision, 128, cls=MRenderer)
    ret = r.render_device(to_torch(b, dev), bw_rows=False)
    keep = keep_of(ret['raw']).cpu()
    assert not bool(inside.view(24, 128)[16:].any())  # the oracle's third chunk has no visible sample ...
    assert not bool(keep.view(24, 128)[16:].any())  # ... and keeps nothing
    assert torch.equal(keep, keep_of(ref_raw))
    check_against(ret, dict(ref, raw=ref_raw), IMAGE_KEYS)
    host = r.render(to_torch(b, dev))  # the plugin's drop-in call: three maps on the host
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        assert torch.equal(host[k], ret[k].cpu()), k
    img = r.render_device(to_torch(b, dev), image_only=True)
    for k in IMAGE_KEYS:
        assert torch.equal(img[k], ret[k]), k


@pytest.mark.parametrize('image_only', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_new_entry_at_64_equals_old_entry(net, dev, precision, image_only):
    """anr_render_ns_fwd at n_samples = 64 against anr_render_fwd / anr_render_image_fwd on G1's 64 rays: every
    output bit for bit (Renderer keeps 64 on the old entries, so the new one is called directly)."""
    from animatable_nerf_amd import _lib
    from animatable_nerf_amd.renderer import _Call
    sc = scene(0.05)
    ro, rd = sc.box_rays(64, seed=2)
    b, _ = batch_np(sc, ro, rd)
    bt = to_torch(b, dev)
    r = make_renderer(net, precision, 64, chunk=2048)
    old = r.render_device(bt, image_only=image_only)
    old_ids = None if image_only else r.row_ids(bt['ray_o'].shape[1])
    old = {k: v.clone() for k, v in old.items()}
    p = r.params()
    R = bt['ray_o'].shape[1]
    c = _Call(r, bt, None)
    c.opts.precision = c.render_precision
    io = 1 if image_only else 0
    lib = r.lib
    nbytes = lib.anr_render_ns_workspace_bytes(R, ctypes.byref(c.opts), ctypes.byref(c.frame), io)
    size_old = lib.anr_render_image_workspace_bytes if image_only else lib.anr_render_workspace_bytes
    assert nbytes == size_old(R, ctypes.byref(c.opts), ctypes.byref(c.frame))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.anr_render_ns_fwd(ctypes.byref(p), ctypes.byref(c.frame), *c.ray_ptrs(), R, ctypes.byref(c.opts),
                                     ctypes.byref(c.out), io, _lib.ptr(ws), nbytes, _lib.stream_ptr(dev)),
               'anr_render_ns_fwd')
    for k, v in (('rgb_map', c.rgb), ('acc_map', c.acc), ('depth_map', c.depth), ('raw', c.raw)):
        assert torch.equal(v, old[k]), k
    if image_only:
        return
    n_kept, m = r._counts(ws, R)
    assert m == old['pbw'].shape[1] and n_kept == int(keep_of(old['raw']).sum())
    pbw, tbw = torch.empty((1, m, 24), device=dev), torch.empty((1, m, 24), device=dev)
    ids = torch.empty((m,), dtype=torch.int32, device=dev)
    _lib.check(lib.anr_render_ns_bw_rows(_lib.ptr(ws), R, 64, _lib.ptr(pbw), _lib.ptr(tbw), _lib.stream_ptr(dev)),
               'anr_render_ns_bw_rows')
    _lib.check(lib.anr_render_ns_row_ids(_lib.ptr(ws), R, 64, _lib.ptr(ids), _lib.stream_ptr(dev)),
               'anr_render_ns_row_ids')
    assert torch.equal(pbw, old['pbw']) and torch.equal(tbw, old['tbw'])
    assert torch.equal(ids.long(), old_ids)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_g15_matches_reference(net, dev, precision):
    """the reference's own 128-sample render: one full 2048-ray chunk and a grazing chunk of 40 rays"""
    g = golden('g15_nsamples')
    b, _ = g15_batch()
    r = make_renderer(net, precision, 128, chunk=2048)
    ret = r.render_device(to_torch(b, dev))
    keep = keep_of(ret['raw']).cpu().numpy()
    assert np.array_equal(np.packbits(keep), g['keep_bits'])
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        err = np.abs(ret[k].cpu().numpy() - g['out_' + k]).max()
        print(k, err)
        assert err <= TOL, (k, err)
    kept_alpha = ret['raw'][0, :, 3].cpu().numpy()[keep]
    assert np.abs(kept_alpha - g['kept_alpha']).max() <= TOL
    assert ret['pbw'].shape[1] == int(g['bw_rows'])
    idx = torch.from_numpy(g['bw_sample_idx']).to(dev)
    assert np.abs(ret['pbw'][0, idx].cpu().numpy() - g['pbw_sample']).max() <= TOL
    assert np.abs(ret['tbw'][0, idx].cpu().numpy() - g['tbw_sample']).max() <= TOL
    assert keep.reshape(-1, 128)[2048:].sum() == 1


@pytest.mark.parametrize('image_only', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_drop_in_render_and_shards_equal_device_render(net, dev, precision, image_only):
    """Renderer.render (outputs on the host, the frame in overlapped parts of whole chunks) and the frame split
    over 2 ranks by whole chunks, at 128 samples: every output equals the one-call device render bit for bit.
    4 x 29 rays at chunk 8 are 15 chunks, so render() takes its overlapped path (>= 2 parts of >= 2 chunks)."""
    from animatable_nerf_amd import parallel
    b = small_batch()
    rep = {k: (np.concatenate([v] * 4, axis=1) if k in ('ray_o', 'ray_d', 'near', 'far', 'occupancy', 'mask_at_box',
                                                        'rgb') else v) for k, v in b.items()}
    bt = to_torch(rep, dev)
    R = bt['ray_o'].shape[1]
    assert R == 116
    r = make_renderer(net, precision, 128, render_image_only=image_only)
    full = r.render_device(bt)
    ref = {k: v.cpu() for k, v in full.items()}
    keys = IMAGE_KEYS if image_only else IMAGE_KEYS + ('pbw', 'tbw')
    assert set(ref) == set(keys)
    with torch.no_grad():
        got = r.render(bt)
    assert set(got) == set(keys)
    for k in keys:
        assert not got[k].is_cuda, k
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert torch.equal(got[k], ref[k]), k
    if not image_only:
        assert r.last_counts == (int(keep_of(ref['raw']).sum()), ref['pbw'].shape[1])
    parts = []
    for rank in range(2):
        sub, (s, e) = parallel.shard_batch(bt, rank, 2, CHUNK)
        assert e > s and s % CHUNK == 0
        parts.append(r.render_device(sub))
    for k in keys:
        assert torch.equal(torch.cat([q[k] for q in parts], dim=1).cpu(), ref[k]), k
    # render_sharded itself (one process: the whole frame as one shard, raw regrouped per ray at 128 samples)
    one = parallel.render_sharded(r, bt, chunk=CHUNK, rows=not image_only)
    assert one['span'] == (0, R)
    for k in keys:
        assert torch.equal(one[k].cpu(), ref[k]), k


def test_training_and_sdf_refuse_other_counts(net, dev):
    """training (NetworkWrapper, FusedStep) and the sdf_pdf renderer take 64 samples only and say so, before any
    library call (a batch they would fail on otherwise: no rays at all)"""
    from animatable_nerf_amd import config
    from animatable_nerf_amd.renderer_sdf import Renderer as SRenderer
    from animatable_nerf_amd.trainer import FusedStep, NetworkWrapper
    from ._common import make_net_sdf, sdf_cfg
    cfg = config.defaults()
    cfg.N_samples = 128
    with pytest.raises(ValueError, match='64 only'):
        NetworkWrapper(net, cfg)({})
    tnet = make_net(dev)
    with pytest.raises(ValueError, match='64 only'):
        FusedStep(tnet, cfg).step({})
    scfg = sdf_cfg()
    scfg.N_samples = 128
    with pytest.raises(ValueError, match='64 only'):
        SRenderer(make_net_sdf(dev), scfg).render_device({})
