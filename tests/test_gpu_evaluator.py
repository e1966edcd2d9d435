"""GPU: the device-side frame evaluator (anr_eval_frame, animatable_nerf_amd.evaluator.Evaluator) against the
float64 restatements of the reference's numbers in ssim_ref.py.

Bounds. Every SSIM quantity is float64 on both sides (roundings ~1e-16 each; the smallest denominator
factor is C2 >= 9e-4, so a pixel's S is off by < ~1e-12): |ssim - ref| <= 1e-9 leaves three orders for the
summation order. mse against the float64 formula: 1e-12 relative; against the reference's float32
``np.mean((p - g)**2)``: 1e-5 relative (float32 rounding of the difference, of the square and of numpy's
pairwise sum at these sizes). psnr = -10 log10(mse) carries the same relative errors as absolute ones times
10 / ln 10.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib, config

from . import ssim_ref

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9
MSE64_RTOL = 1e-12
MSE32_RTOL = 1e-5
PSNR_SCALE = 10.0 / np.log(10.0)  # d psnr = PSNR_SCALE * d mse / mse


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def run_frame(dev, pred, gt, mask, H, W, opts=None, images=True, n_rays=None):
    """One anr_eval_frame call -> (record (12,) float64, images dict) on the host."""
    lib = _lib.load()
    tp = torch.from_numpy(np.ascontiguousarray(pred)).to(dev)
    tg = torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    tm = torch.from_numpy(np.ascontiguousarray(mask.reshape(-1).astype(np.uint8))).to(dev)
    n = tp.shape[0] if n_rays is None else n_rays
    assert tp.shape[0] >= n and tg.shape[0] >= n  # the kernels may read n rows
    out = torch.full((_lib.EVAL_NOUT,), -7.0, dtype=torch.float64, device=dev)
    ws_bytes = lib.anr_eval_workspace_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    imgs = {}
    if images:
        imgs = {'img_pred': torch.full((H, W, 3), -1.0, device=dev), 'img_gt': torch.full((H, W, 3), -1.0, device=dev),
                'img8_pred': torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev),
                'img8_gt': torch.full((H, W, 3), 99, dtype=torch.uint8, device=dev)}
    ip = [_lib.ptr(imgs.get(k)) for k in ('img_pred', 'img_gt', 'img8_pred', 'img8_gt')]
    _lib.check(lib.anr_eval_frame(_lib.ptr(tp), _lib.ptr(tg), n, _lib.ptr(tm), H, W,
                                  ctypes.byref(opts) if opts is not None else None, _lib.ptr(out), *ip,
                                  _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev)), 'anr_eval_frame')
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), {k: v.cpu().numpy() for k, v in imgs.items()}


def check_mse_psnr(rec, pred, gt):
    mse64, mse32 = ssim_ref.mse_f64(pred, gt), float(ssim_ref.mse_f32(pred, gt))
    mse, psnr = rec[_lib.EVAL_MSE], rec[_lib.EVAL_PSNR]
    print('mse', mse, 'f64 ref', mse64, 'rel', abs(mse - mse64) / mse64, 'f32 ref', mse32, 'rel', abs(mse - mse32) / mse32)
    print('psnr', psnr, 'ref', ssim_ref.psnr(mse64), 'f32 ref', ssim_ref.psnr(np.float64(mse32)))
    assert rec[_lib.EVAL_COUNT] == pred.size
    assert abs(rec[_lib.EVAL_SSE] / pred.size - mse64) <= MSE64_RTOL * mse64
    assert abs(mse - mse64) <= MSE64_RTOL * mse64
    assert abs(mse - mse32) <= MSE32_RTOL * mse32
    assert abs(psnr - ssim_ref.psnr(mse64)) <= PSNR_SCALE * MSE64_RTOL + 1e-13
    assert abs(psnr - ssim_ref.psnr(np.float64(mse32))) <= PSNR_SCALE * MSE32_RTOL


@pytest.mark.parametrize('name', ssim_ref.SHAPES)
def test_frame_parity(dev, name):
    c = ssim_ref.reference(name)
    H, W, mask, pred, gt = c['H'], c['W'], c['mask'], c['pred'], c['gt']
    rec, imgs = run_frame(dev, pred, gt, mask, H, W, opts=None)  # NULL opts: the library's defaults
    print(name, 'record', rec.tolist())
    assert rec[_lib.EVAL_STATUS] == _lib.EVAL_OK and rec[11] == 0.0
    assert tuple(int(v) for v in rec[_lib.EVAL_X:_lib.EVAL_H + 1]) == c['rect']
    assert np.array_equal(imgs['img_pred'].view(np.int32), c['img_pred'].view(np.int32))
    assert np.array_equal(imgs['img_gt'].view(np.int32), c['img_gt'].view(np.int32))
    assert np.array_equal(imgs['img8_pred'], ssim_ref.to_u8(c['img_pred']))
    assert np.array_equal(imgs['img8_gt'], ssim_ref.to_u8(c['img_gt']))
    assert rec[_lib.EVAL_SUM_GT] == pytest.approx(float(gt.astype(np.float64).sum()), rel=1e-12)
    check_mse_psnr(rec, pred, gt)
    print('ssim', rec[_lib.EVAL_SSIM], 'ref(2.0)', c['ssim'][2.0], 'diff', abs(rec[_lib.EVAL_SSIM] - c['ssim'][2.0]))
    assert abs(rec[_lib.EVAL_SSIM] - c['ssim'][2.0]) <= SSIM_TOL
    # a default-constructed opts is data_range 2.0: the same bits as NULL opts, and without image outputs
    rec_d, _ = run_frame(dev, pred, gt, mask, H, W, opts=_lib.EvalOpts(), images=False)
    assert np.array_equal(rec_d.view(np.int64), rec.view(np.int64))
    rec1, _ = run_frame(dev, pred, gt, mask, H, W, opts=_lib.EvalOpts(1.0), images=False)
    print('ssim(1.0)', rec1[_lib.EVAL_SSIM], 'ref', c['ssim'][1.0], 'diff', abs(rec1[_lib.EVAL_SSIM] - c['ssim'][1.0]))
    assert abs(rec1[_lib.EVAL_SSIM] - c['ssim'][1.0]) <= SSIM_TOL
    assert abs(c['ssim'][1.0] - c['ssim'][2.0]) > 1e-6  # the two ranges are told apart at this bound
    assert np.array_equal(rec1[:4].view(np.int64), rec[:4].view(np.int64))


def test_u8_rounding_and_clip(dev):
    """0.5 (the one fp32 value whose 255 multiple is a tie: 127.5 -> 128), near-ties, values outside [0, 1]."""
    H, W = 7, 7
    mask = np.ones(H * W, bool)
    vals = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 126.5 / 255, 127.5 / 255, -0.25, 1.75, 0.0, 1.0, 254.5 / 255,
                     0.1, 0.9, 0.5], np.float32)
    gt = np.resize(vals, (H * W, 3)).astype(np.float32)
    pred = np.resize(vals[::-1], (H * W, 3)).astype(np.float32)
    rec, imgs = run_frame(dev, pred, gt, mask, H, W)
    assert rec[_lib.EVAL_STATUS] == _lib.EVAL_OK
    assert np.array_equal(imgs['img8_gt'], ssim_ref.to_u8(gt.reshape(H, W, 3)))
    assert np.array_equal(imgs['img8_pred'], ssim_ref.to_u8(pred.reshape(H, W, 3)))
    assert abs(rec[_lib.EVAL_SSIM] - ssim_ref.frame_ssim(pred, gt, mask, H, W)) <= SSIM_TOL


def test_deterministic(dev):
    c = ssim_ref.reference('polygon_70x131')
    a, _ = run_frame(dev, c['pred'], c['gt'], c['mask'], c['H'], c['W'], images=False)
    b, _ = run_frame(dev, c['pred'], c['gt'], c['mask'], c['H'], c['W'], images=False)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_status_narrow_crop(dev):
    c = ssim_ref.make_case('narrow_6x30')
    rec, _ = run_frame(dev, c['pred'], c['gt'], c['mask'], c['H'], c['W'])
    assert rec[_lib.EVAL_STATUS] == _lib.EVAL_NARROW
    assert tuple(int(v) for v in rec[_lib.EVAL_X:_lib.EVAL_H + 1]) == (4, 5, 30, 6)
    assert np.isnan(rec[_lib.EVAL_SSIM])
    check_mse_psnr(rec, c['pred'], c['gt'])


def test_status_skipped_zero_gt(dev):
    c = ssim_ref.reference('block8x40_12x60')
    rec, _ = run_frame(dev, c['pred'], np.zeros_like(c['gt']), c['mask'], c['H'], c['W'])
    assert rec[_lib.EVAL_STATUS] == _lib.EVAL_SKIPPED and rec[_lib.EVAL_SUM_GT] == 0.0


def test_status_mismatch_more_rays_than_pixels(dev):
    """n_rays larger than the mask's popcount, with buffers of that larger size."""
    c = ssim_ref.reference('block8x40_12x60')
    extra = 37
    pred = np.concatenate([c['pred'], c['pred'][:extra]])
    gt = np.concatenate([c['gt'], c['gt'][:extra]])
    rec, _ = run_frame(dev, pred, gt, c['mask'], c['H'], c['W'])
    assert rec[_lib.EVAL_STATUS] == _lib.EVAL_MISMATCH


# ---- the Evaluator plugin ----------------------------------------------------------------------------------
def _batch(c, dev, gt=None, frame_index=0, on_device=True):
    to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if on_device else \
        (lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    return {'rgb': to((c['gt'] if gt is None else gt)[None]), 'mask_at_box': to(c['mask'][None]),
            'H': torch.tensor([c['H']]), 'W': torch.tensor([c['W']]),
            'frame_index': torch.tensor([frame_index]), 'cam_ind': torch.tensor([3])}


def _evaluator(tmp_path, **kw):
    from animatable_nerf_amd.evaluator import Evaluator
    ev = Evaluator()
    ev.cfg = config.defaults()
    ev.cfg.result_dir = str(tmp_path)
    ev.cfg.merge(config.CfgNode(kw))
    return ev


def test_evaluator_end_to_end(dev, tmp_path, capsys):
    ev = _evaluator(tmp_path)
    cases = [ssim_ref.reference(n) for n in ('diamond_37x53', 'block8x40_12x60', 'polygon_70x131')]
    for i, c in enumerate(cases):
        gt = np.zeros_like(c['gt']) if i == 1 else None  # the middle frame is one the reference skips
        on_device = i != 2  # device tensors (render_device) and CPU tensors (render) are both taken
        to = (lambda a: torch.from_numpy(a).to(dev)) if on_device else torch.from_numpy
        ev.evaluate({'rgb_map': to(c['pred'][None])}, _batch(c, dev, gt, frame_index=i, on_device=on_device))
    m = ev.summarize()
    saved = np.load(os.path.join(str(tmp_path), 'metrics.npy'), allow_pickle=True).item()
    text = capsys.readouterr().out
    assert 'mse: ' in text and 'psnr: ' in text and 'ssim: ' in text
    for got in (m, saved):
        assert sorted(got) == ['mse', 'psnr', 'ssim']
        assert [len(got[k]) for k in ('mse', 'psnr', 'ssim')] == [2, 2, 2]
        for j, c in enumerate((cases[0], cases[2])):
            assert abs(got['ssim'][j] - c['ssim'][2.0]) <= SSIM_TOL
            assert abs(got['mse'][j] - c['mse64']) <= MSE64_RTOL * c['mse64']
            assert abs(got['mse'][j] - c['mse32']) <= MSE32_RTOL * c['mse32']
            assert abs(got['psnr'][j] - ssim_ref.psnr(c['mse64'])) <= PSNR_SCALE * MSE64_RTOL + 1e-13
    again = ev.summarize()
    assert again == {'mse': [], 'psnr': [], 'ssim': []}


def test_evaluator_table_grows(dev, tmp_path):
    ev = _evaluator(tmp_path)
    ev.INITIAL_ROWS = 2
    c = ssim_ref.reference('block7_20x20')
    pred = torch.from_numpy(c['pred'][None]).to(dev)
    b = _batch(c, dev)
    for _ in range(5):
        ev.evaluate({'rgb_map': pred}, b)
    m = ev.summarize()
    assert len(m['ssim']) == 5 and len(set(m['ssim'])) == 1
    assert abs(m['ssim'][0] - c['ssim'][2.0]) <= SSIM_TOL


def test_evaluator_data_range_key(dev, tmp_path):
    ev = _evaluator(tmp_path, eval_data_range=1.0)
    c = ssim_ref.reference('block7_20x20')
    ev.evaluate({'rgb_map': torch.from_numpy(c['pred'][None]).to(dev)}, _batch(c, dev))
    assert abs(ev.summarize()['ssim'][0] - c['ssim'][1.0]) <= SSIM_TOL


def test_evaluator_narrow_frame_raises(dev, tmp_path):
    ev = _evaluator(tmp_path)
    ok, narrow = ssim_ref.reference('block7_20x20'), ssim_ref.make_case('narrow_6x30')
    ev.evaluate({'rgb_map': torch.from_numpy(ok['pred'][None]).to(dev)}, _batch(ok, dev, frame_index=11))
    ev.evaluate({'rgb_map': torch.from_numpy(narrow['pred'][None]).to(dev)}, _batch(narrow, dev, frame_index=12))
    with pytest.raises(ValueError, match='frame_index 12'):
        ev.summarize()
    assert ev.summarize() == {'mse': [], 'psnr': [], 'ssim': []}  # the failed span is dropped


def test_evaluator_mismatch_raises(dev, tmp_path):
    ev = _evaluator(tmp_path)
    c = ssim_ref.reference('block8x40_12x60')
    pred = np.concatenate([c['pred'], c['pred'][:5]])
    gt = np.concatenate([c['gt'], c['gt'][:5]])
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, _batch(c, dev, gt))
    with pytest.raises(RuntimeError, match='mask_at_box'):
        ev.summarize()


def test_one_frame_conveniences(dev, tmp_path):
    ev = _evaluator(tmp_path)
    c = ssim_ref.reference('diamond_37x53')
    assert abs(ev.psnr_metric(c['pred'], c['gt']) - ssim_ref.psnr(c['mse64'])) <= PSNR_SCALE * MSE64_RTOL + 1e-13
    assert abs(ev.ssim_metric(c['pred'], c['gt'], _batch(c, dev)) - c['ssim'][2.0]) <= SSIM_TOL


def test_evaluator_with_renderer(dev, tmp_path):
    """render_device -> evaluate against render (host) -> ssim_ref on a 48 x 40 camera of the synthetic scene:
    rgb_map is the same fp32 data either way, so the bounds are the same."""
    from animatable_nerf_amd import data
    from animatable_nerf_amd.renderer import Renderer
    from ._common import make_net, scene
    sc = scene(0.05)
    H, W = 48, 40
    K = np.array([[150.0, 0, W / 2.0], [0, 150.0, H / 2.0], [0, 0, 1]])  # the box spans ~30 columns, every row
    R = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    T = np.array([[0.0], [0.0], [3.0]])
    ro, rd, near, far, mask, _ = data.get_rays_within_bounds(H, W, K, R, T, sc.bounds, dev)
    n = int(mask.sum())
    assert 1000 <= n < H * W  # about 48 x 30 in-box rays, not the whole raster
    rng = np.random.Generator(np.random.PCG64(5))
    gt = rng.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    b = sc.batch_arrays(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros(1, np.float32),
                        np.zeros(1, np.float32))
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}
    batch.update(ray_o=ro[None], ray_d=rd[None], near=near[None], far=far[None], rgb=torch.from_numpy(gt[None]).to(dev),
                 mask_at_box=mask.reshape(1, -1), H=torch.tensor([H]), W=torch.tensor([W]))
    cfg = config.defaults()
    cfg.perturb = 0
    r = Renderer(make_net(dev).eval(), cfg)
    ev = _evaluator(tmp_path)
    with torch.no_grad():
        ev.evaluate(r.render_device(batch, bw_rows=False), batch)
        host = r.render(batch)
    m = ev.summarize()
    pred = host['rgb_map'][0].numpy()
    mask_np = mask.reshape(-1).cpu().numpy()
    ref = ssim_ref.frame_ssim(pred, gt, mask_np, H, W)
    mse64 = ssim_ref.mse_f64(pred, gt)
    print('n', n, 'rect', ssim_ref.bounding_rect(mask_np, H, W), 'ssim', m['ssim'][0], 'ref', ref, 'mse', m['mse'][0], mse64)
    assert abs(m['ssim'][0] - ref) <= SSIM_TOL
    assert abs(m['mse'][0] - mse64) <= MSE64_RTOL * mse64
    mse32 = float(ssim_ref.mse_f32(pred, gt))
    assert abs(m['mse'][0] - mse32) <= MSE32_RTOL * mse32


def test_write_images(dev, tmp_path):
    Image = pytest.importorskip('PIL.Image')
    ev = _evaluator(tmp_path, eval_write_images=True)
    c = ssim_ref.reference('diamond_37x53')
    ev.evaluate({'rgb_map': torch.from_numpy(c['pred'][None]).to(dev)}, _batch(c, dev, frame_index=7))
    for suffix, img in (('', c['img_pred']), ('_gt', c['img_gt'])):
        path = os.path.join(str(tmp_path), 'comparison', 'frame0007_view0003%s.png' % suffix)
        assert os.path.exists(path), path
        assert np.array_equal(np.asarray(Image.open(path).convert('RGB')), ssim_ref.to_u8(img))
    # crop_bbox: fill_image's paste into the original frame
    ev2 = _evaluator(tmp_path / 'crop', eval_write_images=True)
    b = _batch(c, dev, frame_index=8)
    b.update(orig_H=torch.tensor([60]), orig_W=torch.tensor([80]),
             crop_bbox=torch.tensor([[[10, 5], [10 + c['W'], 5 + c['H']]]]))
    ev2.evaluate({'rgb_map': torch.from_numpy(c['pred'][None]).to(dev)}, b)
    full = np.asarray(Image.open(os.path.join(str(tmp_path), 'crop', 'comparison', 'frame0008_view0003.png')).convert('RGB'))
    want = np.zeros((60, 80, 3), np.uint8)
    want[5:5 + c['H'], 10:10 + c['W']] = ssim_ref.to_u8(c['img_pred'])
    assert np.array_equal(full, want)
    assert len(ev.summarize()['ssim']) == 1
