"""Float64 restatements of the reference evaluator's numbers (lib/evaluators/if_nerf.py:15-74), shared by
test_evaluator.py and test_gpu_evaluator.py. Not a test file.

The reference's SSIM is ``structural_similarity(img_pred, img_gt, multichannel=True)`` (scikit-image
0.16-0.18) on the float64 crop of the zero-filled images: per channel a 7x7 uniform window, K1 0.01,
K2 0.03, sample covariance, the mean of S over the crop minus its 3-pixel border, then the mean over the
channels. scikit-image is not installed, so it is restated twice, independently:
``ssim_uniform_filter`` runs the code scikit-image itself runs (scipy's ``uniform_filter`` on each of the
five moments, then the crop); ``ssim_brute`` loops over every whole 7x7 window.
"""
import functools

import numpy as np

WIN = 7
K1, K2 = 0.01, 0.03


def scatter(rgb, mask, H, W):
    """if_nerf.py:26-29: the zero-filled float64 (H,W,3) image of the in-box rays."""
    img = np.zeros((H, W, 3))
    img[mask.reshape(H, W)] = rgb
    return img


def scatter_f32(rgb, mask, H, W):
    img = np.zeros((H, W, 3), np.float32)
    img[mask.reshape(H, W)] = rgb
    return img


def to_u8(img):
    """rint(clip(255 v, 0, 255)) in float64, half to even."""
    return np.rint(np.clip(255.0 * img.astype(np.float64), 0.0, 255.0)).astype(np.uint8)


def bounding_rect(mask, H, W):
    """cv2.boundingRect of the mask: x, y = smallest column / row holding a set pixel, w, h the extents."""
    m = mask.reshape(H, W)
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def mse_f32(pred, gt):
    """The reference's expression on its float32 arrays (if_nerf.py:67)."""
    return np.mean((pred - gt) ** 2)


def mse_f64(pred, gt):
    d = pred.astype(np.float64) - gt.astype(np.float64)
    return float((d * d).sum() / d.size)


def psnr(mse):
    return -10.0 * np.log(mse) / np.log(10.0)


def _channel_uniform_filter(X, Y, data_range):
    from scipy.ndimage import uniform_filter
    NP = WIN * WIN
    cov_norm = NP / (NP - 1.0)
    ux = uniform_filter(X, size=WIN)
    uy = uniform_filter(Y, size=WIN)
    uxx = uniform_filter(X * X, size=WIN)
    uyy = uniform_filter(Y * Y, size=WIN)
    uxy = uniform_filter(X * Y, size=WIN)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2
    return S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean()


def ssim_uniform_filter(img_pred, img_gt, data_range=2.0):
    """(h,w,3) float64 crops -> mean over the channels of the per-channel mean SSIM."""
    if min(img_pred.shape[:2]) < WIN:
        raise ValueError('win_size exceeds image extent')
    return float(np.mean([_channel_uniform_filter(img_pred[..., c], img_gt[..., c], data_range) for c in range(3)]))


def ssim_brute(img_pred, img_gt, data_range=2.0):
    """The same number from the definition: every whole 7x7 window, moments straight from its 49 samples."""
    h, w = img_pred.shape[:2]
    if min(h, w) < WIN:
        raise ValueError('win_size exceeds image extent')
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    means = []
    for c in range(3):
        X, Y = img_pred[..., c], img_gt[..., c]
        tot = 0.0
        for i in range(h - WIN + 1):
            for j in range(w - WIN + 1):
                a = X[i:i + WIN, j:j + WIN].ravel()
                b = Y[i:i + WIN, j:j + WIN].ravel()
                ux, uy = a.sum() / 49.0, b.sum() / 49.0
                vx = ((a - ux) ** 2).sum() / 48.0
                vy = ((b - uy) ** 2).sum() / 48.0
                vxy = ((a - ux) * (b - uy)).sum() / 48.0
                tot += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        means.append(tot / ((h - WIN + 1) * (w - WIN + 1)))
    return float(np.mean(means))


def frame_ssim(pred, gt, mask, H, W, data_range=2.0, fn=ssim_uniform_filter):
    """if_nerf.py:20-58 without the PNGs: scatter, crop to the mask's bounding rectangle, SSIM."""
    x, y, w, h = bounding_rect(mask, H, W)
    ip = scatter(pred, mask, H, W)[y:y + h, x:x + w]
    ig = scatter(gt, mask, H, W)[y:y + h, x:x + w]
    return fn(ip, ig, data_range)


# ---- the test shapes: the smallest at which each mechanism of the kernels can go wrong --------------------
def _diamond(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    return (np.abs(yy - cy) / (H / 2.0) + np.abs(xx - cx) / (W / 2.0)) <= 1.01  # the four tips are set


def _polygon(H, W, x0, y0):
    """A convex hexagon whose bounding rectangle starts at (x0, y0) and ends one pixel short of the image."""
    yy, xx = np.mgrid[0:H, 0:W]
    h, w = H - 1 - y0, W - 1 - x0
    u, v = (xx - x0) / float(w - 1), (yy - y0) / float(h - 1)
    inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    return inside & (u + v >= 0.3) & (u + v <= 1.7) & (u - v <= 0.8) & (v - u <= 0.8)


def _block(H, W, y0, x0, h, w):
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def shape_mask(name):
    """name -> (H, W, mask (H,W) bool)."""
    if name == 'diamond_37x53':  # a 36 x 52 diamond starting at (1, 1): ragged rows
        m = np.zeros((37, 53), bool)
        m[1:, 1:] = _diamond(36, 52)
        return 37, 53, m
    if name == 'full_64x64':
        return 64, 64, np.ones((64, 64), bool)
    if name == 'polygon_70x131':
        return 70, 131, _polygon(70, 131, 5, 9)
    if name == 'block7_20x20':
        return 20, 20, _block(20, 20, 6, 8, 7, 7)
    if name == 'block8x40_12x60':
        return 12, 60, _block(12, 60, 2, 11, 8, 40)
    if name == 'narrow_6x30':
        return 16, 40, _block(16, 40, 5, 4, 6, 30)
    raise KeyError(name)


SHAPES = ('diamond_37x53', 'full_64x64', 'polygon_70x131', 'block7_20x20', 'block8x40_12x60')


def make_case(name, seed=0):
    """Random float32 gt in [0, 1], pred = clip(gt + 0.1 N(0,1), 0, 1) on the mask's rays."""
    H, W, mask = shape_mask(name)
    n = int(mask.sum())
    rng = np.random.Generator(np.random.PCG64(seed + 17 * len(name)))
    gt = rng.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    pred = np.clip(gt + 0.1 * rng.standard_normal((n, 3)), 0.0, 1.0).astype(np.float32)
    return {'name': name, 'H': H, 'W': W, 'mask': mask.reshape(-1), 'pred': pred, 'gt': gt}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case and its reference numbers, computed once per session and shared (treat as read-only)."""
    c = make_case(name)
    H, W, mask, pred, gt = c['H'], c['W'], c['mask'], c['pred'], c['gt']
    ref = dict(c)
    ref['rect'] = bounding_rect(mask, H, W)
    ref['ssim'] = {r: frame_ssim(pred, gt, mask, H, W, r) for r in (2.0, 1.0)}
    ref['mse64'] = mse_f64(pred, gt)
    ref['mse32'] = float(mse_f32(pred, gt))
    ref['img_pred'] = scatter_f32(pred, mask, H, W)
    ref['img_gt'] = scatter_f32(gt, mask, H, W)
    return ref
