"""Evaluator plugin: ``Evaluator().evaluate(output, batch)`` / ``summarize()`` (lib/evaluators/if_nerf.py:9-91)
on the HIP library.

``evaluate`` enqueues one ``anr_eval_frame`` call (PSNR and the 7x7 windowed SSIM of the frame, float64
on the device) into the next row of a device result table and returns: no copy to the host, no
synchronisation, so the evaluation loop is ``Renderer.render_device`` -> ``evaluate`` with the frame never
leaving HBM. ``summarize`` makes the one D2H copy of the table, drops the frames the reference skips
(``rgb_gt.sum() == 0``), prints the three means and writes ``metrics.npy`` as the reference does.

``batch['H']`` / ``batch['W']`` are read as host integers: keep them on the CPU (a device tensor costs a
one-element copy per frame). SSIM's data range is ``cfg.eval_data_range`` (2.0: what the reference's
``structural_similarity(img_pred, img_gt, multichannel=True)`` call resolves to for float64 images, see
DESIGN.md §8 A18). ``cfg.eval_write_images`` also writes the reference's comparison PNGs (opt-in: writing
a file needs the pixels on the host, which synchronises).

There is no host fallback: the tensors are evaluated on a GPU or not at all.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import config as _config


def _host_int(v):
    if torch.is_tensor(v):
        return int(v.reshape(-1)[0])
    return int(np.asarray(v).reshape(-1)[0])


def fill_image(img, batch):
    """if_nerf.py:94-102: paste the cropped image back into the original frame (any dtype)."""
    orig_H, orig_W = _host_int(batch['orig_H']), _host_int(batch['orig_W'])
    full_img = np.zeros((orig_H, orig_W, 3), img.dtype)
    bbox = batch['crop_bbox'][0].detach().cpu().numpy() if torch.is_tensor(batch['crop_bbox']) else \
        np.asarray(batch['crop_bbox'])[0]
    height = int(bbox[1, 1] - bbox[0, 1])
    width = int(bbox[1, 0] - bbox[0, 0])
    full_img[bbox[0, 1]:bbox[1, 1], bbox[0, 0]:bbox[1, 0]] = img[:height, :width]
    return full_img


class Evaluator:
    INITIAL_ROWS = 64

    def __init__(self):
        self.cfg = _config.active()
        self.mse = []
        self.psnr = []
        self.ssim = []
        self._lib = None
        self._table = None   # (capacity, EVAL_NOUT) float64 on the device
        self._n = 0          # rows enqueued since the last summarize()
        self._names = []     # per row: (frame_index, cam_ind) as given (read only to name a frame in an error)
        self._ws = None

    # ---- device plumbing --------------------------------------------------------------------
    def _device(self, *tensors):
        for t in tensors:
            if torch.is_tensor(t) and t.is_cuda:
                return t.device
        if not torch.cuda.is_available():
            raise RuntimeError('Evaluator: no GPU; the evaluator has no host path')
        return torch.device('cuda', torch.cuda.current_device())

    def _row(self, dev):
        """The next row of the result table (grown by doubling; the copy is a device-side one)."""
        if self._table is None or self._table.device != dev:
            if self._n:
                raise RuntimeError('Evaluator: frames of one summarize() span must be on one device')
            self._table = torch.zeros((self.INITIAL_ROWS, _lib.EVAL_NOUT), dtype=torch.float64, device=dev)
        if self._n == self._table.shape[0]:
            grown = torch.zeros((2 * self._n, _lib.EVAL_NOUT), dtype=torch.float64, device=dev)
            grown[:self._n].copy_(self._table)
            self._table = grown
        return self._table[self._n]

    def _frame(self, rgb_pred, rgb_gt, mask, H, W, out, images=False):
        """Enqueue anr_eval_frame on the current stream; returns the uint8 images when asked for."""
        if self._lib is None:
            self._lib = _lib.load()
        dev = out.device
        pred = rgb_pred.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        gt = rgb_gt.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        mask = mask.detach().to(device=dev).reshape(-1).contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else (mask != 0).view(torch.uint8)
        n = pred.shape[0]
        if gt.shape[0] != n:
            raise ValueError(f'Evaluator: rgb_map has {n} rays, rgb {gt.shape[0]}')
        if mask.numel() != H * W:
            raise ValueError(f'Evaluator: mask_at_box has {mask.numel()} pixels, H x W = {H} x {W}')
        nbytes = self._lib.anr_eval_workspace_bytes(H, W)
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        img8 = (torch.empty((2, H, W, 3), dtype=torch.uint8, device=dev) if images else None)
        opts = _lib.EvalOpts(float(self.cfg.get('eval_data_range', 2.0)), 7)
        with torch.cuda.device(dev):
            _lib.check(self._lib.anr_eval_frame(
                _lib.ptr(pred), _lib.ptr(gt), n, _lib.ptr(mask), H, W, ctypes.byref(opts), _lib.ptr(out),
                None, None, _lib.ptr(img8[0]) if images else None, _lib.ptr(img8[1]) if images else None,
                _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr(dev)), 'anr_eval_frame')
        return img8

    # ---- the reference's interface ------------------------------------------------------------
    def evaluate(self, output, batch):
        rgb_pred, rgb_gt, mask = output['rgb_map'], batch['rgb'], batch['mask_at_box']
        dev = self._device(rgb_pred, rgb_gt, mask)
        H, W = _host_int(batch['H']), _host_int(batch['W'])
        row = self._row(dev)
        write = bool(self.cfg.get('eval_write_images', False))
        if rgb_pred.numel() == 0:  # no in-box ray: rgb_gt.sum() == 0, the reference skips the frame
            row.zero_()
            row[_lib.EVAL_STATUS] = _lib.EVAL_SKIPPED
        else:
            img8 = self._frame(rgb_pred, rgb_gt, mask, H, W, row, images=write)
            if write:
                self._write_images(img8, row, batch)
        self._names.append((batch.get('frame_index'), batch.get('cam_ind')))
        self._n += 1

    def _write_images(self, img8, row, batch):
        """The reference's comparison PNGs (if_nerf.py:34-49), from the device's uint8 images, for the
        frames the reference writes them for (ssim_metric runs after the skip rule)."""
        from PIL import Image
        if int(row[_lib.EVAL_STATUS].item()) in (_lib.EVAL_SKIPPED, _lib.EVAL_MISMATCH):  # synchronises
            return
        host = img8.cpu().numpy()
        result_dir = os.path.join(self.cfg.result_dir, 'comparison')
        os.makedirs(result_dir, exist_ok=True)
        frame_index, view_index = _host_int(batch['frame_index']), _host_int(batch['cam_ind'])
        for img, suffix in ((host[0], ''), (host[1], '_gt')):
            if 'crop_bbox' in batch:
                img = fill_image(img, batch)
            Image.fromarray(np.ascontiguousarray(img)).save(
                '{}/frame{:04d}_view{:04d}{}.png'.format(result_dir, frame_index, view_index, suffix))

    def _name(self, i):
        fi, ci = self._names[i]
        extra = ''
        if fi is not None and ci is not None:
            extra = f' (frame_index {_host_int(fi)}, cam_ind {_host_int(ci)})'
        return f'frame {i} of this run{extra}'

    def summarize(self):
        result_dir = self.cfg.result_dir
        rows = self._table[:self._n].cpu().numpy() if self._n else np.zeros((0, _lib.EVAL_NOUT))  # the one D2H copy
        names_n = self._n
        try:
            for i in range(names_n):
                status = int(rows[i, _lib.EVAL_STATUS])
                if status == _lib.EVAL_SKIPPED:
                    continue
                if status == _lib.EVAL_MISMATCH:
                    raise RuntimeError(f'Evaluator: {self._name(i)}: mask_at_box does not select as many pixels '
                                       f'as rgb_map has rays ({int(rows[i, _lib.EVAL_COUNT]) // 3})')
                if status == _lib.EVAL_NARROW:
                    raise ValueError(f'Evaluator: {self._name(i)}: win_size exceeds image extent: the mask crop is '
                                     f'{int(rows[i, _lib.EVAL_W])} x {int(rows[i, _lib.EVAL_H])}, the SSIM window 7 x 7')
                self.mse.append(float(rows[i, _lib.EVAL_MSE]))
                self.psnr.append(float(rows[i, _lib.EVAL_PSNR]))
                self.ssim.append(float(rows[i, _lib.EVAL_SSIM]))
            print('the results are saved at {}'.format(result_dir))
            result_path = os.path.join(result_dir, 'metrics.npy')
            os.makedirs(os.path.dirname(result_path) or '.', exist_ok=True)
            metrics = {'mse': self.mse, 'psnr': self.psnr, 'ssim': self.ssim}
            np.save(result_path, metrics)
            print('mse: {}'.format(np.mean(self.mse) if self.mse else float('nan')))
            print('psnr: {}'.format(np.mean(self.psnr) if self.psnr else float('nan')))
            print('ssim: {}'.format(np.mean(self.ssim) if self.ssim else float('nan')))
        finally:
            self.mse, self.psnr, self.ssim = [], [], []
            self._n = 0
            self._names = []
        return metrics

    # ---- one-frame conveniences (they synchronise) ------------------------------------------------
    def _one(self, rgb_pred, rgb_gt, mask, H, W):
        as_t = lambda v: v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))  # noqa: E731
        rgb_pred, rgb_gt, mask = as_t(rgb_pred), as_t(rgb_gt), as_t(mask)
        dev = self._device(rgb_pred, rgb_gt, mask)
        out = torch.zeros(_lib.EVAL_NOUT, dtype=torch.float64, device=dev)
        self._frame(rgb_pred, rgb_gt, mask, H, W, out)
        return out.cpu().numpy()

    def psnr_metric(self, img_pred, img_gt):
        """if_nerf.py:15-18 over any two arrays of rgb rows (float64 on the device)."""
        n = int(np.prod(tuple(img_pred.shape))) // 3
        rec = self._one(img_pred, img_gt, torch.ones(n, dtype=torch.bool), 1, n)
        return float(rec[_lib.EVAL_PSNR])

    def ssim_metric(self, rgb_pred, rgb_gt, batch):
        """if_nerf.py:20-58 without the PNGs (cfg.eval_write_images covers those in evaluate)."""
        H, W = _host_int(batch['H']), _host_int(batch['W'])
        rec = self._one(rgb_pred, rgb_gt, batch['mask_at_box'], H, W)
        status = int(rec[_lib.EVAL_STATUS])
        if status == _lib.EVAL_MISMATCH:
            raise RuntimeError('Evaluator: mask_at_box does not select as many pixels as there are rays')
        if status == _lib.EVAL_NARROW:
            raise ValueError(f'Evaluator: win_size exceeds image extent: the mask crop is '
                             f'{int(rec[_lib.EVAL_W])} x {int(rec[_lib.EVAL_H])}, the SSIM window 7 x 7')
        return float(rec[_lib.EVAL_SSIM])
