"""Renderer plugin for the aligned_aninerf_lbw network: ``Renderer(net).render(batch)`` as
``tpose_renderer.py:159-186`` runs it over ``aligned_aninerf_lbw_network.Network`` (``:90-147``), eval only.

One call renders every ray through ``anr_lbw_render_fwd`` (include/aninerf.h): the 5-NN blend over
``pvertices`` with the keep mask (``cfg.norm_th``), the pose-space blend-weight MLP, LBS to the big pose for points
and view directions, the second 5-NN blend over ``tvertices`` and the T-pose blend-weight MLP, the density and
colour nets, compositing and the ``alpha_ind`` rows, with the reference's 2048-ray chunk semantics (forced argmin
keep, forced argmax row, the per-chunk in-place ``tbounds`` widening) kept on the device. Batches are those of
``tpose_pdf_dataset``: the keys ``renderer_sdf`` reads (without ``poses`` / ``occupancy``) plus ``tvertices``.
Output keys and shapes are the reference's: ``raw (1,R*64,4)``, ``rgb_map (1,R,3)``, ``acc_map`` / ``depth_map
(1,R)``, ``pbw`` / ``tbw (1,m,24)``; ``render`` moves them to the CPU and, like the reference, widens
``batch['tbounds']`` in place by 0.05 per chunk. ``image_only`` (``cfg.render_image_only``) skips the second search,
the T-pose MLP and the rows: no ``pbw`` / ``tbw`` keys, the same ``raw`` and maps bit for bit.

``cfg.render_precision``: 'fp32' (exact fp32 MFMA layer GEMMs), 'bf16x3' or 'bf16x6' (the blend-weight, density and
colour networks as one fused launch per batch each, split bf16 with 3 or 6 products). Not covered: training / autograd, ``cfg.test_novel_pose``, the mmsk
visibility filter, ``N_samples != 64``, ``parallel.render_sharded``.
"""
import ctypes

import torch

from . import _lib
from . import config as _config
from .renderer_knn import KnnRenderer, _f32, render_precision

CHUNK = 2048
RAY_KEYS = ('ray_o', 'ray_d', 'near', 'far')
FRAME_KEYS = ('A', 'big_A', 'R', 'Th', 'pvertices', 'tvertices', 'weights', 'tbounds')


def _lbw_precision(cfg):
    return render_precision(cfg, 'renderer_lbw: ')


class Renderer(KnnRenderer):
    widens_tbounds = True  # per chunk, in place (aligned_aninerf_lbw_network.py:124-126)
    params_type = _lib.LbwParams
    name = 'renderer_lbw'
    counts_fn, knn_fn, kept_fn = 'anr_lbw_render_counts', 'anr_lbw_render_knn', 'anr_lbw_render_kept'

    def render_device(self, batch, t_rand=None, image_only=False):
        """All outputs stay in HBM; ``batch['tbounds']`` is widened in place (reference quirk). ``t_rand`` (R, 64):
        the stratification draws (drawn here when perturbing in training mode and none are given)."""
        cfg = self.cfg
        _config.require_64_samples(cfg, 'aligned_aninerf_lbw renderer')
        if cfg.get('test_novel_pose', False):
            raise ValueError('renderer_lbw: cfg.test_novel_pose (novel_pose_bw) is not supported')
        if not cfg.get('tpose_viewdir', True) or not cfg.get('color_with_viewdir', True):
            raise ValueError('renderer_lbw: cfg.tpose_viewdir False / color_with_viewdir False are not supported')
        p = self.params()
        dev = self.device()
        R = batch['ray_o'].shape[1]
        ns = int(cfg.N_samples)
        if t_rand is None and cfg.perturb > 0 and self.net.training:
            t_rand = torch.rand((R, ns), device=dev)
        rays = {k: _f32(batch[k], dev) for k in RAY_KEYS}
        f = _lib.LbwFrame()
        fr = self.fill_frame(f, batch, FRAME_KEYS, dev)  # (kept alive over the call)
        tr = None if t_rand is None else _f32(t_rand, dev).reshape(R, ns)
        o = _lib.RenderOpts()
        o.n_samples, o.chunk = ns, int(cfg.get('chunk', CHUNK))
        o.norm_th, o.train_th = float(cfg.norm_th), float(cfg.train_th)
        o.t_rand = tr.data_ptr() if tr is not None else None
        o.novel_pose = 0
        o.precision = _lbw_precision(cfg)
        img = 1 if image_only else 0
        rgb = torch.empty((1, R, 3), device=dev)
        acc = torch.empty((1, R), device=dev)
        depth = torch.empty((1, R), device=dev)
        raw = torch.empty((1, R * ns, 4), device=dev)
        tb_out = torch.empty((2, 3), device=dev)
        out = _lib.LbwRenderOut(rgb.data_ptr(), acc.data_ptr(), depth.data_ptr(), raw.data_ptr(), tb_out.data_ptr())
        ws_bytes = self.lib.anr_lbw_render_workspace_bytes(R, ctypes.byref(o), img)
        ws = self.workspace(ws_bytes, dev)
        st = _lib.stream_ptr(dev)
        _lib.check(self.lib.anr_lbw_render_fwd(ctypes.byref(p), ctypes.byref(f), *[_lib.ptr(rays[k]) for k in RAY_KEYS],
                                               R, ctypes.byref(o), ctypes.byref(out), img, _lib.ptr(ws), ws_bytes, st),
                   'anr_lbw_render_fwd')
        with torch.no_grad():
            batch['tbounds'].copy_(tb_out.view_as(batch['tbounds']))
        self._last = (R, o, img)
        ret = {'raw': raw, 'rgb_map': rgb, 'acc_map': acc, 'depth_map': depth}
        addr = self.lib.anr_lbw_render_counts(_lib.ptr(ws), R, ctypes.byref(o), img)
        if image_only:
            return ret
        cnt = ws[addr - ws.data_ptr():addr - ws.data_ptr() + 8].view(torch.int32).cpu()  # host sync
        n_kept, m = int(cnt[0]), int(cnt[1])
        self.last_counts = (n_kept, m)
        pbw = torch.empty((1, m, 24), device=dev)
        tbw = torch.empty((1, m, 24), device=dev)
        self.last_row_ids = torch.empty((m,), dtype=torch.int32, device=dev)  # sample id (ray * 64 + sample) per row
        _lib.check(self.lib.anr_lbw_render_rows(_lib.ptr(ws), R, ctypes.byref(o), _lib.ptr(pbw), _lib.ptr(tbw),
                                                _lib.ptr(self.last_row_ids), st), 'anr_lbw_render_rows')
        ret.update({'pbw': pbw, 'tbw': tbw})
        return ret

    def warped(self, n):
        """(tpose (n,3), tpose_dirs (n,3)) of the first n rows of the last render's last batch (tests, debugging)."""
        c0 = self._view(self.lib.anr_lbw_render_points, n * 160).view(torch.float32).view(n, 40)
        return c0[:, 0:3].clone(), c0[:, 3:6].clone()

    def render(self, batch):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters()) and self.net.training:
            raise RuntimeError('aligned_aninerf_lbw: training through this network is not covered; render under '
                               'torch.no_grad() for evaluation')
        with torch.no_grad():
            ret = self.render_device(batch, image_only=bool(self.cfg.get('render_image_only', False)))
        from .renderer import to_host
        return to_host(ret)
