"""Renderer plugin for the aligned_aninerf_pdf network: ``Renderer(net).render(batch)`` as
``tpose_renderer.py:159-186`` runs it over ``aligned_aninerf_pdf_network.Network`` (``:97-138``), eval only.

One call renders every ray through ``anr_pdf_render_fwd`` (include/aninerf.h): the 5-NN blend over ``pvertices``
with the keep mask (the network's hard-coded 0.1, not ``cfg.norm_th``), LBS to the big pose for points and view
directions, the displacement MLP over the pose vector with ``resd = 0.05 tanh(.)``, the density and colour nets
at ``tpose = init_bigpose + resd``, compositing, with the reference's 2048-ray chunk semantics (forced argmin keep,
the per-chunk in-place ``tbounds`` widening) kept on the device. Batches are those of ``tpose_pdf_dataset``.
Output keys and shapes are the reference's: ``raw (1,R*64,4)``, ``rgb_map (1,R,3)``, ``acc_map`` / ``depth_map
(1,R)``, ``resd (1,n',3)``; ``render`` moves them to the CPU and, like the reference, widens ``batch['tbounds']`` in
place by 0.05 per chunk. ``image_only`` (``cfg.render_image_only``) keeps no ``resd`` rows and makes no host read
for them: no ``resd`` key, the same ``raw`` and maps bit for bit.

``cfg.render_precision``: 'fp32' (exact fp32 MFMA layer GEMMs), 'bf16x3' or 'bf16x6' (the displacement, density and
colour networks as one fused launch per batch each, split bf16 with 3 or 6 products). Not covered: training /
autograd, ``cfg.test_novel_pose``, ``N_samples != 64``, ``parallel.render_sharded``.

``alpha_points`` is ``Network.get_alpha`` (``:140-174``) over free points (``anr_pdf_alpha_points``), which
``renderer_pdf_mesh`` puts under marching cubes.
"""
import ctypes

import torch

from . import _lib
from . import config as _config
from .renderer_knn import KnnRenderer, _f32, render_precision

CHUNK = 2048
ALPHA_CHUNK = 2048 * 64  # aninerf_mesh_renderer.py:36
RAY_KEYS = ('ray_o', 'ray_d', 'near', 'far')
FRAME_KEYS = ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses', 'tbounds')


def _pdf_precision(cfg):
    return render_precision(cfg, 'renderer_pdf: ')


class Renderer(KnnRenderer):
    widens_tbounds = True      # per chunk, in place (aligned_aninerf_pdf_network.py:125-127)
    visibility_filter = False  # renderer_pdf_mmsk: the training-view visibility filter of tpose_renderer_mmsk
    params_type = _lib.PdfParams
    name = 'renderer_pdf'
    counts_fn, knn_fn, kept_fn = 'anr_pdf_render_counts', 'anr_pdf_render_knn', 'anr_pdf_render_kept'
    _aws = None  # alpha_points' workspace

    def check_cfg(self):
        cfg = self.cfg
        _config.require_64_samples(cfg, 'aligned_aninerf_pdf renderer')
        if cfg.get('test_novel_pose', False):
            raise ValueError('renderer_pdf: cfg.test_novel_pose is not supported')
        if not cfg.get('tpose_viewdir', True) or not cfg.get('color_with_viewdir', True):
            raise ValueError('renderer_pdf: cfg.tpose_viewdir False / color_with_viewdir False are not supported')
        if cfg.get('init_sdf', False):
            raise ValueError('renderer_pdf: cfg.init_sdf is not supported')
        _pdf_precision(cfg)

    def render_device(self, batch, t_rand=None, image_only=False, chunk_offset=None):
        """All outputs stay in HBM; ``batch['tbounds']`` is widened in place (reference quirk). ``t_rand`` (R, 64):
        the stratification draws (drawn here when perturbing in training mode and none are given)."""
        cfg = self.cfg
        self.check_cfg()
        if chunk_offset is not None:  # parallel.render_sharded passes one to renderers that widen tbounds
            raise ValueError('renderer_pdf: parallel.render_sharded (a chunk offset) is not supported')
        p = self.params()
        dev = self.device()
        R = batch['ray_o'].shape[1]
        ns = int(cfg.N_samples)
        if t_rand is None and cfg.perturb > 0 and self.net.training:
            t_rand = torch.rand((R, ns), device=dev)
        rays = {k: _f32(batch[k], dev) for k in RAY_KEYS}
        f = _lib.PdfFrame()
        fr = self.fill_frame(f, batch, FRAME_KEYS, dev)  # (kept alive over the call)
        tr = None if t_rand is None else _f32(t_rand, dev).reshape(R, ns)
        views = self.fill_views(f, batch, dev) if self.visibility_filter else None  # (kept alive)
        o = _lib.RenderOpts()
        o.n_samples, o.chunk = ns, int(cfg.get('chunk', CHUNK))
        o.norm_th, o.train_th = float(cfg.norm_th), float(cfg.train_th)  # neither is read by this network
        o.t_rand = tr.data_ptr() if tr is not None else None
        o.novel_pose = 0
        o.precision = _pdf_precision(cfg)
        img = 1 if image_only else 0
        rgb = torch.empty((1, R, 3), device=dev)
        acc = torch.empty((1, R), device=dev)
        depth = torch.empty((1, R), device=dev)
        raw = torch.empty((1, R * ns, 4), device=dev)
        tb_out = torch.empty((2, 3), device=dev)
        out = _lib.PdfRenderOut(rgb.data_ptr(), acc.data_ptr(), depth.data_ptr(), raw.data_ptr(), tb_out.data_ptr())
        ws_bytes = self.lib.anr_pdf_render_workspace_bytes(R, ctypes.byref(o), img)
        ws = self.workspace(ws_bytes, dev)
        st = _lib.stream_ptr(dev)
        _lib.check(self.lib.anr_pdf_render_fwd(ctypes.byref(p), ctypes.byref(f), *[_lib.ptr(rays[k]) for k in RAY_KEYS],
                                               R, ctypes.byref(o), ctypes.byref(out), img, _lib.ptr(ws), ws_bytes, st),
                   'anr_pdf_render_fwd')
        with torch.no_grad():
            batch['tbounds'].copy_(tb_out.view_as(batch['tbounds']))
        self._last = (R, o, img)
        ret = {'raw': raw, 'rgb_map': rgb, 'acc_map': acc, 'depth_map': depth}
        if image_only:
            return ret
        n_kept = int(self._view(self.lib.anr_pdf_render_counts, 4).view(torch.int32).item())  # host sync
        self.last_counts = (n_kept,)
        resd = torch.empty((1, n_kept, 3), device=dev)
        self.last_row_ids = torch.empty((n_kept,), dtype=torch.int32, device=dev)  # sample id (ray * 64 + sample) per row
        _lib.check(self.lib.anr_pdf_render_rows(_lib.ptr(ws), R, ctypes.byref(o), _lib.ptr(resd),
                                                _lib.ptr(self.last_row_ids), st), 'anr_pdf_render_rows')
        ret['resd'] = resd
        return ret

    def alpha_points(self, wpts, batch, chunk_pts=ALPHA_CHUNK):
        """``Network.get_alpha`` of (n,3) world points, one network call per ``chunk_pts`` points as
        ``aninerf_mesh_renderer.py:14-23`` batchifies it -> (n,) raw density on the device (0 where dropped)."""
        self.check_cfg()
        p = self.params()
        dev = self.device()
        pts = _f32(wpts, dev).reshape(-1, 3)
        n = pts.shape[0]
        alpha = torch.zeros(n, device=dev)
        if n == 0:
            return alpha
        f = _lib.PdfFrame()
        fr = {k: _f32(batch[k], dev) for k in ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses')}
        for k, t in fr.items():
            setattr(f, k, t.data_ptr())
        f.n_verts = fr['pvertices'].shape[-2]
        o = _lib.AlphaOpts()
        o.chunk_pts, o.norm_th, o.novel_pose, o.precision = int(chunk_pts), 0.1, 0, _pdf_precision(self.cfg)
        nbytes = self.lib.anr_pdf_alpha_workspace_bytes(n, ctypes.byref(o))
        if nbytes == 0:
            raise ValueError('anr_pdf_alpha_workspace_bytes: bad arguments (chunk_pts must be a multiple of 64, '
                             'at most 2^24 points)')
        if self._aws is None or self._aws.numel() < nbytes or self._aws.device != dev:
            self._aws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.anr_pdf_alpha_points(ctypes.byref(p), ctypes.byref(f), _lib.ptr(pts), n, ctypes.byref(o),
                                                 _lib.ptr(alpha), _lib.ptr(self._aws), nbytes, _lib.stream_ptr(dev)),
                   'anr_pdf_alpha_points')
        return alpha

    def warped(self, n):
        """(init_bigpose (n,3), tpose (n,3), tpose_dirs (n,3)) of the first n rows of the last render's last batch
        (tests, debugging)."""
        c0 = self._view(self.lib.anr_pdf_render_points, n * 160).view(torch.float32).view(n, 40)
        pt = self._view(self.lib.anr_pdf_render_bigpose, n * 32).view(torch.float32).view(n, 8)
        return pt[:, 0:3].clone(), c0[:, 0:3].clone(), c0[:, 3:6].clone()

    def render(self, batch):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters()) and self.net.training:
            raise RuntimeError('aligned_aninerf_pdf: training through this network is not covered; render under '
                               'torch.no_grad() for evaluation')
        with torch.no_grad():
            ret = self.render_device(batch, image_only=bool(self.cfg.get('render_image_only', False)))
        from .renderer import to_host
        return to_host(ret)
