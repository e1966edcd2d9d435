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

CHUNK = 2048
ALPHA_CHUNK = 2048 * 64  # aninerf_mesh_renderer.py:36
RAY_KEYS = ('ray_o', 'ray_d', 'near', 'far')
FRAME_KEYS = ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses', 'tbounds')


def _f32(t, device):
    return t.to(device=device, dtype=torch.float32).contiguous()


def _pdf_precision(cfg):
    rprec = cfg.get('render_precision', 'fp32')
    precs = {'fp32': _lib.FP32, 'bf16x3': _lib.BF16X3, 'bf16x6': _lib.BF16X6}
    if rprec not in precs:
        raise ValueError(f"renderer_pdf: render_precision must be one of {sorted(precs)}, got {rprec!r}")
    return precs[rprec]


class Renderer:
    widens_tbounds = True      # per chunk, in place (aligned_aninerf_pdf_network.py:125-127)
    visibility_filter = False  # renderer_pdf_mmsk: the training-view visibility filter of tpose_renderer_mmsk

    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg if cfg is not None else _config.active()
        self.lib = _lib.load()
        self._ws = None
        self._pcache = None
        self.last_counts = None

    def device(self):
        return next(self.net.parameters()).device

    def params(self):
        key = tuple(t.data_ptr() for t in self.net.tensors())
        if self._pcache is not None and self._pcache[0] == key:
            return self._pcache[1]
        ts = [t.detach() for t in self.net.tensors()]
        if ts[0].device.type != 'cuda':
            raise RuntimeError('Renderer: the network must be on a GPU (net.cuda()); there is no CPU path')
        p = _lib.PdfParams()
        for i, t in enumerate(ts):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError('Renderer: parameters must be contiguous float32')
            p.t[i] = t.data_ptr()
        self._pcache = (key, p)
        return p

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
        fr = {k: _f32(batch[k], dev) for k in FRAME_KEYS}
        tr = None if t_rand is None else _f32(t_rand, dev).reshape(R, ns)
        li = batch['latent_index'].to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        f = _lib.PdfFrame()
        for k in FRAME_KEYS:
            setattr(f, k, fr[k].data_ptr())
        f.n_verts = fr['pvertices'].shape[-2]
        f.latent_index = li.data_ptr()
        if self.visibility_filter:  # tpose_renderer_mmsk.py:14-57 on the device
            views = {k: _f32(batch[k], dev) for k in ('Ks', 'RT')}
            views['msks'] = batch['msks'].to(device=dev, dtype=torch.uint8).contiguous()
            f.n_views = int(views['Ks'].shape[1])
            f.Ks, f.RT, f.msks = views['Ks'].data_ptr(), views['RT'].data_ptr(), views['msks'].data_ptr()
            f.img_h, f.img_w = int(batch['H']), int(batch['W'])
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
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != dev:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ws = self._ws
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
        keys = ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses')
        fr = {k: _f32(batch[k], dev) for k in keys}
        f = _lib.PdfFrame()
        for k in keys:
            setattr(f, k, fr[k].data_ptr())
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

    _aws = None

    def _view(self, fn, nbytes):
        R, o, img = self._last
        addr = fn(_lib.ptr(self._ws), R, ctypes.byref(o), img)
        if not addr:
            raise RuntimeError('renderer_pdf: no workspace view')
        off = addr - self._ws.data_ptr()
        return self._ws[off:off + nbytes]

    def knn_records(self):
        """(R*64, 8) int32 view of the last render's KNN records (anr_pdf_render_knn): w0..w4 float bits, then the
        five vertex indices packed as i0 | i1 << 16, i2 | i3 << 16, i4 (tests, debugging)."""
        R = self._last[0]
        return self._view(self.lib.anr_pdf_render_knn, R * 64 * 32).view(torch.int32).view(R * 64, 8)

    def kept_ids(self):
        """(n',) int32 sample ids (ray * 64 + sample) the last render kept, in order (tests, debugging)."""
        n = int(self._view(self.lib.anr_pdf_render_counts, 4).view(torch.int32).item())
        return self._view(self.lib.anr_pdf_render_kept, n * 4).view(torch.int32).clone()

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
