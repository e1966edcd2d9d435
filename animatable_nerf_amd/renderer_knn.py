"""What the renderers of the KNN-skinned networks share (``renderer_sdf``, ``renderer_lbw``, ``renderer_pdf``): the
float32 staging of batch tensors, the ``cfg.render_precision`` map, and a base class with the parameter-struct cache,
the workspace reuse, the frame-struct filling and the workspace views the tests and tools read."""
import ctypes

import torch

from . import _lib
from . import config as _config


def _f32(t, device):
    return t.to(device=device, dtype=torch.float32).contiguous()


def render_precision(cfg, who=''):
    """cfg.render_precision -> include/aninerf.h anr_render_opts.precision; ``who`` prefixes the error text."""
    rprec = cfg.get('render_precision', 'fp32')
    precs = {'fp32': _lib.FP32, 'bf16x3': _lib.BF16X3, 'bf16x6': _lib.BF16X6}
    if rprec not in precs:
        raise ValueError(f"{who}render_precision must be one of {sorted(precs)}, got {rprec!r}")
    return precs[rprec]


class KnnRenderer:
    """Derived classes set ``params_type`` (the ctypes parameter struct), ``name`` (error texts) and the library's
    accessors ``counts_fn`` / ``knn_fn`` / ``kept_fn`` by name; ``self._last`` holds the last render's accessor
    arguments ``(R, opts, *extra)``."""
    params_type = None
    name = 'renderer'
    counts_fn = knn_fn = kept_fn = None

    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg if cfg is not None else _config.active()
        self.lib = _lib.load()
        self._ws = None
        self._pcache = None  # (parameter pointers, parameter struct) of the last call
        self.last_counts = None

    def device(self):
        return next(self.net.parameters()).device

    def params(self):
        # per-call host work: the struct is rebuilt (detach + checks of every tensor, ~0.1 ms of Python that
        # the GPU waits out at every training step's host sync) only when a parameter moved
        key = tuple(t.data_ptr() for t in self.net.tensors())
        if self._pcache is not None and self._pcache[0] == key:
            return self._pcache[1]
        ts = [t.detach() for t in self.net.tensors()]
        if ts[0].device.type != 'cuda':
            raise RuntimeError('Renderer: the network must be on a GPU (net.cuda()); there is no CPU path')
        p = self.params_type()
        for i, t in enumerate(ts):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError('Renderer: parameters must be contiguous float32')
            p.t[i] = t.data_ptr()
        self._pcache = (key, p)
        return p

    def workspace(self, nbytes, dev):
        """The renderer's workspace, reallocated only when it is too small or on another device."""
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    @staticmethod
    def fill_frame(f, batch, keys, dev):
        """Frame struct fields ``keys`` from the batch as float32 device tensors, ``n_verts`` and (when the batch
        has one) ``latent_index`` -> the tensors, which the caller keeps alive over the call."""
        fr = {k: _f32(batch[k], dev) for k in keys}
        for k in keys:
            setattr(f, k, fr[k].data_ptr())
        f.n_verts = fr['pvertices'].shape[-2]
        if 'latent_index' in batch:
            fr['latent_index'] = batch['latent_index'].to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            f.latent_index = fr['latent_index'].data_ptr()
        return fr

    @staticmethod
    def fill_views(f, batch, dev):
        """The visibility filter's training views (tpose_renderer_mmsk.py:14-57 on the device) -> their tensors."""
        views = {k: _f32(batch[k], dev) for k in ('Ks', 'RT')}
        views['msks'] = batch['msks'].to(device=dev, dtype=torch.uint8).contiguous()
        f.n_views = int(views['Ks'].shape[1])
        f.Ks, f.RT, f.msks = views['Ks'].data_ptr(), views['RT'].data_ptr(), views['msks'].data_ptr()
        f.img_h, f.img_w = int(batch['H']), int(batch['W'])
        return views

    def _view(self, fn, nbytes):
        R, o, *extra = self._last
        addr = fn(_lib.ptr(self._ws), R, ctypes.byref(o), *extra)
        if not addr:
            raise RuntimeError(f'{self.name}: no workspace view')
        off = addr - self._ws.data_ptr()
        return self._ws[off:off + nbytes]

    def knn_records(self):
        """(R*64, 8) int32 view of the last render's (first-search) KNN records: w0..w4 float bits, then the five
        vertex indices packed as i0 | i1 << 16, i2 | i3 << 16, i4 (tests, debugging)."""
        R = self._last[0]
        return self._view(getattr(self.lib, self.knn_fn), R * 64 * 32).view(torch.int32).view(R * 64, 8)

    def kept_ids(self):
        """(n',) int32 sample ids (ray * 64 + sample) the last render kept, in order (tests, debugging)."""
        n = int(self._view(getattr(self.lib, self.counts_fn), 4).view(torch.int32).item())
        return self._view(getattr(self.lib, self.kept_fn), n * 4).view(torch.int32).clone()
