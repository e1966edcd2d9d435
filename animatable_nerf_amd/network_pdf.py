"""aligned_aninerf_pdf network plugin (the extended paper's NeRF with a pose-dependent displacement field;
``configs/aligned_nerf_pdf/*``) with the reference parameter layout
(``lib/networks/bw_deform/aligned_aninerf_pdf_network.py:13-39, 177-377``).

Like ``network_lbw.Network`` the modules own the parameters under the reference state_dict names, shapes and
order (so ``load_network(strict=True)`` reads a reference ``latest.pth``); the eval render runs in the HIP library
(``renderer_pdf.Renderer``). ``TPoseHuman`` is aligned_aninerf_lbw's, module for module.

``get_alpha`` runs on the device too (``renderer_pdf.Renderer.alpha_points``). Not covered: training and autograd
through this network, ``cfg.init_sdf``, ``Network.forward`` over free samples.
"""
import torch
import torch.nn as nn

from . import config as _config
from .network_lbw import TPoseHuman


class Network(nn.Module):
    """aligned_aninerf_pdf_network.Network: tpose_human + resd_latent (num_latent_code, 128; unused by the forward)
    + resd_linears (135 -> 8 x 256, skip 391 at 5) + resd_fc (3)."""

    TENSOR_ORDER_LEN = 62

    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg if cfg is not None else _config.active()
        self.__dict__['_anr_cfg'] = cfg
        if not cfg.get('tpose_viewdir', True):
            raise ValueError('network_pdf: cfg.tpose_viewdir False is not supported (the view directions are warped '
                             'to the big pose on the device)')
        if not cfg.get('color_with_viewdir', True):
            raise ValueError('network_pdf: cfg.color_with_viewdir False is not supported')
        if cfg.get('init_sdf', False):
            raise ValueError('network_pdf: cfg.init_sdf is not supported (this network has no sdf_network to load)')
        nlc = int(cfg.get('num_latent_code', -1))
        if nlc < 0:
            nlc = int(cfg.num_train_frame)  # config.py:144-145
        self.tpose_human = TPoseHuman(nlc)
        self.resd_latent = nn.Embedding(nlc, 128)
        self.actvn = nn.ReLU()
        self.skips = [4]
        self.resd_linears = nn.ModuleList(
            [nn.Conv1d(135, 256, 1)] + [nn.Conv1d(256 + 135 if i == 4 else 256, 256, 1) for i in range(7)])
        self.resd_fc = nn.Conv1d(256, 3, 1)
        self.resd_fc.bias.data.fill_(0)

    def tensors(self):
        """The 62 tensors of the C-ABI order (include/aninerf.h ``anr_pdf_params``) = the state_dict order."""
        ts = [t for _, t in self.named_parameters()]
        assert len(ts) == self.TENSOR_ORDER_LEN, len(ts)
        return ts

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop('_anr_renderer', None)  # a copy builds its own device renderer
        return state

    def forward(self, wpts, viewdir, dists, batch):
        raise NotImplementedError('network_pdf: Network.forward over free samples is not covered; render whole '
                                  'frames with renderer_pdf.Renderer(net).render(batch)')

    def _device(self):
        r = self.__dict__.get('_anr_renderer')
        if r is None:
            from .renderer_pdf import Renderer
            r = Renderer(self, self.__dict__['_anr_cfg'])
            self.__dict__['_anr_renderer'] = r
        return r

    def get_alpha(self, wpts, batch):
        """Network.get_alpha (:140-174): (n,3) world points of ONE call (one keep mask with its forced argmin over all
        of them) -> (n,) raw density, 0 where a point is dropped. Eval only, on the device."""
        n = int(wpts.reshape(-1, 3).shape[0])
        with torch.no_grad():
            return self._device().alpha_points(wpts, batch, chunk_pts=max(64, (n + 63) // 64 * 64))
