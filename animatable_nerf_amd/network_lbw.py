"""aligned_aninerf_lbw network plugin (the extended paper's KNN-skinned NeRF; ``configs/aligned_nerf_lbw/*``) with
the reference parameter layout (``lib/networks/bw_deform/aligned_aninerf_lbw_network.py:11-38, 190-206, 230-401``).

Like ``network_sdf.Network`` the modules own the parameters under the reference state_dict names, shapes and
order (so ``load_network(strict=True)`` reads a reference ``latest.pth``); the eval render runs in the HIP library
(``renderer_lbw.Renderer``). Weight-normed layers keep the ``weight_g`` / ``weight_v`` pair of
``nn.utils.weight_norm``; the effective weight is formed on the device per render call.

Not covered: training and autograd through this network, ``cfg.test_novel_pose`` (``novel_pose_bw`` is only
carried so that such checkpoints load), ``get_alpha`` / mesh extraction, ``Network.forward`` over free samples.
"""
import torch
import torch.nn as nn

from . import config as _config
from .network_sdf import WNLinear


class NeRFNetwork(nn.Module):
    """aligned_aninerf_lbw_network.py:263-352: gamma_6 (39) -> 8 x 256 softplus(beta 100), lin3 out 217, skip
    [x, gamma]/sqrt(2) into lin4, lin8 -> 1 + 256 (density, feature)."""
    DIMS = [(39, 256), (256, 256), (256, 256), (256, 217), (256, 256), (256, 256), (256, 256), (256, 256),
            (256, 257)]

    def __init__(self):
        super().__init__()
        for l, (i, o) in enumerate(self.DIMS):
            setattr(self, f'lin{l}', WNLinear(i, o))


class ColorNetwork(nn.Module):
    """aligned_aninerf_lbw_network.py:355-436 (mode 'idr', no normal): 286 -> 256 -> 256 -> 256 || latent 128
    -> 256 -> 3."""

    def __init__(self, num_latent_code):
        super().__init__()
        self.color_latent = nn.Embedding(num_latent_code, 128)
        for l, (i, o) in enumerate([(286, 256), (256, 256), (256, 256), (384, 256), (256, 3)]):
            setattr(self, f'lin{l}', WNLinear(i, o))


class TPoseHuman(nn.Module):
    def __init__(self, num_latent_code):
        super().__init__()
        self.nerf_network = NeRFNetwork()
        self.color_network = ColorNetwork(num_latent_code)


def _bw_linears():
    return nn.ModuleList([nn.Conv1d(191, 256, 1)] + [nn.Conv1d(256 + 191 if i == 4 else 256, 256, 1) for i in range(7)])


class BackwardBlendWeight(nn.Module):
    """aligned_aninerf_lbw_network.py:190-206: parameters only (``cfg.test_novel_pose`` is not rendered)."""

    def __init__(self, num_eval_frame):
        super().__init__()
        self.bw_latent = nn.Embedding(num_eval_frame, 128)
        self.actvn = nn.ReLU()
        self.bw_linears = _bw_linears()
        self.bw_fc = nn.Conv1d(256, 24, 1)


class Network(nn.Module):
    """aligned_aninerf_lbw_network.Network: tpose_human + bw_latent (num_train_frame + 1) + bw_linears (191 ->
    8 x 256, skip 447 at 5) + bw_fc (24) [+ novel_pose_bw under cfg.aninerf_animation]."""

    TENSOR_ORDER_LEN = 62

    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg if cfg is not None else _config.active()
        self.__dict__['_anr_cfg'] = cfg
        if not cfg.get('tpose_viewdir', True):
            raise ValueError('network_lbw: cfg.tpose_viewdir False is not supported (the view directions are warped '
                             'to the big pose on the device)')
        if not cfg.get('color_with_viewdir', True):
            raise ValueError('network_lbw: cfg.color_with_viewdir False is not supported')
        nlc = int(cfg.get('num_latent_code', -1))
        if nlc < 0:
            nlc = int(cfg.num_train_frame)  # config.py:144-145
        self.tpose_human = TPoseHuman(nlc)
        self.bw_latent = nn.Embedding(int(cfg.num_train_frame) + 1, 128)
        self.actvn = nn.ReLU()
        self.skips = [4]
        self.bw_linears = _bw_linears()
        self.bw_fc = nn.Conv1d(256, 24, 1)
        if cfg.get('aninerf_animation', False):
            self.novel_pose_bw = BackwardBlendWeight(int(cfg.num_eval_frame))

    def tensors(self):
        """The 62 tensors of the C-ABI order (include/aninerf.h ``anr_lbw_params``) = the state_dict order
        without the trailing ``novel_pose_bw.*``."""
        ts = [t for n, t in self.named_parameters() if not n.startswith('novel_pose_bw.')]
        assert len(ts) == self.TENSOR_ORDER_LEN, len(ts)
        return ts

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop('_anr_renderer', None)  # a copy builds its own device renderer
        return state

    def _device(self):
        r = self.__dict__.get('_anr_renderer')
        if r is None:
            from .renderer_lbw import Renderer
            r = Renderer(self, self.__dict__['_anr_cfg'])
            self.__dict__['_anr_renderer'] = r
        return r

    def forward(self, wpts, viewdir, dists, batch):
        raise NotImplementedError('network_lbw: Network.forward over free samples is not covered; render whole '
                                  'frames with renderer_lbw.Renderer(net).render(batch)')

    def get_alpha(self, wpts, batch):
        raise NotImplementedError('network_lbw: get_alpha / mesh extraction is not covered')
