"""Mesh renderer plugin over the aligned_aninerf_pdf network (``lib/networks/renderer/aninerf_mesh_renderer.py`` as
configured by ``configs/aligned_nerf_pdf/aligned_aninerf_pdf_s9p.yaml:141-163``, ``mesh_cfg``):
``renderer_mesh.Renderer`` with ``alpha_points`` replaced by this network's ``get_alpha`` on the device
(``renderer_pdf.Renderer.alpha_points`` / ``anr_pdf_alpha_points``: per batchify chunk of 2048 x 64 points the keep
mask ``pnorm < 0.1`` + forced argmin, the displacement MLP and the density net; the raw density, 0 where dropped).
The volume assembly, marching cubes at ``cfg.mesh_th`` and the optional ``mesh_largest_component`` are
``renderer_mesh``'s, untouched. Batches are those of ``aninerf_pdf_mesh_dataset``: ``pts``, ``inside``, ``wbounds``
and the frame keys ``A``, ``big_A``, ``R``, ``Th``, ``pvertices``, ``weights``, ``poses``.
"""
from . import config as _config
from . import renderer_mesh as _renderer_mesh
from . import renderer_pdf as _renderer_pdf


class Renderer(_renderer_mesh.Renderer):
    def __init__(self, net, cfg=None):
        self.net = net
        self.cfg = cfg if cfg is not None else _config.active()
        self._pdf = _renderer_pdf.Renderer(net, self.cfg)
        self.lib = self._pdf.lib

    def alpha_points(self, wpts, batch, chunk_pts=_renderer_mesh.MESH_CHUNK):
        """get_alpha of (n,3) world points -> (n,) raw density on the device (0 where dropped)."""
        return self._pdf.alpha_points(wpts, batch, chunk_pts=chunk_pts)
