"""Test infrastructure only. Child process of tests/test_gpu_pdf.py's batching test: renders G18 with
renderer_pdf.Renderer in the three precisions under whatever ANR_PDF_BATCH the parent set, and saves every output
and the row ids to the .npz named on the command line.  python -m tests._pdf_child OUT.npz"""
import sys

import numpy as np
import torch

from tests import pdf_ref
from tests._common import golden


def main(out):
    from animatable_nerf_amd.renderer_pdf import Renderer
    dev = torch.device('cuda:0')
    g = golden('g18_pdf_tiny')
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    res = {}
    for prec in ('fp32', 'bf16x3', 'bf16x6'):
        cfg = pdf_ref.pdf_cfg(render_precision=prec)
        net = pdf_ref.make_net(P, dev, cfg)
        net.train()
        r = Renderer(net, cfg)
        ret = r.render_device({k: v.clone() for k, v in batch.items()})
        for k, v in ret.items():
            res[prec + '_' + k] = v.cpu().numpy()
        res[prec + '_ids'] = r.last_row_ids.cpu().numpy()
    np.savez(out, **res)


if __name__ == '__main__':
    main(sys.argv[1])
