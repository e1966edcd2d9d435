"""Shared by the N_samples = 128 / 192 / 256 tests: the small four-chunk batch, the G15 batch and the oracle
renders with the sample ids of their alpha_ind rows (each computed once per process)."""
import functools

import numpy as np
import torch

from oracle import restate

from ._common import batch_np, golden, mmsk_batch_np, oracle_params, scene, to_torch

CHUNK = 8
# G2's rays [0:16] + [4096:4104] + [16:21]: 29 hits in four chunks of 8: box, box, grazing, a partial box chunk of 5
SMALL = (slice(0, 16), slice(4096, 4104), slice(16, 21))
G15_RAYS = (slice(0, 2048), slice(4096, 4136))


def keep_of(raw):
    return raw[0, :, :3].abs().sum(-1) != 0


def _g2(slices):
    g = golden('g2_chunks')
    return (np.concatenate([g['ray_o'][s] for s in slices]), np.concatenate([g['ray_d'][s] for s in slices]))


@functools.lru_cache(maxsize=1)
def small_batch():
    b, mask = batch_np(scene(0.05), *_g2(SMALL))
    assert mask.all() and mask.size == 29
    return b


@functools.lru_cache(maxsize=1)
def g15_batch():
    b, mask = batch_np(scene(0.05), *_g2(G15_RAYS))
    return b, mask


def small_t_rand(n):
    return torch.rand((29, n), generator=torch.Generator().manual_seed(11))


class RowTrace:
    """wraps restate.network_forward during an oracle render: per reference chunk, the sample ids (frame
    order) of the alpha_ind rows"""

    def __init__(self):
        self.fn, self.base, self.ids = restate.network_forward, 0, []

    def __call__(self, P, wpts, viewdir, dists, batch, trace=None, **kw):
        t = {}
        ret = self.fn(P, wpts, viewdir, dists, batch, trace=t, **kw)
        kept = torch.nonzero(t['pind'][0])[:, 0] + self.base
        self.ids.append(kept[t['alpha_ind'][0]])
        self.base += wpts.shape[0]
        return ret


@functools.lru_cache(maxsize=None)
def oracle_small(n, stratified=False):
    """restate.render of the small batch at n samples, chunk 8 -> (outputs, alpha_ind sample ids). Read-only."""
    tr = RowTrace()
    restate.network_forward = tr
    try:
        with torch.no_grad():
            ret = restate.render(oracle_params(), to_torch(small_batch()), n_samples=n, chunk=CHUNK,
                                 t_rand=small_t_rand(n) if stratified else None)
    finally:
        restate.network_forward = tr.fn
    return ret, torch.cat(tr.ids)


# rays for the visibility filter at chunk 8: G9's chunk rays [0:16] (two chunks with visible samples) and
# [2048:2056] (its chunk with no visible sample)
MMSK = (slice(0, 16), slice(2048, 2056))


@functools.lru_cache(maxsize=1)
def mmsk_small_batch():
    g = golden('g9_mmsk')
    ro = np.concatenate([g['chunks_ray_o'][s] for s in MMSK])
    rd = np.concatenate([g['chunks_ray_d'][s] for s in MMSK])
    b, mask = mmsk_batch_np(ro, rd)
    return b, mask


@functools.lru_cache(maxsize=1)
def oracle_mmsk(n=128):
    b, _ = mmsk_small_batch()
    tr = {}
    with torch.no_grad():
        ret = restate.render_mmsk(oracle_params(), to_torch(b), chunk=CHUNK, n_samples=n, trace=tr)
    return ret, torch.cat(tr['raw'], dim=1), torch.cat([i.reshape(1, -1) for i in tr['inside']], dim=1)
