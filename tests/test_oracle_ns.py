"""CPU: the oracle at other sample counts. restate.render(..., n_samples=128) against golden G15 (the real
reference run with `N_samples 128`, tools/gen_golden_nsamples.py), and the properties of the small batches the
GPU tests of the 128 / 192 / 256-sample render rely on (tests/_ns_common.py), so that those are not vacuous."""
import numpy as np
import pytest
import torch

from oracle import restate

from ._common import assert_golden_equal, golden, oracle_params, to_torch
from ._ns_common import CHUNK, g15_batch, keep_of, mmsk_small_batch, oracle_mmsk, oracle_small

# the grazing chunk's forced sample: in segment 0 once, in segment 1 twice
GRAZING_S = {128: 48, 192: 73, 256: 97}


def test_g15_oracle_matches_reference():
    g = golden('g15_nsamples')
    n = int(g['n_samples'])
    assert n == 128
    b, mask = g15_batch()
    assert np.array_equal(mask, g['mask']) and int(mask.sum()) == 2088
    with torch.no_grad():
        ret = restate.render(oracle_params(), to_torch(b), n_samples=n, chunk=2048)
    assert ret['raw'].shape == (1, 2088 * n, 4)
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        assert_golden_equal(ret[k].numpy(), g['out_' + k], err_msg=k)
    keep = keep_of(ret['raw']).numpy()
    assert np.array_equal(np.packbits(keep), g['keep_bits'])
    assert_golden_equal(ret['raw'][0, :, 3].numpy()[keep], g['kept_alpha'], err_msg='kept_alpha')
    assert ret['pbw'].shape[1] == int(g['bw_rows']) == ret['tbw'].shape[1]
    assert_golden_equal(ret['pbw'][0, g['bw_sample_idx']].numpy(), g['pbw_sample'], err_msg='pbw')
    assert_golden_equal(ret['tbw'][0, g['bw_sample_idx']].numpy(), g['tbw_sample'], err_msg='tbw')
    # one full chunk, and a 40-ray grazing chunk that keeps exactly its forced argmin sample
    per_ray = keep.reshape(2088, n)
    assert per_ray[:2048].sum() > 50000 and per_ray[2048:].sum() == 1


@pytest.mark.parametrize('n', [128, 192, 256])
def test_small_batch_is_not_vacuous(n):
    ret, ids = oracle_small(n)
    keep = keep_of(ret['raw']).view(29, n)
    per_chunk = [int(keep[i:i + CHUNK].sum()) for i in range(0, 29, CHUNK)]
    assert per_chunk[2] == 1 and min(per_chunk[0], per_chunk[1], per_chunk[3]) > 100, per_chunk
    s = int(torch.nonzero(keep[16:24].reshape(-1))[0]) % n
    assert s == GRAZING_S[n], s
    segs = keep.view(29, n // 64, 64).any(-1).sum(-1)
    assert int((segs > 1).sum()) >= 15, segs
    # the rows: some but not all kept samples, in frame order, every one a kept sample
    assert 0 < ids.numel() == ret['pbw'].shape[1] < int(keep.sum())
    assert bool((ids[1:] > ids[:-1]).all()) and bool(keep.reshape(-1)[ids].all())


def test_small_batch_stratified_differs():
    a, _ = oracle_small(128)
    b, _ = oracle_small(128, True)
    assert not torch.equal(keep_of(a['raw']), keep_of(b['raw'])) or not torch.equal(a['depth_map'], b['depth_map'])


def test_mmsk_small_batch_has_an_invisible_chunk():
    b, mask = mmsk_small_batch()
    assert mask.all() and mask.size == 24
    ret, raw, inside = oracle_mmsk(128)
    vis = inside.view(24, 128)
    keep = keep_of(raw).view(24, 128)
    assert not bool(vis[16:].any()) and not bool(keep[16:].any())  # the third chunk: nothing visible, nothing kept
    assert int(keep[:8].sum()) > 0 and int(keep[8:16].sum()) > 0
    assert not bool(keep[~vis].any())
    assert bool((~vis[:16]).any())  # the filter removes samples in the visible chunks too
