"""GPU: the LDS-resident layer GEMM (anr_lgemm.hip: lgemm_supported, lgemm_image_bytes, lgemm_pack, lgemm_run;
the fp32 and split-bf16 k_lgemm instantiations, the fused head, the softplus forward and backward forms and
the a_softplus_w activations) against the float64 reference and bounds of tests/gemm_ref.py, through the
test entry library, with `cus` passed as 2 and as the device's count.

k_lgemm runs the instantiated layer shapes only (lg_dispatch), so the cases are the members of
M x N x K = {1, 127, 129, 700} x {1, 4, 39, 256, 264} x {3, 39, 217, 256} (+ the 63 + 256 skip layer) that
lgemm_supported admits, and M = 1100, the smallest size at which a wave of the 2-CU launch takes a second
tile. Activation rows are a_rs >= K rounded up to 8 wide with NaN past K ("4-groups wholly past K read
column 0; both masked later"), the weight image buffer has a guard that must stay untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _gemm_hooks as H
from . import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.name for c in R.LG_CASES]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def prepare(c, dev, cus):
    d = R.gemm_data(c)
    bufs, st = R.gemm_buffers(d)
    db = H.DevBufs(bufs, dev)
    g = H.gemm_desc(d, bufs, st, db, {})
    g.cus = cus
    # supported-check and image size first (no image given: nothing launched)
    assert H.lib().anr_test_lgemm(C.byref(g), H.stream_ptr()) == H.E_NULL
    nbytes = int(g.out_image_bytes)
    assert nbytes > 0
    img = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
    g.img, g.img_bytes = img.data_ptr(), nbytes
    return d, db, g, img, nbytes


@pytest.mark.parametrize('cus', ['2', 'device'])
@pytest.mark.parametrize('name', IDS)
def test_lgemm(dev, name, cus):
    c = R.LG_CASES[IDS.index(name)]
    ncu = 2 if cus == '2' else torch.cuda.get_device_properties(dev).multi_processor_count
    d, db, g, img, nbytes = prepare(c, dev, ncu)
    assert R.gemm_threshold_violations(d) == 0
    assert H.lib().anr_test_lgemm(C.byref(g), H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    assert (img[nbytes:] == 0xFF).all(), 'written past the weight image'
    rep = db.check_outputs()
    print(name, cus, {k: f'{v[0]:.3f} of the bound, {v[1]:.2e} abs' for k, v in rep.items()})


def test_image_too_small_is_refused(dev):
    c = R.LG_CASES[0]
    d, db, g, img, nbytes = prepare(c, dev, 2)
    g.img_bytes = nbytes - 1
    assert H.lib().anr_test_lgemm(C.byref(g), H.stream_ptr()) == H.E_SLAB


def test_pack_batch_equals_two_packs(dev):
    """lgemm_pack_batch of two images byte for byte what two lgemm_pack calls write (an fp32 image with a
    partial last k-step and a split-bf16 two-segment one)."""
    L = H.lib()
    a = [c for c in R.LG_CASES if c.name.startswith('lg-fp32-spd-d-divpost')][0]
    b = [c for c in R.LG_CASES if c.name.startswith('lg-x3-seg2-bias-relu')][0]
    single, descs, keep = [], (H.GemmDesc * 2)(), []
    for i, c in enumerate((a, b)):
        d, db, g, img, nbytes = prepare(c, dev, 2)
        assert L.anr_test_lgemm(C.byref(g), H.stream_ptr()) == H.OK   # lgemm_pack (and a run)
        torch.cuda.synchronize()
        single.append(img[:nbytes].cpu().numpy().copy())
        keep.append((db, img))
        descs[i] = g
    imgs = [torch.full((s.size + 256,), 0xFF, dtype=torch.uint8, device=dev) for s in single]
    ptrs = (H.vp * 2)(imgs[0].data_ptr(), imgs[1].data_ptr())
    dd = torch.zeros(4096, dtype=torch.uint8, device=dev)
    ds = torch.zeros(8, dtype=torch.int64, device=dev)
    assert L.anr_test_lgemm_pack_batch(descs, 2, ptrs, dd.data_ptr(), ds.data_ptr(), H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    for s, t in zip(single, imgs):
        got = t.cpu().numpy()
        assert np.array_equal(got[:s.size], s)
        assert (got[s.size:] == 0xFF).all()
