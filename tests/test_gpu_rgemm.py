"""GPU: the bf16 row GEMM (launch_rgemm, anr_tgemm.hip: the five dispatched k_rgemm variants) against the
float64 reference and bounds of tests/gemm_ref.py, through the test entry library.

The weight images are built by the test as plain bf16 rows, k-contiguous, segments zero-padded to 64, with
hi and lo images for x3 (RGemmSeg's comment in anr_train.h); one case per direction goes through
wimg_pack / wimg_view on a real layer tensor to tie the two together. Buffers carry NaN where the contract
says nothing is consumed and a sentinel around the outputs (gemm_ref.rgemm_buffers). bf16 outputs are held
to [rne_bf16(ref - b), rne_bf16(ref + b)], no relative tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _gemm_hooks as H
from . import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.name for c in R.RG_CASES]
DISPATCHED = set()   # (variant, vec_out, vec16, cbf)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def run_case(rc, dev):
    d = R.gemm_data(rc.gemm_case())
    bufs, st = R.rgemm_buffers(rc, d)
    db = H.DevBufs(bufs, dev)
    md = H.dev_int(rc.M_dev, dev) if rc.M_dev is not None else None
    g = H.rgemm_desc(rc, st, db, md)
    assert H.lib().anr_test_rgemm(C.byref(g), H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    vec_out = rc.ldc_kind != 'odd' and rc.N % 4 == 0
    assert g.out_variant == R.RG_VARIANTS.index(rc.variant)
    assert g.out_vec_out == int(vec_out)
    assert g.out_vec16 == int(vec_out and rc.cbf and rc.ldc_kind == 'v16')
    DISPATCHED.add((rc.variant, g.out_vec_out, g.out_vec16, int(rc.cbf)))
    return db


@pytest.mark.parametrize('name', IDS)
def test_rgemm(dev, name):
    rc = R.RG_CASES[IDS.index(name)]
    rep = run_case(rc, dev).check_outputs()
    print(name, {k: f'{v[0]:.3f} of the bound, {v[1]:.2e} abs' for k, v in rep.items()})


def test_dispatch_coverage(dev):
    """All five kernel variants ran, each store path (scalar, 16-B fp32 / 8-B bf16, 16-B bf16) among them."""
    if len(DISPATCHED) == 0:
        for rc in R.RG_CASES:
            run_case(rc, dev)
    assert {t[0] for t in DISPATCHED} == set(R.RG_VARIANTS)
    for var in R.RG_VARIANTS:
        assert {t[1] for t in DISPATCHED if t[0] == var} == {0, 1}, var
        if var != 'x3':
            assert {(t[2], t[3]) for t in DISPATCHED if t[0] == var} >= {(1, 1), (0, 1), (0, 0)}, var
    print('dispatched:', sorted(DISPATCHED))


# ---- wimg_pack / wimg_view on real layer tensors ------------------------------------------------------
# (tensor index, out, in) of the Conv1d weights the images hold (anr_tgemm.hip kWDesc; state_dict order)
WIMG_TENSORS = [(28, 256, 191), (30, 256, 256), (32, 256, 256), (34, 256, 256), (36, 256, 256), (38, 256, 447),
                (40, 256, 256), (42, 256, 256), (44, 24, 256), (1, 256, 63), (3, 256, 256), (5, 256, 256), (7, 256, 256),
                (9, 256, 256), (11, 256, 319), (13, 256, 256), (15, 256, 256), (17, 1, 256), (19, 256, 256),
                (21, 256, 384), (23, 128, 283), (25, 3, 128)]


@pytest.fixture(scope='module')
def wimg(dev):
    """Every weight the images hold, random in [-1, 1], packed once by wimg_pack."""
    L = H.lib()
    rng = np.random.default_rng(77)
    W = {t: rng.uniform(-1, 1, (n, k)).astype(np.float32) for t, n, k in WIMG_TENSORS}
    Wd = {t: torch.from_numpy(w).to(dev) for t, w in W.items()}
    table = (H.vp * 65)()   # ANR_NUM_TENSORS (46) network tensors, then the novel_pose_bw ones: absent (NULL)
    for t, w in Wd.items():
        table[t] = w.data_ptr()
    img = torch.zeros(int(L.anr_test_wimg_bytes()), dtype=torch.uint8, device=dev)
    assert L.anr_test_wimg_pack(table, img.data_ptr(), H.stream_ptr()) == 0
    torch.cuda.synchronize()
    return W, Wd, table, img


@pytest.mark.parametrize('x3', [0, 1])
@pytest.mark.parametrize('which', ['fwd-two-segments', 'bwd'])
def test_rgemm_on_packed_images(dev, wimg, which, x3):
    """pts_linears.5 forward (tensor 11: the skip concatenation's two segments, 63 + 256 inputs) and
    view_fc's input gradient (tensor 23, columns 256..282: 27 outputs from image rows c0 .. c0 + 26)."""
    W, Wd, table, img = wimg
    L = H.lib()
    M = 129
    rng = np.random.default_rng(5 + x3)
    if which == 'fwd-two-segments':
        t, N, segs = 11, 256, [(0, 63), (63, 256)]
        Bs = [W[t][:, c0:c0 + K].T for c0, K in segs]
        views = [(c0, K, 0) for c0, K in segs]
    else:
        t, N, segs = 23, 27, [(256, 128)]
        Bs = [W[t][:, 256:283]]
        views = [(256, 128, 1)]
    rc = R.RCase(f'wimg-{which}-{x3}', M, M - 1, N, tuple(K for _, K in segs), (N,) * len(segs), (0,) * len(segs),
                 variant='x3' if x3 else 'f32', bias=True, relu=True, ldc_kind='v16')
    gc = rc.gemm_case()
    A = [rng.uniform(-1, 1, (M, K)).astype(np.float32) for _, K in segs]
    bias = rng.uniform(-1, 1, N).astype(np.float32)
    z = np.zeros((M, N), np.float32)
    d = R.GemmData()
    d.A, d.B, d.bias, d.c0, d.mask = A, [np.ascontiguousarray(b) for b in Bs], bias, z, z
    d.ref = R.gemm_eval(gc, d.A, d.B, bias, z, np.zeros((2, M), np.float32), z, z)
    bufs, st = R.rgemm_buffers(rc, d)
    db = H.DevBufs(bufs, dev)
    md = H.dev_int(rc.M_dev, dev)
    g = H.rgemm_desc(rc, st, db, md)
    for s, (c0, K, bwd) in enumerate(views):   # the packed image in place of the test-built one
        v = H.WView()
        assert L.anr_test_wimg_view(img.data_ptr(), table, Wd[t].data_ptr(), c0, K, bwd, C.byref(v)) == 1
        g.B[s], g.ldb[s], g.lo_off[s], g.bcol[s], g.rows[s] = v.B, v.ldb, v.lo_off, v.bcol, v.rows
        assert v.rows >= N and v.bcol % 64 == 0
    assert L.anr_test_rgemm(C.byref(g), H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    rep = db.check_outputs()
    print(rc.name, rep)
