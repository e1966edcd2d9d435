"""GPU: the weight-gradient engines of anr_tgemm.hip (launch_wgrad: k_wgrad in its five operand formats +
k_wgrad_reduce / k_wgrad_reduce_det; launch_wgrad_f32: k_wgrad_f32; launch_wgrad_group: k_wgrad_group,
k_wgrad_dma, k_wgrad_reduce_group) against the float64 reference and bounds of tests/gemm_ref.py, through
the test entry library.

dY / X rows past the device sample count and columns past nout / K are NaN, the partial slabs start as NaN
(a partial nobody wrote shows), dW is a window of a wider non-zero tensor that is accumulated into and whose
other elements must come back bit-identical (gemm_ref.wgrad_buffers).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _gemm_hooks as H
from . import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.name for c in R.WG_CASES]
FORMATS = set()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def slab(dev):
    """wgrad_slab_floats() of workspace (anr_train.h: "slab: wgrad_slab_floats() of workspace") and a guard."""
    n = int(H.lib().anr_test_wgrad_slab_floats())
    return n, torch.empty(n + 1024, device=dev)


def outputs(db):
    return {k: db.get(k).copy() for k, b in db.bufs.items() if b.out}


def call_single(wc, dev, slab, skew_x=False):
    n_slab, t_slab = slab
    d = R.gemm_data(wc.gemm_case())
    bufs, st = R.wgrad_buffers(wc, d)
    db = H.DevBufs(bufs, dev)
    md = H.dev_int(wc.M_dev, dev) if wc.M_dev is not None else None
    g = H.wgrad_desc(wc, st, db, md)
    if skew_x:
        g.X = g.X + 4   # off the 16-B boundary: a product k_wgrad_f32 does not take
    call = H.WGradCall()
    call.mode = H.WG_F32 if wc.fmt == 'f32' else H.WG_SINGLE
    call.det, call.n_host, call.nd = int(wc.det), wc.n, 1
    call.d = C.pointer(g)
    call.slab, call.slab_floats = t_slab.data_ptr(), n_slab

    def run():
        t_slab.fill_(float('nan'))
        rc = H.lib().anr_test_wgrad(C.byref(call), H.stream_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(t_slab[n_slab:]).all(), 'written past the slab'
        return rc
    return db, call, run, (g, md)


@pytest.mark.parametrize('name', IDS)
def test_wgrad(dev, slab, name):
    wc = R.WG_CASES[IDS.index(name)]
    db, call, run, keep = call_single(wc, dev, slab)
    assert run() == H.OK
    if wc.fmt == 'f32':
        assert call.out_f32_fits == 1
    else:
        assert call.out_format == R.WG_FORMATS.index(wc.fmt)
    FORMATS.add((wc.fmt, wc.det))
    rep = db.check_outputs()
    print(name, {k: f'{v[0]:.3f} of the bound, {v[1]:.2e} abs' for k, v in rep.items()})
    if wc.det:   # the fixed-order reduction: a second run on fresh outputs is bit-identical
        first = outputs(db)
        for k in first:
            db.reset(k)
        assert run() == H.OK
        for k, v in first.items():
            assert np.array_equal(v.view(np.uint32), db.get(k).view(np.uint32)), f'{name}: {k} differs between two runs'


def test_formats_covered(dev, slab):
    if not FORMATS:
        for wc in R.WG_CASES:
            db, call, run, keep = call_single(wc, dev, slab)
            assert run() == H.OK
            FORMATS.add((wc.fmt, wc.det))
    assert FORMATS >= {(f, d) for f in R.WG_FORMATS for d in (False, True)} | {('f32', False)}


def test_wgrad_f32_refuses_a_product_that_does_not_fit(dev, slab):
    wc = [c for c in R.WG_CASES if c.fmt == 'f32' and c.n == 385 and c.M_dev == 384][0]
    db, call, run, keep = call_single(wc, dev, slab, skew_x=True)
    assert run() == H.LAUNCHER and call.out_f32_fits == 0
    for k, b in db.bufs.items():
        if b.out:
            assert np.array_equal(db.get(k).view(np.uint32), b.flat.view(np.uint32)), f'{k} touched by a refused launch'


# ---- launch_wgrad_group ---------------------------------------------------------------------------------
def group_need(wc, z):
    tiles = ((wc.nout + 127) // 128) * ((wc.K + 127) // 128)
    return z * tiles * 128 * 128 + (z * 256 if (wc.bsum or wc.bsum2) else 0)


def build_group(dev):
    cases = R.wgrad_group_cases()
    md = H.dev_int(cases[0].M_dev, dev)
    dbs, descs = [], (H.WGradDesc * len(cases))()
    a, b = R.WG_GROUP_SHARED
    bufs_of = {}
    for k, wc in enumerate(cases):
        d = R.gemm_data(wc.gemm_case())
        bufs, st = R.wgrad_buffers(wc, d, shared=bufs_of[a] if k == b else None)
        bufs_of[k] = bufs
        db = H.DevBufs(bufs, dev)
        dbs.append(db)
        if k == b:   # the same dW window and column sums as descriptor a
            for nm in ('dW', 'bsum', 'bsum2'):
                if nm in bufs_of[a]:
                    db.bufs[nm], db.t[nm] = dbs[a].bufs[nm], dbs[a].t[nm]
        descs[k] = H.wgrad_desc(wc, st, db, md)
        if k == b:
            for nm in ('dW', 'bsum', 'bsum2'):
                db.bufs.pop(nm, None)   # checked once, through descriptor a
    return cases, dbs, descs, md


# nz x ANR_WG_DMA x ANR_WG_FILL, alternating the smallest slab region (consecutive groups forced, nz halved
# where a descriptor does not fit) and a region that holds every descriptor at once; the fixed-order
# reduction on three of them
GROUP_PARAMS = [(nz, dma, fill, (i + j + k) % 2 == 0, False) for i, nz in enumerate((8, 16, 64))
                for j, dma in enumerate(('0', '1')) for k, fill in enumerate(('0', '1'))] + \
               [(8, '1', '1', True, True), (64, '0', '1', True, True), (16, '1', '0', False, True)]


@pytest.mark.parametrize('nz,dma,fill,min_slab,det', GROUP_PARAMS)
def test_wgrad_group(dev, monkeypatch, nz, dma, fill, min_slab, det):
    monkeypatch.setenv('ANR_WG_DMA', dma)
    monkeypatch.setenv('ANR_WG_FILL', fill)
    cases, dbs, descs, md = build_group(dev)
    # the smallest region every descriptor fits on its own (8 sample ranges): consecutive groups are forced
    n_slab = max(group_need(wc, 8) for wc in cases) if min_slab else sum(group_need(wc, 64) for wc in cases)
    t_slab = torch.empty(n_slab + 1024, device=dev)
    call = H.WGradCall()
    call.mode, call.det, call.n_host, call.nd, call.nz = H.WG_GROUP, int(det), cases[0].n, len(cases), nz
    call.d = descs
    call.slab, call.slab_floats = t_slab.data_ptr(), n_slab

    def run():
        t_slab.fill_(float('nan'))
        rc = H.lib().anr_test_wgrad(C.byref(call), H.stream_ptr())
        torch.cuda.synchronize()
        assert rc == H.OK
        assert torch.isnan(t_slab[n_slab:]).all(), 'written past the slab region'
    run()
    for k, db in enumerate(dbs):
        for nm, b in db.bufs.items():
            if b.out:
                R.check_out(f'{cases[k].name}:{nm}', b, db.get(nm))
    if det:
        first = [outputs(db) for db in dbs]
        for db in dbs:
            for nm, b in db.bufs.items():
                if b.out:
                    db.reset(nm)
        run()
        for db, f in zip(dbs, first):
            for nm, v in f.items():
                assert np.array_equal(v.view(np.uint32), db.get(nm).view(np.uint32)), nm


def test_wgrad_group_region_too_small(dev):
    cases, dbs, descs, md = build_group(dev)
    n_slab = max(group_need(wc, 8) for wc in cases) - 1
    t_slab = torch.empty(n_slab + 1024, device=dev)
    call = H.WGradCall()
    call.mode, call.n_host, call.nd, call.nz = H.WG_GROUP, cases[0].n, 1, 8
    big = int(np.argmax([group_need(wc, 8) for wc in cases]))
    call.d = C.pointer(descs[big])
    call.slab, call.slab_floats = t_slab.data_ptr(), n_slab
    assert H.lib().anr_test_wgrad(C.byref(call), H.stream_ptr()) == H.LAUNCHER
    torch.cuda.synchronize()
