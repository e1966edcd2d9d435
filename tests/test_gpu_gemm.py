"""GPU: the generic strided GEMM (launch_gemm / launch_gemm_det, anr_gemm.hip: k_gemm_t, k_gemm_b and their
epilogues) against the float64 reference and the derived bounds of tests/gemm_ref.py, through the test
entry library (tests/csrc/anr_testapi.hip), at the smallest shapes that cross each tile edge.

Every operand and output lives inside a larger allocation (gemm_ref.gemm_buffers): NaN wherever the
contract says the kernel consumes nothing (an over-read poisons the result), a sentinel around and
between the outputs (an over-write shows as a changed bit).

The epilogue combinations of the sdf executors (the 'sdf-*' cases of gemm_ref.GEMM_CASES), read from
anr_sdf_train.hip and anr_sdf_capi.hip:
  bias + relu, one and two segments (resd_forward);          bias + softplus + deriv (sdf_forward, fwd_sp);
  bias + softplus + deriv + div_post sqrt2 (sdf_forward l=3); bias + softplus without deriv (sp_out_only);
  spd + div_post, no bias (sdf_tangent l = 3);                spd, spd_n < N, + div_pre sqrt2, B n-contiguous
  (sdf_input_grad / bwd);  spd_h with spd_scale sqrt2 or 0 (+ div_pre) (anr_sdf_capi.hip bwd);
  mask (+ accumulate), B n-contiguous (xgrad);  mask without bias (the residual MLP's tangent pass);
  atomic split-K with kper = 0 and row sums (wgrad's fallback).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _gemm_hooks as H
from . import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.name for c in R.GEMM_CASES]
DISPATCHED = set()   # (precision, a_k, b_k, swapped, a_vec, b_vec, vec_out) seen by the hook


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def launch(c, dev, scratch_short=0):
    d = R.gemm_data(c)
    bufs, st = R.gemm_buffers(d)
    db = H.DevBufs(bufs, dev)
    extra = {}
    if c.M_dev is not None:
        extra['M_dev'] = H.dev_int(c.M_dev, dev)
    if c.K_dev is not None:
        extra['K_dev'] = H.dev_int(c.K_dev, dev)
    g = H.gemm_desc(d, bufs, st, db, extra)
    if c.det:
        need = int(H.lib().anr_test_gemm_det_floats(c.M, c.N, c.ksplit))
        # NaN scratch: a partial the reduction reads and nobody wrote shows
        extra['scratch'] = torch.full((need + 64,), float('nan'), device=dev)
        g.scratch, g.scratch_floats = extra['scratch'].data_ptr(), need - scratch_short
    return d, db, g, extra


def run(g):
    rc = H.lib().anr_test_gemm(C.byref(g), H.stream_ptr())
    torch.cuda.synchronize()
    return rc


def expect_dispatch(c, g):
    """Which load / store paths the launcher chose, from the hook's report: the aligned cases prove the 16-B
    paths ran, the skewed ones the scalar fallbacks."""
    a_k = (c.a_k or c.one_row) and not (c.rowsum and c.one_row)
    assert (g.out_a_k, g.out_b_k, g.out_sw) == (int(a_k), int(c.b_k), int(not c.atomic))
    for s in range(len(c.K)):
        assert g.out_a_vec[s] == int(c.aligned and not c.one_row), 'a_vec'
        assert g.out_b_vec[s] == int(c.aligned), 'b_vec'
    assert g.out_vec_out == int(c.aligned and not c.atomic and c.N % 4 == 0), 'vec_out'
    DISPATCHED.add((c.prec, g.out_a_k, g.out_b_k, g.out_sw, g.out_a_vec[0], g.out_b_vec[0], g.out_vec_out))


@pytest.mark.parametrize('name', IDS)
def test_gemm(dev, name):
    c = R.GEMM_CASES[IDS.index(name)]
    d, db, g, extra = launch(c, dev)
    assert R.gemm_threshold_violations(d) == 0
    assert run(g) == H.OK
    expect_dispatch(c, g)
    rep = db.check_outputs()
    print(name, {k: f'{v[0]:.3f} of the bound, {v[1]:.2e} abs' for k, v in rep.items()})
    if c.det:  # a second run on fresh buffers: bit-identical
        first = {k: db.get(k).copy() for k, b in db.bufs.items() if b.out}
        for k in first:
            db.reset(k)
        extra['scratch'].fill_(float('nan'))
        assert run(g) == H.OK
        for k, v in first.items():
            assert np.array_equal(v.view(np.uint32), db.get(k).view(np.uint32)), f'{name}: {k} differs between two runs'


@pytest.mark.parametrize('name', [n for n in IDS if n.startswith('det-') and 'kdev256' in n])
def test_gemm_det_scratch_one_float_short(dev, name):
    c = R.GEMM_CASES[IDS.index(name)]
    d, db, g, extra = launch(c, dev, scratch_short=1)
    assert run(g) == H.LAUNCHER
    for k, b in db.bufs.items():
        if b.out:
            assert np.array_equal(db.get(k).view(np.uint32), b.flat.view(np.uint32)), f'{k} touched by a refused launch'


def test_dispatch_coverage(dev):
    """Every kernel instantiation launch_gemm can reach was launched by the cases above, with the vector
    paths both on and off. Reads what test_gemm recorded; run on its own it launches the cases itself."""
    if len(DISPATCHED) == 0:
        for c in R.GEMM_CASES:
            d, db, g, extra = launch(c, dev)
            assert run(g) == H.OK
            expect_dispatch(c, g)
    kernels = {(p, a, b, sw) for (p, a, b, sw, _, _, _) in DISPATCHED}
    want = {(p, a, b, sw) for p in ('fp32', 'bf16') for a in (0, 1) for b in (0, 1) for sw in (0, 1)} | \
           {('x3', 1, b, sw) for b in (0, 1) for sw in (0, 1)}   # the 20 instantiations of anr_gemm.hip
    assert len(want) == 20
    assert want <= kernels, sorted(want - kernels)
    for flag in (4, 5, 6):
        assert {t[flag] for t in DISPATCHED} == {0, 1}
    print('dispatched:', sorted(DISPATCHED))
