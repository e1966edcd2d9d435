"""CPU: the float64 references and bounds of tests/gemm_ref.py checked against themselves, the descriptor
mirrors of tests/_gemm_hooks.py against the entry library's structs, and the library's precondition
rejections (which return before anything is launched, so they run without a GPU).

The mutation tests prove that the inputs and shapes the GPU tests use would show the faults those tests
exist to catch: every mutated reference must fall outside the bound at every shape it applies to."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from . import _gemm_hooks as H
from . import gemm_ref as R

FAKE = 0x10000  # a 16-B aligned non-NULL address; the rejected calls never touch it


# ---- the entry library -------------------------------------------------------------------------------
def test_struct_sizes():
    L = H.lib()
    for which, T in H.SIZEOF.items():
        assert L.anr_test_sizeof(which) == C.sizeof(T), (which, T.__name__)
    assert L.anr_test_sizeof(99) == -1


def good_gemm():
    g = H.GemmDesc()
    g.M, g.N, g.nseg = 65, 68, 1
    g.K[0] = 33
    g.A[0], g.a_rs[0], g.a_cs[0] = FAKE, 36, 1
    g.B[0], g.b_rs[0], g.b_cs[0] = FAKE, 1, 36
    g.C, g.ldc = FAKE, 72
    g.ksplit = 1
    return g


GEMM_REJECT = {
    'null-C': (lambda g: setattr(g, 'C', None), H.E_NULL),
    'null-A': (lambda g: g.A.__setitem__(0, None), H.E_NULL),
    'M0': (lambda g: setattr(g, 'M', 0), H.E_SHAPE),
    'N0': (lambda g: setattr(g, 'N', 0), H.E_SHAPE),
    'nseg3': (lambda g: setattr(g, 'nseg', 3), H.E_SHAPE),
    'K0': (lambda g: g.K.__setitem__(0, 0), H.E_SHAPE),
    'A-no-unit-stride': (lambda g: (g.a_rs.__setitem__(0, 36), g.a_cs.__setitem__(0, 2)), H.E_LAYOUT),
    'B-no-unit-stride': (lambda g: (g.b_rs.__setitem__(0, 2), g.b_cs.__setitem__(0, 36)), H.E_LAYOUT),
    'seg1-other-layout': (lambda g: (setattr(g, 'nseg', 2), g.K.__setitem__(1, 8), g.A.__setitem__(1, FAKE),
                                     g.B.__setitem__(1, FAKE), g.a_rs.__setitem__(1, 1), g.a_cs.__setitem__(1, 68),
                                     g.b_rs.__setitem__(1, 1), g.b_cs.__setitem__(1, 8)), H.E_LAYOUT),
    'splitk-two-segments': (lambda g: (setattr(g, 'nseg', 2), g.K.__setitem__(1, 8), g.A.__setitem__(1, FAKE),
                                       g.B.__setitem__(1, FAKE), g.a_rs.__setitem__(1, 8), g.a_cs.__setitem__(1, 1),
                                       g.b_rs.__setitem__(1, 1), g.b_cs.__setitem__(1, 8), setattr(g, 'atomic', 1),
                                       setattr(g, 'ksplit', 2)), H.E_SPLITK),
    'splitk-not-atomic': (lambda g: setattr(g, 'ksplit', 2), H.E_SPLITK),
    'splitk-kper-unaligned-vector': (lambda g: (setattr(g, 'atomic', 1), setattr(g, 'ksplit', 2), setattr(g, 'kper', 20)),
                                     H.E_SPLITK),
    'kdev-two-segments': (lambda g: (setattr(g, 'nseg', 2), g.K.__setitem__(1, 8), g.A.__setitem__(1, FAKE),
                                     g.B.__setitem__(1, FAKE), g.a_rs.__setitem__(1, 8), g.a_cs.__setitem__(1, 1),
                                     g.b_rs.__setitem__(1, 1), g.b_cs.__setitem__(1, 8), setattr(g, 'K_dev', FAKE)), H.E_SPLITK),
    'atomic-relu': (lambda g: (setattr(g, 'atomic', 1), setattr(g, 'relu', 1)), H.E_EPILOGUE),
    'atomic-accumulate': (lambda g: (setattr(g, 'atomic', 1), setattr(g, 'accumulate', 1)), H.E_EPILOGUE),
    'atomic-softplus': (lambda g: (setattr(g, 'atomic', 1), setattr(g, 'softplus', 1)), H.E_EPILOGUE),
    'rowsum2-alone': (lambda g: setattr(g, 'rowsum2', FAKE), H.E_EPILOGUE),
    'rowsum-k-contiguous-A': (lambda g: setattr(g, 'rowsum', FAKE), H.E_EPILOGUE),
    'spd_n-past-N': (lambda g: (setattr(g, 'spd', FAKE), setattr(g, 'spd_n', 69)), H.E_EPILOGUE),
    'x3-m-contiguous-A': (lambda g: (setattr(g, 'x3', 1), g.a_rs.__setitem__(0, 1), g.a_cs.__setitem__(0, 68)), H.E_FORMAT),
}


@pytest.mark.parametrize('name', sorted(GEMM_REJECT))
def test_gemm_rejections(name):
    L = H.lib()
    for entry in (L.anr_test_gemm, L.anr_test_lgemm):
        g = good_gemm()
        GEMM_REJECT[name][0](g)
        assert entry(C.byref(g), None) == GEMM_REJECT[name][1]


# ---- the reference against itself ------------------------------------------------------------------------
CASES = R.REF_CASES
GEMM_IDS = [c.name for c in CASES]


def test_case_names_unique():
    assert len(set(GEMM_IDS)) == len(GEMM_IDS)


def _f32_epilogue(c, d, acc):
    """The epilogue of gemm_ref.gemm_eval in plain fp32 (numpy / torch on the CPU), non-atomic launches."""
    import torch
    f = np.float32
    Me = c.M_eff
    v = acc.astype(f)
    out = {}
    if c.bias:
        v = v + d.bias[None, :]
    if c.accumulate:
        v = v + d.c0[:Me]
    if c.div_pre:
        v = v / f(c.div_pre)
    if c.relu:
        v = np.maximum(v, f(0))
    if c.softplus:
        t = torch.from_numpy(np.ascontiguousarray(v))
        z = v * f(100)
        out['deriv'] = np.where(z > 20, f(-1), torch.exp(t * 100.0).numpy())
        v = torch.nn.functional.softplus(t, beta=100, threshold=20).numpy()
    if c.spd:
        s = d.spd[:Me, :c.spd_n]
        if c.spd == 'h':
            fac = f(1) - np.exp(f(-100) * (s * f(c.spd_scale) if c.spd_scale else s))
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                fac = np.where(s >= 0, s / (s + f(1)), f(1)).astype(f)
        v = v.copy()
        v[:, :c.spd_n] = v[:, :c.spd_n] * fac
    if c.mask:
        v = np.where(d.mask[:Me] > 0, v, f(0))
    if c.div_post:
        v = v / f(c.div_post)
    out['C'] = v
    return out


@pytest.mark.parametrize('name', GEMM_IDS)
def test_gemm_fp32_inside_bound(name):
    """A plain fp32 CPU matmul of the same operands (bf16-rounded for the bf16 cases) and an fp32 epilogue
    stay inside the bound around the float64 reference."""
    c = CASES[GEMM_IDS.index(name)]
    d = R.gemm_data(c)
    Me, Ke = c.M_eff, c.K_eff
    A0 = list(d.A)
    if c.atr:   # the activations k_lgemm derives from the stored factors, in plain fp32
        f = np.float32
        dd = A0[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            fa = (f(1) - np.exp(f(-100) * dd)) if c.spd == 'h' else np.where(dd >= 0, dd / (dd + f(1)), f(1)).astype(f)
        A0[0] = (R.atr_weights(c)[None, :] * fa).astype(f)
    A = [(R.rne_bf16(a) if c.prec == 'bf16' else a)[:Me, :k] for a, k in zip(A0, Ke)]
    B = [(R.rne_bf16(b) if c.prec == 'bf16' else b)[:k] for b, k in zip(d.B, Ke)]
    acc = np.zeros((Me, c.N), np.float32)
    for a, b in zip(A, B):
        acc = acc + a.astype(np.float32) @ b.astype(np.float32)
    if c.atomic:
        got = {'C': d.c0[:Me] + acc + (d.bias[None, :] if c.bias else np.float32(0))}
    else:
        got = _f32_epilogue(c, d, acc)
    if c.rowsum:
        rs = sum(a.astype(np.float32)[:Me, :k].sum(1, dtype=np.float32) for a, k in zip(A0, Ke))
        got['rowsum'] = d.rs0[0, :Me] + rs
    for nm in ('C', 'deriv', 'rowsum'):
        if nm in d.ref and nm in got:
            v, b = d.ref[nm]
            err = np.abs(got[nm].astype(np.float64) - v)
            assert (err <= b).all(), (nm, float((err - b).max()))


MUT_PARAMS = [(c.name, m) for c in CASES for m in R.MUTATIONS if R.gemm_mutation_applies(c, m)]


def test_every_mutation_is_exercised():
    assert {m for _, m in MUT_PARAMS} == set(R.MUTATIONS)


@pytest.mark.parametrize('name,mut', MUT_PARAMS)
def test_gemm_mutation_falls_outside(name, mut):
    c = CASES[GEMM_IDS.index(name)]
    d = R.gemm_data(c)
    m = R.gemm_eval(c, d.A, d.B, d.bias, d.c0, d.rs0, d.spd, d.mask, mut=mut, e_sp=d.e_sp)
    assert R.outside(d.ref, m), f'{name}: the mutation {mut} stays inside the bound'


def test_softplus_reference_error():
    """The figure the 16x softplus margin is applied to: torch's fp32 softplus against float64 on the cases'
    own pre-activations. Bounded by reasoning: z = 100 v is one rounding (|dz| <= 20 * 2^-24 below the
    threshold, softplus' <= 1: 1.2e-8 after / 100), exp and log1p a few ulp of a value <= 20 (1.9e-8 per ulp
    after / 100), the final rounding of a value <= 0.21 (1.3e-8): <= 6.5e-8. exp(100 v): |z| <= 50 rounded
    once is 50 * 2^-24 = 3e-6 relative, plus the function's own ulp: <= 3.3e-6."""
    worst = [0.0, 0.0]
    n = 0
    for c in CASES:
        if c.softplus:
            e = R.gemm_data(c).e_sp
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            n += 1
    print(f'softplus reference error over {n} cases: absolute {worst[0]:.3e}, exp relative {worst[1]:.3e}')
    assert n > 0
    assert 0 < worst[0] <= 6.5e-8
    assert 0 < worst[1] <= 3.3e-6


@pytest.mark.parametrize('name', [c.name for c in CASES if c.softplus and c.deriv])
def test_no_preactivation_at_the_deriv_threshold(name):
    d = R.gemm_data(CASES[GEMM_IDS.index(name)])
    assert R.gemm_threshold_violations(d) == 0
    v = d.ref['pre'][0]
    assert np.abs(v).max() <= 0.5 and (100 * v > 20).any() and (100 * v < 20).any()  # both branches are taken


def test_bf16_helpers():
    import torch
    x = np.random.default_rng(5).uniform(-3, 3, 4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]  # ties: to even
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.rne_bf16(x), ref)
    assert np.array_equal(R.rne_bf16_f64(x.astype(np.float64)), ref.astype(np.float64))
    hi, lo = R.split_bf16(x)
    assert (np.abs(x.astype(np.float64) - hi - lo) <= 2.0 ** -16 * np.abs(x)).all()


# ---- rejections of the row GEMM and weight-gradient entries -----------------------------------------------
def good_rgemm():
    g = H.RGemmDesc()
    g.M_host, g.N, g.nseg = 129, 24, 1
    g.K[0], g.bcol[0], g.rows[0] = 100, 64, 24
    g.A[0], g.lda[0] = FAKE, 128
    g.B[0], g.ldb[0], g.lo_off[0] = FAKE, 192, 8192
    g.C, g.ldc = FAKE, 32
    return g


RGEMM_REJECT = {
    'null-C': (lambda g: setattr(g, 'C', None), H.E_NULL),
    'null-B': (lambda g: g.B.__setitem__(0, None), H.E_NULL),
    'N-past-256': (lambda g: (setattr(g, 'N', 257), g.rows.__setitem__(0, 257)), H.E_SHAPE),
    'M0': (lambda g: setattr(g, 'M_host', 0), H.E_SHAPE),
    'x3-with-bf16-rows': (lambda g: (setattr(g, 'x3', 1), setattr(g, 'abf', 1)), H.E_FORMAT),
    'x3-with-bf16-C': (lambda g: (setattr(g, 'x3', 1), setattr(g, 'cbf', 1)), H.E_FORMAT),
    'bf16-C-accumulate': (lambda g: (setattr(g, 'cbf', 1), setattr(g, 'accumulate', 1)), H.E_FORMAT),
    'A-unaligned': (lambda g: g.A.__setitem__(0, FAKE + 4), H.E_ALIGN),
    'lda-not-4': (lambda g: g.lda.__setitem__(0, 130), H.E_ALIGN),
    'abf-lda-not-8': (lambda g: (setattr(g, 'abf', 1), g.lda.__setitem__(0, 132)), H.E_ALIGN),
    'lda-below-K-rounded-to-64': (lambda g: g.lda.__setitem__(0, 100), H.E_SHAPE),
    'bcol-off-chunk': (lambda g: g.bcol.__setitem__(0, 32), H.E_ALIGN),
    'ldb-short': (lambda g: g.ldb.__setitem__(0, 184), H.E_SHAPE),
    'rows-below-N': (lambda g: g.rows.__setitem__(0, 23), H.E_SHAPE),
    'x3-no-lo-image': (lambda g: (setattr(g, 'x3', 1), g.lo_off.__setitem__(0, 0)), H.E_ALIGN),
}


@pytest.mark.parametrize('name', sorted(RGEMM_REJECT))
def test_rgemm_rejections(name):
    g = good_rgemm()
    RGEMM_REJECT[name][0](g)
    assert H.lib().anr_test_rgemm(C.byref(g), None) == RGEMM_REJECT[name][1]


def good_wgrad(mode=H.WG_SINGLE):
    d = H.WGradDesc()
    d.dY, d.ldY, d.X, d.ldX, d.dW, d.ldw = FAKE, 136, FAKE, 72, FAKE, 80
    d.nout, d.K = 129, 63
    c = H.WGradCall()
    c.mode, c.n_host, c.nd, c.nz = mode, 385, 1, 8
    c.d = C.pointer(d)
    c.slab, c.slab_floats = FAKE, H.lib().anr_test_wgrad_slab_floats()
    return c, d


WGRAD_REJECT = {
    'null-slab': (H.WG_SINGLE, lambda c, d: setattr(c, 'slab', None), H.E_NULL),
    'null-dW': (H.WG_SINGLE, lambda c, d: setattr(d, 'dW', None), H.E_NULL),
    'n0': (H.WG_SINGLE, lambda c, d: setattr(c, 'n_host', 0), H.E_SHAPE),
    'nout-past-256': (H.WG_SINGLE, lambda c, d: (setattr(d, 'nout', 257), setattr(d, 'ldY', 264)), H.E_SHAPE),
    'K-past-256': (H.WG_GROUP, lambda c, d: (setattr(d, 'K', 257), setattr(d, 'ldX', 264)), H.E_SHAPE),
    'x3-with-bf16-rows': (H.WG_SINGLE, lambda c, d: (setattr(d, 'x3', 1), setattr(d, 'ybf', 1)), H.E_FORMAT),
    'dY-unaligned': (H.WG_SINGLE, lambda c, d: setattr(d, 'dY', FAKE + 8), H.E_ALIGN),
    'ldX-not-4': (H.WG_GROUP, lambda c, d: setattr(d, 'ldX', 73), H.E_ALIGN),
    'ldY-below-nout': (H.WG_SINGLE, lambda c, d: setattr(d, 'ldY', 128), H.E_SHAPE),
    'j0-off-the-f32-path': (H.WG_SINGLE, lambda c, d: setattr(d, 'j0', 1), H.E_SHAPE),
    'j0-past-3': (H.WG_F32, lambda c, d: setattr(d, 'j0', 4), H.E_SHAPE),
    'slab-short': (H.WG_SINGLE, lambda c, d: setattr(c, 'slab_floats', c.slab_floats - 1), H.E_SLAB),
    'f32-fixed-order': (H.WG_F32, lambda c, d: setattr(c, 'det', 1), H.E_FORMAT),
    'two-descriptors-single': (H.WG_SINGLE, lambda c, d: setattr(c, 'nd', 2), H.E_SHAPE),
}


@pytest.mark.parametrize('name', sorted(WGRAD_REJECT))
def test_wgrad_rejections(name):
    mode, f, code = WGRAD_REJECT[name]
    c, d = good_wgrad(mode)
    f(c, d)
    assert H.lib().anr_test_wgrad(C.byref(c), None) == code


# ---- lgemm_supported: the documented exclusions (anr_train.h, anr_lgemm.hip lgemm_supported) -----------------
def good_lgemm():
    g = good_gemm()
    g.M, g.N = 129, 256
    g.K[0], g.a_rs[0], g.b_cs[0] = 256, 256, 256
    g.ldc = 256
    return g


def _head(g, n=3):
    g.bias, g.relu, g.head_w, g.head_b, g.head_out, g.ldh, g.head_n = FAKE, 1, FAKE, FAKE, FAKE, 4, n


LGEMM_UNSUPPORTED = {
    'bf16': lambda g: setattr(g, 'bf16', 1),
    'accumulate': lambda g: setattr(g, 'accumulate', 1),
    'atomic': lambda g: setattr(g, 'atomic', 1),
    'rowsum': lambda g: (g.a_rs.__setitem__(0, 1), g.a_cs.__setitem__(0, 256), setattr(g, 'rowsum', FAKE)),
    'M_dev': lambda g: setattr(g, 'M_dev', FAKE),
    'mask-x3': lambda g: (setattr(g, 'mask', FAKE), setattr(g, 'ldm', 256), setattr(g, 'x3', 1)),
    'mask-with-spd': lambda g: (setattr(g, 'mask', FAKE), setattr(g, 'ldm', 256), setattr(g, 'spd', FAKE),
                                setattr(g, 'ldsd', 256), setattr(g, 'spd_n', 256)),
    'mask-unaligned': lambda g: (setattr(g, 'mask', FAKE + 4), setattr(g, 'ldm', 256)),
    'spd-N-below-4': lambda g: (setattr(g, 'N', 1), setattr(g, 'spd', FAKE), setattr(g, 'ldsd', 4), setattr(g, 'spd_n', 1)),
    'spd-with-bias': lambda g: (setattr(g, 'spd', FAKE), setattr(g, 'ldsd', 256), setattr(g, 'spd_n', 256), setattr(g, 'bias', FAKE)),
    'A-m-contiguous': lambda g: (g.a_rs.__setitem__(0, 1), g.a_cs.__setitem__(0, 136)),
    'a_rs-below-K-rounded-to-8': lambda g: (g.K.__setitem__(0, 39), g.a_rs.__setitem__(0, 39), g.b_cs.__setitem__(0, 39)),
    'C-unaligned': lambda g: setattr(g, 'C', FAKE + 4),
    'ldc-not-4': lambda g: setattr(g, 'ldc', 257),
    'deriv-unaligned': lambda g: (setattr(g, 'softplus', 1), setattr(g, 'deriv', FAKE + 4), setattr(g, 'ldd', 256)),
    'head-N-not-256': lambda g: (_head(g), setattr(g, 'N', 264), setattr(g, 'ldc', 264)),
    'head_n-5': lambda g: _head(g, 5),
    'head-with-softplus': lambda g: (_head(g), setattr(g, 'softplus', 1)),
    'shape-not-instantiated': lambda g: (g.K.__setitem__(0, 100), g.a_rs.__setitem__(0, 104), g.b_cs.__setitem__(0, 100)),
}


@pytest.mark.parametrize('name', sorted(LGEMM_UNSUPPORTED))
def test_lgemm_unsupported(name):
    g = good_lgemm()
    assert H.lib().anr_test_lgemm(C.byref(g), None) == H.E_NULL   # supported: stops at the missing image
    LGEMM_UNSUPPORTED[name](g)
    assert H.lib().anr_test_lgemm(C.byref(g), None) == H.E_UNSUPPORTED
