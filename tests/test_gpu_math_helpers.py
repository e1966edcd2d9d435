"""GPU: the per-sample __device__ math helpers (anr_common.h, anr_mlp_body.h, anr_lbs.h, embed_d of
anr_sdf_train.hip) against float64 numpy at the fp32 inputs, through the probe kernels of the test entry library
(tests/csrc/anr_testapi_small.hip). Input sets, truths, error measures and the derivations of the bars:
tests/small_ref.py.

A probe pins the helper as written, compiled with the project's flags; it does not pin each instance the compiler
inlined into a fused kernel (those stay with the fused programs' parity tests). Every test prints its measured
maxima before it asserts (run with -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _small_hooks as H
from . import small_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK = 1 << 22  # inputs per launch: bounds the float64 temporaries on the host


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def test_descriptor_sizes():
    for k, T in H.SIZEOF.items():
        assert H.lib().anr_test_small_sizeof(k) == C.sizeof(T), T.__name__
    assert H.lib().anr_test_small_sizeof(0) == -1


def test_probe_preconditions(dev):
    L, s = H.lib(), H.stream_ptr()
    x = torch.zeros(64, 3, device=dev)
    o = torch.zeros(64 * 64, device=dev)
    p = x.data_ptr(), o.data_ptr()
    assert L.anr_test_probe1(7, p[0], p[1], p[1], 64, 0, 0, s) == H.E_SHAPE
    assert L.anr_test_probe1(H.SINCOS, p[0], p[1], None, 64, 0, 0, s) == H.E_NULL
    assert L.anr_test_probe1(H.EXP, p[0], p[1], None, 0, 0, 0, s) == H.E_SHAPE
    assert L.anr_test_probe_inv33(None, p[1], 4, s) == H.E_NULL
    assert L.anr_test_probe_embed(H.EMBED, p[0], 6, p[1], 64, s) == H.E_SHAPE      # no embed<NS> for gamma_6
    assert L.anr_test_probe_embed(H.EMBED_B, p[0], 10, p[1], 48, s) == H.E_SHAPE   # partial waves
    assert L.anr_test_embed_tan(p[0], 3, p[0], 3, 6, 64, p[1], 38, 0, 1.0, s) == H.E_SLAB
    assert L.anr_test_embed_bwd10(p[0], 3, p[1], 62, 64, p[1], 3, s) == H.E_SLAB
    torch.cuda.synchronize()
    assert (o == 0).all()


def probe1(which, x, dev, two=False, p0=0.0, p1=0.0):
    """helper(x) over a float32 array in one launch: the first (and second) result."""
    xt = torch.from_numpy(np.ascontiguousarray(x, F32)).to(dev)
    o0 = torch.full_like(xt, float('nan'))
    o1 = torch.full_like(xt, float('nan')) if two else None
    assert H.lib().anr_test_probe1(which, xt.data_ptr(), o0.data_ptr(), o1.data_ptr() if two else None, xt.numel(),
                                   p0, p1, H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    return (o0.cpu().numpy(), o1.cpu().numpy()) if two else o0.cpu().numpy()


def chunks(x):
    for i in range(0, len(x), CHUNK):
        yield x[i:i + CHUNK]


def worst(err, x):
    i = int(np.argmax(err))
    return float(err[i]), float(x[i])


# ---- sincos_fast and the embedders ---------------------------------------------------------------------------
def test_sincos_fast(dev):
    """<= 2 ulp and <= 1e-7 absolute for sin and cos over every float of +-[32768, 65536], every 37th float of
    [1e-6, 32768], the floats bracketing k pi / 2 (k <= 41,722) and +-0. Measured on the device (MI355X):
    sin 1.526 ulp (x = 60375.379) / 7.09e-8, cos 1.521 ulp (x = 48555.137) / 7.11e-8; a host restatement with fmaf
    gives 1.53 ulp / 7.11e-8. sin(-0.0) comes back as +0.0 (the reduction's fma(-k, c, x) with k = -0.0)."""
    x = S.sincos_inputs()
    mu, ma = [0.0, 0.0], [0.0, 0.0]
    at = [0.0, 0.0]
    for xc in chunks(x):
        got = probe1(H.SINCOS, xc, dev, two=True)
        xd = xc.astype(np.float64)
        for j, ref in enumerate((np.sin(xd), np.cos(xd))):
            u, a = S.ulp_err(got[j], ref), np.abs(got[j] - ref)
            if u.max() > mu[j]:
                mu[j], at[j] = worst(u, xc)
            ma[j] = max(ma[j], float(a.max()))
    print(f'sincos_fast over {len(x)} inputs: sin {mu[0]:.3f} ulp (x = {at[0]!r}) / {ma[0]:.3e} abs, '
          f'cos {mu[1]:.3f} ulp (x = {at[1]!r}) / {ma[1]:.3e} abs')
    assert max(mu) <= 2.0 and max(ma) <= 1e-7
    z = probe1(H.SINCOS, np.array([0.0, -0.0], F32), dev, two=True)
    assert z[0].tolist() == [0.0, 0.0] and z[1].tolist() == [1.0, 1.0]


def embed_points(seed, n):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, (n, 3)).astype(F32)
    x[0] = 0
    x[1] = [0.0, -0.0, 3.0]
    x[2] = [-3.0, 3.0, 0.0]
    return x


def run_embed(which, x, nfreq, width, dev):
    xt = torch.from_numpy(x).to(dev)
    out = torch.full((len(x), width), float('nan'), device=dev)
    assert H.lib().anr_test_probe_embed(which, xt.data_ptr(), nfreq, out.data_ptr(), len(x), H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_embed(name, got, want):
    u, a = S.ulp_err(got, want), np.abs(got - want)
    print(f'{name}: {u.max():.3f} ulp, {a.max():.3e} abs over {got.size} features')
    assert u.max() <= 2.0 and a.max() <= 1e-7, name
    assert (got[want == 0] == 0).all(), f'{name}: a padding feature is not exactly 0'


@pytest.mark.parametrize('nfreq', [4, 6, 10])
def test_embed_feature(dev, nfreq):
    """gamma_nfreq feature by feature (sinf / cosf), features past 3 + 6 nfreq exactly 0."""
    x = embed_points(nfreq, 1031)
    got = run_embed(H.EMBED_FEATURE, x, nfreq, 64, dev)
    want = S.want_embed_feature(x, nfreq)
    assert (want[:, 3 + 6 * nfreq:] == 0).all()
    check_embed(f'embed_feature gamma_{nfreq}', got, want)


@pytest.mark.parametrize('NS,nfreq', [(16, 10), (8, 4)])
def test_embed(dev, NS, nfreq):
    """embed<NS> (the exact-fp32 kernels' layout: feature 4 s + g of lane group g)."""
    x = embed_points(NS, 1031)
    got = run_embed(H.EMBED, x, nfreq, 4 * NS, dev).reshape(-1, 4, NS)
    check_embed(f'embed<{NS}> gamma_{nfreq}', got, S.want_embed(x, nfreq, NS))


@pytest.mark.parametrize('NS,nfreq', [(2, 10), (2, 6), (1, 4)])
def test_embed_b(dev, NS, nfreq):
    """embed_b<NS> (the bf16 fragment layout, sincos_fast): points of [-3, 3]^3 and exact 0; one wave in which a
    single point is past the fast reduction's range (the whole wave takes the library path and is still right);
    and the switch point itself, max|x| 2^(nfreq - 1) = 65536 (fast) and the next float above (library)."""
    x = embed_points(NS + nfreq, 1024)
    big = F32(65536.0 / 2 ** (nfreq - 1))
    x[64 * 3 + 21] = [1.0, F32(1.6) * big, -2.0]       # the only point of its wave (points 208..223) past the range
    x[64 * 7 + 5] = [big, -big, F32(0.3)]              # the last arguments of the fast path
    x[64 * 9 + 40] = [np.nextafter(big, F32(np.inf)), 0.5, -0.25]  # the first of the library path
    got = run_embed(H.EMBED_B, x, nfreq, 32 * NS, dev).reshape(-1, 4, 8 * NS)
    check_embed(f'embed_b<{NS}> gamma_{nfreq}', got, S.want_embed_b(x, nfreq, NS))


def test_embed_d_kernels(dev):
    """embed_d through k_st_embed_tan (gamma_6 and gamma_10), k_st_embed_bwd10 and k_st_embed_rev6 at n = 257:
    the first- and second-derivative contractions against float64, within (N + 4) 2^-24 max omega^2 sum|terms|
    (small_ref's docstring). embed_d's value output is dead in all three kernels."""
    n, L, s = 257, H.lib(), H.stream_ptr()
    rng = np.random.default_rng(257)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32)).to(dev)
    x = rng.uniform(-3, 3, (n, 8)).astype(F32)  # ld 8, as the observed-point rows
    x[0, :3] = 0
    xd = rng.standard_normal((n, 4)).astype(F32)
    xt, xdt = up(x), up(xd)
    for nf, ldo, col0, scale in ((6, 40, 0, 1.0), (6, 256, 217, 2 ** -0.5), (10, 64, 0, 1.0)):
        out = torch.full((n, ldo), float('nan'), device=dev)
        assert L.anr_test_embed_tan(xt.data_ptr(), 8, xdt.data_ptr(), 4, nf, n, out.data_ptr(), ldo, col0, scale,
                                    s) == H.OK
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        F = 3 + 6 * nf
        want, bound = S.embed_tan_ref(x[:, :3], xd[:, :3], nf, scale)
        err = np.abs(got[:, col0:col0 + F] - want)
        print(f'k_st_embed_tan gamma_{nf} col0 {col0}: max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}, '
              f'relative to |term| {np.max(err / np.maximum(np.abs(want), 1e-300)) / S.U24:.2f} x 2^-24')
        assert (err <= bound).all()
        rest = np.ones(ldo, bool)
        rest[col0:col0 + F] = False
        assert np.isnan(got[:, rest]).all(), 'k_st_embed_tan wrote outside its columns'
    # first-order reverse of gamma_10
    G = rng.standard_normal((n, 64)).astype(F32)
    Gt = up(G)
    xb = torch.full((n, 4), float('nan'), device=dev)
    assert L.anr_test_embed_bwd10(xt.data_ptr(), 8, Gt.data_ptr(), 64, n, xb.data_ptr(), 4, s) == H.OK
    torch.cuda.synchronize()
    got = xb.cpu().numpy()
    want, bound = S.embed_bwd10_ref(x[:, :3], G)
    err = np.abs(got[:, :3] - want)
    print(f'k_st_embed_bwd10: max error / bound {np.max(err / bound):.3e}, relative to sum|terms| '
          f'{np.max(err / (bound / (25 * S.U24 * 2.0 ** 18))) / S.U24:.2f} x 2^-24')
    assert (err <= bound).all() and np.isnan(got[:, 3]).all()
    # second-order reverse of [gamma_6(t); J tdot]
    A0 = rng.standard_normal((2 * n, 40)).astype(F32)
    A4 = rng.standard_normal((2 * n, 256)).astype(F32)
    tb0 = rng.standard_normal((n, 4)).astype(F32)
    tb, ttb = up(tb0), torch.full((n, 4), float('nan'), device=dev)
    A0t, A4t = up(A0), up(A4)
    assert L.anr_test_embed_rev6(xt.data_ptr(), 8, xdt.data_ptr(), 4, A0t.data_ptr(), A4t.data_ptr(), n, tb.data_ptr(),
                                 ttb.data_ptr(), s) == H.OK
    torch.cuda.synchronize()
    w_tb, b_tb, w_ttb, b_ttb = S.embed_rev6_ref(x[:, :3], xd[:, :3], A0, A4, tb0)
    g_tb, g_ttb = tb.cpu().numpy(), ttb.cpu().numpy()
    e1, e2 = np.abs(g_tb[:, :3] - w_tb), np.abs(g_ttb[:, :3] - w_ttb)
    print(f'k_st_embed_rev6: tbar max error / bound {np.max(e1 / b_tb):.3e}, ttbar {np.max(e2 / b_ttb):.3e}; relative '
          f'to sum|terms| {np.max(e1 / (b_tb / (17 * S.U24 * 1024))) / S.U24:.2f} and '
          f'{np.max(e2 / (b_ttb / (17 * S.U24 * 1024))) / S.U24:.2f} x 2^-24')
    assert (e1 <= b_tb).all() and (e2 <= b_ttb).all()
    assert (g_tb[:, 3] == tb0[:, 3]).all() and np.isnan(g_ttb[:, 3]).all()
    # ttbar is optional
    tb = up(tb0)
    assert L.anr_test_embed_rev6(xt.data_ptr(), 8, xdt.data_ptr(), 4, A0t.data_ptr(), A4t.data_ptr(), n, tb.data_ptr(),
                                 None, s) == H.OK
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), g_tb)


# ---- softplus and its pieces ---------------------------------------------------------------------------------
_SP_FAC = {}


def softplus_fac_maxima(dev):
    """softplus100_fac's h and fac, and fp32 torch's softplus(beta=100, threshold=20) and its backward on the CPU,
    against torch's definition in float64 over small_ref.softplus_inputs, in units of 2^-24 relative with the
    2^-126 floor: ({name: (maximum, x)} over the whole set, the same where the float64 result is a normal float).
    Measured once for the tests below."""
    if not _SP_FAC:
        x = S.softplus_inputs()
        m = {'h': (0.0, 0.0), 'fac': (0.0, 0.0), 'torch h': (0.0, 0.0), 'torch fac': (0.0, 0.0)}
        mn = dict(m)
        for xc in chunks(x):
            h, fac = probe1(H.SP_FAC, xc, dev, two=True)
            rh, rf = S.softplus100_f64(xc)
            t = torch.from_numpy(xc).requires_grad_()
            th = torch.nn.functional.softplus(t, beta=100, threshold=20)
            th.sum().backward()
            for k, got, ref in (('h', h, rh), ('fac', fac, rf), ('torch h', th.detach().numpy(), rh),
                                ('torch fac', t.grad.numpy(), rf)):
                u = S.rel_units(got, ref)
                m[k] = max(m[k], worst(u, xc))
                mn[k] = max(mn[k], worst(np.where(ref >= S.TINY, u, 0.0), xc))
        _SP_FAC.update(all=m, normal=mn, n=len(x))
    m, mn = _SP_FAC['all'], _SP_FAC['normal']
    print(f'softplus100_fac over {_SP_FAC["n"]} inputs, units of 2^-24: ' +
          ', '.join(f'{k} {v[0]:.2f} (x = {v[1]!r})' for k, v in m.items()) + '; where the result is a normal float: ' +
          ', '.join(f'{k} {v[0]:.2f} (x = {v[1]!r})' for k, v in mn.items()))
    return m, mn


def test_softplus100_fac_no_worse_than_torch_fp32(dev):
    """Bar (i): over the whole input set softplus100_fac must not exceed the error of the reference's own fp32
    arithmetic, torch.nn.functional.softplus(beta=100, threshold=20) and its backward on the CPU (whose RN(100 x)
    is amplified by the exp: ~65 units). Measured on the device (MI355X): h 4.58 / fac 4.02 units against
    torch's 61.82 / 61.30."""
    m, _ = softplus_fac_maxima(dev)
    assert m['h'][0] <= m['torch h'][0] and m['fac'][0] <= m['torch fac'][0]


def test_softplus100_fac_units(dev):
    """Bar (ii): <= 8.5 units over the whole input set (the 4.3 of the documented emulation + 2 for each hardware
    transcendental at its documented 1 ulp), subnormal results included (down to 100 x = -120, where v_exp_f32
    alone would flush), and the ends exact: h(10) = 10, h(-10) = fac(-10) = 0. Measured on the device (MI355X):
    h 4.58 (x = -0.166), fac 4.02 (x = -0.0552)."""
    m, _ = softplus_fac_maxima(dev)
    assert m['h'][0] <= 8.5 and m['fac'][0] <= 8.5
    hz = probe1(H.SP_FAC, np.array([10.0, -10.0], F32), dev, two=True)
    assert hz[0].tolist() == [10.0, 0.0] and hz[1][1] == 0.0


def test_softplus100(dev):
    """The bf16x3 form, by the bars read from its comment: |dh| <= 1e-9 where h < 1e-5, otherwise 2^-16 relative.
    Measured on the device (MI355X): |dh| 6.4e-12 where h < 1e-5, 0.043 x 2^-16
    relative above (at h = 1.7e-5). Before the rounding error of 1 + e was added back: 6.0e-10 and 3.92 x 2^-16."""
    x = S.softplus_inputs()
    small, rel, big = 0.0, (0.0, 0.0), 0.0
    for xc in chunks(x):
        h = probe1(H.SP, xc, dev)
        rh, _ = S.softplus100_f64(xc)
        d = np.abs(h - rh)
        lo = rh < 1e-5
        small = max(small, float(d[lo].max(initial=0.0)))
        big = max(big, float(d[~lo & (rh < 0.007)].max(initial=0.0)))
        rel = max(rel, worst(np.where(lo, 0.0, d / np.maximum(rh, 1e-5)), rh))
    print(f'softplus100: |dh| {small:.3e} where h < 1e-5, {rel[0] / 2.0 ** -16:.4f} x 2^-16 relative elsewhere '
          f'(at h = {rel[1]:.3e}; |dh| {big:.3e} over 1e-5 <= h < 0.007)')
    assert small <= 1e-9
    assert rel[0] <= 2.0 ** -16


def test_fast_exp(dev):
    """<= 3 ulp against float64 exp over every 97th float of [-87, 40] (the comment's ~2 + 1). Measured on the
    device (MI355X): 0.94 ulp (z = -0.8665)."""
    x = S.f32_range(-87, 40, 97)
    m = (0.0, 0.0)
    for xc in chunks(x):
        m = max(m, worst(S.ulp_err(probe1(H.EXP, xc, dev), np.exp(xc.astype(np.float64))), xc))
    print(f'fast_exp over {len(x)} inputs: {m[0]:.3f} ulp (z = {m[1]!r})')
    assert m[0] <= 3.0


def test_fast_log1p(dev):
    """<= 4 ulp against float64 log1p over every 97th float of [0, e^40] and +-1024 floats around the 1/32
    switch (the comment's "a few" held to 3 + 1). Measured on the device (MI355X): 3.78 ulp (e = 4.12e12; the
    hardware log2 and reciprocal and three roundings)."""
    x = np.concatenate([S.f32_range(0, np.exp(40.0), 97), S.around(0.03125, 1024)])
    m = (0.0, 0.0)
    for xc in chunks(x):
        m = max(m, worst(S.ulp_err(probe1(H.LOG1P, xc, dev), np.log1p(xc.astype(np.float64))), xc))
    print(f'fast_log1p over {len(x)} inputs: {m[0]:.3f} ulp (e = {m[1]!r})')
    assert m[0] <= 4.0


def test_softplus_factor_h(dev):
    """|d| <= 1.5e-7 absolute against 1 - exp(-100 h) over every 101st float of [0, 0.5] (float-uniform: dense
    towards 0) and every float of the first 4096 above 0. Measured on the device (MI355X): 7.36e-8."""
    x = np.concatenate([S.f32_range(0, 0.5, 101), np.arange(4096, dtype=np.uint32).view(F32)])
    m = (0.0, 0.0)
    for xc in chunks(x):
        m = max(m, worst(np.abs(probe1(H.SPF_H, xc, dev) + np.expm1(-100.0 * xc.astype(np.float64))), xc))
    print(f'softplus_factor_h over {len(x)} inputs: {m[0]:.3e} absolute (h = {m[1]!r})')
    assert m[0] <= 1.5e-7


DIV_B = [100.0, 2.0 ** 0.5]


def div_operands(b):
    b = F32(b)
    return b, F32(1.0) / b


@pytest.mark.parametrize('b', DIV_B)
def test_div_const(dev, b):
    """Bit-equal to the IEEE quotient for every 1013th float of 1e-30 <= |x| < 2^126, both signs."""
    b, rb = div_operands(b)
    pos = S.f32_range(1e-30, np.nextafter(F32(2.0 ** 126), F32(0)), 1013)
    x = np.concatenate([pos, -pos])
    got = probe1(H.DIV, x, dev, p0=float(b), p1=float(rb))
    want = x / b
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f'div_const b = {b!r}: {bad.size} of {len(x)} quotients differ from IEEE' +
          (f', first x = {x[bad[0]]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}' if bad.size else ''))
    assert bad.size == 0


@pytest.mark.parametrize('b', DIV_B)
def test_div_const_below_1e30(dev, b):
    """Below 1e-30, where div_const runs on 2^64 x so that the residual FMA does not underflow: |d| <= 2 units of
    2^-149 against the IEEE quotient, over every 1013th float of [0, 1e-30), both signs. Measured on the device
    (MI355X): 6,918 of 451,606 quotients differ at b = 100 and 3,898 at sqrt2, each by 1 unit (subnormal
    quotients, rounded twice). Unscaled, sqrt2 was off by up to 2,048 units: tests/test_small_ref.py."""
    b, rb = div_operands(b)
    tiny = S.f32_range(0, np.nextafter(F32(1e-30), F32(0)), 1013)
    xt = np.concatenate([tiny, -tiny])
    gt, wt = probe1(H.DIV, xt, dev, p0=float(b), p1=float(rb)), xt / b
    d = np.abs(gt.astype(np.float64) - wt.astype(np.float64)) / 2.0 ** -149
    u = S.ulp_err(gt, wt.astype(np.float64))
    print(f'div_const b = {b!r} below 1e-30: {np.count_nonzero(d)} of {len(xt)} differ, at most {d.max():.1f} units of '
          f'2^-149 = {u.max():.1f} ulp of the quotient (|x| = {abs(xt[np.argmax(d)])!r})')
    assert u.max() <= 1.0  # never more than the last place of the quotient
    assert d.max() <= 2.0


def test_inv33(dev):
    """4,096 matrices each of rotations, LBS-like convex blends of 24 rotations and near-singular blends of
    near-opposite rotations with one small singular value (cond_2 up to ~1e4) against the float64 inverse:
    max|d| <= 16 * 2^-24 * cond_2(A) * max|A^-1|; and of blends of two near-opposite rotations (two small singular
    values, where the adjugate's error is quadratic in cond_2): max|d| <= 32 * 2^-24 * cond_2^2 max|A^-1| / s_max^3
    (small_ref's docstring derives both)."""
    for name, A in S.inv33_cases().items():
        At = torch.from_numpy(A).to(dev)
        Ri = torch.full((len(A), 9), float('nan'), device=dev)
        assert H.lib().anr_test_probe_inv33(At.data_ptr(), Ri.data_ptr(), len(A), H.stream_ptr()) == H.OK
        torch.cuda.synchronize()
        want, bound = S.inv33_ref(A, quadratic=name == 'two_opposite')
        err = np.abs(Ri.cpu().numpy().astype(np.float64) - want).max(1)
        print(f'inv33 {name}: error / bound max {np.max(err / bound):.3f}, max|d| {err.max():.3e}')
        assert (err <= bound).all(), name
