"""CPU: the references, input sets and bars of tests/small_ref.py checked on their own: the compaction reference
against a naive loop, the float64 embedder against oracle/restate, the ulp measure on known values, and the
inv33 and compositing bars against float32 numpy restatements of the kernels (the bars are reachable by correct
fp32 code)."""
import numpy as np
import pytest
import torch

from oracle import restate
from . import small_ref as S

F32 = np.float32


def test_ulp_measure():
    one = np.array([1.0])
    assert S.ulp_of(one)[0] == 2.0 ** -23
    assert S.ulp_of(np.array([0.75]))[0] == 2.0 ** -24
    assert S.ulp_of(np.array([-3.0]))[0] == 2.0 ** -22
    # the floor: everything below the normal range, 0 included, is measured in units of 2^-149
    assert S.ulp_of(np.array([0.0, 1e-40, 2.0 ** -126]))[[0, 1, 2]].tolist() == [2.0 ** -149] * 3
    x = np.array([1.0, 1.5, 100.0, 1e-3], F32)
    assert (S.ulp_err(np.nextafter(x, F32(np.inf)), x.astype(np.float64)) == 1).all()
    assert S.ulp_err(F32(1.0), 1.0 + 2.0 ** -24) == 0.5
    assert S.rel_units(F32(1.0), 1.0 + 2.0 ** -24) == pytest.approx(1.0, rel=1e-6)
    assert S.rel_units(F32(0.0), 2.0 ** -130) == 2.0 ** -4 / S.U24


def test_float_ranges():
    r = S.f32_range(1.0, 2.0)
    assert len(r) == 2 ** 23 + 1 and r[0] == 1 and r[-1] == 2 and (np.diff(r.view(np.uint32).astype(np.int64)) == 1).all()
    r = S.f32_range(0.7, 0.9, 7)  # float32(0.7) < 0.7: the interval's own floats only
    assert r[0] >= 0.7 and r[0] == np.nextafter(F32(0.7), F32(1)) and r[-1] <= 0.9
    r = S.f32_range(0.1, 0.2)  # float32(0.1) > 0.1, float32(0.2) > 0.2
    assert r[0] == F32(0.1) and r[-1] == np.nextafter(F32(0.2), F32(0))
    r = S.f32_range(-1e-44, 1e-44)  # across the signed zeros, in increasing order: 7 subnormals a side
    assert len(r) == 16 and (np.diff(r.astype(np.float64)) >= 0).all() and (r[7:9] == 0).all()
    assert np.signbit(r).tolist() == [True] * 8 + [False] * 8 and -r[0] == r[-1] == F32(7 * 2.0 ** -149)
    r = S.f32_range(-1.2, 0.5, 64)
    assert r[0] == np.nextafter(F32(-1.2), F32(0)) and r.min() >= -1.2 and r.max() <= 0.5 and (np.diff(r.astype(np.float64)) > 0).all()
    # counted from -1.2, so the floats do not all end in zero bits: 100 x is inexact for most of them
    assert ((r.view(np.uint32) & 63) != 0).all()
    assert ((r * F32(100)).astype(np.float64) != r.astype(np.float64) * 100).mean() > 0.5
    assert len(S.around(0.4, 1)) == 3 and S.around(0.4, 1)[1] == F32(0.4)
    x = S.sincos_inputs()
    assert np.abs(x).max() > 65536 and (np.abs(x) == 65536).sum() == 2 and len(x) > 2 ** 24
    k = np.arange(1, 41723) * (np.pi / 2)
    lo, hi = x[-2 - 2 * 41722:-2 - 41722].astype(np.float64), x[-2 - 41722:-2].astype(np.float64)
    assert (lo <= k).all() and (k <= hi).all() and (hi.astype(F32) == np.nextafter(lo.astype(F32), F32(np.inf))).all()


def test_softplus_truth_is_torch_float64():
    x = np.concatenate([np.linspace(-1.2, 0.5, 4001), [0.2, 0.2000001, 10, -10, 0.0]]).astype(F32)
    h, fac = S.softplus100_f64(x)
    t = torch.from_numpy(x).double().requires_grad_()
    ht = torch.nn.functional.softplus(t, beta=100, threshold=20)
    ht.sum().backward()
    assert np.allclose(h, ht.detach().numpy(), rtol=1e-15, atol=1e-300)
    # torch's backward factor is z / (z + 1) below the threshold and 1 above: sigmoid(100 x) to 3e-9 there
    assert np.allclose(fac, t.grad.numpy(), rtol=1e-14, atol=3e-9)


@pytest.mark.parametrize('nfreq', [4, 6, 10])
def test_gamma64_against_oracle(nfreq):
    rng = np.random.default_rng(nfreq)
    x = rng.uniform(-3, 3, (257, 3)).astype(F32)
    want = restate.embed(torch.from_numpy(x).double(), nfreq).numpy()
    got = S.gamma64(x, nfreq)
    assert got.shape == want.shape == (257, 3 + 6 * nfreq)
    assert np.abs(got - want).max() <= 1e-15 * 2.0 ** nfreq
    # the layouts place every feature once and leave the padding at 0
    ef = S.want_embed_feature(x, nfreq)
    assert (ef[:, :min(64, got.shape[1])] == got[:, :64]).all() and (ef[:, got.shape[1]:] == 0).all()
    for NS in ((16,) if nfreq == 10 else (8,) if nfreq == 4 else ()):
        e = S.want_embed(x, nfreq, NS)
        for f in range(4 * NS):
            assert (e[:, f % 4, f // 4] == (got[:, f] if f < got.shape[1] else 0)).all()
    NS = 1 if nfreq == 4 else 2
    eb = S.want_embed_b(x, nfreq, NS).reshape(len(x), -1)
    assert sorted(np.abs(eb[5]).tolist()) == sorted(np.abs(got[5]).tolist() + [0.0] * (eb.shape[1] - got.shape[1]))
    assert (eb[:, :3] == x[:, :3]).all() and (eb[:, 3] == 0).all() and (eb[:, 4] == got[:, 3]).all() \
        and (eb[:, 5] == got[:, 6]).all()


def test_gamma_derivatives_against_autograd():
    rng = np.random.default_rng(3)
    x = rng.uniform(-3, 3, (33, 3)).astype(F32)
    comp, om, d1, d2 = S.gamma_d64(x, 6)
    t = torch.from_numpy(x).double().requires_grad_()
    g = restate.embed(t, 6)
    for f in range(39):
        (gr,) = torch.autograd.grad(g[:, f].sum(), t, create_graph=True, retain_graph=True)
        assert np.allclose(gr.detach().numpy()[:, comp[f]], d1[:, f], rtol=1e-12, atol=1e-12)
        if f < 3:  # the raw inputs: a constant first derivative
            assert (d2[:, f] == 0).all()
            continue
        (gr2,) = torch.autograd.grad(gr[:, comp[f]].sum(), t, retain_graph=True)
        assert np.allclose(gr2.numpy()[:, comp[f]], d2[:, f], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('R,chunk,off', [(1, 2048, 0), (257, 100, 0), (300, 2048, 100), (1025, 100, 0)])
def test_compact_ref_against_naive(R, chunk, off):
    rng = np.random.default_rng(R)
    mask = rng.integers(0, 2 ** 63, R, dtype=np.uint64) & rng.integers(0, 2 ** 63, R, dtype=np.uint64)
    mask[rng.random(R) < 0.2] = 0
    nch = (R + chunk - 1) // chunk
    cm = np.full(nch, S.NO_KEY)
    for c in range(nch):
        if c % 3 != 2:
            ray = rng.integers(c * chunk, min(R, (c + 1) * chunk))
            cm[c] = np.uint64((0x3DCCCCCD << 32) | (((ray + off) % chunk) * 64 + int(rng.integers(0, 64))))
    a, b = S.compact_ref(mask, cm, chunk, off), S.compact_naive(mask, cm, chunk, off)
    for u, v in zip(a[:3], b[:3]):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    assert a[3] == b[3] == len(a[2])
    assert a[3] > sum(bin(int(m)).count('1') for m in mask) - 1  # the forced bits only add


def test_alpha_ref_first_maximum_and_signed_zero():
    sig = np.array([-1, -0.0, 0.0, -2, 0.5, 0.7, 0.7, 0.5, -3, -3], F32)
    ray_off = np.array([0, 4, 8, 8, 10], np.int32)  # chunks of one ray; ray 2 keeps nothing
    row, tot = S.alpha_ref(sig, ray_off, 1, 0.5)
    # chunk 0: all <= th, the first zero (-0.0) is the argmax; chunk 1: 0.7 > th twice (0.5 is not > 0.5)
    assert row.tolist() == [-1, 0, -1, -1, -1, 1, 2, -1, 3, -1] and tot == 4


def div_const_restated(x, b, rb, scale=True):
    """anr_common.h div_const in IEEE arithmetic: below 1e-30 on 2^64 x, scaled back; q = RN(x rb), r = fma(-q, b,
    x), fma(r, rb, q). The float32 products are exact in float64 and x - q b cancels exactly, so each fma rounds
    once (the last one twice in rare cases: float64, then float32)."""
    tiny = (np.abs(x) < F32(1e-30)) & scale
    xs = x * np.where(tiny, F32(2.0 ** 64), F32(1))
    q = xs * rb
    r = (xs.astype(np.float64) - q.astype(np.float64) * float(b)).astype(F32)
    return (r.astype(np.float64) * float(rb) + q.astype(np.float64)).astype(F32) * np.where(tiny, F32(2.0 ** -64), F32(1))


@pytest.mark.parametrize('b', [100.0, 2.0 ** 0.5])
def test_div_const_restatement(b):
    """The sweep of the device test in IEEE arithmetic on the host: no mismatch for 1e-30 <= x < 2^126, and below
    1e-30 within the device test's 2 units of 2^-149 (the scaled quotient rounds a second time only where it is
    subnormal). Without the scaling the residual is subnormal there and the quotient is off by one ulp of itself
    in 1.9 % of the cases at sqrt2, up to 2,048 units: the reason the scaling is there."""
    b = F32(b)
    rb = F32(1.0) / b
    x = S.f32_range(1e-30, np.nextafter(F32(2.0 ** 126), F32(0)), 1013)
    assert np.array_equal(div_const_restated(x, b, rb).view(np.uint32), (x / b).view(np.uint32))
    t = S.f32_range(0, np.nextafter(F32(1e-30), F32(0)), 1013)
    want = (t / b).astype(np.float64)
    for scale in (True, False):
        got = div_const_restated(t, b, rb, scale)
        units = np.abs(got - want) / 2.0 ** -149
        print(f'div_const restated, b = {b!r}, below 1e-30, scaling {scale}: {np.count_nonzero(units)} of {len(t)} '
              f'differ, at most {units.max():.0f} units of 2^-149')
        assert S.ulp_err(got, want).max() <= 1.0
        assert units.max() <= 2 if scale else units.max() == (2048 if b != 100 else 1)


def test_inv33_bar_holds_for_fp32_restatement():
    for name, A in S.inv33_cases().items():
        want, bound = S.inv33_ref(A, quadratic=name == 'two_opposite')
        err = np.abs(S.inv33_f32(A).astype(np.float64) - want).max(1)
        assert (err <= bound).all(), name
        cond = np.linalg.cond(A.astype(np.float64).reshape(-1, 4, 4)[:, :3, :3], 2)
        if name == 'near_opposite':
            assert 3e3 < cond.max() < 3e4
        if name == 'two_opposite':  # two small singular values: past the linear bound, inside the quadratic one
            sv = np.linalg.svd(A.astype(np.float64).reshape(-1, 4, 4)[:, :3, :3], compute_uv=False)
            assert 300 < cond.max() < 3e3 and (sv[:, 1] / sv[:, 2]).max() < 1.01
        print(f'inv33 {name}: cond_2 max {cond.max():.3g}, fp32 restatement error / bound max {(err / bound).max():.3f}')


@pytest.mark.parametrize('R', [1, 5, 1027])
def test_composite_bar_holds_for_fp32_restatement(R):
    rng = np.random.default_rng(R)
    near = rng.uniform(0.5, 2, (1, R)).astype(F32)
    far = near + rng.uniform(0.5, 2, (1, R)).astype(F32)
    o = torch.zeros(1, R, 3)
    for t_rand in (None, torch.from_numpy(rng.uniform(0, 1, (1, R, 64)).astype(F32))):
        z = restate.sample_points(o, o, torch.from_numpy(near), torch.from_numpy(far), 64, t_rand)[1][0].numpy()
        assert z.dtype == F32
        for name, raw in S.composite_alphas(R, R).items():
            val, mag = S.composite_ref(raw, z)
            got = S.composite_f32(raw, z)
            for g, v, m in zip(got, val, mag):
                assert (np.abs(g.astype(np.float64) - v) <= S.composite_bound(m)).all(), name
            # the float64 reference is the oracle's raw2outputs
            rgb, acc, depth, w = restate.raw2outputs(torch.from_numpy(raw).double(), torch.from_numpy(z).double())
            for a, b in zip(val, (w, rgb, depth, acc)):
                assert np.allclose(a, b.numpy(), rtol=1e-13, atol=1e-300)
