"""GPU: the integer plumbing kernels and the compositing kernel of anr_rays.hip on their own, launched as
anr_capi.hip launches them through the test entry library (tests/csrc/anr_testapi_small.hip), against the numpy
references of tests/small_ref.py: k_scan_blocks across its 1,024-sum carry, the ordered compaction (k_compact1
and k_count + k_scan_blocks + k_compact), the alpha_ind rows (both paths) and k_composite. The integer results
must be exact; every buffer carries a guard band that must come back untouched.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import restate
from . import _small_hooks as H
from . import small_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64
SENT = -0x5A5A5A5B  # int32 sentinel of the guard bands and of everything a kernel must leave alone


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def ibuf(n, dev, fill=SENT):
    """n int32 behind and before GUARD sentinels: (whole tensor, pointer to element 0)."""
    t = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
    t[GUARD:GUARD + n] = fill
    return t, t.data_ptr() + 4 * GUARD


def body(t, n):
    a = t.cpu().numpy()
    assert (a[:GUARD] == SENT).all() and (a[GUARD + n:] == SENT).all(), 'a guard band changed'
    return a[GUARD:GUARD + n]


# ---- k_scan_blocks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1, 63, 64, 1023, 1024, 1025, 2048, 2049, 5000])
def test_scan_blocks(dev, nb):
    """Exclusive offsets in place and the total, exact, through the 1,024-sum carry loop; the word after the
    array stays untouched."""
    rng = np.random.default_rng(nb)
    cnt = rng.integers(0, 16385, nb).astype(np.int32)
    t, p = ibuf(nb, dev)
    t[GUARD:GUARD + nb] = torch.from_numpy(cnt).to(dev)
    tot, pt = ibuf(1, dev)
    assert H.lib().anr_test_scan_blocks(p, nb, pt, H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    want = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    assert np.array_equal(body(t, nb), want[:-1].astype(np.int32))
    assert body(tot, 1)[0] == want[-1]
    assert H.lib().anr_test_scan_blocks(p, 0, pt, H.stream_ptr()) == H.E_SHAPE
    assert H.lib().anr_test_scan_blocks(None, nb, pt, H.stream_ptr()) == H.E_NULL


# ---- compaction ------------------------------------------------------------------------------------------------
def make_case(R, chunk, density, off=0, seed=0):
    """Keep masks of the given bit density (rays with mask 0 among them, and for four or more chunks one chunk
    that keeps nothing and has no argmin key) and chunk_min keys whose forced sample is, chunk by chunk in turn,
    (a) already kept, (b) on a ray with mask 0, (c) any sample; the last (partial) chunk always has a key."""
    rng = np.random.default_rng([R, chunk, int(density * 100), off, seed])
    bits = rng.random((R, 64)) < density
    if 0 < density < 1:
        bits[rng.random(R) < 0.1] = False
    nch = (R + chunk - 1) // chunk
    cm = np.full(nch, S.NO_KEY)
    empty = 2 if nch >= 4 else -1
    for c in range(nch):
        r0, r1 = c * chunk, min(R, (c + 1) * chunk)
        if c == empty:
            bits[r0:r1] = False
            continue
        kind = c % 3
        ray, lane = int(rng.integers(r0, r1)), int(rng.integers(0, 64))
        kept = np.argwhere(bits[r0:r1])
        zero = np.flatnonzero(~bits[r0:r1].any(1))
        if kind == 0 and len(kept):
            k = kept[rng.integers(len(kept))]
            ray, lane = r0 + int(k[0]), int(k[1])
        elif kind == 1 and len(zero):
            ray = r0 + int(zero[rng.integers(len(zero))])
        pn = F32(rng.uniform(0, 0.05))
        cm[c] = np.uint64((int(pn.view(np.uint32)) << 32) | (((ray + off) % chunk) * 64 + lane))
    mask = np.packbits(bits, axis=1, bitorder='little').view(np.uint64).reshape(R)
    return mask, cm


def run_compact(mask, cm, chunk, off, path, dev):
    """One compaction on fresh buffers: (mask, ray_off (R + 1), list (64 R, sentinel past the total), total)."""
    R = len(mask)
    m = torch.from_numpy(mask.view(np.int64)).to(dev)
    c = torch.from_numpy(cm.view(np.int64)).to(dev)
    ro, p_ro = ibuf(R + 1, dev)
    bs, p_bs = ibuf((R + 255) // 256, dev)
    ls, p_ls = ibuf(64 * R, dev)
    tot, p_tot = ibuf(1, dev)
    d = H.Compact(n_rays=R, chunk=chunk, ray_offset=off, path=path, mask=m.data_ptr(), chunk_min=c.data_ptr(),
                  ray_off=p_ro, block_sum=p_bs, list=p_ls, total=p_tot, list_cap=64 * R)
    assert H.lib().anr_test_compact_run(d, H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    body(bs, (R + 255) // 256)
    assert np.array_equal(c.cpu().numpy().view(np.uint64), cm), 'chunk_min changed'
    dev_bufs = dict(mask=m, ray_off=ro, p_ray_off=p_ro, list=ls, p_list=p_ls, total=tot, p_total=p_tot)
    return (m.cpu().numpy().view(np.uint64), body(ro, R + 1).copy(), body(ls, 64 * R).copy(),
            int(body(tot, 1)[0])), dev_bufs


def check_compact(got, want, who):
    mask, ray_off, lst, total = want
    assert got[3] == total, f'{who}: total {got[3]} != {total}'
    assert np.array_equal(got[0], mask), f'{who}: mask'
    assert np.array_equal(got[1], ray_off), f'{who}: ray_off'
    assert np.array_equal(got[2][:total], lst), f'{who}: list'
    assert (got[2][total:] == SENT).all(), f'{who}: list written past the total'


RS = [1, 255, 256, 257, 1023, 1024, 1025, 4099]


@functools.lru_cache(maxsize=None)
def compact_cases(density):
    """(R, chunk, ray_offset, mask, chunk_min, reference) of every compaction case of one density."""
    out = []
    for chunk in (2048, 100):
        for R in RS:
            mask, cm = make_case(R, chunk, density)
            out.append((R, chunk, 0, mask, cm, S.compact_ref(mask, cm, chunk, 0)))
    mask, cm = make_case(257, 2048, density, off=100)  # a ray split's second part: rays 100.. of the chunk
    out.append((257, 2048, 100, mask, cm, S.compact_ref(mask, cm, 2048, 100)))
    return out


def test_compact_preconditions(dev):
    mask, cm = make_case(1025, 2048, 0.37)
    m = torch.from_numpy(mask.view(np.int64)).to(dev)
    c = torch.from_numpy(cm.view(np.int64)).to(dev)
    ro, p_ro = ibuf(1026, dev)
    d = H.Compact(n_rays=1025, chunk=2048, ray_offset=0, path=H.PATH_ONE, mask=m.data_ptr(), chunk_min=c.data_ptr(),
                  ray_off=p_ro, block_sum=p_ro, list=p_ro, total=p_ro, list_cap=64 * 1025)
    L, s = H.lib(), H.stream_ptr()
    assert L.anr_test_compact_run(d, s) == H.E_SHAPE  # k_compact1 holds 1,024 rays
    d.path, d.list_cap = H.PATH_AUTO, 64 * 1025 - 1
    assert L.anr_test_compact_run(d, s) == H.E_SLAB
    d.list_cap, d.list = 64 * 1025, None
    assert L.anr_test_compact_run(d, s) == H.E_NULL
    d.list, d.chunk = p_ro, 0
    assert L.anr_test_compact_run(d, s) == H.E_SHAPE
    torch.cuda.synchronize()
    assert (body(ro, 1026) == SENT).all() and np.array_equal(m.cpu().numpy().view(np.uint64), mask)


@pytest.mark.parametrize('density', [0.0, 0.03, 0.37, 1.0])
def test_compact(dev, density):
    """mask, ray_off[0..R], list[0..total) and the total equal the reference (unpack the bits, OR in the forced
    bit, nonzero) as the library selects the path; for R <= 1024 also through the three launches, byte for byte
    like k_compact1."""
    for R, chunk, off, mask, cm, want in compact_cases(density):
        who = f'R {R} chunk {chunk} offset {off} density {density}'
        got, _ = run_compact(mask, cm, chunk, off, H.PATH_AUTO, dev)
        check_compact(got, want, who)
        if R <= 1024:
            gen, _ = run_compact(mask, cm, chunk, off, H.PATH_GENERAL, dev)
            check_compact(gen, want, who + ' (three launches)')
            for a, b in zip(got[:3], gen[:3]):
                assert a.tobytes() == b.tobytes(), f'{who}: k_compact1 differs from the three launches'


def test_compact_carry_in_situ(dev):
    """R = 262,145 rays at density 0.03: 1,025 block sums, so k_scan_blocks carries inside the compaction."""
    R, chunk = 262145, 2048
    mask, cm = make_case(R, chunk, 0.03)
    got, _ = run_compact(mask, cm, chunk, 0, H.PATH_AUTO, dev)
    check_compact(got, S.compact_ref(mask, cm, chunk, 0), f'R {R}')


# ---- alpha_ind rows --------------------------------------------------------------------------------------------
TH = 0.5


def make_sigma(want, R, chunk, rng):
    """sigma' per compact sample from a coarse grid (ties at the maximum, values equal to train_th, negatives,
    signed zeros). With several chunks, the last is entirely at or below the threshold with its maximum tied and
    the first holds signed zeros only, -0.0 first; a single chunk is the one or the other or left random in turn
    (by R), so that the two-launch path sees each."""
    ray_off, n = want[1], want[3]
    sig = (rng.integers(-4, 5, n) / 4).astype(F32)
    sig[(sig == 0) & (rng.random(n) < 0.5)] = F32(-0.0)
    spans = [(int(ray_off[r0]), int(ray_off[min(R, r0 + chunk)])) for r0 in range(0, R, chunk)]
    full = [sp for sp in spans if sp[1] - sp[0] >= 3]
    below = full[-1] if len(full) >= 2 or (len(full) == 1 and R % 4 == 1) else None
    zeros = full[0] if len(full) >= 2 or (len(full) == 1 and R % 4 == 3) else None
    if below:
        s0, s1 = below
        sig[s0:s1] = np.minimum(sig[s0:s1], F32(TH))
        sig[s0 + (s1 - s0) // 2] = sig[s1 - 1] = F32(TH)
    if zeros:
        s0, s1 = zeros
        sig[s0:s1] = np.where(rng.random(s1 - s0) < 0.5, F32(0.0), F32(-0.0))
        sig[s0], sig[s0 + 1] = F32(-0.0), F32(0.0)
    return sig


def run_alpha(dv, sig, R, chunk, off, path, dev):
    n = len(sig)
    nch = (R + chunk - 1) // chunk
    nb2 = (R * 64 + 1023) // 1024
    sg = torch.from_numpy(sig).to(dev)
    cmx = torch.zeros(nch, dtype=torch.int64, device=dev)
    fl = torch.full((64 * R + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    bs, p_bs = ibuf(nb2, dev)
    orow, p_or = ibuf(64 * R, dev)
    tot, p_tot = ibuf(1, dev)
    d = H.Alpha(n_rays=R, chunk=chunk, ray_offset=off, path=path, train_th=TH, ray_off=dv['p_ray_off'],
                n_kept=dv['p_total'], sigma=sg.data_ptr(), chunk_max=cmx.data_ptr(), flags=fl.data_ptr() + GUARD,
                block_sum=p_bs, out_row=p_or, list=dv['p_list'], mask=dv['mask'].data_ptr(), total=p_tot)
    assert H.lib().anr_test_alpha_run(d, H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    body(bs, nb2)
    f = fl.cpu().numpy()
    assert (f[:GUARD] == 0x5A).all() and (f[GUARD + n:] == 0x5A).all(), 'flags written outside 0..n'
    rows = body(orow, 64 * R)
    assert (rows[n:] == SENT).all(), 'out_row written past n'
    return rows[:n].copy(), int(body(tot, 1)[0])


@pytest.mark.parametrize('density', [0.0, 0.03, 0.37, 1.0])
def test_alpha_ind(dev, density):
    """out_row and the row total equal the reference over the compaction outputs (n' from a handful to 262,336,
    across 1,024 and 65,536): strict sigma' > train_th, the first maximum of every chunk forced (ties, signed
    zeros, a chunk entirely below the threshold, a chunk that keeps nothing); with one chunk and at most 64 blocks
    the two-launch path equals the general one."""
    seen = []
    for R, chunk, off, mask, cm, want in compact_cases(density):
        who = f'R {R} chunk {chunk} offset {off} density {density}'
        got, dv = run_compact(mask, cm, chunk, off, H.PATH_AUTO, dev)
        check_compact(got, want, who)
        n = want[3]
        if n == 0:
            continue
        seen.append(n)
        sig = make_sigma(want, R, chunk, np.random.default_rng([R, chunk, n]))
        ref_rows, ref_tot = S.alpha_ref(sig, want[1], chunk, TH)
        rows, tot = run_alpha(dv, sig, R, chunk, off, H.PATH_AUTO, dev)
        assert tot == ref_tot, f'{who}: row total {tot} != {ref_tot}'
        bad = np.flatnonzero(rows != ref_rows)
        assert bad.size == 0, f'{who}: out_row differs at compact sample {bad[:1]} (sigma {sig[bad[:1]]})'
        if (R + chunk - 1) // chunk == 1 and R <= 1024 and off == 0:
            g_rows, g_tot = run_alpha(dv, sig, R, chunk, off, H.PATH_GENERAL, dev)
            assert g_tot == tot and g_rows.tobytes() == rows.tobytes(), f'{who}: the two paths differ'
    if density == 1.0:
        assert 65536 in seen and max(seen) > 65536 and min(seen) < 1024
    print(f'alpha_ind density {density}: n\' in {sorted(set(seen))}')


def test_alpha_preconditions(dev):
    mask, cm = make_case(300, 100, 0.37)
    got, dv = run_compact(mask, cm, 100, 0, H.PATH_AUTO, dev)
    orow, p_or = ibuf(64 * 300, dev)
    d = H.Alpha(n_rays=300, chunk=100, ray_offset=0, path=H.PATH_ONE, train_th=TH, ray_off=dv['p_ray_off'],
                n_kept=dv['p_total'], sigma=p_or, chunk_max=p_or, flags=p_or, block_sum=p_or, out_row=p_or,
                list=dv['p_list'], mask=dv['mask'].data_ptr(), total=p_or)
    assert H.lib().anr_test_alpha_run(d, H.stream_ptr()) == H.E_SHAPE  # three chunks: no two-launch path
    d.path, d.sigma = H.PATH_GENERAL, None
    assert H.lib().anr_test_alpha_run(d, H.stream_ptr()) == H.E_NULL
    torch.cuda.synchronize()
    assert (body(orow, 64 * 300) == SENT).all()


# ---- k_composite -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [1, 3, 4, 5, 1027])
def test_composite(dev, R):
    """raw2outputs in float64 on the fp32 raw and the oracle's fp32 z: every weight and every map within
    200 * 2^-24 of sum|terms| (63 factors x 3 roundings + the products and the 6-level reduction; small_ref's
    docstring), with and without t_rand and weights, for alpha random / all 0 / exactly 1 at lane 0 / at lane 63 /
    1 - 2^-24 / a ray of 64 ones."""
    rng = np.random.default_rng(R)
    near = rng.uniform(0.5, 2, R).astype(F32)
    far = near + rng.uniform(0.5, 2, R).astype(F32)
    trand = rng.uniform(0, 1, (R, 64)).astype(F32)
    o = torch.zeros(1, R, 3)
    up = lambda a: torch.from_numpy(a).to(dev)
    nr, fr, tr = up(near), up(far), up(trand)
    worst = 0.0
    for use_t in (False, True):
        z = restate.sample_points(o, o, torch.from_numpy(near)[None], torch.from_numpy(far)[None], 64,
                                  torch.from_numpy(trand)[None] if use_t else None)[1][0].numpy()
        for name, raw in S.composite_alphas(R, R).items():
            val, mag = S.composite_ref(raw, z)
            rw = up(raw)
            for use_w in (True, False):
                outs = [ibuf(k, dev) for k in (64 * R, 3 * R, R, R)]  # weights, rgb, depth, acc (float bits)
                d = H.Composite(n_rays=R, raw=rw.data_ptr(), near_=nr.data_ptr(), far_=fr.data_ptr(),
                                t_rand=tr.data_ptr() if use_t else None, rgb=outs[1][1], depth=outs[2][1],
                                acc=outs[3][1], weights=outs[0][1] if use_w else None)
                assert H.lib().anr_test_composite_run(d, H.stream_ptr()) == H.OK
                torch.cuda.synchronize()
                got = [body(t, k).view(F32) for (t, _), k in zip(outs, (64 * R, 3 * R, R, R))]
                if not use_w:
                    assert (got[0].view(np.int32) == SENT).all()
                for j, (g, v, m) in enumerate(zip(got, val, mag)):
                    if j == 0 and not use_w:
                        continue
                    err = np.abs(g.reshape(v.shape).astype(np.float64) - v)
                    bound = S.composite_bound(m)
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), f'R {R} {name} t_rand {use_t}: {("weights", "rgb", "depth", "acc")[j]}'
    print(f'k_composite R {R}: max error / bound {worst:.3f}')
    assert H.lib().anr_test_composite_run(H.Composite(n_rays=R), H.stream_ptr()) == H.E_NULL
