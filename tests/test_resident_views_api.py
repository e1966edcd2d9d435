"""CPU: the pieces of the device batch sampler (anr_train_ray_sample / data.ResidentViews) that need no
GPU: the numpy Philox4x32-10 the GPU tests compare against (Random123 known answers), the entry's
argument rejections (all before any HIP call), and that the cases of tests/test_gpu_resident_views.py
exercise what they claim (round counts under this draw scheme, from the float64 restatement)."""
import ctypes
import os

import numpy as np
import pytest

from animatable_nerf_amd import _lib
from oracle import restate

from ._common import golden
from .philox_ref import PhiloxDraws, philox4x32_10, slot_words

SEED, STEP = 1234, 7


def _hex(w):
    return ' '.join('%08x' % int(x) for x in w)


@pytest.mark.parametrize('ctr, key, want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    assert _hex(philox4x32_10(np.array(ctr, dtype=np.uint32), key)) == want
    # batched counters give the same words
    assert _hex(philox4x32_10(np.array([ctr, ctr], dtype=np.uint32), key)[1]) == want


def test_philox_draws_slot_layout():
    """Slot i of round r is word i & 3 at counter (i >> 2, r, step_lo, step_hi) under key (seed_lo,
    seed_hi), whatever the split of the round over randint calls; index = (x * n) >> 32."""
    seed, step = (5 << 32) | 1234, (9 << 32) | 7
    rng = PhiloxDraws(seed, step, calls_per_round=3)
    got = [rng.randint(0, n, k) for n, k in ((1000, 5), (49, 3), (7777, 6), (1000, 2), (49, 0), (7777, 3))]
    assert rng.rounds == 2 and rng.round_slots == [14, 5]
    ns = [1000] * 5 + [49] * 3 + [7777] * 6
    for i in range(14):
        w = philox4x32_10(np.array([i >> 2, 0, 7, 9], dtype=np.uint32), (1234, 5))[i & 3]
        assert int(np.concatenate(got[:3])[i]) == (int(w) * ns[i]) >> 32
    w1 = slot_words(seed, step, 1, 0, 5)
    assert np.array_equal(np.concatenate(got[3:]), (w1.astype(np.uint64) * np.array([1000] * 2 + [7777] * 3,
                                                                                      dtype=np.uint64)) >> np.uint64(32))
    two = PhiloxDraws(seed, step, calls_per_round=2)
    a = np.concatenate([two.randint(0, 1000, 5), two.randint(0, 7777, 9)])
    assert two.rounds == 1 and np.array_equal(a[:5], got[0]) and np.array_equal(a[8:], got[2][:])
    with pytest.raises(ValueError):
        two.randint(0, 0, 4)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


_PTRS = ('Kinv', 'R', 'T', 'origin', 'bounds', 'img', 'bound_mask', 'occ_mask', 'list_body', 'list_face', 'list_bound',
         'ray_o', 'ray_d', 'rgb', 'near', 'far', 'coord', 'mask_at_box', 'occupancy', 'n_out', 'shortfall')
_ORDER = ('H', 'W', 'Kinv', 'R', 'T', 'origin', 'fp64', 'bounds', 'img', 'bound_mask', 'occ_mask', 'list_body',
          'list_face', 'list_bound', 'n_body_px', 'n_face_px', 'n_bound_px', 'mask_bkgd', 'body_ratio', 'face_ratio',
          'nrays', 'max_rounds', 'seed', 'step', 'ray_o', 'ray_d', 'rgb', 'near', 'far', 'coord', 'mask_at_box',
          'occupancy', 'n_out', 'shortfall', 'stream')


def _call(lib, **change):
    """anr_train_ray_sample with an acceptable argument list (pointers: host dummies, never
    dereferenced by a rejected call) and the given arguments replaced."""
    buf = (ctypes.c_double * 16)()
    a = dict(H=120, W=100, fp64=1, n_body_px=10, n_face_px=5, n_bound_px=20, mask_bkgd=1, body_ratio=0.5,
             face_ratio=0.25, nrays=64, max_rounds=8, seed=SEED, step=STEP, stream=None)
    for k in _PTRS:
        a[k] = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double)) if k in _ORDER[2:6] else ctypes.c_void_p(
            ctypes.addressof(buf))
    assert not set(change) - set(a)
    a.update(change)
    return lib.anr_train_ray_sample(*[a[k] for k in _ORDER])


REJECTED = ([{k: None} for k in _PTRS if k not in ('occ_mask', 'occupancy', 'list_body', 'list_face')] + [
    {'occ_mask': None}, {'occupancy': None},  # one without the other
    {'list_body': None}, {'list_face': None},  # NULL with a non-zero length
    {'nrays': 0}, {'nrays': -5}, {'nrays': 65537},
    {'body_ratio': -0.1}, {'body_ratio': 1.5}, {'face_ratio': -0.1}, {'face_ratio': 1.01},
    {'body_ratio': 0.6, 'face_ratio': 0.5}, {'body_ratio': float('nan')},
    {'n_bound_px': 0}, {'n_bound_px': -1}, {'n_body_px': 0}, {'n_body_px': -3},
    {'max_rounds': 0}, {'max_rounds': 1025}, {'H': 0}, {'W': -1}])


@pytest.mark.parametrize('change', REJECTED, ids=lambda c: ','.join(f'{k}={v}' for k, v in c.items()))
def test_sample_rejects_before_any_device_call(lib, change):
    assert _call(lib, **change) == 2  # ANR_E_ARG
    assert b'anr_train_ray_sample' in lib.anr_last_error()


def shrunk(bounds, f):
    """The box scaled by f about its centre."""
    b = np.asarray(bounds)
    c = (b[0] + b[1]) / 2
    return np.stack([c - (c - b[0]) * f, c + (b[1] - c) * f]).astype(b.dtype)


def restated(g, case, nrays, scale, face_ratio=None):
    """restate.sample_ray_train of G12 camera `case` under the device sampler's draws -> (rows, rng)."""
    p = f'c{case}_'
    n_face_px = int(((g[p + 'msk'] * g[p + 'bound_mask']) == 13).sum())
    rng = PhiloxDraws(SEED, STEP, 3 if n_face_px > 0 else 2)
    fr = float(g[p + 'face_ratio']) if face_ratio is None else face_ratio
    res = restate.sample_ray_train(g[p + 'img'], g[p + 'msk'], g[p + 'K'], g[p + 'R'], g[p + 'T'],
                                   shrunk(g['bounds'], scale), nrays, g[p + 'bound_mask'], True, 0.5, fr, rng)
    return res, rng


def rows_after(rng, nrays, max_rounds):
    """Rays in hand when round `max_rounds` would begin. Valid where a round's slots are all the rays
    still missing (no face slots lost to an empty list): round r then hands out nrays - n_sampled."""
    return nrays if rng.rounds <= max_rounds else nrays - rng.round_slots[max_rounds]


def test_gpu_cases_are_not_vacuous():
    """The GPU cases do what their names say: one round and several, across the 1,024-slot stride,
    never at the default cap of 64 rounds; and the round-cap case stops short with some rays."""
    g = golden('g12_train_rays')
    assert float(g['c0_face_ratio']) == 0.0 and ((g['c0_msk'] * g['c0_bound_mask']) == 13).sum() == 0
    assert g['c1_K'].dtype == np.float32 and g['c0_K'].dtype == np.float64
    assert ((g['c1_msk'] * g['c1_bound_mask']) == 13).sum() == 49
    rounds = {(c, n, s): restated(g, c, n, s)[1].rounds for c in (0, 1) for n, s in ((1024, 1.0), (1025, 0.5))}
    assert rounds == {(0, 1024, 1.0): 1, (1, 1024, 1.0): 6, (0, 1025, 0.5): 14, (1, 1025, 0.5): 34}
    # the first round of 1,025 rays has 1,025 slots: one past the workgroup's stride
    assert restated(g, 1, 1025, 0.5)[1].round_slots[0] == 1025
    for c, hits in ((0, 172), (1, 140)):
        res, rng = restated(g, c, 300, 0.25)
        assert rng.rounds > 8 and rows_after(rng, 300, 8) == hits
    # an empty face list with a face ratio: its slots are dropped, the round is short of `rem`
    res, rng = restated(g, 0, 65, 1.0, face_ratio=0.25)
    assert rng.round_slots[0] == 65 - int(65 * 0.25) and len(res['near']) == 65 and rng.rounds > 1
