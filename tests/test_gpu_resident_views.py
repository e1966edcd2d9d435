"""GPU: data.ResidentViews / anr_train_ray_sample, the train-split batch drawn on the device in one
launch, against the float64 restatement (oracle.restate.sample_ray_train) and the existing device
path (data.sample_ray_h36m), both replaying the same counter-based draws (tests/philox_ref.py).

Fixture: G12 (120 x 100; c0 a float64 camera without face pixels, c1 a float32 camera with 49 face
pixels and face ratio 0.2), seed 1234, step 7. Both cameras compare bit for bit with both references
(G12's own test holds the restatement to the reference's bits for the float32 camera too), so no case
is held to the device path alone."""
import functools

import numpy as np
import pytest
import torch

from ._common import golden, make_net, scene
from .philox_ref import PhiloxDraws
from .test_resident_views_api import SEED, STEP, restated, rows_after, shrunk

pytestmark = pytest.mark.gpu

FLOAT_KEYS = ('rgb', 'ray_o', 'ray_d', 'near', 'far')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _g12():
    return golden('g12_train_rays')


@functools.lru_cache(maxsize=None)
def _restated(case, nrays, scale, face_ratio=None):
    """computed once per case, shared by the tests, never written to"""
    return restated(_g12(), case, nrays, scale, face_ratio)


def _views(dev, case, nrays, scale, face_ratio=None, **kw):
    from animatable_nerf_amd.data import ResidentViews
    g, p = _g12(), f'c{case}_'
    fr = float(g[p + 'face_ratio']) if face_ratio is None else face_ratio
    rv = ResidentViews(dev, nrays=nrays, seed=SEED, mask_bkgd=True, body_sample_ratio=0.5, face_sample_ratio=fr, **kw)
    # the occupancy mask: any (H, W) u8 image will do; the dataset's is the uncropped human mask
    rv.add('v', g[p + 'img'], g[p + 'msk'], g[p + 'K'], g[p + 'R'], g[p + 'T'], shrunk(g['bounds'], scale),
           bound_mask=g[p + 'bound_mask'], orig_msk=g[p + 'msk'])
    return rv, fr


def _np(out):
    return {k: v[0].cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_rows(got, ref, n, what):
    """rows < n of the sampler's output equal the restatement's, bit for bit"""
    for k in FLOAT_KEYS + ('coord',):
        r = np.asarray(ref[k])[:n]
        if k != 'coord':
            assert r.dtype == np.float32, k
        assert np.array_equal(_bits(got[k][:n]), _bits(r.astype(got[k].dtype))), f'{what}: {k}'


CASES = [(c, n, s, None) for c in (0, 1) for n in (1, 65, 1024, 1025) for s in (1.0, 0.5)] + [(0, 65, 1.0, 0.25),
                                                                                             (0, 1025, 0.5, 0.25)]


@pytest.mark.parametrize('case, nrays, scale, face_ratio', CASES)
def test_sample_bit_exact(dev, case, nrays, scale, face_ratio):
    """Every output of one launch equals (a) the float64 restatement and (b) sample_ray_h36m's round-per-
    launch device path under the same draws: one round and up to 34, 1 ray to 1,025 (one slot past the
    workgroup's stride), and a face ratio on a view without face pixels (face_ratio 0.25 on c0)."""
    from animatable_nerf_amd import data
    g, p = _g12(), f'c{case}_'
    rv, fr = _views(dev, case, nrays, scale, face_ratio)
    out = rv.sample('v', STEP)
    assert set(out['anr_volatile']) == {'rgb', 'ray_o', 'ray_d', 'near', 'far', 'mask_at_box', 'coord', 'occupancy'}
    got = _np(out)
    assert int(rv.n_out.item()) == nrays
    assert got['mask_at_box'].dtype == np.uint8 and got['mask_at_box'].shape == (nrays,) and (got['mask_at_box'] == 1).all()
    assert rv.shortfall() == 0
    ref, rng = _restated(case, nrays, scale, face_ratio)
    assert rng.rounds <= 64
    _assert_rows(got, ref, nrays, 'vs restatement')
    assert np.array_equal(got['occupancy'], g[p + 'msk'][ref['coord'][:, 0], ref['coord'][:, 1]])
    n_face_px = int(((g[p + 'msk'] * g[p + 'bound_mask']) == 13).sum())
    rng2 = PhiloxDraws(SEED, STEP, 3 if n_face_px > 0 else 2)
    rgb, ro, rd, near, far, coord, mab = data.sample_ray_h36m(
        g[p + 'img'], g[p + 'msk'], g[p + 'K'], g[p + 'R'], g[p + 'T'], shrunk(g['bounds'], scale), nrays, 'train',
        mask_bkgd=True, body_sample_ratio=0.5, face_sample_ratio=fr, bound_mask=g[p + 'bound_mask'], rng=rng2,
        device=dev)
    assert rng2.round_slots == rng.round_slots
    dev_ref = {'rgb': rgb, 'ray_o': ro, 'ray_d': rd, 'near': near, 'far': far, 'coord': coord}
    _assert_rows(got, {k: v.cpu().numpy() for k, v in dev_ref.items()}, nrays, 'vs sample_ray_h36m')
    for k in FLOAT_KEYS:
        assert out[k].dtype == torch.float32 and out[k].is_contiguous() and out[k].device == dev


@pytest.mark.parametrize('case', [0, 1])
def test_round_cap_and_shortfall(dev, case):
    """Quarter-size box, 300 rays, max_rounds 8: the kernel stops after round 7 with some rays (the
    restatement's first 8 rounds: 172 for c0, 140 for c1, recomputed here), the rest are masked-out
    rays of the documented form, and shortfall() accumulates over calls."""
    nrays, cap = 300, 8
    rv, _ = _views(dev, case, nrays, 0.25, max_rounds=cap)
    ref, rng = _restated(case, nrays, 0.25)
    n = rows_after(rng, nrays, cap)
    assert 0 < n < nrays and n == (172, 140)[case]
    out = rv.sample('v', STEP)
    got = _np(out)
    assert int(rv.n_out.item()) == n
    _assert_rows(got, ref, n, 'rows < n_out')
    assert (got['mask_at_box'][:n] == 1).all() and (got['mask_at_box'][n:] == 0).all()
    g, p = _g12(), f'c{case}_'
    origin = (-np.dot(g[p + 'R'].T, g[p + 'T']).ravel()).astype(np.float32)
    m = nrays - n
    assert np.array_equal(_bits(got['ray_o'][n:]), _bits(np.broadcast_to(origin, (m, 3))))
    assert np.array_equal(_bits(got['ray_d'][n:]), _bits(np.broadcast_to(np.float32([0, 0, 1]), (m, 3))))
    for k in ('near', 'far', 'rgb', 'coord', 'occupancy'):
        assert not got[k][n:].any(), k
        if got[k].dtype == np.float32:
            assert not _bits(got[k][n:]).any(), k  # +0, not -0
    assert rv.shortfall() == m
    rv.sample('v', STEP)
    assert rv.shortfall() == 2 * m


def test_same_seed_and_step_same_bits(dev):
    rv, _ = _views(dev, 1, 1024, 1.0)
    a = {k: v.copy() for k, v in _np(rv.sample('v', STEP)).items()}
    rv.sample('v', STEP + 1)
    b = {k: v.copy() for k, v in _np(rv.sample('v', STEP + 1)).items()}
    c = _np(rv.sample('v', STEP))
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(c[k])), k
    assert not np.array_equal(a['coord'], b['coord'])
    rv2, _ = _views(dev, 1, 1024, 1.0)  # another object, the same function of (seed, step)
    d = _np(rv2.sample('v', STEP))
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(d[k])), k


def _small_view():
    """A 64 x 64 float64 camera on the synthetic subject's box, a random image, the projected box as
    both masks (every pixel of it a body pixel)."""
    from animatable_nerf_amd import data
    sc = scene(0.05)
    K = np.array([[75.0, 0, 32.0], [0, 75.0, 32.0], [0, 0, 1]])
    R = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    T = np.array([[0.0], [0.0], [3.0]])
    bm = data.get_bound_2d_mask(sc.bounds, K, np.concatenate([R, T], axis=1), 64, 64)
    img = np.random.Generator(np.random.PCG64(5)).random((64, 64, 3), dtype=np.float32)
    return sc, img, bm.copy(), K, R, T, bm


@pytest.mark.parametrize('graph', ['0', '1'])
def test_in_place_batches_reach_the_step(dev, monkeypatch, graph):
    """Three deterministic training steps fed by sample(key, 0..2), no synchronise in between, equal
    three steps fed by freshly built host batches of the same draws bit for bit (losses and weights
    after every step): a step that cached the rays of an earlier sample() (a kept _Call, or
    _static_call skipping the copy of a tensor whose version did not move) would differ. The host
    batches are dropped after their step, so the next one's tensors may take their addresses:
    _static_call keeps its sources referenced for that reason."""
    from animatable_nerf_amd import config
    from animatable_nerf_amd.data import ResidentViews
    from animatable_nerf_amd.trainer import FusedStep
    from oracle import restate
    monkeypatch.setenv('ANR_TRAIN_GRAPH', graph)
    for k in ('ANR_TRAIN_SERIAL', 'ANR_TRAIN_ON_CALLER', 'ANR_TRAIN_DETERMINISTIC'):
        monkeypatch.delenv(k, raising=False)
    nrays, steps = 256, 3
    sc, img, msk, K, R, T, bm = _small_view()
    cfg = config.defaults()
    cfg.perturb = 1
    t_rand = torch.rand((steps, nrays, int(cfg.N_samples)), generator=torch.Generator().manual_seed(3)).to(dev)
    z = np.zeros((1, 3), np.float32)
    frame = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
             for k, v in sc.batch_arrays(z, z, np.zeros(1, np.float32), np.zeros(1, np.float32)).items()
             if k not in ('ray_o', 'ray_d', 'near', 'far', 'rgb', 'mask_at_box', 'occupancy')}

    def run(feed):
        net = make_net(dev)
        net.train()
        st = FusedStep(net, cfg, deterministic=True)
        assert st.lr > 0
        seen = []
        for s in range(steps):
            st.step(feed(s), t_rand=t_rand[s])
            seen.append((st.loss3.clone(), st.flat.clone()))
        return seen

    rv = ResidentViews(dev, nrays=nrays, seed=SEED)
    rv.add('v', img, msk, K, R, T, sc.bounds, bound_mask=bm)

    def resident(s):
        b = dict(frame)
        b.update(rv.sample('v', s))
        return b

    def host(s):
        r = restate.sample_ray_train(img, msk, K, R, T, sc.bounds, nrays, bm, True, 0.5, 0.0, PhiloxDraws(SEED, s, 2))
        b = sc.batch_arrays(r['ray_o'], r['ray_d'], r['near'], r['far'], rgb=r['rgb'])
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b.items()}

    a = run(resident)
    b = run(host)
    assert rv.shortfall() == 0
    coords = [restate.sample_ray_train(img, msk, K, R, T, sc.bounds, nrays, bm, True, 0.5, 0.0,
                                       PhiloxDraws(SEED, s, 2))['coord'] for s in (0, 1)]
    assert not np.array_equal(coords[0], coords[1])  # the steps do see different rays
    for s in range(steps):
        for i, what in enumerate(('loss3', 'weights')):
            x, y = a[s][i], b[s][i]
            assert bool(torch.isfinite(x).all()), (s, what)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f'step {s}: {what} differ'
    assert not torch.equal(a[0][1], a[1][1])  # and the weights moved


def test_add_rejects_a_view_without_body_pixels(dev):
    from animatable_nerf_amd.data import ResidentViews
    g = _g12()
    rv = ResidentViews(dev, nrays=64)
    with pytest.raises(ValueError):
        rv.add('v', g['c1_img'], np.zeros_like(g['c1_msk']), g['c1_K'], g['c1_R'], g['c1_T'], g['bounds'],
               bound_mask=g['c1_bound_mask'])
    with pytest.raises(KeyError):
        rv.sample('v', 0)
