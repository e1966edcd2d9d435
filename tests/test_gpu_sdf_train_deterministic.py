"""Deterministic training mode on the sdf_pdf trainer (config 5): anr_sdf_train_step(_hooked) through
trainer_sdf.SdfStep / NetworkWrapper and anr_sdf_network_train_bwd through network_sdf.Network under
autograd. Same weights, batch, t_rand and iter_step -> the same bits on every run.

Scene: tests/test_gpu_sdf_train.py::test_sdf_train_step_larger_batch_matches_oracle's (pdf_scene, ~700 box
rays in one chunk, a mask_at_box with holes, iter_step 25000): its kept samples span several 512-sample
splits and several slab ranges and reach lin8's 257 outputs and the colour net's 289 inputs. "Equal" is
equality of the bit patterns (int32 views: NaN-safe, and tells -0 from +0)."""
import ctypes

import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib, trainer_sdf

from . import test_gpu_sdf_train as S
from ._common import golden, make_net_sdf, pdf_batch_np, pdf_scene, sdf_cfg, to_torch
from .test_oracle_sdf_train import g13_batch

pytestmark = pytest.mark.gpu

STEPS = 10
ENV = ('ANR_TRAIN_DETERMINISTIC', 'ANR_SDF_WG32', 'ANR_SDF_LG32', 'ANR_SDF_X3_PARTS', 'ANR_SDF_PACK_PLAN')
NL = trainer_sdf.NLOSS
KEY = {k: i for i, k in enumerate(trainer_sdf.LOSS_KEYS)}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    before = lib.anr_train_deterministic(-1)
    yield
    lib.anr_train_deterministic(before)


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


_batches = {}


def _batch(dev, rays):
    """the larger-batch test's scene at `rays` box rays (host arrays built once per size)"""
    if rays not in _batches:
        sc = pdf_scene()
        ro, rd = sc.box_rays(rays, seed=41)
        bnp, _ = pdf_batch_np(sc, ro, rd)
        R = bnp['ray_o'].shape[1]
        rng = np.random.default_rng(5)
        bnp['rgb'] = rng.random((1, R, 3)).astype(np.float32)
        bnp['mask_at_box'] = rng.random((1, R)) < 0.8
        _batches[rays] = bnp
    b = to_torch(_batches[rays], dev)
    b['iter_step'] = 25000
    return b


class Run:
    """per step the gradient blob (63 gradients, then the LOSS_KEYS floats); at the end weights and moments"""

    def __init__(self):
        self.blobs = []
        self.flat = self.m = self.v = self.sizes = self.step = None

    def loss(self, it):
        return self.blobs[it][-NL:]

    def views(self, it):
        out, off = [], 0
        for k in self.sizes:
            out.append(self.blobs[it][off:off + k])
            off += k
        return out


def _run(dev, prec, n=STEPS, rays=700, lr=None, det=True, mask_off=False, fixed=False, keep_step=False):
    b = _batch(dev, rays)
    if mask_off:
        b['mask_at_box'] = torch.zeros_like(b['mask_at_box'])
    tb0 = b['tbounds'].clone()
    R = int(b['ray_o'].shape[1])
    cfg = sdf_cfg()
    cfg.perturb = 1
    cfg.sdf_train_precision = prec
    net = make_net_sdf(dev)
    net.train()
    st = trainer_sdf.SdfStep(net, cfg, lr=lr, deterministic=det)
    assert st.deterministic is det
    assert st.lr > 0 or lr == 0.0
    g = torch.Generator(device='cpu')
    g.manual_seed(11)
    out = Run()
    out.sizes = [v.numel() for v in st.grad_views]
    t_rand = None
    for it in range(n):
        if t_rand is None or not fixed:
            t_rand = torch.rand((R, 64), generator=g).to(dev)
        b['tbounds'].copy_(tb0)  # the step widens them in place
        st.step(b, t_rand=t_rand)
        out.blobs.append(st.grad.detach().clone())
    torch.cuda.synchronize(dev)
    out.flat, out.m, out.v = st.flat.clone(), st.m.clone(), st.v.clone()
    if keep_step:
        out.step, out.batch, out.tb0, out.t_rand = st, b, tb0, t_rand
    return out


def _assert_identical(a, b, what):
    assert len(a.blobs) == len(b.blobs)
    for it, (x, y) in enumerate(zip(a.blobs, b.blobs)):
        if not _same(x, y):
            for i, (u, v) in enumerate(zip(a.views(it), b.views(it))):
                assert _same(u, v), f'{what}: first difference at (step {it}, tensor {i}), rel {_rel(u, v):.3e}'
            raise AssertionError(f'{what}: the losses differ at step {it}: {a.loss(it)} {b.loss(it)}')
    for name in ('flat', 'm', 'v'):
        assert _same(getattr(a, name), getattr(b, name)), f'{what}: {name} differs after the last step'


def _assert_sane(r, what):
    for it, blob in enumerate(r.blobs):
        assert bool(torch.isfinite(blob).all()), (what, it, r.loss(it))
    kept = [r.loss(it)[KEY['n_kept']].item() for it in range(len(r.blobs))]
    obs = [r.loss(it)[KEY['n_observed']].item() for it in range(len(r.blobs))]
    assert max(kept) > 0 and max(obs) > 0, (what, kept, obs)  # the observed-gradient branch ran


@pytest.mark.parametrize('prec', S.PRECS)
def test_same_run_twice(dev, prec):
    """10 steps at the cfg's lr, a fresh t_rand per step: every gradient, the losses, and at the end the
    weights and Adam moments are bit-identical between two runs"""
    a = _run(dev, prec)
    b = _run(dev, prec)
    _assert_sane(a, prec)
    _assert_identical(a, b, f'{prec}: two runs')


@pytest.mark.parametrize('env', ['ANR_SDF_WG32', 'ANR_SDF_LG32'])
def test_other_kernel_routes_are_reproducible(dev, monkeypatch, env):
    """ANR_SDF_WG32=0 (every exact weight gradient on the generic split-K kernel, launch_gemm_det) and
    ANR_SDF_LG32=0 (the exact forward / input-gradient products on k_gemm_t) each reproduce themselves.
    They need not equal the default route bit for bit: the split-K route sums a product in 512-sample
    splits (in steps of the generic kernel's k tile) where the slab kernel sums at most 64 sample ranges
    sized to fill the chip in 32-sample stages, and k_gemm_t accumulates a dot product over k in another
    order than k_lgemm's MFMA chain, so the fp32 rounding differs although the terms are the same."""
    monkeypatch.setenv(env, '0')
    a = _run(dev, 'fp32', n=3)
    b = _run(dev, 'fp32', n=3)
    _assert_sane(a, env)
    _assert_identical(a, b, f'{env}=0: two runs')


_oracles = {}


@pytest.mark.parametrize('prec', S.PRECS)
@pytest.mark.parametrize('case', ['g13', 'larger_batch'])
def test_parity_with_mode_on(dev, prec, case, monkeypatch):
    """tests/test_gpu_sdf_train.py's own comparisons against the reference step (G13) and the oracle, at its
    own tolerances (LOSS_RTOL 1e-4, GRAD_TOL 5e-3), with the library's mode on. The CPU oracle of a case
    (the same for both precisions, and only read by the comparison) is computed once."""
    oracle = S._oracle

    def shared(b, t_rand):
        if case not in _oracles:
            _oracles[case] = oracle(b, t_rand)
        return _oracles[case]
    monkeypatch.setattr(S, '_oracle', shared)
    with _lib.deterministic(True):
        if case == 'g13':
            S.test_g13_sdf_train_step_matches_reference_and_oracle(dev, prec)
        else:
            S.test_sdf_train_step_larger_batch_matches_oracle(dev, prec)
        assert _lib.load().anr_train_deterministic(-1) == 1


@pytest.mark.parametrize('prec', S.PRECS)
def test_edge_eight_rays(dev, prec):
    """8 box rays: most sample ranges and 512-sample splits are empty, so a reducer that read an unwritten
    slab or partial would show as a difference or a non-finite value"""
    a = _run(dev, prec, n=2, rays=8)
    b = _run(dev, prec, n=2, rays=8)
    for it in range(2):
        assert bool(torch.isfinite(a.blobs[it]).all()), (it, a.loss(it))
    assert a.loss(0)[KEY['n_kept']].item() > 0
    _assert_identical(a, b, f'{prec}: 8 rays')


@pytest.mark.parametrize('prec', S.PRECS)
def test_edge_no_ray_in_the_mask(dev, prec):
    """the 8-ray batch with mask_at_box all zero: img_loss = 0 / 0 as the reference's mse over an empty
    selection. Two runs agree, the NaN pattern of the losses is default mode's, every gradient is finite."""
    a = _run(dev, prec, n=1, rays=8, mask_off=True)
    b = _run(dev, prec, n=1, rays=8, mask_off=True)
    _assert_identical(a, b, f'{prec}: empty mask')
    d = _run(dev, prec, n=1, rays=8, mask_off=True, det=False)
    assert torch.equal(torch.isnan(a.loss(0)), torch.isnan(d.loss(0))), (a.loss(0), d.loss(0))
    assert bool(torch.isnan(a.loss(0)[KEY['img_loss']]))
    for r in (a, d):
        assert bool(torch.isfinite(r.blobs[0][:-NL]).all())


def _net_cfg(dev, det):
    from animatable_nerf_amd import network, network_sdf
    from ._common import state_dict_sdf_np
    cfg = sdf_cfg()
    cfg.train_deterministic = det
    net = network_sdf.Network(cfg)
    network.load_numpy_state(net, state_dict_sdf_np())
    net = net.to(dev)
    net.train()
    return net


def _free_samples(dev):
    """the G13 rays' 64 samples each as one Network.forward call, with fixed upstream weights"""
    from oracle import restate
    g = golden('g13_sdf_train')
    bt = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g13_batch(g).items()}
    t_rand = torch.from_numpy(g['t_rand'])[None].to(dev)  # G13's own samples: some have |sdf| < 0.02
    with torch.no_grad():
        pts, z = restate.sample_points(bt['ray_o'], bt['ray_d'], bt['near'], bt['far'], 64, t_rand)
        wpts = pts.reshape(-1, 3).contiguous()
        vd = bt['ray_d'][:, :, None].repeat(1, 1, 64, 1).reshape(-1, 3).contiguous()
        dists = torch.full((wpts.shape[0],), 0.005, device=dev)
    gen = torch.Generator(device='cpu').manual_seed(5)
    n = wpts.shape[0]
    d_raw = (torch.rand((n, 4), generator=gen) - 0.5).to(dev)
    d_sdf = (torch.rand((n,), generator=gen) - 0.5).to(dev)
    return bt, wpts, vd, dists, d_raw, d_sdf


def test_network_forward_under_autograd(dev):
    """network_sdf.Network.forward under autograd (anr_sdf_network_train_fwd / _bwd) with cfg
    train_deterministic: two passes into fresh gradients give the same bits"""
    bt, wpts, vd, dists, d_raw, d_sdf = _free_samples(dev)

    def once():
        net = _net_cfg(dev, True)
        b = dict(bt, tbounds=bt['tbounds'].clone())
        ret = net(wpts, vd, dists, b)
        loss = (ret['raw'][0] * d_raw).sum() + (ret['sdf'][0, :, 0] * d_sdf).sum() + (ret['resd'] ** 2).sum() \
            + ((ret['gradients'].norm(dim=-1) - 1) ** 2).sum()
        assert 'observed_gradients' in ret  # the second-order observed pass is part of what is compared
        loss = loss + ((ret['observed_gradients'].norm(dim=-1) - 1) ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()
        assert _lib.load().anr_train_deterministic(-1) == 0  # the scope restored the mode
        return [p.grad.clone() for p in net.parameters() if p.grad is not None]

    ga, gb = once(), once()
    assert len(ga) == len(gb) >= 60
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert bool(torch.isfinite(a).all()), i
        assert _same(a, b), (i, _rel(a, b))


@pytest.mark.parametrize('prec', S.PRECS)
def test_network_train_bwd_accumulates_in_fixed_order(dev, prec):
    """anr_sdf_network_train_bwd ACCUMULATES: called directly, a second pass added into the now non-zero
    buffers equals a fresh run of the same two passes bit for bit, and is about twice the first"""
    lib = _lib.load()
    bt, wpts, vd, dists, d_raw, d_sdf = _free_samples(dev)

    def direct():
        net = _net_cfg(dev, False)
        r = net._device()
        p = r.params()
        c = r._net_frame(bt)
        c['opts'].precision = {'fp32': _lib.FP32, 'bf16x3': _lib.BF16X3}[prec]
        wp, v, x = r._samples(wpts, vd, dists, dev)
        n = x.n_pts
        nbytes = lib.anr_sdf_network_train_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        raw = torch.empty((1, n, 4), device=dev)
        sdf = torch.empty((1, n, 1), device=dev)
        tb_out = torch.empty((2, 3), device=dev)
        grads = [torch.zeros_like(t) for t in net.tensors()]
        gp = (ctypes.c_void_p * _lib.NUM_SDF_TENSORS)(*[g.data_ptr() for g in grads])
        st = _lib.stream_ptr(dev)
        after = []
        with _lib.deterministic(True):
            for _ in range(2):
                _lib.check(lib.anr_sdf_network_train_fwd(ctypes.byref(p), ctypes.byref(c['frame']), ctypes.byref(x),
                                                         ctypes.byref(c['opts']), _lib.ptr(raw), _lib.ptr(sdf),
                                                         _lib.ptr(tb_out), _lib.ptr(ws), nbytes, st),
                           'anr_sdf_network_train_fwd')
                _lib.check(lib.anr_sdf_network_train_bwd(ctypes.byref(p), gp, ctypes.byref(c['frame']), ctypes.byref(x),
                                                         ctypes.byref(c['opts']), _lib.ptr(d_raw), _lib.ptr(d_sdf), None,
                                                         None, None, _lib.ptr(ws), nbytes, st),
                           'anr_sdf_network_train_bwd')
                torch.cuda.synchronize()
                after.append([g.clone() for g in grads])
        return after

    xa, xb = direct(), direct()
    for k in range(2):
        for i, (a, b) in enumerate(zip(xa[k], xb[k])):
            assert bool(torch.isfinite(a).all()), (k, i)
            assert _same(a, b), ('pass', k, i, _rel(a, b))
    big = max(range(len(xa[0])), key=lambda i: xa[0][i].abs().max().item())
    assert xa[0][big].abs().max().item() > 0
    assert _rel(xa[1][big], 2 * xa[0][big]) <= 2e-3


def test_toggle_between_steps(dev):
    """one SdfStep at lr = 0 on a fixed batch, `deterministic` flipped between steps: every deterministic
    step equals the first bit for bit; every default step stays inside test_gpu_sdf_train.py's bars
    (LOSS_RTOL, GRAD_TOL of each tensor's largest magnitude) relative to a default-mode reference step"""
    ref = _run(dev, 'fp32', n=1, lr=0.0, det=False, fixed=True)
    r = _run(dev, 'fp32', n=2, lr=0.0, fixed=True, keep_step=True)
    assert _same(r.blobs[0], r.blobs[1])
    st = r.step
    for mode in (False, True, False, False, True):
        st.deterministic = mode
        r.batch['tbounds'].copy_(r.tb0)
        st.step(r.batch, t_rand=r.t_rand)
        torch.cuda.synchronize(dev)
        blob = st.grad.detach().clone()
        if mode:
            assert _same(blob, r.blobs[0]), 'a deterministic step after a toggle differs'
            continue
        off = 0
        for i, k in enumerate(r.sizes):
            want = ref.blobs[0][off:off + k]
            err = (blob[off:off + k] - want).abs().max().item()
            assert err <= S.GRAD_TOL * want.abs().max().item() + 1e-9, (i, err)
            off += k
        la, lb = blob[-NL:-NL + 6].double(), ref.loss(0)[:6].double()
        assert bool(((la - lb).abs() <= S.LOSS_RTOL * lb.abs() + 1e-6).all()), (la, lb)
        assert torch.equal(blob[-NL + 6:], ref.loss(0)[6:])  # the counts are exact


def test_network_wrapper_with_cfg_key(dev):
    """trainer_sdf.NetworkWrapper with cfg train_deterministic = True on the G13 batch: two forward +
    backward passes give bit-identical .grad on every parameter"""
    g = golden('g13_sdf_train')
    b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g13_batch(g).items()}
    t_rand = torch.from_numpy(g['t_rand']).to(dev)

    def once():
        net = make_net_sdf(dev)
        net.train()
        cfg = sdf_cfg()
        cfg.perturb = 1
        cfg.train_deterministic = True
        w = trainer_sdf.NetworkWrapper(net, cfg)
        _, loss, _, _ = w(dict(b, tbounds=b['tbounds'].clone()), t_rand=t_rand)
        loss.backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters()], loss.detach().clone()

    (ga, la), (gb, lb) = once(), once()
    assert _same(la.reshape(1), lb.reshape(1))
    for i, (x, y) in enumerate(zip(ga, gb)):
        assert bool(torch.isfinite(x).all()), i
        assert _same(x, y), (i, _rel(x, y))
