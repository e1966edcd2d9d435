"""Deterministic training mode (anr_train_deterministic, FusedStep(deterministic=True)): same seed, same
weights, same batches -> the same bits, whatever streams the executor uses.

Set up like test_gpu_train.py::test_grouped_wgrad_from_legacy_default_stream: quality.frame(64 k rays),
quality.make_net(cfg, 1234), a seeded generator for ray indices and t_rand, 1,024 rays per step (the
single-chunk count / scatter path at 64 blocks and capacity-sized grids), 20 steps at the cfg's lr > 0.
"Equal" below is equality of the bit patterns (int32 views: NaN-safe, and stricter than torch.equal
only in telling -0 from +0)."""
import ctypes

import pytest
import torch

from animatable_nerf_amd import _lib, config
from animatable_nerf_amd.trainer import FusedStep, NetworkWrapper

from . import test_gpu_train as T
from . import test_gpu_train_bf16 as B
from ._common import make_net
from .quality import frame, make_net as qnet, sub

pytestmark = pytest.mark.gpu

STEPS = 20
RAYS = 1024
EXEC_ENV = ('ANR_TRAIN_SERIAL', 'ANR_TRAIN_ON_CALLER', 'ANR_WG_DMA', 'ANR_WG_GROUP', 'ANR_TRAIN_GRAPH',
            'ANR_TRAIN_DETERMINISTIC')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def data(dev):
    return frame(dev, frame_rays=64 * 1024)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in EXEC_ENV:
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    before = lib.anr_train_deterministic(-1)
    yield
    lib.anr_train_deterministic(before)


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Run:
    """per step: the gradient blob (every gradient view, then loss3 in its tail) and m_rows; at the end
    the weights and Adam moments"""

    def __init__(self):
        self.blobs, self.m_rows = [], []
        self.flat = self.m = self.v = None
        self.sizes = None

    def loss3(self, it):
        return self.blobs[it][-4:-1]

    def views(self, it):
        out, off = [], 0
        for k in self.sizes:
            out.append(self.blobs[it][off:off + k])
            off += k
        return out


def _run(dev, data, prec, det=True, n=STEPS, rays=RAYS, lr=None, mask_off=False, fixed=False):
    batch, gt = data
    R = int(batch['ray_o'].shape[1])
    cfg = config.subject('aninerf_313', perturb=1, train_precision=prec)
    net = qnet(cfg, 1234, dev)
    net.train()
    st = FusedStep(net, cfg, lr=lr, deterministic=det)
    assert st.lr > 0 or lr == 0.0
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = Run()
    out.sizes = [v.numel() for v in st.grad_views]
    b = t_rand = None
    for it in range(n):
        if b is None or not fixed:
            idx = torch.randint(0, R, (rays,), device=dev, generator=g)
            t_rand = torch.rand((rays, 64), device=dev, generator=g)
            b = sub(batch, idx, gt[idx])
            if mask_off:
                b['mask_at_box'] = torch.zeros_like(b['mask_at_box'])
        st.step(b, t_rand=t_rand)
        out.blobs.append(st.grad.detach().clone())
        out.m_rows.append(st.renderer._counts(st.renderer._tws, rays)[1])
    torch.cuda.synchronize(dev)
    out.flat, out.m, out.v = st.flat.clone(), st.m.clone(), st.v.clone()
    out.step = st
    return out


def _assert_identical(a, b, what):
    assert len(a.blobs) == len(b.blobs)
    for it, (x, y) in enumerate(zip(a.blobs, b.blobs)):
        if not _same(x, y):
            for i, (u, v) in enumerate(zip(a.views(it), b.views(it))):
                assert _same(u, v), f'{what}: first difference at (step {it}, tensor {i}), rel {T._rel(u, v):.3e}'
            assert _same(a.loss3(it), b.loss3(it)), f'{what}: loss3 differs at step {it}: {a.loss3(it)} {b.loss3(it)}'
            raise AssertionError(f'{what}: gradient blob differs at step {it}')
    for i, name in enumerate(('flat', 'm', 'v')):
        assert _same(getattr(a, name), getattr(b, name)), f'{what}: {name} differs after the last step'


def _assert_sane(r):
    for it, blob in enumerate(r.blobs):
        l3 = r.loss3(it)
        assert bool(torch.isfinite(l3).all()), (it, l3)
        if r.m_rows[it] > 1:
            assert l3[2].item() > 0, (it, l3, r.m_rows[it])
        assert bool(torch.isfinite(blob).all()), it


_cache = {}


def _default_exec(dev, data, prec):
    """the 20 deterministic steps on the default executor, run once per precision"""
    if prec not in _cache:
        _cache[prec] = _run(dev, data, prec)
        _cache[prec].step = None
    return _cache[prec]


@pytest.mark.parametrize('prec', ['fp32', 'bf16', 'bf16_all'])
def test_same_run_twice(dev, data, prec):
    a = _default_exec(dev, data, prec)
    b = _run(dev, data, prec)
    _assert_sane(a)
    _assert_identical(a, b, f'{prec}: two runs')


@pytest.mark.parametrize('env', [('ANR_TRAIN_SERIAL', '1'), ('ANR_TRAIN_ON_CALLER', '0')])
@pytest.mark.parametrize('prec', ['fp32', 'bf16_all'])
def test_executor_independence(dev, data, monkeypatch, prec, env):
    """One stream for everything (ANR_TRAIN_SERIAL=1) and the fork onto the library's own main stream
    (ANR_TRAIN_ON_CALLER=0) give the default executor's bits: exact, no 'up to atomics order'."""
    ref = _default_exec(dev, data, prec)
    monkeypatch.setenv(*env)
    got = _run(dev, data, prec)
    _assert_identical(ref, got, f'{prec}: default executor vs {env[0]}={env[1]}')


@pytest.mark.parametrize('env', [('ANR_WG_DMA', '0'), ('ANR_WG_GROUP', '0')])
def test_other_wgrad_kernels_are_reproducible(dev, data, monkeypatch, env):
    """ANR_WG_DMA=0 and ANR_WG_GROUP=0 legitimately use another summation tree than the default, so they
    need not (and do not) equal it bitwise; each must equal itself over two runs. Why the trees differ:
    a product's sample ranges are summed in range order, but the NUMBER of ranges differs — the grouped
    launcher gives k_wgrad_dma products up to 32 ranges sized to fill the chip with one workgroup per
    (product, range), k_wgrad_group products (ANR_WG_DMA=0) up to 64 ranges sized per 128 x 128 tile, and
    the ungrouped launch_wgrad (ANR_WG_GROUP=0) one range per 384 samples of capacity — and the kernels walk
    a range in different step sizes (64-row stages vs 32-sample MFMA steps), which changes the fp32
    accumulation order inside a range too."""
    ref = _default_exec(dev, data, 'bf16_all')
    monkeypatch.setenv(*env)
    a = _run(dev, data, 'bf16_all')
    b = _run(dev, data, 'bf16_all')
    _assert_sane(a)
    _assert_identical(a, b, f'bf16_all {env[0]}={env[1]}: two runs')
    # and the mode still only reorders sums: step 0 within the order-noise bound of the default tree
    for i, (u, v) in enumerate(zip(a.views(0), ref.views(0))):
        assert T._rel(u, v) <= 2e-3, (i, T._rel(u, v))


@pytest.mark.parametrize('prec', ['fp32', 'bf16', 'bf16_all'])
def test_mode_changes_only_the_order(dev, data, prec):
    """step 0 from identical weights: deterministic vs default mode within the existing step-0 bound of
    test_grouped_wgrad_from_legacy_default_stream (2e-3 of each tensor's max), losses within 2e-5"""
    det = _default_exec(dev, data, prec)
    dflt = _run(dev, data, prec, det=False, n=1)
    for i, (a, b) in enumerate(zip(det.views(0), dflt.views(0))):
        assert T._rel(a, b) <= 2e-3, (i, T._rel(a, b))
    la, lb = det.loss3(0).double(), dflt.loss3(0).double()
    assert bool(((la - lb).abs() <= 2e-5 * lb.abs()).all()), (la, lb)


def test_parity_fp32_oracle_with_mode_on(dev):
    """test_gpu_train.py::test_gradients_match_oracle's own checks (split API through NetworkWrapper, G4's
    256-ray batch, its tolerances) with the library's mode on"""
    with _lib.deterministic(True):
        T.test_gradients_match_oracle(dev)
        assert _lib.load().anr_train_deterministic(-1) == 1


@pytest.mark.parametrize('policy', ['bf16', 'bf16_all'])
def test_parity_bf16_oracle_with_mode_on(dev, policy):
    """the default-executor case ('chains') of test_gpu_train_bf16.py, its comparison and tolerances"""
    _, bt, t_rand = T._g4_batch(dev)
    net = make_net(dev)
    net.train()
    step = FusedStep(net, B._cfg(policy), lr=0.0, deterministic=True)
    loss3 = step.step(bt, t_rand=t_rand.to(dev)).clone()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    B._compare(f'{policy}/chains/deterministic', loss3[:3].cpu(), grads, policy)


@pytest.mark.parametrize('prec', ['fp32', 'bf16_all'])
def test_edge_eight_rays(dev, data, prec):
    """8 rays of the frame: most sample ranges (and most 512-sample splits) are empty, so a reducer that
    read an unwritten slab or partial would show as a difference or a non-finite value"""
    a = _run(dev, data, prec, n=2, rays=8)
    b = _run(dev, data, prec, n=2, rays=8)
    _assert_sane(a)
    _assert_identical(a, b, f'{prec}: 8 rays')


@pytest.mark.parametrize('prec', ['fp32', 'bf16_all'])
def test_edge_no_ray_in_the_mask(dev, data, prec):
    """the 8-ray batch with mask_at_box all zero (quality.sub gathers in-box rays only, so it cannot make a
    batch that misses the box). Existing semantics, as the reference's mse over an empty selection:
    img_loss = 0 / 0 = NaN and so is the total; bw_loss is finite; the image loss sends no gradient, so
    every gradient is finite. Default mode gives the same NaN pattern and bw_loss."""
    a = _run(dev, data, prec, n=1, rays=8, mask_off=True)
    b = _run(dev, data, prec, n=1, rays=8, mask_off=True)
    _assert_identical(a, b, f'{prec}: empty mask')
    d = _run(dev, data, prec, det=False, n=1, rays=8, mask_off=True)
    for r in (a, d):
        l3 = r.loss3(0)
        assert bool(torch.isnan(l3[0])) and bool(torch.isnan(l3[1])), l3
        assert bool(torch.isfinite(l3[2])) and (l3[2].item() > 0 or r.m_rows[0] <= 1), (l3, r.m_rows)
        assert bool(torch.isfinite(r.blobs[0][:-4]).all())
    assert abs(a.loss3(0)[2].item() - d.loss3(0)[2].item()) <= 2e-5 * abs(d.loss3(0)[2].item())
    for i, (u, v) in enumerate(zip(a.views(0), d.views(0))):
        assert T._rel(u, v) <= 2e-3, (i, T._rel(u, v))


def test_graph_replay(dev, data, monkeypatch):
    """ANR_TRAIN_GRAPH=1 with the mode on, one fixed batch: the steps (issued eagerly, captured, replayed)
    equal four eager deterministic steps bit for bit; and the graph cache keys on the mode."""
    eager = _run(dev, data, 'bf16_all', n=4, fixed=True)
    monkeypatch.setenv('ANR_TRAIN_GRAPH', '1')
    graph = _run(dev, data, 'bf16_all', n=4, fixed=True)
    _assert_identical(eager, graph, 'graph replay vs eager')
    # toggling: lr = 0 keeps the weights, so every deterministic step must give the same bits and every
    # default-mode step must stay within the order-noise bound of a default-mode eager reference
    monkeypatch.setenv('ANR_TRAIN_GRAPH', '0')
    ref = _run(dev, data, 'bf16_all', det=False, n=1, lr=0.0, fixed=True)
    monkeypatch.setenv('ANR_TRAIN_GRAPH', '1')
    r = _run(dev, data, 'bf16_all', n=3, lr=0.0, fixed=True)  # eager, capture, replay (deterministic)
    st = r.step
    batch, gt = data
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    idx = torch.randint(0, int(batch['ray_o'].shape[1]), (RAYS,), device=dev, generator=g)
    t_rand = torch.rand((RAYS, 64), device=dev, generator=g)
    b = sub(batch, idx, gt[idx])
    assert _same(r.blobs[0], r.blobs[1]) and _same(r.blobs[0], r.blobs[2])
    for mode in (False, False, False, True, False, True):
        st.deterministic = mode
        st.step(b, t_rand=t_rand)
        torch.cuda.synchronize(dev)
        blob = st.grad.detach().clone()
        if mode:
            assert _same(blob, r.blobs[0]), 'a deterministic step after a toggle differs'
        else:
            off = 0
            for i, k in enumerate(r.sizes):
                assert T._rel(blob[off:off + k], ref.blobs[0][off:off + k]) <= 2e-3, i
                off += k
            la, lb = blob[-4:-1].double(), ref.loss3(0).double()
            assert bool(((la - lb).abs() <= 2e-5 * lb.abs()).all()), (la, lb)


def test_split_api(dev):
    """anr_train_fwd + anr_train_bwd on G4's batch with the mode on. Through NetworkWrapper: two passes give
    the same bits. The entry point ACCUMULATES, so it is also called directly: one pass into zeroed
    gradients and a second pass added into the same (now non-zero) buffers equals a fresh run of the same
    two passes."""
    from animatable_nerf_amd.renderer import _Call
    _, bt, t_rand = T._g4_batch(dev)
    t_rand = t_rand.to(dev)
    lib = _lib.load()

    def wrapped(policy):
        net = make_net(dev)
        net.train()
        cfg = B._cfg(policy)
        cfg.train_deterministic = True
        wrap = NetworkWrapper(net, cfg)
        wrap(bt, t_rand=t_rand)[1].backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters()]

    def direct(policy):
        net = make_net(dev)
        net.train()
        r = NetworkWrapper(net, B._cfg(policy)).renderer
        p = r.params(pack=False)
        c = _Call(r, bt, t_rand)
        nbytes = lib.anr_train_workspace_bytes(c.R, ctypes.byref(c.opts), ctypes.byref(c.frame))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        grads = [torch.zeros_like(t) for t in net.core_tensors()]
        gp = (ctypes.c_void_p * _lib.NUM_TENSORS)(*[g.data_ptr() for g in grads])
        gen = torch.Generator(device='cpu').manual_seed(5)
        d_rgb = (torch.rand((c.R, 3), generator=gen) - 0.5).to(dev)
        after = []
        with _lib.deterministic(True):
            for _ in range(2):
                _lib.check(lib.anr_train_fwd(ctypes.byref(p), ctypes.byref(c.frame), *c.ray_ptrs(), c.R,
                                             ctypes.byref(c.opts), ctypes.byref(c.out), _lib.ptr(ws), nbytes,
                                             _lib.stream_ptr(dev)), 'anr_train_fwd')
                _lib.check(lib.anr_train_bwd(ctypes.byref(p), gp, ctypes.byref(c.frame), *c.ray_ptrs(), c.R,
                                             ctypes.byref(c.opts), _lib.ptr(d_rgb), None, None, _lib.ptr(ws), nbytes,
                                             _lib.stream_ptr(dev)), 'anr_train_bwd')
                torch.cuda.synchronize()
                after.append([g.clone() for g in grads])
        return after

    for policy in ('fp32', 'bf16_all'):
        ga, gb = wrapped(policy), wrapped(policy)
        for i, (a, b) in enumerate(zip(ga, gb)):
            assert bool(torch.isfinite(a).all()), (policy, i)
            assert _same(a, b), (policy, i, T._rel(a, b))
        xa, xb = direct(policy), direct(policy)
        for k in range(2):
            for i, (a, b) in enumerate(zip(xa[k], xb[k])):
                assert _same(a, b), (policy, 'pass', k, i, T._rel(a, b))
        # the second pass really accumulated (into non-zero contents): about twice the first
        big = max(range(len(xa[0])), key=lambda i: xa[0][i].abs().max().item())
        assert T._rel(xa[1][big], 2 * xa[0][big]) <= 2e-3
