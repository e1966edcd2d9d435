"""CPU: the aligned_aninerf_lbw render entries are declared and exported, size their workspace and reject bad
arguments before any HIP call (these run where there is no GPU: a HIP call would return ANR_E_HIP instead), the
network plugin has the reference's state_dict names and shapes (golden G16, dumped from the real reference by
tools/gen_golden_lbw.py) and loads under a stand-in ``lib.config`` the way the reference's factories load it."""
import ctypes
import imp
import json
import os
import sys
import types

import pytest
import torch

from animatable_nerf_amd import _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'animatable_nerf_amd')
G16 = os.path.join(ROOT, 'tests', 'golden', 'g16_state_dict.json')
E_ARG, E_WORKSPACE = 2, 3
ENTRIES = ('anr_lbw_render_workspace_bytes', 'anr_lbw_render_fwd', 'anr_lbw_render_counts', 'anr_lbw_render_rows')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def _opts(n_samples=64, precision=_lib.FP32, novel=0):
    return _lib.RenderOpts(n_samples, 2048, 0.05, 0.0, None, novel, precision)


def _valid(n_verts=6890):
    """Structs with non-NULL (never dereferenced) pointers everywhere."""
    one = ctypes.c_void_p(256)
    p = _lib.LbwParams()
    for i in range(_lib.NUM_LBW_TENSORS):
        p.t[i] = 256
    f = _lib.LbwFrame(one, one, one, one, one, one, one, n_verts, one, one)
    out = _lib.LbwRenderOut(one, one, one, one, one)
    return p, f, out, one


def _fwd(lib, p, f, out, o, ws, ws_bytes, n_rays=10, image=0, ray=ctypes.c_void_p(256)):
    return lib.anr_lbw_render_fwd(ctypes.byref(p) if p is not None else None, ctypes.byref(f), ray, ray, ray, ray,
                                  n_rays, ctypes.byref(o), ctypes.byref(out), image, ws, ws_bytes, None)


def test_exports(lib):
    for name in ENTRIES + ('anr_lbw_render_knn',):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    header = open(os.path.join(ROOT, 'include', 'aninerf.h')).read()
    for name in ENTRIES:
        assert name + '(' in header, name
    assert '#define ANR_LBW_NUM_TENSORS 62' in header and _lib.NUM_LBW_TENSORS == 62


def test_workspace_bytes_is_host_arithmetic(lib):
    o = _opts()
    a = lib.anr_lbw_render_workspace_bytes(64, ctypes.byref(o), 0)
    b = lib.anr_lbw_render_workspace_bytes(4136, ctypes.byref(o), 0)
    img = lib.anr_lbw_render_workspace_bytes(4136, ctypes.byref(o), 1)
    assert 0 < a < b
    # an image-only call carries no pbw / tbw rows, no alpha_ind state and no second search
    assert img + 2 * 4136 * 64 * 24 * 4 < b
    assert lib.anr_lbw_render_workspace_bytes(0, ctypes.byref(o), 0) == 0
    assert lib.anr_lbw_render_workspace_bytes(64, None, 0) == 0
    assert lib.anr_lbw_render_workspace_bytes(262144, ctypes.byref(o), 0) < 16 * 2 ** 30
    assert not lib.anr_lbw_render_counts(None, 64, ctypes.byref(o), 0)


def test_batch_override_changes_only_the_batch_buffers(lib, monkeypatch):
    o = _opts()
    full = lib.anr_lbw_render_workspace_bytes(4136, ctypes.byref(o), 0)
    monkeypatch.setenv('ANR_LBW_BATCH', '1024')
    small = lib.anr_lbw_render_workspace_bytes(4136, ctypes.byref(o), 0)
    assert 0 < small < full
    monkeypatch.setenv('ANR_LBW_BATCH', '1000')  # not a multiple of 256: ignored
    assert lib.anr_lbw_render_workspace_bytes(4136, ctypes.byref(o), 0) == full


def test_rejections_come_before_any_hip_call(lib):
    p, f, out, ws = _valid()
    o = _opts()
    big = 1 << 40
    assert _fwd(lib, None, f, out, o, ws, big) == E_ARG and b'NULL' in lib.anr_last_error()
    q = _lib.LbwParams()
    assert _fwd(lib, q, f, out, o, ws, big) == E_ARG and b'NULL parameter tensor' in lib.anr_last_error()
    _, f2, _, _ = _valid(n_verts=6913)
    assert _fwd(lib, p, f2, out, o, ws, big) == E_ARG and b'n_verts' in lib.anr_last_error()
    _, f0, _, _ = _valid(n_verts=0)
    assert _fwd(lib, p, f0, out, o, ws, big) == E_ARG and b'n_verts' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(n_samples=128), ws, big) == E_ARG and b'N_samples' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(novel=1), ws, big) == E_ARG and b'novel' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(precision=_lib.BF16), ws, big) == E_ARG and b'precision' in lib.anr_last_error()
    need = lib.anr_lbw_render_workspace_bytes(10, ctypes.byref(o), 0)
    assert _fwd(lib, p, f, out, o, ws, need - 1) == E_WORKSPACE and b'workspace' in lib.anr_last_error()
    # an image-only call needs no tvertices; a full one does
    f.tvertices = None
    assert _fwd(lib, p, f, out, o, ws, big) == E_ARG and b'frame' in lib.anr_last_error()
    need_img = lib.anr_lbw_render_workspace_bytes(10, ctypes.byref(o), 1)
    assert _fwd(lib, p, f, out, o, ws, need_img - 1, image=1) == E_WORKSPACE
    assert lib.anr_lbw_render_rows(None, 10, ctypes.byref(o), None, None, None, None) == E_ARG


def test_state_dict_matches_reference():
    from animatable_nerf_amd import network_lbw
    g = json.load(open(G16))
    net = network_lbw.Network(config.subject('aligned_aninerf_lbw_s9p'))
    ours = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert ours == [[k, list(v)] for k, v in g.items()]
    assert len(net.tensors()) == _lib.NUM_LBW_TENSORS
    assert [tuple(t.shape) for t in net.tensors()] == [tuple(v) for v in g.values()]


def test_animation_checkpoints_load():
    """cfg.aninerf_animation adds novel_pose_bw (BackwardBlendWeight, num_eval_frame rows) after the 62 tensors."""
    from animatable_nerf_amd import network_lbw
    cfg = config.subject('aligned_aninerf_lbw_s9p', aninerf_animation=True)
    net = network_lbw.Network(cfg)
    names = list(net.state_dict())
    assert names[:62] == list(json.load(open(G16)))
    assert names[62] == 'novel_pose_bw.bw_latent.weight' and len(names) == 62 + 19
    assert tuple(net.novel_pose_bw.bw_latent.weight.shape) == (133, 128)
    assert tuple(net.novel_pose_bw.bw_linears[5].weight.shape) == (256, 447, 1)
    assert len(net.tensors()) == 62
    net2 = network_lbw.Network(cfg)
    net2.load_state_dict(net.state_dict(), strict=True)


def test_preset_and_unsupported_options():
    from animatable_nerf_amd import network_lbw, renderer_lbw
    cfg = config.subject('aligned_aninerf_lbw_s9p')
    assert cfg.num_train_frame == 260 and cfg.num_latent_code == 260 and cfg.norm_th == 0.05
    assert cfg.tpose_viewdir and cfg.use_bigpose
    with pytest.raises(ValueError, match='tpose_viewdir'):
        network_lbw.Network(config.subject('aligned_aninerf_lbw_s9p', tpose_viewdir=False))
    with pytest.raises(ValueError, match='color_with_viewdir'):
        network_lbw.Network(config.subject('aligned_aninerf_lbw_s9p', color_with_viewdir=False))
    with pytest.raises(ValueError, match='render_precision'):
        renderer_lbw._lbw_precision(config.subject('aligned_aninerf_lbw_s9p', render_precision='bf16'))
    assert renderer_lbw._lbw_precision(config.subject('aligned_aninerf_lbw_s9p', render_precision='bf16x6')) == _lib.BF16X6
    net = network_lbw.Network(cfg)
    with pytest.raises(NotImplementedError):
        net.get_alpha(None, None)


@pytest.fixture
def ref_cfg(monkeypatch):
    cfg = config.CfgNode({'N_samples': 64, 'N_rand': 1024, 'perturb': 1, 'norm_th': 0.05, 'train_th': 0.0,
                          'num_train_frame': 60, 'num_eval_frame': 1000, 'num_latent_code': 60,
                          'aninerf_animation': False, 'test_novel_pose': False, 'white_bkgd': False,
                          'tpose_viewdir': True, 'use_bigpose': True})
    lib = types.ModuleType('lib')
    lib.__path__ = []
    libcfg = types.ModuleType('lib.config')
    libcfg.cfg = cfg
    lib.config = libcfg
    monkeypatch.setitem(sys.modules, 'lib', lib)
    monkeypatch.setitem(sys.modules, 'lib.config', libcfg)
    for m in ('network_lbw', 'renderer_lbw'):  # imp.load_source replaces the package's modules: restore them
        name = 'animatable_nerf_amd.' + m
        __import__(name)
        monkeypatch.setitem(sys.modules, name, sys.modules[name])
    return cfg


def test_plugins_read_the_reference_cfg(ref_cfg):
    load = lambda m: imp.load_source('animatable_nerf_amd.' + m, os.path.join(PKG, m + '.py'))
    net = load('network_lbw').Network()
    sd = net.state_dict()
    assert tuple(sd['bw_latent.weight'].shape) == (61, 128)
    assert tuple(sd['tpose_human.color_network.color_latent.weight'].shape) == (60, 128)
    r = load('renderer_lbw').Renderer(net)
    assert r.cfg.norm_th == 0.05 and r.cfg.get('render_precision') == 'fp32'
    ref_cfg.perturb = 0  # run.py:50, after make_network
    assert r.cfg.perturb == 0
    with pytest.raises(RuntimeError, match='GPU'):
        r.render_device({'ray_o': torch.zeros(1, 4, 3)})
