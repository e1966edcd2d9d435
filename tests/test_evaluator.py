"""CPU: the evaluator's yardstick (two independent float64 restatements of the reference's SSIM call agree),
the plugin loads the way the reference's ``make_evaluator`` loads it, and the host-side contract of
``anr_eval_workspace_bytes`` / ``anr_eval_frame`` (sizes, argument validation). No compute calls (no GPU)."""
import ctypes
import imp
import os
import sys

import pytest

from animatable_nerf_amd import _lib

from . import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'animatable_nerf_amd')


@pytest.mark.parametrize('name', ssim_ref.SHAPES)
@pytest.mark.parametrize('data_range', [2.0, 1.0])
def test_restatements_agree(name, data_range):
    """uniform_filter (the code scikit-image runs) against the brute-force window loop: 1e-12."""
    c = ssim_ref.reference(name)
    a = c['ssim'][data_range]
    b = ssim_ref.frame_ssim(c['pred'], c['gt'], c['mask'], c['H'], c['W'], data_range, ssim_ref.ssim_brute)
    print(name, data_range, a, b, abs(a - b))
    assert 0.9 < a < 1.0
    assert abs(a - b) <= 1e-12


def test_rects_are_the_shapes_the_kernels_need():
    assert ssim_ref.reference('diamond_37x53')['rect'] == (1, 1, 52, 36)
    assert ssim_ref.reference('full_64x64')['rect'] == (0, 0, 64, 64)
    assert ssim_ref.reference('polygon_70x131')['rect'][:2] == (5, 9)
    assert ssim_ref.reference('block7_20x20')['rect'][2:] == (7, 7)
    assert ssim_ref.reference('block8x40_12x60')['rect'][2:] == (40, 8)
    H, W, m = ssim_ref.shape_mask('narrow_6x30')
    assert ssim_ref.bounding_rect(m, H, W)[2:] == (30, 6)


def test_evaluator_loads_like_make_evaluator(monkeypatch):
    """make_evaluator: imp.load_source(cfg.evaluator_module, cfg.evaluator_path).Evaluator(), no GPU needed."""
    name = 'animatable_nerf_amd.evaluator'
    __import__(name)
    monkeypatch.setitem(sys.modules, name, sys.modules[name])  # imp.load_source replaces it: restore after
    ev = imp.load_source(name, os.path.join(PKG, 'evaluator.py')).Evaluator()
    assert ev.mse == [] and ev.psnr == [] and ev.ssim == []
    assert ev.cfg.get('eval_data_range') == 2.0 and ev.cfg.get('eval_write_images') is False
    for attr in ('evaluate', 'summarize', 'psnr_metric', 'ssim_metric'):
        assert callable(getattr(ev, attr))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def test_opts_defaults():
    o = _lib.EvalOpts()
    assert o.struct_size == ctypes.sizeof(_lib.EvalOpts) == 24
    assert o.data_range == 2.0 and o.win == 7


def test_workspace_positive_and_monotone(lib):
    sizes = [(7, 7), (20, 20), (37, 53), (64, 64), (70, 131), (512, 512), (1002, 1000), (1024, 1024)]
    got = [lib.anr_eval_workspace_bytes(h, w) for h, w in sizes]
    assert all(b > 0 for b in got)
    assert got == sorted(got)
    assert got[-1] > got[0]
    assert got[-1] >= 4 * 1024 * 1024  # at least the pixel -> ray-row map
    assert got[-1] < 64 * 2 ** 20
    assert lib.anr_eval_workspace_bytes(0, 10) == 0 and lib.anr_eval_workspace_bytes(10, -1) == 0


def test_argument_errors_do_not_launch(lib):
    """Rejected on the host before any HIP call: fake non-null pointers are never dereferenced."""
    P = ctypes.c_void_p
    one = P(256)
    H, W, n = 20, 20, 49
    ws = lib.anr_eval_workspace_bytes(H, W)
    o = _lib.EvalOpts()

    def call(pred=one, gt=one, n_rays=n, mask=one, h=H, w=W, opts=o, out=one, work=one, ws_bytes=ws):
        return lib.anr_eval_frame(pred, gt, n_rays, mask, h, w, ctypes.byref(opts) if opts is not None else None,
                                  out, None, None, None, None, work, ws_bytes, None)

    for kw in ({'pred': None}, {'gt': None}, {'mask': None}, {'out': None}, {'work': None}):
        assert call(**kw) == 2, kw
        assert b'NULL' in lib.anr_last_error()
    for kw in ({'n_rays': 0}, {'n_rays': -3}, {'h': 0}, {'w': -1}):
        assert call(**kw) == 2, kw
        assert b'positive' in lib.anr_last_error()
    assert call(ws_bytes=ws - 1) == 3 and b'workspace' in lib.anr_last_error()
    assert call(ws_bytes=0) == 3
    assert call(opts=_lib.EvalOpts(2.0, 11)) == 2 and b'win' in lib.anr_last_error()
    assert call(opts=_lib.EvalOpts(2.0, 0)) == 2
    assert call(opts=_lib.EvalOpts(0.0, 7)) == 2 and b'data_range' in lib.anr_last_error()
    bad = _lib.EvalOpts()
    bad.struct_size = 8
    assert call(opts=bad) == 2 and b'struct_size' in lib.anr_last_error()
