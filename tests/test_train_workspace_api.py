"""CPU: every aninerf training entry point sizes its workspace from the same layout as its
*_workspace_bytes call and rejects a smaller one before any HIP call (no GPU needed), in the style of
test_capi.test_argument_errors_do_not_launch. The pointers are dummies that a rejected call never
dereferences."""
import ctypes
import os

import pytest

from animatable_nerf_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def test_training_entry_points_check_the_workspace_before_any_launch(lib):
    D = ctypes.c_void_p(1)
    n = 64  # rays, or free points
    o = _lib.RenderOpts(64, 2048, 0.05, 0.0, None, 0, _lib.BF16)
    p = _lib.Params()
    for i in range(_lib.NUM_TENSORS):
        p.t[i] = 1
    for i in range(_lib.NUM_NOVEL_TENSORS):
        p.novel[i] = 1
    f = _lib.Frame()
    for name in ('A', 'R', 'Th', 'pbw', 'pbounds', 'tbw', 'tbounds', 'latent_index', 'bw_latent_index'):
        setattr(f, name, 1)
    for i, d in enumerate((5, 6, 7)):
        f.pbw_dims[i] = d
        f.tbw_dims[i] = d
    out = _lib.RenderOut(1, 1, 1, None)
    x = _lib.Samples(1, 1, 1, n)
    grads = (ctypes.c_void_p * _lib.NUM_TENSORS)(*([1] * _lib.NUM_TENSORS))
    ngrads = (ctypes.c_void_p * _lib.NUM_NOVEL_TENSORS)(*([1] * _lib.NUM_NOVEL_TENSORS))
    P, F, O, OUT, X = ctypes.byref(p), ctypes.byref(f), ctypes.byref(o), ctypes.byref(out), ctypes.byref(x)
    train_ws = lib.anr_train_workspace_bytes(n, O, F)
    net_ws = lib.anr_network_train_workspace_bytes(n, O, F)
    pts_ws = lib.anr_points_workspace_bytes(n)
    anim_ws = lib.anr_anim_workspace_bytes(n)
    li = ctypes.c_void_p(1)
    # (entry point, the name its message carries, bytes needed, call with a workspace of `ws` bytes)
    cases = [
        ('anr_train_fwd', b'anr_train_fwd', train_ws,
         lambda ws: lib.anr_train_fwd(P, F, D, D, D, D, n, O, OUT, D, ws, None)),
        ('anr_train_bwd', b'anr_train_bwd', train_ws,
         lambda ws: lib.anr_train_bwd(P, grads, F, D, D, D, D, n, O, D, D, D, D, ws, None)),
        ('anr_train_step', b'anr_train_step', train_ws,
         lambda ws: lib.anr_train_step(P, grads, F, D, D, D, D, n, O, D, D, OUT, D, D, ws, None)),
        # the hooked step reports under the name of the step it is
        ('anr_train_step_hooked', b'anr_train_step', train_ws,
         lambda ws: lib.anr_train_step_hooked(P, grads, F, D, D, D, D, n, O, D, D, OUT, D, None, D, ws, None)),
        ('anr_network_train_fwd', b'anr_network_train_fwd', net_ws,
         lambda ws: lib.anr_network_train_fwd(P, F, X, O, D, D, ws, None)),
        ('anr_network_train_bwd', b'anr_network_train_bwd', net_ws,
         lambda ws: lib.anr_network_train_bwd(P, grads, F, X, O, D, D, D, D, ws, None)),
        ('anr_anim_step', b'anr_anim_step', anim_ws,
         lambda ws: lib.anr_anim_step(P, ngrads, F, D, n, D, n, O, D, D, ws, None)),
        ('anr_blend_weights', b'anr_blend_weights', pts_ws,
         lambda ws: lib.anr_blend_weights(P, 0, D, D, n, li, 1, D, D, ws, None)),
        ('anr_canonical_alpha', b'anr_canonical_alpha', pts_ws,
         lambda ws: lib.anr_canonical_alpha(P, D, n, D, D, ws, None)),
    ]
    for entry, who, needed, call in cases:
        assert needed > 0, entry
        assert call(needed - 1) == 3, (entry, lib.anr_last_error())
        err = lib.anr_last_error()
        assert who in err and b'workspace' in err, (entry, err)
        assert call(0) == 3, (entry, lib.anr_last_error())
