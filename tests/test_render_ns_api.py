"""CPU: the entries of the render at 64, 128, 192 or 256 samples per ray (anr_render_ns_workspace_bytes /
anr_render_ns_fwd / anr_render_ns_bw_rows / anr_render_ns_row_ids) are declared and exported, size their
workspaces with n_rays * n_samples (at 64 exactly as the 64-sample entries do), and reject bad arguments before
any HIP call (dummy pointers, no GPU needed); the Python callers refuse other sample counts, and the 64-only
paths say so, before any library call."""
import ctypes
import os
import re

import pytest

from animatable_nerf_amd import _lib, config

ARG, WORKSPACE = 2, 3
BIG = 1 << 44
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aninerf.h')
SYMBOLS = ('anr_render_ns_workspace_bytes', 'anr_render_ns_fwd', 'anr_render_ns_bw_rows', 'anr_render_ns_row_ids')
RAYS = (1, 29, 2048, 262144)
SAMPLES = (64, 128, 192, 256)
BAD_SAMPLES = (0, -64, 32, 96, 100, 320)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def p(v):
    return ctypes.c_void_p(v) if v else None


def frame(tbw=True, **kw):
    """a frame of dummy non-NULL device pointers (never dereferenced when the call is rejected)"""
    f = _lib.Frame()
    f.A, f.R, f.Th, f.pbw, f.pbounds, f.tbounds, f.latent_index, f.bw_latent_index = (1,) * 8
    for i, d in enumerate((20, 30, 10)):
        f.pbw_dims[i] = d
    if tbw:
        f.tbw = 1
        for i, d in enumerate((24, 28, 12)):
            f.tbw_dims[i] = d
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def opts(n_samples=128, chunk=2048, novel_pose=0):
    o = _lib.RenderOpts()
    o.n_samples, o.chunk, o.norm_th, o.train_th, o.novel_pose, o.precision = n_samples, chunk, 0.05, 0.0, novel_pose, 0
    return o


def size(lib, R, o, f, image):
    return lib.anr_render_ns_workspace_bytes(R, ctypes.byref(o) if o is not None else None,
                                             ctypes.byref(f) if f is not None else None, image)


def fwd(lib, image=0, params=True, f=True, o=True, out=True, ws=1, ws_bytes=BIG, n_rays=300, rays=(1, 1, 1, 1),
        packed=1, maps=(1, 1, 1), fr=None, op=None):
    pr = _lib.Params()
    pr.packed = packed
    fr = fr if fr is not None else frame(tbw=not image)
    op = op if op is not None else opts()
    ro = _lib.RenderOut(*maps, None)
    return lib.anr_render_ns_fwd(ctypes.byref(pr) if params else None, ctypes.byref(fr) if f else None,
                                 *[p(r) for r in rays], n_rays, ctypes.byref(op) if o else None,
                                 ctypes.byref(ro) if out else None, image, p(ws), ws_bytes, None)


def test_symbols_declared_and_exported(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r'\b(anr_[a-z_0-9]+)\s*\(', src))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTS, s
        assert getattr(lib, s) is not None
    assert lib.anr_version() == 2


@pytest.mark.parametrize('image', [0, 1])
def test_workspace_bytes(lib, image):
    f = frame()
    table = {}
    for ns in SAMPLES:
        for R in RAYS:
            a = size(lib, R, opts(ns), f, image)
            assert a > 0 and a % 256 == 0, (ns, R, a)
            table[ns, R] = a
    for ns in SAMPLES:  # strictly growing with the rays ...
        row = [table[ns, R] for R in RAYS]
        assert all(x < y for x, y in zip(row, row[1:])), (ns, row)
    for R in RAYS:  # ... and with the samples
        col = [table[ns, R] for ns in SAMPLES]
        assert all(x < y for x, y in zip(col, col[1:])), (R, col)
    # at 64 samples: the 64-sample entry's size
    old = lib.anr_render_image_workspace_bytes if image else lib.anr_render_workspace_bytes
    for R in RAYS:
        for chunk in (8, 2048, 1 << 20):
            o = opts(64, chunk)
            assert size(lib, R, o, f, image) == old(R, ctypes.byref(o), ctypes.byref(f)), (R, chunk)
    # bad arguments
    assert size(lib, 300, None, f, image) == 0
    assert size(lib, 300, opts(), None, image) == 0
    assert size(lib, 0, opts(), f, image) == 0
    assert size(lib, -1, opts(), f, image) == 0
    assert size(lib, 300, opts(chunk=0), f, image) == 0
    for ns in BAD_SAMPLES:
        assert size(lib, 300, opts(ns), f, image) == 0, ns
    bad = frame()
    bad.pbw_dims[1] = 0
    assert size(lib, 300, opts(), bad, image) == 0


def test_image_size_below_full_and_without_tbw(lib):
    f = frame()
    f0, f1 = frame(tbw=False), frame()
    for i in range(3):
        f1.tbw_dims[i] = 512
    for ns in SAMPLES:
        for R in RAYS:
            o = opts(ns)
            img, full = size(lib, R, o, f, 1), size(lib, R, o, f, 0)
            assert 0 < img <= full - 2 * R * ns * 96, (ns, R, img, full)  # the pbw / tbw rows at the least
            assert size(lib, R, o, f0, 1) == img == size(lib, R, o, f1, 1)
            assert size(lib, R, o, f1, 0) > full  # the full program's does hold the T-pose volume
    assert size(lib, 300, opts(), f0, 0) == 0  # which it cannot do without


@pytest.mark.parametrize('image', [0, 1])
@pytest.mark.parametrize('ns', BAD_SAMPLES)
def test_rejected_sample_counts(lib, image, ns):
    assert fwd(lib, image, op=opts(ns)) == ARG
    msg = lib.anr_last_error()
    assert b'N_samples' in msg and b'64, 128, 192 or 256' in msg, msg
    for fn in (lib.anr_render_ns_bw_rows, lib.anr_render_ns_row_ids):
        args = (p(1), 300, ns, p(1), p(1), None) if fn is lib.anr_render_ns_bw_rows else (p(1), 300, ns, p(1), None)
        assert fn(*args) == ARG and b'N_samples' in lib.anr_last_error()


@pytest.mark.parametrize('image', [0, 1])
@pytest.mark.parametrize('kw', [dict(params=False), dict(f=False), dict(o=False), dict(out=False), dict(ws=0),
                                dict(rays=(0, 1, 1, 1)), dict(rays=(1, 0, 1, 1)), dict(rays=(1, 1, 0, 1)),
                                dict(rays=(1, 1, 1, 0)), dict(maps=(0, 1, 1)), dict(maps=(1, 0, 1)),
                                dict(maps=(1, 1, 0)), dict(packed=0)])
def test_null_arguments(lib, image, kw):
    assert fwd(lib, image, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('image', [0, 1])
@pytest.mark.parametrize('field', ['A', 'R', 'Th', 'pbw', 'pbounds', 'tbounds', 'latent_index', 'tbw'])
def test_null_frame_tensors(lib, image, field):
    fr = frame()
    setattr(fr, field, None)
    if image and field == 'tbw':  # not an argument of the image program: the next complaint is the workspace
        assert fwd(lib, image, fr=fr, ws_bytes=1) == WORKSPACE
        assert fwd(lib, image, fr=frame(tbw=False), ws_bytes=1) == WORKSPACE
        return
    assert fwd(lib, image, fr=fr) == ARG
    assert b'NULL frame tensor' in lib.anr_last_error()


@pytest.mark.parametrize('image', [0, 1])
@pytest.mark.parametrize('ns', SAMPLES)
def test_sizes_and_workspace(lib, image, ns):
    assert fwd(lib, image, op=opts(ns, chunk=0)) == ARG and b'chunk' in lib.anr_last_error()
    assert fwd(lib, image, op=opts(ns, chunk=-5)) == ARG
    assert fwd(lib, image, op=opts(ns), n_rays=0) == ARG and b'n_rays' in lib.anr_last_error()
    assert fwd(lib, image, op=opts(ns), n_rays=-3) == ARG
    most = (0x7fffffff // 24) // ns  # 24 n_rays n_samples stays below 2^31
    assert fwd(lib, image, op=opts(ns), n_rays=most + 1) == ARG and b'too many rays' in lib.anr_last_error()
    assert most >= 512 * 512  # a 512 x 512 frame fits at every count
    bad = frame()
    bad.pbw_dims[2] = 0
    assert fwd(lib, image, op=opts(ns), fr=bad) == ARG and b'dims' in lib.anr_last_error()
    assert fwd(lib, image, op=opts(ns, novel_pose=1)) == ARG and b'novel_pose' in lib.anr_last_error()
    assert fwd(lib, image, op=opts(ns), fr=frame(n_views=2)) == ARG and b'views' in lib.anr_last_error()
    assert fwd(lib, image, op=opts(ns), fr=frame(n_views=-1)) == ARG
    # a short workspace; out.raw is NULL here, so the size with raw inside is the one to meet
    f, o = frame(), opts(ns)
    need = size(lib, 300, o, f, image)
    assert fwd(lib, image, op=o, fr=f, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    assert fwd(lib, image, op=o, fr=f, ws_bytes=0) == WORKSPACE
    assert fwd(lib, image, op=o, fr=f, n_rays=most, ws_bytes=need) == WORKSPACE  # the largest count gets to the size


def test_old_entries_still_take_64_only(lib):
    """the 64-sample entries keep their rejection (their own tests pin the message)"""
    pr = _lib.Params()
    pr.packed = 1
    f, o, ro = frame(), opts(128), _lib.RenderOut(1, 1, 1, None)
    for fn in (lib.anr_render_fwd, lib.anr_render_image_fwd):
        assert fn(ctypes.byref(pr), ctypes.byref(f), p(1), p(1), p(1), p(1), 300, ctypes.byref(o), ctypes.byref(ro),
                  p(1), BIG, None) == ARG
        assert b'only N_samples == 64' in lib.anr_last_error()


class _Net:
    """stands in for a network: the callers must refuse before they touch it"""
    training = True

    def parameters(self):
        raise AssertionError('device work before the argument check')

    core_tensors = novel_tensors = parameters


@pytest.mark.parametrize('ns', [0, 32, 96, 100, 320, 63])
def test_python_refuses_other_counts_before_the_library(lib, ns):
    from animatable_nerf_amd.renderer import Renderer
    from animatable_nerf_amd.renderer_mmsk import Renderer as MRenderer
    cfg = config.defaults()
    assert cfg.N_samples == 64
    cfg.N_samples = ns
    for cls in (Renderer, MRenderer):
        r = cls(_Net(), cfg)
        with pytest.raises(ValueError, match='N_samples'):
            r.render_device({})
        with pytest.raises(ValueError, match='N_samples'):
            r.render_device({}, bw_rows=False, image_only=True)
    import torch
    with torch.no_grad(), pytest.raises(ValueError, match='N_samples'):
        Renderer(_Net(), cfg).render({'ray_o': torch.zeros(1, 5, 3)})


@pytest.mark.parametrize('ns', [128, 192, 256])
def test_python_accepts_the_render_counts(lib, ns):
    """an accepted count passes the check: the call goes on (and here meets the stand-in network)"""
    from animatable_nerf_amd.renderer import Renderer
    cfg = config.defaults()
    cfg.N_samples = ns
    with pytest.raises(AssertionError):
        Renderer(_Net(), cfg).render_device({})


def test_training_and_sdf_say_64_only(lib):
    from animatable_nerf_amd.renderer import Renderer
    from animatable_nerf_amd.renderer_sdf import Renderer as SRenderer
    cfg = config.defaults()
    cfg.N_samples = 128
    with pytest.raises(ValueError, match='64 only'):
        Renderer(_Net(), cfg).render_train({})
    scfg = config.subject('anisdf_pdf_s9p', perturb=0)
    scfg.N_samples = 128
    with pytest.raises(ValueError, match='64 only'):
        SRenderer(_Net(), scfg).render_device({})
