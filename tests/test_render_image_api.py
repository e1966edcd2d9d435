"""CPU: the image-only render entries (anr_render_image_workspace_bytes / anr_render_image_fwd) are declared and
exported, size their workspace below the full render's by at least the pbw / tbw rows, and reject bad arguments
before any HIP call (no GPU needed); Renderer.render_device refuses image_only together with bw_rows before any
device work, and the cfg key render_image_only defaults to False."""
import ctypes
import os
import re

import pytest

from animatable_nerf_amd import _lib, config

ARG, WORKSPACE = 2, 3
BIG = 1 << 44
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aninerf.h')
SYMBOLS = ('anr_render_image_workspace_bytes', 'anr_render_image_fwd')
RAYS = (1, 64, 2048, 262144)


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


def opts(n_samples=64, chunk=2048, novel_pose=0):
    o = _lib.RenderOpts()
    o.n_samples, o.chunk, o.norm_th, o.train_th, o.novel_pose, o.precision = n_samples, chunk, 0.05, 0.0, novel_pose, 0
    return o


def fwd(lib, params=True, f=True, o=True, out=True, ws=1, ws_bytes=BIG, n_rays=300, rays=(1, 1, 1, 1), packed=1,
        maps=(1, 1, 1), fr=None, op=None):
    pr = _lib.Params()
    pr.packed = packed
    fr = fr if fr is not None else frame(tbw=False)
    op = op if op is not None else opts()
    ro = _lib.RenderOut(*maps, None)
    return lib.anr_render_image_fwd(ctypes.byref(pr) if params else None, ctypes.byref(fr) if f else None,
                                    *[p(r) for r in rays], n_rays, ctypes.byref(op) if o else None,
                                    ctypes.byref(ro) if out else None, p(ws), ws_bytes, None)


def test_symbols_declared_and_exported(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r'\b(anr_[a-z_0-9]+)\s*\(', src))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTS, s
        assert getattr(lib, s) is not None
    assert lib.anr_version() == 2


def test_workspace_bytes(lib):
    img, full = lib.anr_render_image_workspace_bytes, lib.anr_render_workspace_bytes
    f, o = frame(), opts()
    sizes = []
    for R in RAYS:
        a, b = img(R, ctypes.byref(o), ctypes.byref(f)), full(R, ctypes.byref(o), ctypes.byref(f))
        assert 0 < a <= b - 2 * R * 64 * 96, (R, a, b)
        assert a % 256 == 0
        sizes.append(a)
    assert all(x < y for x, y in zip(sizes, sizes[1:])), sizes
    # the T-pose volume does not enter the size: absent from the frame, or as large as one likes
    f0, f1 = frame(tbw=False), frame()
    for i in range(3):
        f1.tbw_dims[i] = 512
    for R in RAYS:
        assert img(R, ctypes.byref(o), ctypes.byref(f0)) == img(R, ctypes.byref(o), ctypes.byref(f)) == \
            img(R, ctypes.byref(o), ctypes.byref(f1))
    # bad arguments
    assert img(300, None, ctypes.byref(f)) == 0
    assert img(300, ctypes.byref(o), None) == 0
    assert img(0, ctypes.byref(o), ctypes.byref(f)) == 0
    assert img(-1, ctypes.byref(o), ctypes.byref(f)) == 0
    assert img(300, ctypes.byref(opts(chunk=0)), ctypes.byref(f)) == 0
    bad = frame()
    bad.pbw_dims[1] = 0
    assert img(300, ctypes.byref(o), ctypes.byref(bad)) == 0


@pytest.mark.parametrize('kw', [dict(params=False), dict(f=False), dict(o=False), dict(out=False), dict(ws=0),
                                dict(rays=(0, 1, 1, 1)), dict(rays=(1, 0, 1, 1)), dict(rays=(1, 1, 0, 1)),
                                dict(rays=(1, 1, 1, 0)), dict(maps=(0, 1, 1)), dict(maps=(1, 0, 1)),
                                dict(maps=(1, 1, 0)), dict(packed=0)])
def test_null_arguments(lib, kw):
    assert fwd(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('field', ['A', 'R', 'Th', 'pbw', 'pbounds', 'tbounds', 'latent_index'])
def test_null_frame_tensors(lib, field):
    assert fwd(lib, fr=frame(tbw=False, **{field: None})) == ARG
    assert b'NULL frame tensor' in lib.anr_last_error()


def test_sizes_and_workspace(lib):
    assert fwd(lib, op=opts(n_samples=32)) == ARG and b'N_samples' in lib.anr_last_error()
    assert fwd(lib, op=opts(n_samples=128)) == ARG
    assert fwd(lib, op=opts(chunk=0)) == ARG and b'chunk' in lib.anr_last_error()
    assert fwd(lib, op=opts(chunk=-5)) == ARG
    assert fwd(lib, n_rays=0) == ARG and b'n_rays' in lib.anr_last_error()
    assert fwd(lib, n_rays=-3) == ARG
    most = (0x7fffffff // 24) // 64  # anr_render_fwd's limit: 24 n_rays 64 stays below 2^31
    assert fwd(lib, n_rays=most + 1) == ARG and b'too many rays' in lib.anr_last_error()
    bad = frame(tbw=False)
    bad.pbw_dims[2] = 0
    assert fwd(lib, fr=bad) == ARG and b'dims' in lib.anr_last_error()
    # novel_pose needs its tensors; the visibility filter its views
    assert fwd(lib, op=opts(novel_pose=1)) == ARG and b'novel_pose' in lib.anr_last_error()
    assert fwd(lib, fr=frame(tbw=False, n_views=2)) == ARG and b'views' in lib.anr_last_error()
    assert fwd(lib, fr=frame(tbw=False, n_views=-1)) == ARG
    # a short workspace; out.raw is NULL here, so the size with raw inside is the one to meet
    f, o = frame(tbw=False), opts()
    need = lib.anr_render_image_workspace_bytes(300, ctypes.byref(o), ctypes.byref(f))
    assert fwd(lib, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    assert fwd(lib, ws_bytes=0) == WORKSPACE
    assert fwd(lib, n_rays=most, ws_bytes=need) == WORKSPACE  # the largest accepted ray count gets as far as the size


def test_tbw_is_not_an_argument(lib):
    """what anr_render_fwd rejects for the T-pose volume passes the image entry's checks: with everything else in
    place the next complaint is the workspace"""
    for fr in (frame(tbw=False), frame(tbw=True)):
        assert fwd(lib, fr=fr, ws_bytes=1) == WORKSPACE


class _Net:
    """stands in for a network: render_device must refuse before it touches it"""

    def parameters(self):
        raise AssertionError('device work before the argument check')

    core_tensors = novel_tensors = parameters


def test_python_guard_and_default(lib):
    from animatable_nerf_amd.renderer import Renderer
    assert config.defaults().render_image_only is False
    assert config.defaults().get('render_image_only', None) is False
    r = Renderer(_Net(), config.defaults())
    with pytest.raises(ValueError):
        r.render_device({}, bw_rows=True, image_only=True)
    cfg = config.defaults()
    cfg.render_image_only = True
    with pytest.raises(ValueError):
        Renderer(_Net(), cfg).render_device({}, bw_rows=True)
    # image_only=False overrides the key: the call goes on (and here meets the stand-in network)
    with pytest.raises(AssertionError):
        Renderer(_Net(), cfg).render_device({}, bw_rows=True, image_only=False)


def test_render_sharded_refuses_rows_under_the_key():
    from animatable_nerf_amd import parallel
    from animatable_nerf_amd.renderer import Renderer
    cfg = config.defaults()
    cfg.render_image_only = True
    with pytest.raises(ValueError):
        parallel.render_sharded(Renderer(_Net(), cfg), {}, rows=True)
