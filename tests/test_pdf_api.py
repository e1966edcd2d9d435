"""CPU: the aligned_aninerf_pdf render entries are declared and exported, size their workspace and reject bad
arguments before any HIP call (these run where there is no GPU: a HIP call would return ANR_E_HIP instead), the
network plugin has the reference's state_dict names and shapes (golden G18, dumped from the real reference by
tools/gen_golden_pdf.py), and the plugins refuse the options they do not cover."""
import ctypes
import json
import os

import pytest
import torch

from animatable_nerf_amd import _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = os.path.join(ROOT, 'tests', 'golden', 'g18_state_dict.json')
E_ARG, E_WORKSPACE = 2, 3
ENTRIES = ('anr_pdf_render_workspace_bytes', 'anr_pdf_render_fwd', 'anr_pdf_render_counts', 'anr_pdf_render_rows')
VIEWS = ('anr_pdf_render_knn', 'anr_pdf_render_kept', 'anr_pdf_render_points', 'anr_pdf_render_bigpose')
SUBJECT = 'aligned_aninerf_pdf_s9p'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def _opts(n_samples=64, precision=_lib.FP32, novel=0, chunk=2048):
    return _lib.RenderOpts(n_samples, chunk, 0.05, 0.0, None, novel, precision)


def _valid(n_verts=6890):
    """Structs with non-NULL (never dereferenced) pointers everywhere."""
    one = ctypes.c_void_p(256)
    p = _lib.PdfParams()
    for i in range(_lib.NUM_PDF_TENSORS):
        p.t[i] = 256
    f = _lib.PdfFrame(one, one, one, one, one, one, one, one, one, n_verts, 0, None, None, None, 0, 0)
    out = _lib.PdfRenderOut(one, one, one, one, one)
    return p, f, out, one


def _fwd(lib, p, f, out, o, ws, ws_bytes, n_rays=10, image=0, ray=ctypes.c_void_p(256)):
    return lib.anr_pdf_render_fwd(ctypes.byref(p) if p is not None else None, ctypes.byref(f) if f is not None else None,
                                  ray, ray, ray, ray, n_rays, ctypes.byref(o) if o is not None else None,
                                  ctypes.byref(out) if out is not None else None, image, ws, ws_bytes, None)


def test_exports(lib):
    for name in ENTRIES + VIEWS:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    header = open(os.path.join(ROOT, 'include', 'aninerf.h')).read()
    for name in ENTRIES + VIEWS:
        assert name + '(' in header, name
    assert '#define ANR_PDF_NUM_TENSORS 62' in header and _lib.NUM_PDF_TENSORS == 62


def test_workspace_bytes_is_host_arithmetic(lib):
    o = _opts()
    sizes = [lib.anr_pdf_render_workspace_bytes(r, ctypes.byref(o), 0) for r in (1, 64, 1000, 4136, 262144)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))  # monotone in rays
    img = lib.anr_pdf_render_workspace_bytes(4136, ctypes.byref(o), 1)
    assert img + 4136 * 64 * 3 * 4 <= sizes[3]  # an image-only call carries no resd rows
    assert sizes[-1] < 16 * 2 ** 30
    assert lib.anr_pdf_render_workspace_bytes(0, ctypes.byref(o), 0) == 0
    assert lib.anr_pdf_render_workspace_bytes(-3, ctypes.byref(o), 0) == 0
    assert lib.anr_pdf_render_workspace_bytes(64, None, 0) == 0
    assert lib.anr_pdf_render_workspace_bytes(64, ctypes.byref(_opts(chunk=0)), 0) == 0
    for name in ('anr_pdf_render_counts',) + VIEWS:
        assert not getattr(lib, name)(None, 64, ctypes.byref(o), 0), name
        assert not getattr(lib, name)(ctypes.c_void_p(256), 0, ctypes.byref(o), 0), name


def test_batch_override_changes_only_the_batch_buffers(lib, monkeypatch):
    o = _opts()
    full = lib.anr_pdf_render_workspace_bytes(4136, ctypes.byref(o), 0)
    monkeypatch.setenv('ANR_PDF_BATCH', '1024')
    small = lib.anr_pdf_render_workspace_bytes(4136, ctypes.byref(o), 0)
    assert 0 < small < full
    monkeypatch.setenv('ANR_PDF_BATCH', '1000')  # not a multiple of 256: ignored
    assert lib.anr_pdf_render_workspace_bytes(4136, ctypes.byref(o), 0) == full
    monkeypatch.setenv('ANR_PDF_BATCH', str(1 << 19))  # above the built-in capacity: ignored
    assert lib.anr_pdf_render_workspace_bytes(4136, ctypes.byref(o), 0) == full


def test_rejections_come_before_any_hip_call(lib):
    p, f, out, ws = _valid()
    o = _opts()
    big = 1 << 40
    assert _fwd(lib, None, f, out, o, ws, big) == E_ARG and b'NULL' in lib.anr_last_error()
    assert _fwd(lib, p, None, out, o, ws, big) == E_ARG and b'NULL' in lib.anr_last_error()
    assert _fwd(lib, p, f, None, o, ws, big) == E_ARG and b'NULL' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, None, ws, big) == E_ARG and b'NULL' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, o, None, big) == E_ARG and b'NULL' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, o, ws, big, ray=None) == E_ARG and b'NULL' in lib.anr_last_error()
    q = _lib.PdfParams()
    assert _fwd(lib, q, f, out, o, ws, big) == E_ARG and b'NULL parameter tensor' in lib.anr_last_error()
    p.t[43] = None  # resd_latent is not read by the forward
    need = lib.anr_pdf_render_workspace_bytes(10, ctypes.byref(o), 0)
    assert _fwd(lib, p, f, out, o, ws, need - 1) == E_WORKSPACE and b'workspace' in lib.anr_last_error()
    p.t[60] = None
    assert _fwd(lib, p, f, out, o, ws, big) == E_ARG and b'NULL parameter tensor' in lib.anr_last_error()
    p.t[60] = 256
    for field in ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses', 'tbounds', 'latent_index'):
        _, g, _, _ = _valid()
        setattr(g, field, None)
        assert _fwd(lib, p, g, out, o, ws, big) == E_ARG and b'frame' in lib.anr_last_error(), field
    for field in ('rgb_map', 'acc_map', 'depth_map', 'raw'):
        _, _, out2, _ = _valid()
        setattr(out2, field, None)
        assert _fwd(lib, p, f, out2, o, ws, big) == E_ARG and b'output' in lib.anr_last_error(), field
    for nv in (0, -1, 6913):
        _, f2, _, _ = _valid(n_verts=nv)
        assert _fwd(lib, p, f2, out, o, ws, big) == E_ARG and b'n_verts' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(n_samples=128), ws, big) == E_ARG and b'N_samples' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(novel=1), ws, big) == E_ARG and b'novel' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(precision=_lib.BF16), ws, big) == E_ARG and b'precision' in lib.anr_last_error()
    assert _fwd(lib, p, f, out, _opts(chunk=0), ws, big) == E_ARG
    assert _fwd(lib, p, f, out, o, ws, big, n_rays=0) == E_ARG
    _, fv, _, _ = _valid()
    fv.n_views = 3  # views without their tensors
    assert _fwd(lib, p, fv, out, o, ws, big) == E_ARG and b'views' in lib.anr_last_error()
    fv.n_views = -1
    assert _fwd(lib, p, fv, out, o, ws, big) == E_ARG and b'views' in lib.anr_last_error()
    need_img = lib.anr_pdf_render_workspace_bytes(10, ctypes.byref(o), 1)
    assert _fwd(lib, p, f, out, o, ws, need_img - 1, image=1) == E_WORKSPACE
    assert lib.anr_pdf_render_rows(None, 10, ctypes.byref(o), None, None, None) == E_ARG
    assert lib.anr_pdf_render_rows(ws, 10, None, None, None, None) == E_ARG


def test_state_dict_matches_reference():
    from animatable_nerf_amd import network_pdf
    g = json.load(open(G18))
    net = network_pdf.Network(config.subject(SUBJECT))
    ours = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert ours == [[k, list(v)] for k, v in g.items()]
    assert len(net.tensors()) == _lib.NUM_PDF_TENSORS
    assert [tuple(t.shape) for t in net.tensors()] == [tuple(v) for v in g.values()]
    names = list(g)
    assert names[0] == 'tpose_human.nerf_network.lin0.bias' and names[27] == 'tpose_human.color_network.color_latent.weight'
    assert names[43] == 'resd_latent.weight' and names[44] == 'resd_linears.0.weight' and names[60:] == ['resd_fc.weight', 'resd_fc.bias']
    assert float(net.resd_fc.bias.detach().abs().max()) == 0.0
    net2 = network_pdf.Network(config.subject(SUBJECT))
    net2.load_state_dict(net.state_dict(), strict=True)


def test_preset_and_unsupported_options():
    from animatable_nerf_amd import network_pdf, renderer_pdf
    cfg = config.subject(SUBJECT)
    # the yaml's shapes: 260 training frames (the latent tables), 64 samples, norm_th 0.05 (which the network ignores)
    assert cfg.num_train_frame == 260 and cfg.num_latent_code == 260 and cfg.norm_th == 0.05 and cfg.N_samples == 64
    assert cfg.tpose_viewdir and cfg.use_bigpose
    assert cfg.network_module == 'animatable_nerf_amd.network_pdf' and cfg.renderer_module == 'animatable_nerf_amd.renderer_pdf'
    with pytest.raises(ValueError, match='tpose_viewdir'):
        network_pdf.Network(config.subject(SUBJECT, tpose_viewdir=False))
    with pytest.raises(ValueError, match='color_with_viewdir'):
        network_pdf.Network(config.subject(SUBJECT, color_with_viewdir=False))
    with pytest.raises(ValueError, match='init_sdf'):
        network_pdf.Network(config.subject(SUBJECT, init_sdf='some_run'))
    with pytest.raises(ValueError, match='render_precision'):
        renderer_pdf._pdf_precision(config.subject(SUBJECT, render_precision='bf16'))
    assert renderer_pdf._pdf_precision(config.subject(SUBJECT, render_precision='bf16x6')) == _lib.BF16X6
    net = network_pdf.Network(cfg)
    assert tuple(net.resd_latent.weight.shape) == (260, 128) and tuple(net.resd_linears[5].weight.shape) == (256, 391, 1)
    with pytest.raises(NotImplementedError):
        net(None, None, None, None)


def test_renderer_refuses_what_it_does_not_cover(lib):
    from animatable_nerf_amd import network_pdf, renderer_pdf
    batch = {'ray_o': torch.zeros(1, 4, 3)}
    net = network_pdf.Network(config.subject(SUBJECT))
    with pytest.raises(ValueError, match='N_samples'):
        renderer_pdf.Renderer(net, config.subject(SUBJECT, N_samples=128)).render_device(batch)
    for kw in ({'tpose_viewdir': False}, {'color_with_viewdir': False}):
        with pytest.raises(ValueError, match='viewdir'):
            renderer_pdf.Renderer(net, config.subject(SUBJECT, **kw)).render_device(batch)
    with pytest.raises(ValueError, match='init_sdf'):
        renderer_pdf.Renderer(net, config.subject(SUBJECT, init_sdf='x')).render_device(batch)
    r = renderer_pdf.Renderer(net, config.subject(SUBJECT))
    with pytest.raises(ValueError, match='render_sharded'):
        r.render_device(batch, chunk_offset=0)
    net.train()
    with pytest.raises(RuntimeError, match='training'):  # under grad, in training mode
        r.render(batch)
    with pytest.raises(RuntimeError, match='GPU'):  # no CPU path
        r.render_device(batch)


def test_alpha_entry_sizes_and_rejects(lib):
    header = open(os.path.join(ROOT, 'include', 'aninerf.h')).read()
    for name in ('anr_pdf_alpha_workspace_bytes', 'anr_pdf_alpha_points'):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + '(' in header, name
    o = _lib.AlphaOpts(2048 * 64, 0.1, 0, _lib.FP32)
    a = lib.anr_pdf_alpha_workspace_bytes(1000, ctypes.byref(o))
    b = lib.anr_pdf_alpha_workspace_bytes(100000, ctypes.byref(o))
    c = lib.anr_pdf_alpha_workspace_bytes(1 << 22, ctypes.byref(o))  # more than one chunk: sized by the chunk
    assert 0 < a < b <= c == lib.anr_pdf_alpha_workspace_bytes(1 << 23, ctypes.byref(o))
    assert lib.anr_pdf_alpha_workspace_bytes(0, ctypes.byref(o)) == 0
    assert lib.anr_pdf_alpha_workspace_bytes((1 << 24) + 1, ctypes.byref(o)) == 0
    assert lib.anr_pdf_alpha_workspace_bytes(1000, None) == 0
    assert lib.anr_pdf_alpha_workspace_bytes(1000, ctypes.byref(_lib.AlphaOpts(1000, 0.1, 0, _lib.FP32))) == 0
    p, f, _, one = _valid()
    big = 1 << 40
    call = lambda p_, f_, o_, n=1000, pts=one, out=one, ws=one, wsb=big: lib.anr_pdf_alpha_points(
        ctypes.byref(p_) if p_ is not None else None, ctypes.byref(f_) if f_ is not None else None, pts, n,
        ctypes.byref(o_) if o_ is not None else None, out, ws, wsb, None)
    for kw in ({'pts': None}, {'out': None}, {'ws': None}):
        assert call(p, f, o, **kw) == E_ARG and b'NULL' in lib.anr_last_error()
    assert call(None, f, o) == E_ARG and call(p, None, o) == E_ARG and call(p, f, None) == E_ARG
    assert call(p, f, o, n=0) == E_ARG and call(p, f, _lib.AlphaOpts(100, 0.1, 0, _lib.FP32)) == E_ARG
    assert call(p, f, _lib.AlphaOpts(2048 * 64, 0.1, 1, _lib.FP32)) == E_ARG and b'novel' in lib.anr_last_error()
    assert call(p, f, _lib.AlphaOpts(2048 * 64, 0.1, 0, _lib.BF16)) == E_ARG and b'precision' in lib.anr_last_error()
    assert call(_lib.PdfParams(), f, o) == E_ARG and b'parameter' in lib.anr_last_error()
    for field in ('A', 'big_A', 'R', 'Th', 'pvertices', 'weights', 'poses'):
        _, g, _, _ = _valid()
        setattr(g, field, None)
        assert call(p, g, o) == E_ARG and b'frame' in lib.anr_last_error(), field
    _, g, _, _ = _valid(n_verts=7000)
    assert call(p, g, o) == E_ARG and b'n_verts' in lib.anr_last_error()
    _, g, _, _ = _valid()
    g.n_views = 2
    assert call(p, g, o) == E_ARG and b'n_views' in lib.anr_last_error()
    assert call(p, f, o, wsb=a - 1) == E_WORKSPACE
