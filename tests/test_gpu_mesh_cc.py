"""GPU: the device component pass (anr_mesh_cc_count / anr_mesh_cc_emit, largest_component_device) against
the host ``renderer_sdf_mesh.largest_component``: vertices and triangles by exact equality on every mesh of
tests/meshcc_cases.py (tests/test_mesh_cc_api.py holds those meshes to their properties), labels against
the host's union-find roots, the counts, the status paths, determinism, and the two renderers that use it."""
import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib
from animatable_nerf_amd.renderer_mesh import marching_cubes
from animatable_nerf_amd.renderer_sdf_mesh import largest_component, largest_component_device

from . import meshcc_cases as mc
from ._common import golden, make_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


def _to(dev, v, t):
    return torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(t)).to(dev)


def _raw(dev, v, t, want_labels=True, fill=None):
    """the C entries directly -> (counts (6,), labels, out_vertices, out_triangles) as numpy; with `fill`
    the outputs have the inputs' sizes and are preset to that value instead of being sized by the counts"""
    lib = _lib.load()
    dv, dt = _to(dev, v, t)
    nv, nt = len(v), len(t)
    nbytes = lib.anr_mesh_cc_workspace_bytes(nv, nt)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.full((6,), -7, dtype=torch.int32, device=dev)
    labels = torch.full((nt,), -7, dtype=torch.int32, device=dev) if want_labels else None
    st = _lib.stream_ptr(dev)
    _lib.check(lib.anr_mesh_cc_count(_lib.ptr(dt), nt, nv, _lib.ptr(counts), _lib.ptr(labels), _lib.ptr(ws), nbytes, st),
               'anr_mesh_cc_count')
    c = counts.cpu().numpy()
    if fill is None:
        ov = torch.empty((int(c[0]), 3), dtype=torch.float64, device=dev)
        ot = torch.empty((int(c[1]), 3), dtype=torch.int64, device=dev)
    else:
        ov = torch.full((nv, 3), float(fill), dtype=torch.float64, device=dev)
        ot = torch.full((nt, 3), int(fill), dtype=torch.int64, device=dev)
    if ov.numel() or ot.numel():
        _lib.check(lib.anr_mesh_cc_emit(_lib.ptr(dv), _lib.ptr(dt), nt, nv, _lib.ptr(ov), _lib.ptr(ot), _lib.ptr(ws),
                                        nbytes, st), 'anr_mesh_cc_emit')
    torch.cuda.synchronize(dev)
    return c, (labels.cpu().numpy() if want_labels else None), ov.cpu().numpy(), ot.cpu().numpy()


@pytest.mark.parametrize('name', mc.CASES)
def test_device_pass_equals_host_pass(dev, name):
    v, t = mc.case(name)
    hv, ht = mc.host(name)
    kv, kt, lab = largest_component_device(*_to(dev, v, t), return_labels=True)
    assert kv.dtype == torch.float64 and kt.dtype == torch.int64 and kv.is_cuda and kt.is_cuda
    assert kv.shape == hv.shape and kt.shape == ht.shape
    assert np.array_equal(kv.cpu().numpy(), hv)
    assert np.array_equal(kt.cpu().numpy(), ht)
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), mc.labels(name))
    kv2, kt2 = largest_component_device(*_to(dev, v, t))  # without labels: the same mesh
    assert torch.equal(kv2, kv) and torch.equal(kt2, kt)


@pytest.mark.parametrize('name', ['boxes3', 'glued', 'tets65o', 'shared_vertex', 'dup_degenerate', 'pieces'])
def test_counts(dev, name):
    v, t = mc.case(name)
    comps = mc.components(t)
    wt = {r: n for r, (ok, n) in comps.items() if ok}
    kept = min(r for r, n in wt.items() if n == max(wt.values()))
    c, lab, ov, ot = _raw(dev, v, t)
    hv, ht = mc.host(name)
    assert c.tolist() == [len(hv), len(ht), len(comps), len(wt), kept, 0]
    assert np.array_equal(ov, hv) and np.array_equal(ot, ht) and np.array_equal(lab, mc.labels(name))


def test_no_watertight_piece_is_the_identity(dev):
    v, t = mc.case('open')
    c, lab, ov, ot = _raw(dev, v, t)
    assert c.tolist() == [len(v), len(t), 1, 0, -1, 1]
    assert np.array_equal(ov, v) and np.array_equal(ot, t) and np.all(lab == 0)
    kv, kt = largest_component_device(*_to(dev, v, t))
    assert np.array_equal(kv.cpu().numpy(), v) and np.array_equal(kt.cpu().numpy(), t)


def test_empty_input(dev):
    v, t = mc.case('empty')
    c, lab, ov, ot = _raw(dev, v, t)
    assert c.tolist() == [len(v), 0, 0, 0, -1, 1]
    assert np.array_equal(ov, v) and ot.shape == (0, 3)
    kv, kt, lab = largest_component_device(*_to(dev, v, t), return_labels=True)
    assert np.array_equal(kv.cpu().numpy(), v) and kt.shape == (0, 3) and lab.shape == (0,)
    kv, kt = largest_component_device(torch.zeros((0, 3), dtype=torch.float64, device=dev),
                                      torch.zeros((0, 3), dtype=torch.int64, device=dev))
    assert kv.shape == (0, 3) and kt.shape == (0, 3)


@pytest.mark.parametrize('bad', [-1, 'nv', 1 << 40])
def test_out_of_range_index(dev, bad):
    v, t = mc.case('boxes3')
    t = t.copy()
    t[17, 1] = len(v) if bad == 'nv' else bad
    c, lab, ov, ot = _raw(dev, v, t, fill=-3)
    assert c.tolist() == [0, 0, 0, 0, -1, 2]
    assert np.all(lab == -1)
    assert np.all(ov == -3.0) and np.all(ot == -3)  # emit wrote nothing
    with pytest.raises(ValueError):
        largest_component_device(*_to(dev, v, t))


def test_multi_piece_marching_cubes_mesh(dev):
    vol = mc.pieces_volume()
    v, t = marching_cubes(torch.from_numpy(vol).to(dev), 0.0, 0)
    rv, rt = mc.case('pieces')
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(t.cpu().numpy(), rt)
    kv, kt = largest_component_device(v, t)
    hv, ht = mc.host('pieces')
    assert np.array_equal(kv.cpu().numpy(), hv) and np.array_equal(kt.cpu().numpy(), ht)


@pytest.mark.parametrize('name', ['tets1025o', 'tube_random', 'pieces'])
def test_deterministic(dev, name):
    v, t = mc.case(name)
    a = _raw(dev, v, t)
    b = _raw(dev, v, t)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_one_workspace_reused_across_meshes(dev):
    """the pass clears what it needs itself: a workspace dirtied by another mesh (and by 0xff) changes nothing"""
    lib = _lib.load()
    big = lib.anr_mesh_cc_workspace_bytes(2000, 9000)
    ws = torch.full((big,), 0xff, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    for name in ('tets65o', 'dup_degenerate', 'tets63', 'open', 'bipyramid'):
        v, t = mc.case(name)
        dv, dt = _to(dev, v, t)
        counts = torch.zeros(6, dtype=torch.int32, device=dev)
        _lib.check(lib.anr_mesh_cc_count(_lib.ptr(dt), len(t), len(v), _lib.ptr(counts), None, _lib.ptr(ws), big, st),
                   'anr_mesh_cc_count')
        c = counts.cpu().numpy()
        ov = torch.empty((int(c[0]), 3), dtype=torch.float64, device=dev)
        ot = torch.empty((int(c[1]), 3), dtype=torch.int64, device=dev)
        _lib.check(lib.anr_mesh_cc_emit(_lib.ptr(dv), _lib.ptr(dt), len(t), len(v), _lib.ptr(ov), _lib.ptr(ot),
                                        _lib.ptr(ws), big, st), 'anr_mesh_cc_emit')
        hv, ht = mc.host(name)
        assert np.array_equal(ov.cpu().numpy(), hv) and np.array_equal(ot.cpu().numpy(), ht), name


def test_mesh_renderer_opt_in(dev):
    """renderer_mesh.Renderer.render: with mesh_largest_component the host pass of the default output,
    without it (unset or False) today's output"""
    from animatable_nerf_amd import config, synthetic
    from animatable_nerf_amd.renderer_mesh import MC_PAD, Renderer
    g = golden('g10_mesh')
    b = synthetic.mesh_scene(voxel=0.02)
    batch = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in b.items()}
    net = make_net(dev)
    iso = float(np.median(g['alpha_inside'][g['alpha_inside'] != 0]))

    def render(**keys):
        cfg = config.load_cfg(opts=['vis_posed_mesh', 'True', 'render_precision', 'fp32'])
        cfg.mesh_th = iso
        cfg.voxel_size = [0.02, 0.02, 0.02]
        for k, x in keys.items():
            setattr(cfg, k, x)
        return Renderer(net, cfg).render(batch)
    base = render()
    assert not config.load_cfg(opts=['vis_posed_mesh', 'True']).get('mesh_largest_component', False)
    # today's output: the marching cubes of the alpha volume, transformed, every piece of it
    r = Renderer(net, config.load_cfg(opts=['vis_posed_mesh', 'True', 'render_precision', 'fp32']))
    v, t = marching_cubes(r.alpha_volume(batch), iso, MC_PAD)
    wmin = batch['wbounds'][0, 0].cpu().numpy()
    assert np.array_equal(base['triangle'], t.cpu().numpy())
    assert np.array_equal(base['vertex'], (v.cpu().numpy() - MC_PAD) * 0.02 + wmin)
    off = render(mesh_largest_component=False)
    assert all(np.array_equal(off[k], base[k]) for k in base)
    on = render(mesh_largest_component=True)
    hv, ht = largest_component(base['vertex'], base['triangle'])
    assert np.array_equal(on['vertex'], hv) and np.array_equal(on['triangle'], ht)
    assert np.array_equal(on['posed_vertex'], hv) and set(on) == set(base)
