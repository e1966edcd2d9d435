"""GPU: the device-built blend-weight volumes (anr_bw_volume, animatable_nerf_amd.volumes) against the
float64 restatements of tests/bwvol_ref.py.

Acceptance, with D the float64 distance matrix (voxels x primitives) and k = index[n] the kernel's winner:
  D[n, k] <= min_j D[n, j] + DELTA;  |dist_out - D[n, k]| <= DELTA;
  weights within 1e-6 of the float64 interpolation on face k (vertex mode: bit-equal to skin[k]).
DELTA = 1e-6 m. The float32 numpy restatement of the kernel's formula (bwvol_ref.tri_d2_f32: every
candidate is |p - q|^2 for a point q of the triangle, no fused multiply-adds) over every voxel of mesh A's
grids measured, on the CPU: worst float32 distance error 3.7e-8 m (vsize 0.05) / 3.6e-8 m (0.04), worst
excess of the float32-selected triangle over the true minimum 1.1e-16 m / 2.5e-9 m
(tests/test_bwvol_ref.py::test_float32_search_figures_on_mesh_a prints and bounds both). DELTA keeps more
than 25x over the arithmetic it has to cover; dist_out itself is a float64 result rounded to float32 once
(3e-8 m at 0.6 m).
"""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from animatable_nerf_amd import _lib, config, network, synthetic, volumes
from animatable_nerf_amd.renderer import Renderer
from oracle import restate

from . import _common
from . import bwvol_ref as R

pytestmark = pytest.mark.gpu

DELTA = 1e-6
W_TOL = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


# ---- references, computed once ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def surface_case(name):
    """(verts, faces, skin, vsize, origin, dims, P, D) of a surface-mode case."""
    if name == 'A':
        (v, f), vsize, nb = R.mesh_a(), 0.05, 24
    elif name == 'B':
        (v, f), vsize, nb = R.mesh_b(), 0.04, 52
    elif name == 'A_degenerate':  # the first face again, an edge-degenerate face and a point face
        (v, f), vsize, nb = R.mesh_a(), 0.05, 24
        f = np.concatenate([f, f[:1], [[f[0, 0], f[0, 0], f[0, 1]], [5, 5, 5]]]).astype(np.int32)
    skin = R.skin_weights(len(v), nb)
    origin, dims = volumes.grid(v, vsize)
    P = R.grid_points(origin, dims, vsize)
    return v, f, skin, vsize, origin, dims, P, R.tri_distance_matrix(P, v, f)


@functools.lru_cache(maxsize=None)
def scene_case():
    sc = _common.scene(0.05)
    origin, dims = volumes.grid(sc.verts, 0.05)
    P = R.grid_points(origin, dims, 0.05)
    return sc, origin, dims, P, R.vert_distance_matrix(P, sc.verts, chunk=256)


def check_selection(D, idx, dist_out):
    n = np.arange(len(D))
    k = idx.reshape(-1).astype(np.int64)
    assert k.min() >= 0 and k.max() < D.shape[1]
    excess = (D[n, k] - D.min(axis=1)).max()
    derr = np.abs(dist_out.reshape(-1).astype(np.float64) - D[n, k]).max()
    print(f'selection excess {excess:.3g} m, distance error {derr:.3g} m')
    assert excess <= DELTA
    assert derr <= DELTA
    return k


def check_surface(case, vol, idx):
    v, f, skin, vsize, origin, dims, P, D = case
    vol, idx = vol.cpu().numpy(), idx.cpu().numpy()
    nb = skin.shape[1]
    assert vol.shape == dims + (nb + 1,) and vol.dtype == np.float32 and idx.shape == dims
    assert np.all(np.isfinite(vol))
    k = check_selection(D, idx, vol[..., nb])
    w, _ = R.tri_weights(P, v, f, skin, k)
    werr = np.abs(vol[..., :nb].reshape(-1, nb).astype(np.float64) - w).max()
    print(f'weight error {werr:.3g}')
    assert werr <= W_TOL
    return k


def run_raw(dev, verts, skin, faces, vsize, search=_lib.BWV_DEFAULT, stream=None):
    """One anr_bw_volume call into NaN / -1 pre-filled outputs; returns (volume, index) device tensors."""
    lib = _lib.load()
    origin, dims = volumes.grid(verts, vsize)
    nv, nb = skin.shape
    dv = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(dev)
    ds = torch.from_numpy(np.ascontiguousarray(skin, dtype=np.float32)).to(dev)
    df = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(dev) if faces is not None else None
    nf = 0 if faces is None else len(faces)
    vol = torch.full(dims + (nb + 1,), float('nan'), dtype=torch.float32, device=dev)
    idx = torch.full(dims, -1, dtype=torch.int32, device=dev)
    nbytes = lib.anr_bw_volume_workspace_bytes(nv, nf, *dims)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    opts = _lib.BwvOpts(_lib.BWV_VERTEX if faces is None else _lib.BWV_SURFACE, search)
    org = (ctypes.c_double * 3)(*[float(x) for x in origin])
    torch.cuda.synchronize(dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _lib.check(lib.anr_bw_volume(_lib.ptr(dv), nv, _lib.ptr(df), nf, _lib.ptr(ds), nb, org, vsize, dims[0], dims[1],
                                 dims[2], ctypes.byref(opts), _lib.ptr(vol), _lib.ptr(idx), _lib.ptr(ws), nbytes,
                                 ctypes.c_void_p(s.cuda_stream)), 'anr_bw_volume')
    s.synchronize()
    return vol, idx


# ---- 1: vertex mode on the synthetic scene ------------------------------------------------------------
def test_vertex_mode_scene(dev):
    sc, origin, dims, P, D = scene_case()
    vol, idx = volumes.blend_weight_volume(sc.verts, sc.skin, vsize=0.05, device=dev, return_index=True)
    vol, idx = vol.cpu().numpy(), idx.cpu().numpy()
    assert vol.shape == sc.volume.shape and vol.dtype == np.float32
    k = check_selection(D, idx, vol[..., 24])
    assert np.array_equal(vol[..., :24].reshape(-1, 24).view(np.uint32), sc.skin[k].view(np.uint32))
    host_k, _ = synthetic._nearest_vertex(P, sc.verts.astype(np.float64))
    same = host_k == k
    print(f'index equals the host argmin on {same.sum()} of {same.size} voxels')
    assert same.mean() > 0.99  # they part only where two vertices are equidistant to float32 rounding
    got, want = vol.reshape(-1, 25)[same], sc.volume.reshape(-1, 25)[same]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 2, 3: surface mode ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B'])
def test_surface_mode(dev, name):
    case = surface_case(name)
    v, f, skin, vsize = case[:4]
    if name == 'B':
        assert np.prod(case[5]) % 256 != 0 and len(f) % 64 != 0
    vol, idx = volumes.blend_weight_volume(v, skin, faces=f, vsize=vsize, device=dev, return_index=True)
    check_surface(case, vol, idx)


# ---- 4: ties and degenerates --------------------------------------------------------------------------
def test_duplicate_and_zero_area_faces(dev):
    case = surface_case('A_degenerate')
    v, f, skin, vsize = case[:4]
    vol, idx = volumes.blend_weight_volume(v, skin, faces=f, vsize=vsize, device=dev, return_index=True)
    k = check_surface(case, vol, idx)
    assert not np.any(k == 352)  # the copy of face 0 never wins: the lowest index does
    # and as the only face, a zero-area triangle is its edge / its point
    for face in ([[3, 3, 40]], [[5, 5, 5]]):
        fz = np.array(face, np.int32)
        vol, idx = volumes.blend_weight_volume(v, skin, faces=fz, vsize=vsize, device=dev, return_index=True)
        P = case[6]
        w, d = R.tri_weights(P, v, fz, skin, np.zeros(len(P), np.int64))
        vol = vol.cpu().numpy().reshape(len(P), -1)
        assert np.all(np.isfinite(vol)) and not idx.any()
        assert np.abs(vol[:, 24] - d).max() <= DELTA
        assert np.abs(vol[:, :24] - w).max() <= W_TOL


def test_duplicate_vertex(dev):
    v, _ = R.mesh_a()
    skin = R.skin_weights(len(v), 24)
    v2 = np.concatenate([v, v[17:18], v[:1]])
    s2 = np.concatenate([skin, skin[40:41], skin[41:42]])  # other weights: the winner shows in the volume
    vol, idx = volumes.blend_weight_volume(v2, s2, vsize=0.05, device=dev, return_index=True)
    vol, idx = vol.cpu().numpy(), idx.cpu().numpy()
    origin, dims = volumes.grid(v2, 0.05)
    D = R.vert_distance_matrix(R.grid_points(origin, dims, 0.05), v2)
    k = check_selection(D, idx, vol[..., 24])
    assert not np.any(k >= len(v))
    assert np.any(k == 17) and np.any(k == 0)
    assert np.array_equal(vol[..., :24].reshape(-1, 24).view(np.uint32), s2[k].view(np.uint32))


# ---- 5: exhaustive against the default ---------------------------------------------------------------
@pytest.mark.parametrize('which', ['scene', 'B'])
def test_exhaustive_equals_default(dev, which):
    if which == 'scene':
        sc = _common.scene(0.05)
        args = dict(verts=sc.verts, skin=sc.skin, faces=None, vsize=0.05)
    else:
        v, f, skin, vsize = surface_case('B')[:4]
        args = dict(verts=v, skin=skin, faces=f, vsize=vsize)
    outs = [volumes.blend_weight_volume(device=dev, return_index=True, exhaustive=e, **args)
            for e in (False, True, _lib.BWV_PRUNED)]
    for vol, idx in outs[1:]:
        assert torch.equal(idx, outs[0][1])
        assert torch.equal(vol.view(torch.int32), outs[0][0].view(torch.int32))


# ---- 6: streams, repeatability, coverage ----------------------------------------------------------------
@pytest.mark.parametrize('which', ['vertex', 'surface'])
def test_two_streams_same_bits_and_full_coverage(dev, which):
    v, f, skin, vsize = surface_case('B')[:4]
    faces = f if which == 'surface' else None
    a_vol, a_idx = run_raw(dev, v, skin, faces, vsize)
    side = torch.cuda.Stream(device=dev)
    b_vol, b_idx = run_raw(dev, v, skin, faces, vsize, stream=side)
    assert not torch.isnan(a_vol).any() and not torch.isnan(b_vol).any()
    assert int(a_idx.min()) >= 0 and int(b_idx.min()) >= 0
    assert torch.equal(a_idx, b_idx)
    assert torch.equal(a_vol.view(torch.int32), b_vol.view(torch.int32))
    # the Python entry gives the same bits as the raw call
    vol = volumes.blend_weight_volume(v, skin, faces=faces, vsize=vsize, device=dev)
    assert torch.equal(vol.view(torch.int32), a_vol.view(torch.int32))


# ---- 7: end to end ------------------------------------------------------------------------------------------
def test_attach_pose_volume_renders(dev):
    sc = _common.scene(0.05)
    ro, rd = sc.box_rays(256, seed=3)
    near, far, mask = restate.near_far(sc.bounds, ro, rd)
    b = sc.batch_arrays(ro[mask], rd[mask], near.astype(np.float32), far.astype(np.float32))
    bt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
    gpu = {k: v.to(dev) for k, v in bt.items()}
    del gpu['pbw'], gpu['pbounds']
    volumes.attach_pose_volume(gpu, sc.verts, sc.skin, vsize=0.05, device=dev)
    assert gpu['pbw'].shape == (1,) + sc.volume.shape and gpu['pbw'].is_cuda
    assert torch.equal(gpu['pbounds'].cpu(), bt['pbounds'])
    net = network.Network()
    sd = _common.state_dict_np()
    network.load_numpy_state(net, sd)
    net = net.to(dev)
    cfg = config.defaults()
    cfg.perturb = 0
    cfg.render_precision = 'fp32'
    out = Renderer(net, cfg).render_device(gpu)
    torch.cuda.synchronize(dev)
    bt['pbw'] = gpu['pbw'].cpu()
    with torch.no_grad():
        ref = restate.render({k: torch.from_numpy(v) for k, v in sd.items()}, bt)
    for k in ('rgb_map', 'acc_map', 'depth_map', 'raw', 'pbw', 'tbw'):
        assert out[k].shape == ref[k].shape, k
        err = (out[k].cpu() - ref[k]).abs().max().item()
        assert err <= 1e-4, (k, err)


# ---- 8: the tool -----------------------------------------------------------------------------------------------
def test_tool_writes_the_reference_layout(dev, tmp_path):
    v, f = R.mesh_a()
    skin = R.skin_weights(len(v), 24)
    rng = np.random.Generator(np.random.PCG64(8))
    joints = rng.uniform(-0.2, 0.2, (24, 3))
    parents = synthetic.PARENTS
    data = tmp_path / 'subject'
    (data / 'vertices').mkdir(parents=True)
    (data / 'params').mkdir()
    frames = []
    for i in range(2):
        poses = rng.normal(0.0, 0.1, (24, 3))
        poses[0] = 0.0
        Rh = rng.normal(0.0, 0.3, (1, 3))
        Th = rng.normal(0.0, 0.5, (1, 3))
        A = synthetic.rigid_transformation(poses, joints, parents)
        pverts = synthetic.lbs_vertices(v, skin, A).astype(np.float64)
        rot = synthetic.batch_rodrigues(Rh)[0]
        world = pverts @ rot.T + Th
        np.save(data / 'vertices' / f'{i}.npy', world)
        np.save(data / 'params' / f'{i}.npy', {'Rh': Rh, 'Th': Th, 'poses': poses.reshape(1, 72), 'shapes': np.zeros((1, 10))})
        frames.append((world, rot, Th, poses))
    for name, arr in (('faces', f), ('skin', skin), ('joints', joints), ('parents', parents)):
        np.save(tmp_path / f'{name}.npy', arr)
    argv = ['--data', str(data), '--vsize', '0.05', '--device', str(dev)]
    for name in ('faces', 'skin', 'joints', 'parents'):
        argv += ['--' + name, str(tmp_path / f'{name}.npy')]
    spec = importlib.util.spec_from_file_location('build_blend_volumes',
                                                  os.path.join(ROOT, 'tools', 'build_blend_volumes.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(argv)  # the command line, in this process
    lbs = data / 'lbs'
    assert sorted(os.listdir(lbs)) == ['bweights', 'tbw.npy', 'tvertices.npy']
    assert sorted(os.listdir(lbs / 'bweights')) == ['0.npy', '1.npy']
    for i, (world, rot, Th, poses) in enumerate(frames):
        pxyz = np.dot(world - Th, rot)
        want = volumes.blend_weight_volume(pxyz, skin, vsize=0.05, device=dev).cpu().numpy()
        got = np.load(lbs / 'bweights' / f'{i}.npy')
        assert got.dtype == np.float32 and got.shape == want.shape and got.shape[3] == 25
        assert np.array_equal(got, want)
    world, rot, Th, poses = frames[0]
    pxyz = np.dot(world - Th, rot)
    tv = volumes.tpose_vertices(pxyz, skin, synthetic.rigid_transformation(poses, joints, parents))
    assert np.abs(tv - v).max() <= 1e-5  # inverse LBS undoes the forward LBS (float32 A and posed vertices)
    got_tv = np.load(lbs / 'tvertices.npy')
    assert got_tv.shape == (len(v), 3) and np.array_equal(got_tv, tv)
    want = volumes.blend_weight_volume(tv, skin, faces=f, vsize=0.05, device=dev).cpu().numpy()
    got = np.load(lbs / 'tbw.npy')
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
