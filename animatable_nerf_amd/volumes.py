"""Blend-weight volumes built on the device from a posed SMPL mesh (``anr_bw_volume``).

The reference makes the per-frame ``bweights/{i}.npy`` (closest vertex) and the per-subject ``tbw.npy`` /
``bigpose_bw.npy`` (closest surface point) offline with ``tools/custom_dataset/prepare_blend_weights.py``
(:156-211, :229-283), which needs psbody.mesh, open3d and trimesh. Here the same volumes, in the same
``(X, Y, Z, nb + 1)`` float32 layout, come from three HIP launches on the current stream:

  * ``grid`` forms the reference's grid on the host with numpy's own ``arange``, so X, Y, Z are its dims;
  * ``blend_weight_volume`` runs the closest-vertex (``faces=None``) or closest-surface-point search;
  * ``tpose_vertices`` is the inverse LBS that gives the T-pose mesh ``tbw`` is built over (:252-256);
  * ``attach_pose_volume`` is the novel-pose entry: a batch gets ``pbw`` / ``pbounds`` for new posed
    vertices without any ``bweights/`` file.

The kernels take float32 vertices; a float64 mesh is rounded once. There is no host fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import synthetic

_ws = {}  # device -> uint8 workspace tensor


def grid(xyz, vsize=0.025, pad=0.05):
    """The reference's grid over ``xyz`` (``prepare_blend_weights.py:156-168``): origin float64 (3,) and
    (X, Y, Z) = the lengths of ``np.arange(lo, hi + vsize, vsize)`` per axis, lo / hi = min / max -+ pad."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    lo = xyz.min(axis=0) - pad
    hi = xyz.max(axis=0) + pad
    dims = tuple(int(len(np.arange(lo[c], hi[c] + vsize, vsize))) for c in range(3))
    return lo, dims


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _workspace(lib, dev, nv, nf, dims):
    nbytes = lib.anr_bw_volume_workspace_bytes(nv, nf, *dims)
    if nbytes == 0:
        raise ValueError(f'blend_weight_volume: grid {dims} is empty or above 2^28 voxels')
    ws = _ws.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[dev] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def blend_weight_volume(verts, skin, faces=None, vsize=0.025, pad=0.05, device='cuda', return_index=False,
                        exhaustive=False):
    """(X, Y, Z, nb + 1) float32 device tensor: per voxel the skinning weights and the distance of the
    closest vertex (``faces=None``) or of the closest point of the triangle mesh. ``return_index`` also
    returns the winning vertex / face id per voxel, (X, Y, Z) int32. ``exhaustive`` (True, or one of
    ``_lib.BWV_*``) selects the search; every search writes the same bits. Enqueued on the current
    stream of ``device``; the vertices are read on the host once to form the grid."""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('blend_weight_volume: the volume is built on a GPU; there is no host path')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    hv = np.ascontiguousarray(_host(verts), dtype=np.float32).reshape(-1, 3)
    hs = np.ascontiguousarray(_host(skin), dtype=np.float32)
    if hs.ndim != 2 or hs.shape[0] != hv.shape[0]:
        raise ValueError(f'blend_weight_volume: skin {hs.shape} does not give one row per vertex ({hv.shape[0]})')
    nv, nb = hs.shape
    origin, dims = grid(hv, vsize, pad)
    dv = torch.from_numpy(hv).to(dev)
    ds = torch.from_numpy(hs).to(dev)
    df, nf, mode = None, 0, _lib.BWV_VERTEX
    if faces is not None:
        hf = np.ascontiguousarray(_host(faces)).reshape(-1, 3)
        if hf.size and (hf.min() < 0 or hf.max() >= nv):
            raise ValueError('blend_weight_volume: a face index lies outside [0, nv)')
        df = torch.from_numpy(hf.astype(np.int32)).to(dev)
        nf, mode = hf.shape[0], _lib.BWV_SURFACE
    search = _lib.BWV_EXHAUSTIVE if exhaustive is True else int(exhaustive)
    opts = _lib.BwvOpts(mode, search)
    vol = torch.empty(dims + (nb + 1,), dtype=torch.float32, device=dev)
    idx = torch.empty(dims, dtype=torch.int32, device=dev) if return_index else None
    org = (ctypes.c_double * 3)(*[float(v) for v in origin])
    with torch.cuda.device(dev):
        ws = _workspace(lib, dev, nv, nf, dims)
        _lib.check(lib.anr_bw_volume(_lib.ptr(dv), nv, _lib.ptr(df), nf, _lib.ptr(ds), nb, org, float(vsize),
                                     dims[0], dims[1], dims[2], ctypes.byref(opts), _lib.ptr(vol), _lib.ptr(idx),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), 'anr_bw_volume')
        # the inputs were uploaded for this call alone: keep them until the stream has used them
        for t in (dv, ds, df):
            if t is not None:
                t.record_stream(torch.cuda.current_stream(dev))
    return (vol, idx) if return_index else vol


def tpose_vertices(pverts, skin, A):
    """Inverse LBS (``prepare_blend_weights.py:252-256``): pose-space vertices (V, 3) -> T-pose vertices,
    x = R_v^-1 (p - t_v) with [R_v | t_v] = sum_j skin[v, j] A[j]; float64 numpy on the host."""
    p = np.asarray(pverts, dtype=np.float64)
    w = np.asarray(skin, dtype=np.float64)
    T = (w @ np.asarray(A, dtype=np.float64).reshape(w.shape[1], 16)).reshape(-1, 4, 4)
    return np.einsum('vij,vj->vi', np.linalg.inv(T[:, :3, :3]), p - T[:, :3, 3])


def attach_pose_volume(batch, pverts, skin, vsize=0.025, device='cuda'):
    """Novel-pose entry: ``batch['pbw']`` = the (1, X, Y, Z, nb + 1) closest-vertex volume of the posed
    vertices, built on the device, and ``batch['pbounds']`` = their padded bounds (1, 2, 3)."""
    hv = _host(pverts)
    vol = blend_weight_volume(hv, skin, vsize=vsize, device=device)
    batch['pbw'] = vol[None]
    batch['pbounds'] = torch.from_numpy(synthetic.get_bounds(hv.reshape(-1, 3))[None]).to(vol.device)
    return batch
