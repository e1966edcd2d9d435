"""Mesh evaluator plugin: ``Evaluator().evaluate(output, batch)`` / ``summarize()``
(lib/evaluators/mesh_evaluator.py:13-136; if_nerf_mesh.py is the same code) on the HIP library.

``evaluate`` takes the extracted mesh (``output['posed_vertex']``, ``output['triangle']``; numpy arrays or
device tensors, e.g. of ``renderer_sdf_mesh.Renderer.render_device``) and the frame's target mesh, and
enqueues one ``anr_mesh_metrics`` call into the next row of a device table: surface samples on both meshes,
closest-point distances both ways, Chamfer and point-to-surface (P2S), all in HIP on the current stream. It
returns without a copy to the host or a synchronisation. ``summarize`` makes the one D2H copy, writes
``<cfg.result_dir>/mesh_metrics.npy`` = ``{'p2s': [...], 'chamfer': [...]}`` and prints the two means, as
the reference does.

The target is ``batch['tgt_vertex']`` / ``batch['tgt_triangle']`` when present, else the reference's
``<cfg.test_dataset.data_root>/object/{frame_index:06d}.obj`` read by ``read_obj`` (open3d is not needed).

The reference samples with ``trimesh.sample.sample_surface`` and measures with
``trimesh.proximity.closest_point``. trimesh is not installed here, so both are restated from its documented
behaviour and the reference's call sites: parity with trimesh is unpinned (like PyMCubes and ``split()``).
The uniforms come from the host: ``u`` is the ``(12000, 3)`` array (rows: 1000 Chamfer source, 1000 Chamfer
target, 10000 P2S source; columns: the face pick, then the two lengths), or a numpy Generator, or ``None``
for ``np.random.random`` — drawn in the reference's order, per call ``n`` picks then ``(n, 2)`` lengths.

Vertices are rounded to float32 once (the kernels' input type); distances are float64. There is no host
fallback: the meshes are evaluated on a GPU or not at all.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import config as _config

N_CHAMFER = 1000   # mesh_evaluator.py:100
N_P2S = 10000      # :124


# ---- files ----------------------------------------------------------------------------------------------
def read_obj(path):
    """Vertices (V,3) float64 and faces (F,3) int32 of a Wavefront .obj: ``v x y z`` and ``f a b c`` lines,
    the ``a/b/c`` index forms, 1-based or negative (relative) indices; triangles only."""
    verts, faces = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            s = line.split()
            if not s:
                continue
            if s[0] == 'v':
                if len(s) < 4:
                    raise ValueError(f'{path}:{ln}: a vertex needs three coordinates')
                verts.append((float(s[1]), float(s[2]), float(s[3])))
            elif s[0] == 'f':
                if len(s) != 4:
                    raise ValueError(f'{path}:{ln}: only triangles are read, this face has {len(s) - 1} corners')
                idx = []
                for tok in s[1:]:
                    i = int(tok.split('/')[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                faces.append(idx)
    v = np.array(verts, dtype=np.float64).reshape(-1, 3)
    t = np.array(faces, dtype=np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f'{path}: a face index lies outside the {len(v)} vertices')
    return v, t.astype(np.int32)


def write_ply(path, vertices, triangles):
    """ASCII PLY of a triangle mesh (what ``trimesh.Trimesh.export('x.ply')`` carries: vertices and faces)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\n')
        f.write(f'element vertex {len(v)}\nproperty double x\nproperty double y\nproperty double z\n')
        f.write(f'element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n')
        for p in v:
            f.write(f'{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n')  # repr: the shortest exact text
        for a in t:
            f.write(f'3 {int(a[0])} {int(a[1])} {int(a[2])}\n')


# ---- device plumbing ---------------------------------------------------------------------------------------
def _device(device, *tensors):
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((t.device for t in tensors if torch.is_tensor(t) and t.is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError('evaluator_mesh: no GPU; the mesh evaluator has no host path')
            dev = torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise RuntimeError('evaluator_mesh: meshes are evaluated on a GPU; there is no host path')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _as_tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _mesh(verts, faces, dev):
    """float32 (V,3) vertices and int32 (F,3) faces on the device (a float64 mesh is rounded once)."""
    v = _as_tensor(verts).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    f = _as_tensor(faces).detach().to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    if f.shape[0] > _lib.MESH_MAX_FACES:
        raise ValueError(f'evaluator_mesh: {f.shape[0]} faces, the limit is 2^26')
    return v, f


def _f64(a, dev, cols):
    return _as_tensor(a).detach().to(device=dev, dtype=torch.float64).reshape(-1, cols).contiguous()


_ws = {}  # device -> uint8 workspace tensor


def _workspace(lib, dev, nf, npts):
    nbytes = lib.anr_mesh_dist_workspace_bytes(max(int(nf), 1), int(npts))
    if nbytes == 0:
        raise ValueError(f'evaluator_mesh: {nf} faces / {npts} points are outside the limits (2^26 / 1..2^24)')
    ws = _ws.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[dev] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def draw_uniforms(rng=None, n_chamfer=N_CHAMFER, n_p2s=N_P2S):
    """The (2 n_chamfer + n_p2s, 3) uniforms of one frame in the reference's order of draws
    (mesh_evaluator.py:103-107, 126-127): Chamfer source, Chamfer target, P2S source; each
    ``sample_surface`` call draws its ``n`` face picks, then its ``(n, 2)`` lengths."""
    random = np.random.random if rng is None else rng.random
    parts = []
    for n in (n_chamfer, n_chamfer, n_p2s):
        pick = random(n)
        lengths = random((n, 2))
        parts.append(np.concatenate([pick[:, None], lengths], axis=1))
    return np.concatenate(parts, axis=0)


# ---- public helpers ----------------------------------------------------------------------------------------
def mesh_sample(verts, faces, u, device=None, check=True):
    """``trimesh.sample.sample_surface(mesh, n)`` restated (parity unpinned): ``u`` (n,3) uniforms, or an int
    ``n`` (then drawn from ``np.random.random``: n picks, then (n,2) lengths). -> points (n,3) float64 and
    face (n,) int32 device tensors. ``check`` reads the status word (it synchronises) and raises ValueError
    for a mesh with no face or no finite positive area."""
    lib = _lib.load()
    dev = _device(device, verts, faces, u)
    if isinstance(u, (int, np.integer)):
        n = int(u)
        u = np.concatenate([np.random.random(n)[:, None], np.random.random((n, 2))], axis=1)
    du = _f64(u, dev, 3)
    n = du.shape[0]
    v, f = _mesh(verts, faces, dev)
    points = torch.empty((n, 3), dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(lib, dev, f.shape[0], n)
        _lib.check(lib.anr_mesh_sample(_lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], _lib.ptr(du), n,
                                       _lib.ptr(points), _lib.ptr(face), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr(dev)), 'anr_mesh_sample')
        for t in (v, f, du):
            t.record_stream(torch.cuda.current_stream(dev))
    if check and int(status.item()):
        raise ValueError('mesh_sample: the mesh has no face, or its total area is zero or not finite')
    return points, face


def mesh_point_distance(verts, faces, points, exhaustive=False, device=None, return_mean=False):
    """``trimesh.proximity.closest_point(mesh, points)``'s distances and faces: dist (n,) float64 and face (n,)
    int32 device tensors; ``return_mean`` adds the device's mean (one float64, NaN distances as 0).
    ``exhaustive`` (True, one of ``_lib.BWV_*``, or ``_lib.MESHDIST_PRUNED_CELLS``) selects the search; every
    search writes the same bits."""
    lib = _lib.load()
    dev = _device(device, verts, faces, points)
    v, f = _mesh(verts, faces, dev)
    p = _f64(points, dev, 3)
    n = p.shape[0]
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError('mesh_point_distance: the mesh has no face')
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    mean = torch.zeros(1, dtype=torch.float64, device=dev) if return_mean else None
    opts = _lib.MeshDistOpts(_lib.BWV_EXHAUSTIVE if exhaustive is True else int(exhaustive))
    with torch.cuda.device(dev):
        ws = _workspace(lib, dev, f.shape[0], n)
        _lib.check(lib.anr_mesh_point_dist(_lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], _lib.ptr(p), n,
                                           ctypes.byref(opts), _lib.ptr(dist), _lib.ptr(face), _lib.ptr(mean),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), 'anr_mesh_point_dist')
        for t in (v, f, p):
            t.record_stream(torch.cuda.current_stream(dev))
    return (dist, face, mean) if return_mean else (dist, face)


def _host_int(v):
    if torch.is_tensor(v):
        return int(v.reshape(-1)[0])
    return int(np.asarray(v).reshape(-1)[0])


# ---- the reference's interface ------------------------------------------------------------------------------
class Evaluator:
    INITIAL_ROWS = 64

    def __init__(self):
        self.cfg = _config.active()
        self.p2ss = []
        self.chamfers = []
        self._lib = None
        self._table = None  # (capacity, MESHM_NOUT) float64 on the device
        self._n = 0         # rows enqueued since the last summarize()
        self._names = []

    def _row(self, dev):
        if self._table is None or self._table.device != dev:
            if self._n:
                raise RuntimeError('mesh Evaluator: frames of one summarize() span must be on one device')
            self._table = torch.zeros((self.INITIAL_ROWS, _lib.MESHM_NOUT), dtype=torch.float64, device=dev)
        if self._n == self._table.shape[0]:
            grown = torch.zeros((2 * self._n, _lib.MESHM_NOUT), dtype=torch.float64, device=dev)
            grown[:self._n].copy_(self._table)
            self._table = grown
        return self._table[self._n]

    def _dataset(self, key, default=None):
        node = self.cfg.get('test_dataset', None)
        return node.get(key, default) if node is not None else default

    def _target(self, batch):
        if 'tgt_vertex' in batch and 'tgt_triangle' in batch:
            return batch['tgt_vertex'], batch['tgt_triangle']
        data_root = self._dataset('data_root')
        if data_root is None:
            raise KeyError("mesh Evaluator: no target mesh: give batch['tgt_vertex'] / batch['tgt_triangle'] "
                           "or cfg.test_dataset.data_root")
        return read_obj(os.path.join(data_root, 'object/{:06d}.obj'.format(_host_int(batch['frame_index']))))

    def evaluate(self, output, batch, u=None):
        if self._lib is None:
            self._lib = _lib.load()
        lib = self._lib
        vertices, triangles = output['posed_vertex'], output['triangle']
        dev = _device(None, vertices, triangles)
        tv, tt = self._target(batch)
        sv, sf = _mesh(vertices, triangles, dev)
        if 'rp' in str(self._dataset('human', '')):  # mesh_evaluator.py:22-27
            sv = torch.stack([sv[:, 0], sv[:, 2], -sv[:, 1]], dim=1).contiguous()
        tv, tf = _mesh(tv, tt, dev)
        if u is None or isinstance(u, np.random.Generator):
            u = draw_uniforms(u)
        du = _f64(u, dev, 3)
        if du.shape[0] != 2 * N_CHAMFER + N_P2S:
            raise ValueError(f'mesh Evaluator: u has {du.shape[0]} rows, a frame takes {2 * N_CHAMFER + N_P2S}')
        row = self._row(dev)
        opts = _lib.MeshDistOpts(_lib.BWV_DEFAULT, N_CHAMFER, N_P2S)
        with torch.cuda.device(dev):
            ws = _workspace(lib, dev, max(sf.shape[0], tf.shape[0]), du.shape[0])
            _lib.check(lib.anr_mesh_metrics(_lib.ptr(sv), sv.shape[0], _lib.ptr(sf), sf.shape[0], _lib.ptr(tv),
                                            tv.shape[0], _lib.ptr(tf), tf.shape[0], _lib.ptr(du), ctypes.byref(opts),
                                            _lib.ptr(row), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                       'anr_mesh_metrics')
            for t in (sv, sf, tv, tf, du):
                t.record_stream(torch.cuda.current_stream(dev))
        self._names.append(batch.get('frame_index'))
        self._n += 1
        if self.cfg.get('eval_write_meshes', False):
            self._write_mesh(sv, sf, batch)

    def _write_mesh(self, sv, sf, batch):
        """The reference's posed_mesh/{frame:04d}.ply (mesh_evaluator.py:46-55); the copy synchronises."""
        result_dir = os.path.join('data/animation/{}'.format(self.cfg.get('exp_name', 'hello')), 'posed_mesh')
        os.makedirs(result_dir, exist_ok=True)
        frame_index = _host_int(batch['frame_index'])
        write_ply(os.path.join(result_dir, '{:04d}.ply'.format(frame_index)), sv.cpu().numpy(), sf.cpu().numpy())

    def summarize(self):
        result_dir = self.cfg.result_dir
        rows = self._table[:self._n].cpu().numpy() if self._n else np.zeros((0, _lib.MESHM_NOUT))  # the one D2H copy
        try:
            for i in range(self._n):
                status = int(rows[i, _lib.MESHM_STATUS])
                if status:
                    which = ' and '.join(w for b, w in ((_lib.MESHM_BAD_SOURCE, 'extracted'), (_lib.MESHM_BAD_TARGET, 'target'))
                                         if status & b)
                    fi = self._names[i]
                    name = f'frame {i} of this run' + (f' (frame_index {_host_int(fi)})' if fi is not None else '')
                    raise ValueError(f'mesh Evaluator: {name}: the {which} mesh has no face, or its total area is '
                                     'zero or not finite: there is nothing to sample')
                self.p2ss.append(float(rows[i, _lib.MESHM_P2S]))
                self.chamfers.append(float(rows[i, _lib.MESHM_CHAMFER]))
            print('the results are saved at {}'.format(result_dir))
            result_path = os.path.join(result_dir, 'mesh_metrics.npy')
            os.makedirs(os.path.dirname(result_path) or '.', exist_ok=True)
            metrics = {'p2s': self.p2ss, 'chamfer': self.chamfers}
            np.save(result_path, metrics)
            print('p2s: {}'.format(np.mean(self.p2ss) if self.p2ss else float('nan')))
            print('chamfer: {}'.format(np.mean(self.chamfers) if self.chamfers else float('nan')))
        finally:
            self.p2ss, self.chamfers = [], []
            self._n = 0
            self._names = []
        return metrics
