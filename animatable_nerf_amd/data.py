"""Ray pipelines on the device, ``lib/utils/if_nerf/if_nerf_data_utils.py``:

* eval split: ``get_rays`` / ``get_rays_within_bounds`` (:64-89, 310-339) through ``anr_camera_rays``;
* train split: ``sample_ray_h36m(split='train')`` (:198-283) through ``anr_train_ray_lists`` /
  ``anr_train_ray_gather``: the pixel lists, rays, float64 box test, rgb gather and hit compaction
  run on the GPU; the np.random draws stay on the host so the random stream is the reference's.
  ``ResidentViews`` keeps a view's image, masks and pixel lists in HBM and draws a whole batch in one
  launch (``anr_train_ray_sample``: counter-based draws, no host in the loop).

The 3x3 inverse of K and the camera origin -R^T T are formed with numpy on the host exactly as the
reference does. ``get_bound_2d_mask`` (:114-136) is per-frame host work like the reference's; it
uses cv2.fillPoly there (cv2 is not installed here), restated below as the filled convex hull of
the projected box corners (unpinned at the polygon boundary).
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _camera(K, R, T):
    K = np.asarray(K)
    R = np.asarray(R)
    T = np.asarray(T)
    fp64 = K.dtype == np.float64 or R.dtype == np.float64 or T.dtype == np.float64
    Kinv = np.linalg.inv(K)                  # if_nerf_data_utils.py:81
    origin = -np.dot(R.T, T).ravel()         # :76
    as_d = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    return as_d(Kinv), as_d(R), as_d(T), as_d(origin), fp64


def get_rays_within_bounds(H, W, K, R, T, bounds, device='cuda'):
    """-> ray_o (n,3), ray_d (n,3), near (n,), far (n,), mask_at_box (H,W) bool, coord (n,2) int32,
    all on ``device`` (the reference returns numpy arrays of the same values)."""
    lib = _lib.load()
    dev = torch.device(device)
    Kinv, Rd, Td, o, fp64 = _camera(K, R, T)
    P = H * W
    b = torch.as_tensor(np.asarray(bounds, dtype=np.float32).reshape(2, 3)).to(dev)
    ray_o = torch.empty((P, 3), device=dev)
    ray_d = torch.empty((P, 3), device=dev)
    near = torch.empty(P, device=dev)
    far = torch.empty(P, device=dev)
    coord = torch.empty((P, 2), dtype=torch.int32, device=dev)
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.anr_camera_rays_workspace_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(lib.anr_camera_rays(H, W, dp(Kinv), dp(Rd), dp(Td), dp(o), 1 if fp64 else 0, _lib.ptr(b),
                                   _lib.ptr(ray_o), _lib.ptr(ray_d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(coord),
                                   _lib.ptr(mask), _lib.ptr(count), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev)),
               'anr_camera_rays')
    n = int(count.item())
    return ray_o[:n], ray_d[:n], near[:n], far[:n], mask.view(H, W).bool(), coord[:n]


def _project(xyz, K, RT):
    """lib/utils/base_utils.py:86-95."""
    xyz = np.dot(xyz, RT[:, :3].T) + RT[:, 3:].T
    xyz = np.dot(xyz, K.T)
    return xyz[:, :2] / xyz[:, 2:]


def get_bound_corners(bounds):
    """if_nerf_data_utils.py:92-111 (x-major corner order)."""
    (x0, y0, z0), (x1, y1, z1) = bounds
    return np.array([[x0, y0, z0], [x0, y0, z1], [x0, y1, z0], [x0, y1, z1],
                     [x1, y0, z0], [x1, y0, z1], [x1, y1, z0], [x1, y1, z1]])


def get_bound_2d_mask(bounds, K, pose, H, W):
    """if_nerf_data_utils.py:114-136: the six projected box faces filled with 1 (u8 (H, W)). Their
    union is the convex hull of the 8 rounded projected corners; filled here as every pixel inside
    or on that hull (cv2.fillPoly's boundary rasterisation is not reproduced: cv2 is absent)."""
    c2 = np.round(_project(get_bound_corners(np.asarray(bounds)), np.asarray(K), np.asarray(pose))).astype(np.int64)
    mask = np.zeros((H, W), dtype=np.uint8)
    pts = sorted(set(map(tuple, c2.tolist())))
    if len(pts) < 3:
        return mask

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:  # monotone chain, counter-clockwise in (x, y)
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]
    if len(hull) < 3:
        return mask
    xs = [p[0] for p in hull]
    ys = [p[1] for p in hull]
    x0, x1 = max(min(xs), 0), min(max(xs), W - 1)
    y0, y1 = max(min(ys), 0), min(max(ys), H - 1)
    if x0 > x1 or y0 > y1:
        return mask
    gx, gy = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), indexing='xy')
    inside = np.ones(gx.shape, dtype=bool)
    for k in range(len(hull)):
        a, b = hull[k], hull[(k + 1) % len(hull)]
        inside &= (b[0] - a[0]) * (gy - a[1]) - (b[1] - a[1]) * (gx - a[0]) >= 0
    mask[y0:y1 + 1, x0:x1 + 1] = inside
    return mask


def sample_ray_h36m(img, msk, K, R, T, bounds, nrays, split, mask_bkgd=True, body_sample_ratio=0.5,
                    face_sample_ratio=0.0, bound_mask=None, rng=None, device='cuda'):
    """if_nerf_data_utils.py:198-307 on the device. -> rgb (n,3), ray_o (n,3), ray_d (n,3), near (n,),
    far (n,), coord (n,2) int32, mask_at_box (torch tensors on ``device``; the reference returns the
    same values as numpy arrays). ``cfg.mask_bkgd`` / ``cfg.body_sample_ratio`` /
    ``cfg.face_sample_ratio`` are arguments; ``rng`` (default ``np.random``) makes the draws, in the
    reference's call order, so a seeded run draws exactly the reference's pixels. ``bound_mask``
    overrides ``get_bound_2d_mask``."""
    lib = _lib.load()
    dev = torch.device(device)
    rng = np.random if rng is None else rng
    H, W = img.shape[:2]
    if bound_mask is None:
        pose = np.concatenate([np.asarray(R), np.asarray(T).reshape(3, 1)], axis=1)
        bound_mask = get_bound_2d_mask(bounds, K, pose, H, W)
    Kinv, Rd, Td, o, fp64 = _camera(K, R, T)
    b = torch.as_tensor(np.asarray(bounds, dtype=np.float32).reshape(2, 3)).to(dev)
    img_d = torch.as_tensor(np.ascontiguousarray(img, dtype=np.float32)).to(dev)
    bm_d = torch.as_tensor(np.ascontiguousarray(bound_mask, dtype=np.uint8)).to(dev)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    stream = _lib.stream_ptr(dev)
    if split != 'train':
        ray_o, ray_d, near, far, mask, coord = get_rays_within_bounds(H, W, K, R, T, bounds, device=device)
        img_z = img_d * (bm_d == 1).unsqueeze(-1) if mask_bkgd else img_d  # :228
        rgb = img_z[coord[:, 0].long(), coord[:, 1].long()]
        return rgb, ray_o, ray_d, near, far, coord, mask.reshape(-1)
    msk_d = torch.as_tensor(np.ascontiguousarray(msk, dtype=np.uint8)).to(dev)
    P = H * W
    lists = torch.empty(3 * P, dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    ws_bytes = lib.anr_train_ray_workspace_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.anr_train_ray_lists(H, W, _lib.ptr(msk_d), _lib.ptr(bm_d), _lib.ptr(lists), _lib.ptr(counts),
                                       _lib.ptr(ws), ws_bytes, stream), 'anr_train_ray_lists')
    n_body_px, n_face_px, n_bound_px = (int(v) for v in counts.cpu())
    ray_o = torch.empty((nrays, 3), device=dev)
    ray_d = torch.empty((nrays, 3), device=dev)
    rgb = torch.empty((nrays, 3), device=dev)
    near = torch.empty(nrays, device=dev)
    far = torch.empty(nrays, device=dev)
    coord = torch.empty((nrays, 2), dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    nsampled = 0
    while nsampled < nrays:  # :236-271, one device round per loop iteration
        n_body = int((nrays - nsampled) * body_sample_ratio)
        n_face = int((nrays - nsampled) * face_sample_ratio)
        n_rand = (nrays - nsampled) - n_body - n_face
        d_body = rng.randint(0, n_body_px, n_body)
        if n_face_px > 0:
            d_face = rng.randint(0, n_face_px, n_face)
        else:
            d_face = np.zeros(0, dtype=np.int64)
        d_rand = rng.randint(0, n_bound_px, n_rand)
        draws = torch.as_tensor(np.concatenate([d_body, d_face, d_rand]).astype(np.int32)).to(dev)
        _lib.check(lib.anr_train_ray_gather(H, W, dp(Kinv), dp(Rd), dp(Td), dp(o), 1 if fp64 else 0, _lib.ptr(b),
                                            _lib.ptr(img_d), _lib.ptr(bm_d), 1 if mask_bkgd else 0, _lib.ptr(lists),
                                            _lib.ptr(draws), len(d_body), len(d_face), len(d_rand), nrays,
                                            _lib.ptr(ray_o), _lib.ptr(ray_d), _lib.ptr(rgb), _lib.ptr(near),
                                            _lib.ptr(far), _lib.ptr(coord), _lib.ptr(n_out), stream),
                   'anr_train_ray_gather')
        nsampled = int(n_out.item())
    mask_at_box = torch.ones(nrays, dtype=torch.bool, device=dev)
    return rgb, ray_o, ray_d, near, far, coord, mask_at_box


class ResidentViews:
    """Training views kept resident in HBM, and the train-split batch drawn from them on the device.

    ``sample_ray_h36m(split='train')`` uploads the image and masks, rebuilds the pixel lists, reads
    their counts back, draws with np.random on the host and reads ``n_out`` once per resampling round:
    host round trips in front of every training step. Here ``add`` does the per-view work once (upload,
    ``anr_train_ray_lists``, one read of the counts) and ``sample`` is one ``anr_train_ray_sample``
    launch that runs the whole loop of if_nerf_data_utils.py:236-271 on the device with counter-based
    draws (Philox4x32-10 keyed by ``seed``, counted by ``step``, the round and the slot; see
    include/aninerf.h): no host sync, no H2D copy, no host RNG between two steps. The rays are NOT the
    ones np.random would draw; they are the same function of (seed, step) on every run.

    Multi-rank training: every rank must draw different rays, so the caller folds its rank into
    ``seed`` (e.g. ``seed = base_seed * world_size + rank``); ``step`` is the global iteration.

    A batch can fall short of ``nrays`` only when ``max_rounds`` rounds did not find enough rays that
    hit the box; the missing rows are rays with ``mask_at_box == 0`` (the training losses skip them)
    and are counted in ``shortfall()``."""

    VOLATILE = ('rgb', 'ray_o', 'ray_d', 'near', 'far', 'mask_at_box', 'coord', 'occupancy')

    def __init__(self, device='cuda', nrays=1024, seed=0, mask_bkgd=True, body_sample_ratio=0.5,
                 face_sample_ratio=0.0, max_rounds=64):
        self.lib = _lib.load()
        self.device = dev = torch.device(device)
        self.nrays, self.seed, self.max_rounds = int(nrays), int(seed), int(max_rounds)
        self.mask_bkgd = bool(mask_bkgd)
        self.body_ratio, self.face_ratio = float(body_sample_ratio), float(face_sample_ratio)
        if not 1 <= self.nrays <= 65536:
            raise ValueError(f'ResidentViews: nrays must be in 1..65536, got {nrays}')
        if not 1 <= self.max_rounds <= 1024:
            raise ValueError(f'ResidentViews: max_rounds must be in 1..1024, got {max_rounds}')
        if not (0.0 <= self.body_ratio <= 1.0 and 0.0 <= self.face_ratio <= 1.0
                and self.body_ratio + self.face_ratio <= 1.0):
            raise ValueError('ResidentViews: the sample ratios must lie in [0,1] and sum to at most 1')
        R = self.nrays
        self._out = {'rgb': torch.zeros((1, R, 3), device=dev), 'ray_o': torch.zeros((1, R, 3), device=dev),
                     'ray_d': torch.zeros((1, R, 3), device=dev), 'near': torch.zeros((1, R), device=dev),
                     'far': torch.zeros((1, R), device=dev),
                     'mask_at_box': torch.zeros((1, R), dtype=torch.uint8, device=dev),
                     'coord': torch.zeros((1, R, 2), dtype=torch.int32, device=dev)}
        self._occupancy = torch.zeros((1, R), dtype=torch.uint8, device=dev)
        self.n_out = torch.zeros(1, dtype=torch.int32, device=dev)
        self._shortfall = torch.zeros(1, dtype=torch.int32, device=dev)
        self._views = {}

    def add(self, key, img, msk, K, R, T, bounds, bound_mask=None, orig_msk=None):
        """Make view ``key`` resident (one-time work per (frame, view); synchronises once). Arguments as
        ``sample_ray_h36m``; ``orig_msk`` is the occupancy mask of tpose_dataset.py:229-233, already
        through ``crop_mask_edge`` where the caller applies it. ValueError where no batch could be
        drawn: an empty bound list, or an empty body list with a body ratio above 0."""
        dev = self.device
        H, W = img.shape[:2]
        if bound_mask is None:
            pose = np.concatenate([np.asarray(R), np.asarray(T).reshape(3, 1)], axis=1)
            bound_mask = get_bound_2d_mask(bounds, K, pose, H, W)
        v = {'H': H, 'W': W}
        v['cam'] = _camera(K, R, T)
        v['bounds'] = torch.as_tensor(np.asarray(bounds, dtype=np.float32).reshape(2, 3)).to(dev)
        v['img'] = torch.as_tensor(np.ascontiguousarray(img, dtype=np.float32)).to(dev)
        v['bm'] = torch.as_tensor(np.ascontiguousarray(bound_mask, dtype=np.uint8)).to(dev)
        v['occ'] = None
        if orig_msk is not None:
            if tuple(np.shape(orig_msk)) != (H, W):
                raise ValueError(f'ResidentViews.add: orig_msk {np.shape(orig_msk)} is not the image size {(H, W)}')
            v['occ'] = torch.as_tensor(np.ascontiguousarray(orig_msk, dtype=np.uint8)).to(dev)
        msk_d = torch.as_tensor(np.ascontiguousarray(msk, dtype=np.uint8)).to(dev)
        P = H * W
        lists = torch.empty(3 * P, dtype=torch.int32, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        ws_bytes = self.lib.anr_train_ray_workspace_bytes(H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.anr_train_ray_lists(H, W, _lib.ptr(msk_d), _lib.ptr(v['bm']), _lib.ptr(lists),
                                                _lib.ptr(counts), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev)),
                   'anr_train_ray_lists')
        n = [int(c) for c in counts.cpu()]
        if n[2] <= 0:
            raise ValueError(f'ResidentViews.add({key!r}): no pixel in the bound mask')
        if n[0] <= 0 and self.body_ratio > 0:
            raise ValueError(f'ResidentViews.add({key!r}): no body pixel (msk == 1) with body_sample_ratio > 0')
        v['n'] = n
        v['lists'] = [lists[k * P:k * P + n[k]].clone() for k in range(3)]  # the used prefixes only
        Kinv, Rd, Td, o, fp64 = v['cam']
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        lp = lambda t: _lib.ptr(t) if t.numel() else None
        has_occ = v['occ'] is not None
        # everything of the call but (seed, step, stream)
        v['head'] = (H, W, dp(Kinv), dp(Rd), dp(Td), dp(o), 1 if fp64 else 0, _lib.ptr(v['bounds']), _lib.ptr(v['img']),
                     _lib.ptr(v['bm']), _lib.ptr(v['occ']) if has_occ else None, lp(v['lists'][0]), lp(v['lists'][1]),
                     lp(v['lists'][2]), n[0], n[1], n[2], 1 if self.mask_bkgd else 0, self.body_ratio, self.face_ratio,
                     self.nrays, self.max_rounds)
        out = self._out
        v['tail'] = tuple(_lib.ptr(out[k]) for k in ('ray_o', 'ray_d', 'rgb', 'near', 'far', 'coord', 'mask_at_box')) + (
            _lib.ptr(self._occupancy) if has_occ else None, _lib.ptr(self.n_out), _lib.ptr(self._shortfall))
        self._views[key] = v

    def sample(self, key, step):
        """One launch: the batch of view ``key`` at iteration ``step`` written into the object's fixed
        buffers. -> dict of ``rgb, ray_o, ray_d (1,R,3)``, ``near, far (1,R)`` float32, ``mask_at_box
        (1,R)`` uint8, ``coord (1,R,2)`` int32, ``occupancy (1,R)`` uint8 when the view has ``orig_msk``
        — the same tensor objects on every call, valid until the next ``sample`` — and
        ``'anr_volatile'``, the names of those keys: they are rewritten in place without a bump of
        their version counters, so whoever caches copies by version (FusedStep) must copy them anew."""
        v = self._views[key]
        _lib.check(self.lib.anr_train_ray_sample(*v['head'], self.seed & 0xFFFFFFFFFFFFFFFF,
                                                 int(step) & 0xFFFFFFFFFFFFFFFF, *v['tail'],
                                                 _lib.stream_ptr(self.device)), 'anr_train_ray_sample')
        out = dict(self._out)
        if v['occ'] is not None:
            out['occupancy'] = self._occupancy
        out['anr_volatile'] = tuple(k for k in self.VOLATILE if k in out)
        return out

    def shortfall(self):
        """Rays missing from all batches so far (reads the device counter: the one synchronising call,
        meant for once per epoch)."""
        return int(self._shortfall.item())

    def resident_bytes(self):
        ts = [t for v in self._views.values() for t in [v['img'], v['bm'], v['bounds'], v['occ']] + v['lists']
              if t is not None]
        return sum(t.numel() * t.element_size() for t in ts)


class ResidentFrames:
    """Per-frame batch tensors kept resident in HBM across steps ("the
    per-image H2D of pbw/tbw volumes"). The reference's ``Trainer.to_cuda`` (trainer.py:39-48) moves
    the frame's blend-weight volumes (~29 MB, tpose_dataset.py:157-217) and transforms host to device
    with every batch; a whole sequence fits in one MI355X's 288 GB (300 frames x 29 MB = 8.7 GB),
    so here each frame's tensors cross PCIe once and later batches of that frame reuse them.

    ``to_device(batch)`` -> a batch on ``device``: the ``keys`` (per-frame, never written by the
    renderers) come from the cache keyed by (frame_index, key) — or by the subject for ``SUBJECT_KEYS`` —
    and everything else is copied as usual. A batch must hold a single frame (all frame_index equal).
    ``tbounds`` is not cached: the sdf_pdf renderer widens it in place per chunk, as the reference does."""

    KEYS = ('pbw', 'tbw', 'A', 'big_A', 'pbounds', 'wbounds', 'R', 'Th')
    # the same tensor for every frame of a subject: tbw is the T-pose template's volume
    # (lbs_root/tbw.npy, tpose_dataset.py:213-216), big_A the fixed big pose (tpose_pdf_dataset.py:81,
    # 91-100); cached once, not once per frame (~11 MB per frame saved for tbw)
    SUBJECT_KEYS = ('tbw', 'big_A')

    def __init__(self, device='cuda', keys=KEYS):
        self.device = torch.device(device)
        self.keys = tuple(keys)
        self._cache = {}
        self.uploads = 0

    def _frame(self, batch):
        fi = batch.get('frame_index')
        if fi is None:
            raise KeyError("ResidentFrames needs the batch's 'frame_index' (tpose_dataset.py:277)")
        fis = torch.as_tensor(fi).reshape(-1)
        if fis.numel() == 0:
            raise ValueError('ResidentFrames: empty frame_index')
        # the cached tensors are one frame's: a batch that mixes frames (train.batch_size > 1 over
        # several images) would silently get the first frame's volumes and transforms
        if not bool((fis == fis[0]).all()):
            raise ValueError(f'ResidentFrames: a batch must hold one frame, got frame_index {fis.tolist()}')
        return int(fis[0])

    def to_device(self, batch):
        fi = self._frame(batch)
        out = {}
        for k, v in batch.items():
            if k in self.keys:
                key = ('subject', k) if k in self.SUBJECT_KEYS else (fi, k)
                t = self._cache.get(key)
                if t is None:
                    t = torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v)
                    t = t.to(self.device).contiguous()
                    self._cache[key] = t
                    self.uploads += 1
                out[k] = t
            elif isinstance(v, np.ndarray):
                out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
            elif torch.is_tensor(v):
                out[k] = v.to(self.device)
            else:
                out[k] = v
        return out

    def resident_bytes(self):
        return sum(t.numel() * t.element_size() for t in self._cache.values())

    def clear(self):
        self._cache.clear()
