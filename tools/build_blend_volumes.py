#!/usr/bin/env python
"""Build a subject's blend-weight volumes on the GPU, in the layout the datasets load
(``tpose_dataset.py:158, 216``): what the reference's ``tools/custom_dataset/prepare_blend_weights.py``
writes under ``lbs/``, without psbody.mesh, open3d, trimesh, cv2 or the SMPL pickle.

  python tools/build_blend_volumes.py --data <subject dir> --faces faces.npy --skin weights.npy \\
         --joints joints.npy --parents parents.npy [--out <subject dir>/lbs] [--frames 0 300 1]

Inputs: ``<data>/vertices/{i}.npy`` (V,3) world-space SMPL vertices and ``<data>/params/{i}.npy`` (a
pickled dict with ``Rh`` (1,3), ``Th`` (1,3), ``poses`` (1,72)) per frame; the model's faces (F,3), skinning
weights (V,24), T-pose joints (24,3) and kinematic parents (24,) as .npy files.

Outputs under ``--out``: ``bweights/{i}.npy`` (closest-vertex volume of the frame's pose-space mesh),
``tvertices.npy`` (inverse LBS of the first frame) and ``tbw.npy`` (closest-surface-point volume of the
T-pose mesh), all float32 ``(X, Y, Z, 25)`` except ``tvertices.npy`` (V,3) float64.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from animatable_nerf_amd import synthetic, volumes  # noqa: E402


def frame_ids(data, spec):
    if spec:
        begin, end, step = spec
        return list(range(begin, end, step))
    ids = [int(os.path.splitext(f)[0]) for f in os.listdir(os.path.join(data, 'vertices')) if f.endswith('.npy')]
    return sorted(ids)


def pose_space(data, i):
    """Frame i: pose-space vertices (V,3) float64 = (world - Th) R, and its axis-angle poses (24,3)."""
    params = np.load(os.path.join(data, 'params', f'{i}.npy'), allow_pickle=True).item()
    verts = np.load(os.path.join(data, 'vertices', f'{i}.npy')).astype(np.float64)
    R = synthetic.batch_rodrigues(np.asarray(params['Rh'], dtype=np.float64).reshape(1, 3))[0]
    Th = np.asarray(params['Th'], dtype=np.float64).reshape(1, 3)
    return np.dot(verts - Th, R), np.asarray(params['poses'], dtype=np.float64).reshape(-1, 3)


def build(data, faces, skin, joints, parents, out=None, frames=None, vsize=0.025, device='cuda'):
    """Write the volumes; returns the list of files written."""
    out = out or os.path.join(data, 'lbs')
    os.makedirs(os.path.join(out, 'bweights'), exist_ok=True)
    ids = frame_ids(data, frames)
    if not ids:
        raise SystemExit(f'no frames under {data}/vertices')
    written = []
    for n, i in enumerate(ids):
        pxyz, poses = pose_space(data, i)
        if n == 0:
            A = synthetic.rigid_transformation(poses, joints.astype(np.float64), parents)
            tverts = volumes.tpose_vertices(pxyz, skin, A)
            np.save(os.path.join(out, 'tvertices.npy'), tverts)
            tbw = volumes.blend_weight_volume(tverts, skin, faces=faces, vsize=vsize, device=device)
            np.save(os.path.join(out, 'tbw.npy'), tbw.cpu().numpy())
            written += [os.path.join(out, 'tvertices.npy'), os.path.join(out, 'tbw.npy')]
        vol = volumes.blend_weight_volume(pxyz, skin, vsize=vsize, device=device)
        path = os.path.join(out, 'bweights', f'{i}.npy')
        np.save(path, vol.cpu().numpy())
        written.append(path)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data', required=True)
    for name in ('faces', 'skin', 'joints', 'parents'):
        ap.add_argument('--' + name, required=True, help=f'{name} .npy')
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', type=int, nargs=3, metavar=('BEGIN', 'END', 'STEP'), default=None)
    ap.add_argument('--vsize', type=float, default=0.025)
    ap.add_argument('--device', default='cuda')
    a = ap.parse_args(argv)
    written = build(a.data, np.load(a.faces).astype(np.int32), np.load(a.skin).astype(np.float32),
                    np.load(a.joints), np.load(a.parents).astype(np.int64), a.out, a.frames, a.vsize, a.device)
    print(f'wrote {len(written)} files under {a.out or os.path.join(a.data, "lbs")}')


if __name__ == '__main__':
    main()
