"""ORACLE — test infrastructure only. Golden G15 (tests/golden/g15_nsamples.npz): the REAL reference rendered
with ``N_samples 128`` as a command-line override (the recipe of oracle/gen_goldens.py, which this imports and
does not edit), on CPU with one thread, over G2's rays [0:2048] + [4096:4136]: one full reference chunk of box
rays and a 40-ray chunk of corner-grazing rays that keeps exactly its forced argmin sample. Stores what G2
stores: the three maps, the packed keep bits, the kept samples' alpha, the alpha_ind row count and every 37th
pbw / tbw row.

Run:  python tools/gen_golden_nsamples.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N_SAMPLES = 128
RAYS = (slice(0, 2048), slice(4096, 4136))  # of G2's ray arrays


def main():
    import torch
    torch.set_num_threads(1)
    from oracle import gen_goldens
    from animatable_nerf_amd.synthetic import Scene, init_state_dict
    g2 = np.load(os.path.join(gen_goldens.OUT, 'g2_chunks.npz'))
    ro = np.concatenate([g2['ray_o'][s] for s in RAYS])
    rd = np.concatenate([g2['ray_d'][s] for s in RAYS])
    cfg, make_network, make_renderer = gen_goldens.import_reference(opts=('N_samples', str(N_SAMPLES)))
    assert int(cfg.N_samples) == N_SAMPLES
    from lib.utils.if_nerf import if_nerf_data_utils as dutils

    net = make_network(cfg)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = init_state_dict(shapes)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    cfg.perturb = 0
    net.train()  # run.py evaluates in train() mode with perturb = 0
    renderer = make_renderer(cfg, net)

    scene = Scene(vsize=0.05)
    near, far, mask = dutils.get_near_far(scene.bounds, ro, rd)
    b = scene.batch_arrays(ro[mask], rd[mask], near.astype(np.float32), far.astype(np.float32))
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
    with torch.no_grad():
        ret = renderer.render(batch)
    R = int(mask.sum())
    assert ret['raw'].shape == (1, R * N_SAMPLES, 4), ret['raw'].shape
    keep = (ret['raw'][0, :, :3].abs().sum(-1) != 0).numpy()
    rows = np.arange(0, ret['pbw'].shape[1], 37)
    out = dict(ray_o=ro, ray_d=rd, mask=mask, n_samples=np.int64(N_SAMPLES),
               **{'out_' + k: ret[k].numpy() for k in ('rgb_map', 'acc_map', 'depth_map')},
               keep_bits=np.packbits(keep), kept_alpha=ret['raw'][0, keep, 3].numpy(),
               bw_rows=np.int64(ret['pbw'].shape[1]), bw_sample_idx=rows,
               pbw_sample=ret['pbw'][0, rows].numpy(), tbw_sample=ret['tbw'][0, rows].numpy())
    path = os.path.join(gen_goldens.OUT, 'g15_nsamples.npz')
    np.savez_compressed(path, **out)
    per_chunk = [int(keep.reshape(R, N_SAMPLES)[i:i + 2048].sum()) for i in range(0, R, 2048)]
    print(f'{path}: {R} hits, kept per chunk {per_chunk}, {int(out["bw_rows"])} alpha_ind rows, '
          f'{os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
