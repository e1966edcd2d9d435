"""CPU pin of tests/pdf_ref.py (the aligned_aninerf_pdf restatement) to the reference's own outputs: G18 (64 rays
with intermediates) and G19 (4,136 rays in chunks of 2048 / 2048 / 40 over a shrunk tbounds), both written by
tools/gen_golden_pdf.py from the real reference, and G20 (get_alpha over a coarse grid). Bit-exact: keep mask, tbounds, the box decisions. Within 1e-6:
everything else. Also re-asserts the generator's non-vacuity conditions from the stored arrays, and that the float32
and float64 restatements decide the box test alike except at the stored fp32-edge samples, which stay under 0.1 % of
the kept samples."""
import functools
import importlib.util
import os

import numpy as np
import torch

from tests import pdf_ref
from tests._common import golden

ATOL = 1e-6
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref, what):
    got = np.asarray(got.detach().numpy() if hasattr(got, 'detach') else got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    print(f'{what}: max |err| {err:.3e}')
    assert err <= ATOL, (what, err)


class _one_thread:
    """The goldens are the reference on one CPU thread; torch's fp32 matmuls sum in another order on more threads,
    so the float32 pin runs on one thread too (tests/test_lbw_ref.py)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


@functools.lru_cache(maxsize=1)
def _g18():
    g = golden('g18_pdf_tiny')
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    trace = {}
    with _one_thread():
        ret = pdf_ref.render(P, batch, trace=trace)
    return g, batch, ret, trace['chunks'][0]


@functools.lru_cache(maxsize=2)
def _g19(dtype):
    g = golden('g19_pdf_chunks')
    batch, P = pdf_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    batch['tbounds'] = torch.from_numpy(g['tbounds_before'].copy())
    if dtype != torch.float32:
        P, batch = pdf_ref.to_dtype(P, batch, dtype)
    trace = {}
    if dtype == torch.float32:
        with _one_thread():
            ret = pdf_ref.render(P, batch, trace=trace)
    else:
        ret = pdf_ref.render(P, batch, trace=trace)
    return g, batch, ret, trace


def _keep18(g):
    pn = g['pnorm'][0, :, 0]
    keep = pn < pdf_ref.NORM_TH
    keep[int(pn.argmin())] = True
    return pn, keep


def test_g18_inputs_are_the_generators():
    g, batch, _, _ = _g18()
    assert np.array_equal(batch['near'].numpy(), g['near']) and np.array_equal(batch['far'].numpy(), g['far'])


def test_g18_is_not_vacuous():
    """The generator's conditions, from the stored arrays alone."""
    g = golden('g18_pdf_tiny')
    pn, keep = _keep18(g)
    n = int(keep.sum())
    assert n == g['resd'].shape[1] and n % 128 != 0           # the last 128-row tile is partial
    assert int(((pn >= 0.05) & (pn < 0.1)).sum()) > 0        # the hard-coded 0.1 decides samples the yaml's 0.05 drops
    rmax = float(np.abs(g['resd']).max())
    assert 0.01 < rmax < 0.05, rmax                           # beyond tanh's linear range, short of saturation
    assert float(np.abs(g['resd']).min()) < 0.005             # and well inside it
    assert int(g['latent_index']) != 0


def test_g18_mask_tbounds_bit_exact():
    g, batch, ret, c = _g18()
    _, keep = _keep18(g)
    assert np.array_equal(c['pind'][0].numpy(), keep)
    assert np.array_equal(batch['tbounds'].numpy(), g['tbounds_after'])
    assert not np.array_equal(g['tbounds_before'], g['tbounds_after'])
    assert ret['resd'].shape == g['out_resd'].shape == (1, int(keep.sum()), 3)


def test_g18_intermediates_and_outputs():
    g, _, ret, c = _g18()
    _close(c['pnorm'][..., None], g['pnorm'], 'pnorm')
    _close(c['pbw'], g['pbw'], 'pbw')
    for k in ('init_bigpose', 'resd', 'tpose', 'tpose_dirs'):
        _close(c[k][None], g[k], k)
    _close(c['th_raw'], g['th_raw'], 'th_raw')
    _close(c['init_bigpose'] + c['resd'], g['tpose'][0], 'init_bigpose + resd')
    for k in ('raw', 'rgb_map', 'acc_map', 'depth_map', 'resd'):
        _close(ret[k], g['out_' + k], 'out_' + k)


def _kept(trace):
    return torch.cat([c['pind'][0] for c in trace['chunks']]).numpy()


def test_g19_mask_tbounds_box_decisions_bit_exact():
    g, batch, ret, trace = _g19(torch.float32)
    assert np.array_equal(np.packbits(_kept(trace)), g['keep_bits'])
    assert np.array_equal(batch['tbounds'].numpy(), g['tbounds_after'])
    assert ret['resd'].shape[1] == int(g['n_kept'])
    out = torch.cat([c['outside'] for c in trace['chunks']]).numpy()
    assert np.array_equal(np.packbits(out), g['outside_bits'])


def test_g19_outputs():
    g, _, ret, trace = _g19(torch.float32)
    keep = _kept(trace)
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        _close(ret[k], g['out_' + k], k)
    ka = ret['raw'][0, torch.from_numpy(keep)]
    _close(ka[::2, 3], g['kept_alpha_even'], 'kept alpha (every second)')
    assert int((ka[:, 3] > 0).sum()) == int(g['alpha_pos_count'])
    rows = g['row_sample_idx']
    _close(ret['resd'][0, rows], g['resd_sample'], 'resd rows')
    _close(torch.cat([c['tpose'] for c in trace['chunks']])[rows], g['tpose_sample'], 'tpose rows')
    _close(ka[rows, :3], g['rgb_sample'], 'rgb rows')


def _generator():
    spec = importlib.util.spec_from_file_location('gen_golden_lbw', os.path.join(REPO, 'tools', 'gen_golden_lbw.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_g19_is_not_vacuous():
    """The generator's conditions, from the stored arrays alone."""
    g = golden('g19_pdf_chunks')
    gen = _generator()
    R = int(g['mask'].sum())
    keep = np.unpackbits(g['keep_bits'])[:R * 64].astype(bool)
    per_chunk = [int(keep.reshape(R, 64)[i:i + 2048].sum()) for i in range(0, R, 2048)]
    n = int(keep.sum())
    assert [2048, 2048, 40] == [min(2048, R - i) for i in range(0, R, 2048)]
    assert per_chunk[-1] == 1                      # the 40-ray chunk keeps exactly its forced argmin
    # decided by the per-chunk widening: inside their own chunk's box, outside chunk 1's
    late = int(gen.late_samples(g['late_idx'].astype(np.int64), g['late_tpose'], per_chunk, g['tbounds_before']).sum())
    assert late == g['late_idx'].shape[0] >= 1000
    assert int(g['alpha_pos_count']) >= 0.5 * n    # pinned to the restatement's count by test_g19_outputs
    # decided by the displacement: init_bigpose and tpose on different sides of their chunk's strict box test
    boxes = np.stack(gen.chunk_boxes(g['tbounds_before'], len(per_chunk)))
    own = boxes[np.searchsorted(np.cumsum(per_chunk), g['side_idx'].astype(np.int64), side='right')]
    ins = lambda x: ((x > own[:, 0]) & (x < own[:, 1])).all(axis=1)
    side = int((ins(g['side_big']) != ins(g['side_tpose'])).sum())
    assert side == g['side_idx'].shape[0] >= 100
    assert g['edge_pid'].shape[0] <= 0.001 * n
    assert int(g['latent_index']) != 0
    print(f'kept per chunk {per_chunk}, {late} late samples stored, {side} side changes stored, '
          f'{100.0 * int(g["alpha_pos_count"]) / n:.1f} % with alpha > 0, {g["edge_pid"].shape[0]} edge samples')


def test_g19_float64_margin_names_the_fp32_edges():
    """float32 vs float64 restatement: the box decisions agree except at samples the float64 run puts within
    EDGE_MARGIN of a box face (the stored edge list), and those stay under 0.1 % of the kept samples: the cap
    tests/test_gpu_pdf.py allows for exclusions."""
    g, _, _, t32 = _g19(torch.float32)
    _, _, _, t64 = _g19(torch.float64)
    edges = pdf_ref.edge_samples(t64)
    assert np.array_equal(edges, g['edge_pid'])
    keep = _kept(t32)
    assert np.array_equal(keep, _kept(t64))
    kept_pid = np.nonzero(keep)[0]
    o32 = torch.cat([c['outside'] for c in t32['chunks']]).numpy()
    o64 = torch.cat([c['outside'] for c in t64['chunks']]).numpy()
    differ = kept_pid[o32 != o64]
    print(f'{edges.shape[0]} samples on the edge, {differ.shape[0]} decided differently, of {kept_pid.shape[0]} kept')
    assert np.isin(differ, edges).all(), differ
    assert edges.shape[0] <= 0.001 * kept_pid.shape[0]
    assert pdf_ref.box_side_changes(t64) >= 100


def test_g20_get_alpha():
    """Network.get_alpha over G20's grid points in one call: keep mask bit-exact, alpha within 1e-6; the fixture has
    both kept and dropped points and non-trivial densities of both signs."""
    g = golden('g20_pdf_alpha')
    g18, batch, _, _ = _g18()
    _, P = pdf_ref.scene_batch(g18['ray_o'], g18['ray_d'], latent_index=int(g18['latent_index']))
    trace = {}
    with _one_thread(), torch.no_grad():
        alpha = pdf_ref.get_alpha(P, torch.from_numpy(g['pts']), batch, trace=trace)
    keep = trace['keep'][0].numpy()
    assert np.array_equal(np.packbits(keep), g['keep_bits']) and int(keep.sum()) == int(g['n_kept'])
    assert 2000 <= g['pts'].shape[0] <= 9000 and 0 < keep.sum() < keep.shape[0]
    assert (g['alpha'][~keep] == 0).all() and g['alpha'].min() < 0 < g['alpha'].max()
    _close(alpha, g['alpha'], 'alpha')
