"""CPU pin of tests/lbw_ref.py (the aligned_aninerf_lbw restatement) to the reference's own outputs: G16 (64 rays
with intermediates) and G17 (4,136 rays in chunks of 2048 / 2048 / 40 over a shrunk tbounds), both written by
tools/gen_golden_lbw.py from the real reference. Bit-exact: keep mask, tbounds, alpha_ind row count. Within 1e-6:
everything else. Also re-asserts G17's non-vacuity conditions from the stored arrays, and that the float32 and
float64 restatements decide ``alpha > 0`` alike except at the stored fp32-edge samples, which stay under 0.1 % of
the alpha_ind rows."""
import functools
import importlib.util
import os

import numpy as np
import torch

from tests import lbw_ref
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
    """The goldens are the reference on one CPU thread; torch's fp32 matmuls sum in another order on more threads
    (measured here on the tbw rows: 1.0e-6 with 8 threads, 0 with one), so the float32 pin runs on one thread too."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


@functools.lru_cache(maxsize=1)
def _g16():
    g = golden('g16_lbw_tiny')
    batch, P = lbw_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    trace = {}
    with _one_thread():
        ret = lbw_ref.render(P, batch, trace=trace)
    return g, batch, ret, trace['chunks'][0]


@functools.lru_cache(maxsize=2)
def _g17(dtype):
    g = golden('g17_lbw_chunks')
    batch, P = lbw_ref.scene_batch(g['ray_o'], g['ray_d'], latent_index=int(g['latent_index']))
    batch['tbounds'] = torch.from_numpy(g['tbounds_before'].copy())
    if dtype != torch.float32:
        P, batch = lbw_ref.to_dtype(P, batch, dtype)
    trace = {}
    if dtype == torch.float32:
        with _one_thread():
            ret = lbw_ref.render(P, batch, trace=trace)
    else:
        ret = lbw_ref.render(P, batch, trace=trace)
    return g, batch, ret, trace


def test_g16_inputs_are_the_generators():
    g, batch, _, _ = _g16()
    assert np.array_equal(batch['near'].numpy(), g['near']) and np.array_equal(batch['far'].numpy(), g['far'])


def test_g16_mask_tbounds_rows_bit_exact():
    g, batch, ret, c = _g16()
    pn = g['pnorm'][0, :, 0]
    keep = pn < lbw_ref.NORM_TH
    keep[int(pn.argmin())] = True
    assert np.array_equal(c['pind'][0].numpy(), keep)
    assert np.array_equal(batch['tbounds'].numpy(), g['tbounds_after'])
    assert not np.array_equal(g['tbounds_before'], g['tbounds_after'])
    assert ret['pbw'].shape == g['out_pbw'].shape and ret['tbw'].shape == g['out_tbw'].shape


def test_g16_intermediates_and_outputs():
    g, _, ret, c = _g16()
    _close(c['pnorm'][..., None], g['pnorm'], 'pnorm')
    for k in ('init_pbw', 'init_tbw', 'pbw', 'tbw', 'tpose', 'tpose_dirs', 'th_raw'):
        _close(c[k], g[k], k)
    for k in ('raw', 'rgb_map', 'acc_map', 'depth_map', 'pbw', 'tbw'):
        _close(ret[k], g['out_' + k], 'out_' + k)


def _kept(trace):
    return torch.cat([c['pind'][0] for c in trace['chunks']]).numpy()


def test_g17_mask_tbounds_rows_bit_exact():
    g, batch, ret, trace = _g17(torch.float32)
    assert np.array_equal(np.packbits(_kept(trace)), g['keep_bits'])
    assert np.array_equal(batch['tbounds'].numpy(), g['tbounds_after'])
    assert ret['pbw'].shape[1] == int(g['bw_rows']) == ret['tbw'].shape[1]
    ai = torch.cat([c['alpha_ind'] for c in trace['chunks']]).numpy()
    assert np.array_equal(np.packbits(ai), g['bw_row_bits'])


def test_g17_outputs():
    g, _, ret, trace = _g17(torch.float32)
    keep = _kept(trace)
    for k in ('rgb_map', 'acc_map', 'depth_map'):
        _close(ret[k], g['out_' + k], k)
    _close(ret['raw'][0, torch.from_numpy(keep), 3], g['kept_alpha'], 'kept alpha')
    rows = g['bw_sample_idx']
    _close(ret['pbw'][0, rows], g['pbw_sample'], 'pbw rows')
    _close(ret['tbw'][0, rows], g['tbw_sample'], 'tbw rows')


def _generator():
    spec = importlib.util.spec_from_file_location('gen_golden_lbw', os.path.join(REPO, 'tools', 'gen_golden_lbw.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_g17_is_not_vacuous():
    """The generator's conditions, from the stored arrays alone."""
    g = golden('g17_lbw_chunks')
    gen = _generator()
    R = int(g['mask'].sum())
    keep = np.unpackbits(g['keep_bits'])[:R * 64].astype(bool)
    per_chunk, late, frac = gen.nonvacuity(keep, g['kept_alpha'], g['late_idx'], g['late_tpose'], g['tbounds_before'], R)
    print(f'kept per chunk {per_chunk}, {late} late samples, {100 * frac:.1f} % with alpha > 0')
    assert [2048, 2048, 40] == [min(2048, R - i) for i in range(0, R, 2048)]
    assert per_chunk[-1] == 1                      # the 40-ray chunk keeps exactly its forced argmin
    assert late >= 50 and late == g['late_idx'].shape[0]   # decided by the per-chunk widening
    assert 0.05 <= frac <= 0.95
    assert int(g['latent_index']) != 0


def test_g17_float64_margin_names_the_fp32_edges():
    """float32 vs float64 restatement: the alpha_ind decisions agree except at samples the float64 run puts within
    EDGE_MARGIN of the decision (the stored edge list), and the samples decided differently stay under 0.1 % of
    the rows: the cap tests/test_gpu_lbw.py allows for exclusions."""
    g, _, _, t32 = _g17(torch.float32)
    _, _, _, t64 = _g17(torch.float64)
    edges = lbw_ref.edge_samples(t64)
    assert np.array_equal(edges, g['edge_pid'])
    keep = _kept(t32)
    assert np.array_equal(keep, _kept(t64))
    kept_pid = np.nonzero(keep)[0]
    a32 = torch.cat([c['alpha_ind'] for c in t32['chunks']]).numpy()
    a64 = torch.cat([c['alpha_ind'] for c in t64['chunks']]).numpy()
    differ = kept_pid[a32 != a64]
    print(f'{edges.shape[0]} samples on the edge, {differ.shape[0]} decided differently, of {int(g["bw_rows"])} rows')
    assert np.isin(differ, edges).all(), differ
    assert differ.shape[0] <= 0.001 * int(g['bw_rows'])
