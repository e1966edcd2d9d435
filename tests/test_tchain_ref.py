"""CPU: the restated tables, image layout, mask-bit layout and layer reference of tests/tchain_ref.py checked
against the library's host functions, against themselves and against oracle/restate.py's bf16 emulation; the
conditions that keep the GPU cases of test_gpu_tchain.py from being vacuous; and the precondition rejections
of the two chain entries of the test library (which return before anything is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _tchain_hooks as H
from . import gemm_ref as R
from . import tchain_ref as T

FAKE = 0x10000  # a 16-B aligned non-NULL address; the rejected calls never touch it


# ---- tables and the image -------------------------------------------------------------------------------
def test_struct_sizes():
    L = H.lib()
    for which, S in H.SIZEOF.items():
        assert L.anr_test_tchain_sizeof(which) == C.sizeof(S), (which, S.__name__)
    assert L.anr_test_tchain_sizeof(4) == -1 and L.anr_test_tchain_sizeof(7) == -1


def test_tables_restated():
    assert [T.nslices(p) for p in range(4)] == [68, 89, 65, 86]
    L = H.lib()
    for p in range(4):
        assert T.image_bytes(p) == L.anr_test_tchain_image_bytes(p), p
    assert L.anr_test_tchain_image_bytes(4) == 0 and L.anr_test_tchain_image_bytes(-1) == 0
    assert [T.bits_rows_read(M) for M in (0, 1, 112, 113, 128, 341)] == [0, 128, 128, 240, 240, 464]


@pytest.mark.parametrize('prog', range(4))
def test_image_restatement_is_the_natural_order_reference(prog):
    """Decoded back to dense matrices, the restated image equals rne_bf16(W) at [natural neuron, natural k]
    and is 0 elsewhere: the image and layer_mats (what the layer reference multiplies by) agree."""
    W = T.gen_weights(prog, np.random.default_rng(11), False)
    img = T.restate_image(prog, W)
    assert img.size * 2 == T.image_bytes(prog)
    dense = T.decode_image(prog, img)
    nonzero = 0
    for l, (Dm, Dp) in enumerate(dense):
        Wm, Wp = T.layer_mats(prog, l, W)
        for D, Wn in ((Dm, Wm), (Dp, Wp)):
            want = np.zeros_like(D)
            want[:, :Wn.shape[1]] = R.rne_bf16(Wn)
            assert np.array_equal(D, want), (prog, l)
            nonzero += int((want != 0).sum())
    # the natural matrices hold every weight element the program consumes, once
    pd = T.pack_desc(prog)
    expect = 0
    for l, L in enumerate(T.PROGS[prog]):
        d = pd[l]
        if not T.bwd(prog):
            expect += (d['n1'] + d['n2']) * ((d['kmem_cols'] if L.kmem else 0) + (d['kprev_cols'] if L.kprev else 0))
        else:
            expect += (d['oa'] + d['nb']) * ((d['kmem_cols'] if L.kmem else 0) + (d['kprev_cols'] if L.kprev else 0))
    assert nonzero == expect   # (uniform weights: none rounds to 0)


def test_nrn_is_a_permutation_within_each_block_pair():
    for s in range(10):
        got = sorted(T.nrn(o, m) for o in (2 * s, 2 * s + 1) for m in range(16))
        assert got == list(range(32 * s, 32 * s + 32))


# ---- mask bits ---------------------------------------------------------------------------------------------
def test_mask_bits_roundtrip_and_formula():
    rng = np.random.default_rng(3)
    m = rng.uniform(0, 1, (37, 256)) < 0.5
    enc = T.encode_bits(m)
    assert enc.shape == (37, 32) and np.array_equal(T.decode_bits(enc), m)
    raw = rng.integers(0, 256, (19, 32)).astype(np.uint8)
    assert np.array_equal(T.encode_bits(T.decode_bits(raw)), raw)
    # spot values against the comment's formula, through little-endian dwords
    for n in (0, 1, 2, 7, 8, 31, 32, 127, 128, 129, 200, 255):
        one = np.zeros((1, 256), bool)
        one[0, n] = True
        dw = T.encode_bits(one).view('<u4')[0]
        s, h, j, e = n >> 5, (n >> 3) & 3, (n >> 1) & 3, n & 1
        want = np.zeros(8, np.uint32)
        want[2 * h + ((4 * s + j) >> 4)] = np.uint32(1) << np.uint32(((4 * s + j) & 15) + 16 * e)
        assert np.array_equal(dw, want), n


# ---- the chain reference against oracle/restate.py's bf16 emulation ----------------------------------------
def _oracle_weights():
    from ._common import oracle_params
    P = oracle_params()
    W = {}
    for l in range(8):
        W[f'bw{l}'] = P[f'bw_linears.{l}.weight'][:, :, 0].numpy()
        W[f'nf{l}'] = P[f'tpose_human.pts_linears.{l}.weight'][:, :, 0].numpy()
    W['bwfc'] = P['bw_fc.weight'][:, :, 0].numpy()
    for k in ('alpha', 'feature', 'latent', 'view', 'rgb'):
        W[k] = P[f'tpose_human.{k}_fc.weight'][:, :, 0].numpy()
    for k, v in W.items():
        assert v.shape == T.WEIGHT_SHAPES[k], k
    return P, W


def _fold(P, layer, lat_name, li, c0, c1):
    """k_fold_latent: bias + W[:, latent columns] . latent in fp32; the latent row is then zero for the oracle."""
    Wl = P[layer + '.weight'][:, c0:c1, 0]
    return (P[layer + '.bias'] + Wl @ P[lat_name][li]).to(torch.float32)


@pytest.mark.parametrize('prog', (0, 1))
def test_chain_reference_agrees_with_restate_bf16_products(prog, monkeypatch):
    from oracle import restate
    P, W = _oracle_weights()
    n, li = 96, 2
    rng = np.random.default_rng(21)
    pts = torch.from_numpy(rng.uniform(-1, 1, (1, n, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.uniform(-1, 1, (1, n, 3)).astype(np.float32))
    # the latent folded into the biases in fp32, as the device does; the oracle gets the folded biases and a
    # zero latent, so both sides add the same fp32 bias to the same bf16 products
    P = dict(P)
    if prog == 0:
        for layer in ('bw_linears.0', 'bw_linears.5'):
            P[layer + '.bias'] = _fold(P, layer, 'bw_latent.weight', li, 63, 191)
        P['bw_latent.weight'] = torch.zeros_like(P['bw_latent.weight'])
        names = [f'bw_linears.{l}' for l in range(8)] + ['bw_fc']
    else:
        P['tpose_human.latent_fc.bias'] = _fold(P, 'tpose_human.latent_fc', 'tpose_human.nf_latent.weight', li, 256, 384)
        P['tpose_human.nf_latent.weight'] = torch.zeros_like(P['tpose_human.nf_latent.weight'])
        names = [f'tpose_human.pts_linears.{l}' for l in range(8)] + \
                [f'tpose_human.{k}_fc' for k in ('feature', 'latent', 'view', 'rgb')]
    rec = {}
    conv = restate._conv

    def recording(Pp, name, x):
        y = conv(Pp, name, x)
        rec[name] = y.detach()[0].numpy().T.copy()     # (n, out): the layer's fp32 output before any ReLU
        return y
    monkeypatch.setattr(restate, '_conv', recording)
    with torch.no_grad(), restate.bf16_products('bf16_all'):
        if prog == 0:
            restate.neural_blend_weights(P, pts, torch.full((1, 24, n), 1 / 24.), torch.tensor([li]))
        else:
            restate.nerf_alpha_rgb(P, pts, vd, torch.tensor([li]))
    d = T.CaseData()
    d.cs = T.Case(prog, n)
    d.W = W
    d.bias = [P[nm + '.bias'].numpy() for nm in names]
    d.bias2 = P['tpose_human.alpha_fc.bias'].numpy()
    d.mem = np.full((n, 64), np.nan, np.float32)
    d.mem[:, :63] = R.rne_bf16(restate.embed(pts, 10)[0].numpy())
    d.mem2 = np.full((n, 64), np.nan, np.float32)
    d.mem2[:, :27] = R.rne_bf16(restate.embed(vd, 4)[0].numpy())
    d.bits_in = {}
    st = T.simulate(d, via_f32=True)
    total = same = 0
    for l, nm in enumerate(names):
        want = rec[nm]
        got = st[f'ref{l}'].ref[:, :want.shape[1]].astype(np.float32)
        # float64 sums of the same exact products in two orders, each rounded once to fp32
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-30).all(), (prog, l, nm)
        total += want.size
        same += int((got == want).sum())
    if prog == 1:
        want = rec['tpose_human.alpha_fc']
        got = st['ref8'].ref[:, 256:257].astype(np.float32)
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-30).all()
    assert same >= 0.999 * total, (same, total)
    # and the stored rows are the oracle's values as the next product rounds them
    h0 = R.bits_f32(st['out0'])
    assert np.array_equal(h0, R.rne_bf16(np.maximum(rec[names[0]], 0)))


# ---- the cases are not vacuous ------------------------------------------------------------------------------
CASES = [c for c in T.all_cases() if c.M > 0]
IDS = [c.name for c in T.all_cases()]


def test_case_names_unique():
    assert len(set(IDS)) == len(IDS)


def test_case_table_covers_the_issue():
    sc = T.shape_cases()
    for p in range(4):
        got = {(c.M, c.cap_eff, c.cus) for c in sc if c.prog == p}
        assert got == {(1, 1, 0), (17, 17, 0), (111, 111, 0), (112, 112, 0), (113, 113, 0), (113, 1024, 0),
                       (341, 341, 1), (341, 341, 3), (0, 224, 0)}
    assert len(T.exact_cases()) == 4


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_cases_are_not_vacuous(name):
    """On the self-fed reference: it passes its own layer checks; every ReLU layer has 25-75 % positive
    outputs; at most 10 % of the checked elements have an interval holding more than one value; an exact case
    holds at least 32 ties."""
    cs = CASES[[c.name for c in CASES].index(name)]
    d = T.case_data(cs)
    st = T.simulate(d)
    rep = T.check_layers(d, st)
    print(name, 'checked', rep.checked, 'multi-valued', rep.multi, 'ties', rep.ties,
          'relu', {k: round(v, 3) for k, v in rep.relu_pos.items()})
    if not T.bwd(cs.prog):
        assert len(rep.relu_pos) == (8 if cs.prog == 0 else 9)
    for l, f in rep.relu_pos.items():
        assert 0.25 <= f <= 0.75, (l, f)
    assert rep.checked > 0 and rep.multi <= 0.10 * rep.checked
    if cs.exact:
        assert rep.ties >= 32
    if T.bwd(cs.prog):
        for l, m in T.masks_of(d, st).items():
            assert 0.25 <= m[:, :T.out_layout(cs.prog, l)[1]].mean() <= 0.75, l


@pytest.mark.parametrize('cs', [T.Case(0, 113), T.Case(1, 17, bits='null'), T.Case(2, 113, bits='random', aux='acc'),
                                T.Case(3, 113, bits='random', aux='null'), T.Case(1, 0, cap=224)],
                         ids=lambda c: c.name)
def test_buffers_hold_the_logical_blocks(cs):
    """The allocations of a case: the self-fed result written at the defined elements comes back through
    logical(), everything else is guarded, and a changed pad element is reported."""
    d = T.case_data(cs)
    st = T.simulate(d)
    bufs, shape = T.buffers(d)
    got = {k: b.flat.copy() for k, b in bufs.items()}
    for k, (r, c) in shape.items():
        if bufs[k].idx.size:
            got[k][bufs[k].idx] = np.asarray(st[k]).reshape(-1)
    for k, b in bufs.items():
        T.untouched(k, b, got[k])
    back = T.logical(bufs, shape, got)
    for k in back:
        assert np.array_equal(back[k].view(np.uint8), np.ascontiguousarray(st[k]).view(np.uint8)), k
    if cs.M:
        st2 = dict(back, bits_in=st['bits_in'])
        T.check_layers(d, st2)
    # pad columns and rows >= M are outside the defined elements
    name = {0: 'out8', 1: 'out11', 2: 'aux', 3: 'aux'}[cs.prog]
    ld, cols = {0: (32, 24), 1: (4, 3), 2: (64, 63), 3: (64, 63)}[cs.prog]
    for elem in (cols, cs.M * ld, -1):
        bad = got[name].copy()
        bad[bufs[name].off + elem] = 1.0
        with pytest.raises(AssertionError, match='leaves alone'):
            T.untouched(name, bufs[name], bad)


# ---- the checks bite (on the CPU: a mutated self-fed result must fail) ---------------------------------------
def _trunc_bf16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize('prog', range(4))
def test_one_ulp_in_one_element_fails(prog):
    cs = T.Case(prog, 113, cus=1, bits='random' if T.bwd(prog) else 'set')
    d = T.case_data(cs)
    st = T.simulate(d)
    l = 2
    live = T.masks_of(d, st)[l] if T.PROGS[prog][l].mask else R.bits_f32(st[f'out{l}']) > 0
    r, n = np.argwhere(live)[5]
    st[f'out{l}'] = st[f'out{l}'].copy()
    st[f'out{l}'][r, n] += 1
    with pytest.raises(AssertionError, match=f'layer {l} row {r} neuron {n}'):
        T.check_layers(d, st)


@pytest.mark.parametrize('prog', range(4))
def test_truncation_fails_the_exact_case(prog):
    """A device that truncated instead of rounding to nearest even fails the exact case: in layer 0 where it
    stores bf16 rows, in layer 1 where layer 0 stores fp32 rows (program 3: the operand rounding of d view)."""
    cs = T.exact_cases()[prog]
    d = T.case_data(cs)
    st = T.simulate(d)
    lr = st['ref0']
    if T.PROGS[prog][0].out == T.F32:
        # d view is stored as fp32; the rounding under test is the operand rounding of layer 1
        v = np.where(T.masks_of(d, st)[0][:, :128], lr.ref[:, :128], 0).astype(np.float32)
        st2 = dict(st)
        st2['out0'] = v
        x = R.bits_f32(_trunc_bf16(v)).astype(np.float64)      # what a truncating tc_cvt2 would feed layer 1
        Wp = R.rne_bf16(T.layer_mats(prog, 1, d.W)[1]).astype(np.float64)
        st2['out1'] = R.bf16_bits((x @ Wp.T).astype(np.float32))
        with pytest.raises(AssertionError, match='layer 1 row'):
            T.check_layers(d, st2)
        return
    v = lr.ref[:, :256].astype(np.float32)
    if T.PROGS[prog][0].relu:
        v = np.maximum(v, 0)
    else:
        v = np.where(T.masks_of(d, st)[0], v, np.float32(0))
    st2 = dict(st)
    st2['out0'] = _trunc_bf16(v)
    with pytest.raises(AssertionError, match='layer 0 row'):
        T.check_layers(d, st2)


def test_stale_mask_row_fails():
    """A mask row taken from the neighbouring sample (a stale slot, a tile-edge slip) fails at that row."""
    cs = T.Case(2, 341, cus=1, bits='random')
    d = T.case_data(cs)
    st = T.simulate(d)
    l, r = 4, 112
    st[f'out{l}'] = st[f'out{l}'].copy()
    other = T.masks_of(d, st)[l][r + 1]
    st[f'out{l}'][r] = np.where(other, st[f'out{l}'][r] | 0x3C00, 0)
    with pytest.raises(AssertionError, match=f'layer {l} row {r} '):
        T.check_layers(d, st)


# ---- rejections of the two entries -----------------------------------------------------------------------------
def good_pack(prog):
    L = (H.TcPackLayer * 12)()
    for l, d in enumerate(T.pack_desc(prog)):
        for k in T.PACK_FIELDS:
            setattr(L[l], k, (FAKE if d[k] else None) if k in ('W', 'W2') else d[k])
    return L


PACK_REJECT = {
    'prog-4': (lambda a: a.__setitem__('prog', 4), H.E_SHAPE),
    'prog-negative': (lambda a: a.__setitem__('prog', -1), H.E_SHAPE),
    'null-layers': (lambda a: a.__setitem__('L', None), H.E_NULL),
    'null-image': (lambda a: a.__setitem__('img', None), H.E_NULL),
    'null-W-last-layer': (lambda a: setattr(a['L'][len(T.PROGS[a['prog']]) - 1], 'W', None), H.E_NULL),
    'null-W2': (lambda a: setattr(a['L'][8 if a['prog'] == 1 else (3 if a['prog'] == 3 else 0)], 'W2', None), H.E_NULL),
    'image-short': (lambda a: a.__setitem__('bytes', a['bytes'] - 1), H.E_SLAB),
    'image-unaligned': (lambda a: a.__setitem__('img', FAKE + 8), H.E_ALIGN),
}


@pytest.mark.parametrize('prog', range(4))
@pytest.mark.parametrize('name', sorted(PACK_REJECT))
def test_tchain_pack_rejections(name, prog):
    if name == 'null-W2' and prog == 0:
        prog = 2   # program 0 has no second source; the transposed bw_fc reads W2
    a = {'prog': prog, 'L': good_pack(prog), 'img': FAKE, 'bytes': T.image_bytes(prog)}
    PACK_REJECT[name][0](a)
    assert H.lib().anr_test_tchain_pack(a['prog'], a['L'], a['img'], a['bytes'], None) == PACK_REJECT[name][1]


def good_run(prog, M=128):
    g = H.TcRun()
    g.prog, g.cap, g.cus, g.M_host = prog, M, 256, M
    g.img, g.M_dev, g.bias2 = FAKE, FAKE, FAKE
    for l, L in enumerate(T.PROGS[prog]):
        g.bias[l] = FAKE
        lay = T.out_layout(prog, l)
        if lay:
            g.out[l], g.ldo[l], g.nout[l], g.out_rows[l] = FAKE, lay[0], lay[2], M
        if L.relu or L.mask:
            g.bits[l], g.bits_rows[l] = FAKE, T.bits_rows_read(M)
    g.out2, g.out2_rows = FAKE, M
    g.mem, g.ld_mem, g.kmem_cols, g.mem_rows = FAKE, T.MEM[prog][0], T.MEM[prog][1], M
    g.mem_f32 = int(T.bwd(prog))
    if prog in T.MEM2:
        g.mem2, g.ld_mem2, g.kmem2_cols, g.mem2_rows = FAKE, T.MEM2[prog][0], T.MEM2[prog][1], M
    g.aux, g.ld_aux, g.aux_cols, g.aux_rows = FAKE, T.AUX_LD, T.AUX_COLS, M
    return g


def _set(field, value):
    return lambda g: setattr(g, field, value)


def _seti(field, i, value):
    return lambda g: getattr(g, field).__setitem__(i, value)


# name -> (programs it applies to, mutation, code)
RUN_REJECT = {
    'prog-4': ((0,), _set('prog', 4), H.E_SHAPE),
    'cus-0': ((0, 1, 2, 3), _set('cus', 0), H.E_SHAPE),
    'cap-negative': ((0, 1, 2, 3), _set('cap', -1), H.E_SHAPE),
    'M-negative': ((0, 1, 2, 3), _set('M_host', -1), H.E_SHAPE),
    'null-img': ((0, 1, 2, 3), _set('img', None), H.E_NULL),
    'null-M_dev': ((0, 1, 2, 3), _set('M_dev', None), H.E_NULL),
    'null-mem': ((0, 1, 2, 3), _set('mem', None), H.E_NULL),
    'null-mem2': ((1, 3), _set('mem2', None), H.E_NULL),
    'null-bias': ((0, 1), _seti('bias', 5, None), H.E_NULL),
    'null-bias2': ((0, 1), _set('bias2', None), H.E_NULL),
    'null-out': ((0, 1, 2, 3), _seti('out', 3, None), H.E_NULL),
    'null-out-head': ((0,), _seti('out', 8, None), H.E_NULL),
    'null-out2': ((1,), _set('out2', None), H.E_NULL),
    'null-bits-masked-layer': ((2, 3), _seti('bits', 0, None), H.E_NULL),
    'kmem_cols-0': ((0, 1, 2, 3), _set('kmem_cols', 0), H.E_SHAPE),
    'kmem_cols-past-the-k-steps': ((2, 3), _set('kmem_cols', 33), H.E_SHAPE),
    'ld_mem-below-cols': ((0, 1), _set('ld_mem', 62), H.E_SHAPE),
    'ld_mem2-below-cols': ((1,), _set('ld_mem2', 26), H.E_SHAPE),
    'ldo-below-256': ((0, 1, 2, 3), _seti('ldo', 2, 248), H.E_SHAPE),
    'nout-0-forward': ((0, 1), _seti('nout', 2, 0), H.E_SHAPE),
    'nout-past-the-blocks-head': ((0,), _seti('nout', 8, 33), H.E_SHAPE),
    'ldo-below-nout-head': ((0,), _seti('ldo', 8, 20), H.E_SHAPE),
    'ld_aux-below-cols': ((2, 3), _set('ld_aux', 62), H.E_SHAPE),
    'aux_cols-65': ((2, 3), _set('aux_cols', 65), H.E_SHAPE),
    'bf16-rows-ldo-not-8': ((0, 1, 2, 3), _seti('ldo', 2, 260), H.E_ALIGN),
    'bf16-rows-base-not-16B': ((0, 1, 2, 3), _seti('out', 2, FAKE + 8), H.E_ALIGN),
    'fp32-rows-vector-store-unaligned': ((0,), _seti('out', 8, FAKE + 4), H.E_ALIGN),
    'fp32-rows-vector-store-ld-not-4': ((0,), _seti('ldo', 8, 31), H.E_ALIGN),
    'fp32-rows-not-4B': ((1,), _seti('out', 11, FAKE + 2), H.E_ALIGN),
    'mem-bf16-not-2B': ((0, 1), _set('mem', FAKE + 1), H.E_ALIGN),
    'mem-fp32-not-4B': ((2, 3), _set('mem', FAKE + 2), H.E_ALIGN),
    'img-not-16B': ((0, 1, 2, 3), _set('img', FAKE + 8), H.E_ALIGN),
    'bits-not-8B': ((0, 1, 2, 3), _seti('bits', 4, FAKE + 4), H.E_ALIGN),
    'aux-not-4B': ((2, 3), _set('aux', FAKE + 2), H.E_ALIGN),
    # the size the old TcArgs comment allowed: ceil(128 / 128) x 128 rows at M = 128 (two tiles: 240 are read)
    'bits-rows-of-the-old-comment': ((2, 3), _seti('bits_rows', 4, 128), H.E_SLAB),
    'bits-rows-one-short': ((2, 3), _seti('bits_rows', 4, 239), H.E_SLAB),
    'bits-rows-below-M-forward': ((0, 1), _seti('bits_rows', 4, 127), H.E_SLAB),
    'out-rows-below-M': ((0, 1, 2, 3), _seti('out_rows', 1, 127), H.E_SLAB),
    'out2-rows-below-M': ((1,), _set('out2_rows', 127), H.E_SLAB),
    'mem-rows-below-M': ((0, 1, 2, 3), _set('mem_rows', 127), H.E_SLAB),
    'mem2-rows-below-M': ((1, 3), _set('mem2_rows', 127), H.E_SLAB),
    'aux-rows-below-M': ((2, 3), _set('aux_rows', 127), H.E_SLAB),
}
RUN_PARAMS = [(n, p) for n in sorted(RUN_REJECT) for p in RUN_REJECT[n][0]]


@pytest.mark.parametrize('name,prog', RUN_PARAMS)
def test_tchain_run_rejections(name, prog):
    g = good_run(prog)
    RUN_REJECT[name][1](g)
    assert H.lib().anr_test_tchain_run(C.byref(g), None) == RUN_REJECT[name][2]


def test_tchain_run_good_descriptors_pass_the_checks():
    """The descriptors the rejections start from pass every check (anr_test_tchain_check: the checks of
    anr_test_tchain_run alone, no launch), also with what is optional left out: NULL bits on a forward
    program, a NULL aux on a backward one, and M = 0 with no capacity at all."""
    chk = H.lib().anr_test_tchain_check
    for prog in range(4):
        g = good_run(prog)
        assert chk(C.byref(g)) == H.OK, prog
        if T.bwd(prog):
            g.aux, g.aux_rows = None, 0
        else:
            for l in range(12):
                g.bits[l], g.bits_rows[l] = None, 0
        assert chk(C.byref(g)) == H.OK, prog
        g.M_host = 0
        for l in range(12):
            g.out_rows[l] = g.bits_rows[l] = 0
        g.mem_rows = g.mem2_rows = g.aux_rows = g.out2_rows = 0
        assert chk(C.byref(g)) == H.OK, prog
