"""GPU: the four fused chain programs of anr_tchain.hip (k_tchain_bw / nf / bwb / nfb) layer by layer against
the float64 reference and derived bounds of tests/tchain_ref.py, through the test entry library.

Every case packs the weight image (compared bit for bit with the restated image, guards intact: a pack error
is told from a chain error), runs the program once, copies everything back and checks each layer's stored
output against a reference computed from the DEVICE's stored output of the layer before (tchain_ref's
docstring: bounds, exact equalities). Every guard band and every element the contract leaves alone (rows >= M
of the outputs and the mask bits, logit columns 24..31, rgb column 3, aux column 63, alpha past M) must come
back bit-identical. Inputs carry NaN wherever the contract says nothing is consumed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _tchain_hooks as H
from . import gemm_ref as R
from . import tchain_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU test run without a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


_IMAGES = {}


def expected_image(d):
    """The restated image of the case's weights (they depend on program, seed and exactness only)."""
    key = (d.cs.prog, d.cs.seed, d.cs.exact)
    if key not in _IMAGES:
        _IMAGES[key] = T.restate_image(d.cs.prog, d.W)
    return _IMAGES[key]


def pack(d, dev):
    """tchain_pack of the case's weights; the image on the device, checked against the restated image."""
    prog = d.cs.prog
    Wd = {k: torch.from_numpy(v).to(dev) for k, v in d.W.items()}
    L = (H.TcPackLayer * 12)()
    for l, pd in enumerate(T.pack_desc(prog)):
        for k in T.PACK_FIELDS:
            setattr(L[l], k, (Wd[pd[k]].data_ptr() if pd[k] else None) if k in ('W', 'W2') else pd[k])
    n = T.image_bytes(prog) // 2
    flat = np.full(R.GUARD + n + R.GUARD, R.SENTINEL16, np.uint16)
    img = torch.from_numpy(flat.view(np.int16).copy()).to(dev)
    ptr = img.data_ptr() + 2 * R.GUARD
    assert H.lib().anr_test_tchain_pack(prog, L, ptr, 2 * n, H.stream_ptr()) == H.OK
    torch.cuda.synchronize()
    got = img.cpu().numpy().view(np.uint16)
    who = f'{T.PROG_NAMES[prog]} [{d.cs.name}] image'
    assert (got[:R.GUARD] == R.SENTINEL16).all() and (got[-R.GUARD:] == R.SENTINEL16).all(), f'{who}: guards changed'
    want = expected_image(d)
    bad = np.flatnonzero(got[R.GUARD:-R.GUARD] != want)
    assert bad.size == 0, f'{who}: {bad.size} elements differ from the restated image, first at element {bad[0]} ' \
                          f'(fragment {bad[0] // 512}, lane {bad[0] // 8 % 64}, j {bad[0] % 8})'
    return img, ptr, Wd


class Run:
    pass


def run_case(cs, dev, ncus, fwd=None):
    """One launch of the case; fwd: the forward Run whose device mask bits a bits='forward' case reads."""
    d = T.case_data(cs)
    prog, M = cs.prog, cs.M
    bufs, shape = T.buffers(d)
    for l, b in enumerate(d.bias):
        if b is not None:
            bufs[f'bias{l}'] = R.in_buf(b[None, :], b.size, 1, True)
    if d.bias2 is not None:
        bufs['bias_alpha'] = R.in_buf(d.bias2[None, :], 1, 1, True)   # ('bias2' is layer 2's)
    db = H.DevBufs(bufs, dev)
    r = Run()
    r.d, r.bufs, r.shape, r.db = d, bufs, shape, db
    r.img, img_ptr, r.Wd = pack(d, dev)
    r.M_dev = H.dev_int(M, dev)
    g = H.TcRun()
    g.prog, g.cap, g.cus, g.M_host = prog, cs.cap_eff, cs.cus or ncus, M
    g.img, g.M_dev = img_ptr, r.M_dev.data_ptr()
    ra = M + 3
    for l, L in enumerate(T.PROGS[prog]):
        g.bias[l] = db.ptr(f'bias{l}')
        lay = T.out_layout(prog, l)
        if lay:
            g.out[l], g.ldo[l], g.nout[l], g.out_rows[l] = db.ptr(f'out{l}'), lay[0], lay[2], ra
        if not T.bwd(prog) and L.relu and cs.bits == 'set':
            g.bits[l], g.bits_rows[l] = db.ptr(f'bits{l}'), d.bits_rows
        if T.bwd(prog) and L.mask:
            if cs.bits == 'forward':
                g.bits[l] = fwd.db.ptr(f'bits{T.handoff(prog)[l]}')
            else:
                g.bits[l] = db.ptr(f'bits{l}')
            g.bits_rows[l] = d.bits_rows
    g.bias2 = db.ptr('bias_alpha')
    if prog == 1:
        g.out2, g.out2_rows = db.ptr('alpha'), ra
    g.mem, g.ld_mem, g.kmem_cols, g.mem_rows, g.mem_f32 = db.ptr('mem'), T.MEM[prog][0], T.MEM[prog][1], ra, cs.memf
    if prog in T.MEM2:
        g.mem2, g.ld_mem2, g.kmem2_cols, g.mem2_rows = db.ptr('mem2'), T.MEM2[prog][0], T.MEM2[prog][1], ra
        g.mem2_f32 = cs.mem2_f32
    if T.bwd(prog):
        g.ld_aux, g.aux_cols, g.aux_acc, g.aux_rows = T.AUX_LD, T.AUX_COLS, int(cs.aux == 'acc'), ra
        g.aux = db.ptr('aux') if cs.aux != 'null' else None
    assert H.lib().anr_test_tchain_run(C.byref(g), H.stream_ptr()) == H.OK, cs.name
    torch.cuda.synchronize()
    r.got = {k: db.get(k) for k in bufs}
    return r


def check_case(r, fwd=None):
    d, cs = r.d, r.d.cs
    who = f'{T.PROG_NAMES[cs.prog]} [{cs.name}] '
    for k, b in r.bufs.items():
        T.untouched(k, b, r.got[k], who)       # inputs whole, outputs outside their defined elements
    st = T.logical(r.bufs, r.shape, r.got)
    if T.bwd(cs.prog):
        if cs.bits == 'forward':
            full = {fl: fwd.got[f'bits{fl}'][R.GUARD:R.GUARD + d.bits_rows * 32].reshape(d.bits_rows, 32)
                    for fl in T.handoff(cs.prog).values()}
            st['bits_in'] = T.bits_from_forward(d, full)
        else:
            st['bits_in'] = d.bits_in
    rep = T.check_layers(d, st)
    print(cs.name, 'checked', rep.checked, 'multi-valued', rep.multi, 'ties', rep.ties)
    return rep


ALL = T.all_cases()
IDS = [c.name for c in ALL]


@pytest.mark.parametrize('name', IDS)
def test_tchain(dev, cus, name):
    cs = ALL[IDS.index(name)]
    fwd = None
    if cs.bits == 'forward':   # the executor's hand-off: the forward program writes the bits this one reads
        fwd = run_case(T.forward_case(cs), dev, cus)
        check_case(fwd)
    r = run_case(cs, dev, cus, fwd)
    rep = check_case(r, fwd)
    if fwd is not None:        # the backward program only reads them
        for k in fwd.bufs:
            assert fwd.db.get(k).tobytes() == fwd.got[k].tobytes(), (cs.name, k)
    if cs.M == 0:
        assert rep.checked == 0
    if cs.exact:
        assert rep.ties >= 32


@pytest.mark.parametrize('prog', range(4))
@pytest.mark.parametrize('one_cu', (True, False))
def test_tchain_repeatable(dev, cus, prog, one_cu):
    """No atomics: two runs of one case into freshly filled buffers are byte-identical."""
    cs = T.Case(prog, 341, cus=1 if one_cu else 0, bits='random' if T.bwd(prog) else 'set', seed=6)
    a = run_case(cs, dev, cus)
    b = run_case(cs, dev, cus)
    check_case(a)
    for k in a.bufs:
        assert a.got[k].tobytes() == b.got[k].tobytes(), f'{T.PROG_NAMES[prog]} [{cs.name}] {k}: two runs differ'
    assert a.img.cpu().numpy().tobytes() == b.img.cpu().numpy().tobytes()
