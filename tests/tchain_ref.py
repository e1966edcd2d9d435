"""Float64 layer references, derived bounds and cases for the fused chain programs of anr_tchain.hip
(k_tchain_bw / nf / bwb / nfb), shared by test_tchain_ref.py (CPU) and test_gpu_tchain.py. Not a test file.

Why layer by layer
------------------
A whole-chain comparison cannot be tight: the fp32 summation order flips bf16 roundings and 9 to 12 layers
amplify the flips. Every program stores every layer's output, and the next layer's operand is exactly that
stored value (for fp32 rows its RNE bf16 rounding, which tc_cvt2 applies to the same fp32 number). So layer l
is checked on its own: the float64 reference takes the DEVICE's stored output of layer l - 1 and the memory
operands as the kernel sees them, the RNE-bf16 weights and the fp32 bias, and the device's stored output of
layer l must lie inside the interval of the bound below.

Bound (gemm_ref's algebra: U = 2^-24, gamma(n) = n U / (1 - n U))
-----------------------------------------------------------------
  ref = bias + sum x rne(W)                 (bf16 x bf16 products are exact in fp32)
  b   = gamma(K + 2) (sum |x| |rne(W)| + |bias|),  K = the consumed input columns of the layer
the fp32 accumulation of K exact products and the bias in any order, as the row-GEMM tests hold the same
MFMA to. A stored bf16 value must lie in [f(rne(ref - b)), f(rne(ref + b))], f = ReLU where the layer has one
(RNE and ReLU are monotone); an fp32 output obeys |out - f(ref)| <= b + U |ref|. Backward layers have no bias;
where the mask bit is 0 the stored value must be +0 exactly, where it is 1 the interval holds without ReLU.
aux = [aux0 if aux_acc] + g5 + g0: the two product bounds plus U per fp32 add on the running value. In the
exact cases layer 0's operands are 8-bit integers scaled by 2^-4 against weights in {-2..2} and biases that are
multiples of 0.5: every fp32 partial sum is exact in any order, so b = 0 and the stored value is rne(exact).

Exact equalities (no tolerance): forward mask bits == (stored value > 0), masked zeros, every element the
contract leaves alone (guards, rows >= M, pad columns), the packed image, the exact cases' layer 0.
"""
import collections
import dataclasses
import functools

import numpy as np

from . import gemm_ref as R

U, gamma = R.U, R.gamma
TR = 112                                   # rows of a tile (TC_TR)
BF16, F32, FA, SPLIT, AUX = range(5)       # output formats (TC_*)
BITS_SENTINEL = np.uint8(0xA5)
NAN16 = np.uint16(0x7FC0)

TcL = collections.namedtuple('TcL', 'ob kmem kprev mem_first relu out mem2 mask aux_add')

# the four layer tables (kProgBW, kProgNF, kProgBWB, kProgNFB)
_H = TcL(16, 0, 8, 0, 1, BF16, 0, 0, 0)            # a 256 -> 256 ReLU layer
_B = TcL(16, 0, 8, 0, 0, BF16, 0, 1, 0)            # its transposed, masked layer
PROGS = {
    0: [TcL(16, 2, 0, 1, 1, BF16, 0, 0, 0), _H, _H, _H, _H, TcL(16, 2, 8, 1, 1, BF16, 0, 0, 0), _H, _H,
        TcL(2, 0, 8, 0, 0, F32, 0, 0, 0)],
    1: [TcL(16, 2, 0, 1, 1, BF16, 0, 0, 0), _H, _H, _H, _H, TcL(16, 2, 8, 1, 1, BF16, 0, 0, 0), _H, _H,
        TcL(17, 0, 8, 0, 0, FA, 0, 0, 0), TcL(16, 0, 8, 0, 0, BF16, 0, 0, 0), TcL(8, 1, 8, 0, 1, F32, 1, 0, 0),
        TcL(1, 0, 4, 0, 0, F32, 0, 0, 0)],
    2: [TcL(16, 1, 0, 1, 0, BF16, 0, 1, 0), _B, _B, TcL(20, 0, 8, 0, 0, SPLIT, 0, 1, 0), _B, _B, _B, _B,
        TcL(4, 0, 8, 0, 0, AUX, 0, 0, 1)],
    3: [TcL(8, 1, 0, 1, 0, F32, 0, 1, 0), TcL(16, 0, 4, 0, 0, BF16, 0, 0, 0), TcL(16, 0, 8, 0, 0, BF16, 0, 0, 0),
        TcL(16, 1, 8, 0, 0, BF16, 1, 1, 0), _B, _B, TcL(20, 0, 8, 0, 0, SPLIT, 0, 1, 0), _B, _B, _B, _B,
        TcL(4, 0, 8, 0, 0, AUX, 0, 0, 1)],
}
PROG_NAMES = {0: 'k_tchain_bw', 1: 'k_tchain_nf', 2: 'k_tchain_bwb', 3: 'k_tchain_nfb'}


def bwd(prog):
    return prog >= 2


def nrows(L):
    """Neuron rows the out-blocks of a layer span (tc_nrn interleaves block pairs: an odd last block reaches
    into the second half of its pair's 32 neurons)."""
    return 32 * ((L.ob + 1) // 2)


def nslices(prog):
    return sum(L.kmem + L.kprev for L in PROGS[prog])


def image_bytes(prog):
    """One 1-KiB fragment (16 neurons x 32 inputs, bf16) per out-block of every slice."""
    return sum((L.kmem + L.kprev) * L.ob for L in PROGS[prog]) * 1024


def bits_rows_read(M):
    """Rows of 32 B a backward program's mask DMA reads: 128 from every tile's first row, tiles 112 apart."""
    return 0 if M <= 0 else ((M + TR - 1) // TR - 1) * TR + 128


# ---- weights and the executor's pack descriptors (chain_pack, chain_pack_bwd) -----------------------------
BW_IN = (191, 256, 256, 256, 256, 447, 256, 256)     # [gamma 63, latent 128 (folded) [, h4 256]]
NF_IN = (63, 256, 256, 256, 256, 319, 256, 256)      # [gamma 63 [, h4 256]]
WEIGHT_SHAPES = dict(
    [(f'bw{l}', (256, BW_IN[l])) for l in range(8)] + [('bwfc', (24, 256))] +
    [(f'nf{l}', (256, NF_IN[l])) for l in range(8)] +
    [('alpha', (1, 256)), ('feature', (256, 256)), ('latent', (256, 384)), ('view', (128, 283)), ('rgb', (3, 128))])
PROG_WEIGHTS = {0: [f'bw{l}' for l in range(8)] + ['bwfc'],
                1: [f'nf{l}' for l in range(8)] + ['alpha', 'feature', 'latent', 'view', 'rgb']}
PROG_WEIGHTS[2], PROG_WEIGHTS[3] = PROG_WEIGHTS[0], PROG_WEIGHTS[1]

PACK_FIELDS = ('W', 'in_ch', 'n1', 'W2', 'in_ch2', 'n2', 'cmem', 'kmem_cols', 'cprev', 'kprev_cols', 'oc0', 'oa',
               'oc1', 'nb', 'ob_b0')


def _pl(**kw):
    d = dict.fromkeys(PACK_FIELDS, 0)
    d['W'] = d['W2'] = None
    d.update(kw)
    return d


@functools.lru_cache(maxsize=None)
def pack_desc(prog):
    """The TcPackLayer fields the executor fills, weights by name."""
    if prog == 0:
        return [_pl(W=f'bw{l}' if l < 8 else 'bwfc', in_ch=BW_IN[l] if l < 8 else 256, n1=256 if l < 8 else 24,
                    kmem_cols=63, cprev=191 if l == 5 else 0, kprev_cols=256) for l in range(9)]
    if prog == 1:
        return [_pl(W=f'nf{l}', in_ch=NF_IN[l], n1=256, kmem_cols=63, cprev=63 if l == 5 else 0, kprev_cols=256)
                for l in range(8)] + [
            _pl(W='feature', in_ch=256, n1=256, W2='alpha', in_ch2=256, n2=1, kprev_cols=256),   # feature_fc || alpha_fc
            _pl(W='latent', in_ch=384, n1=256, kprev_cols=256),                                  # latent folded
            _pl(W='view', in_ch=283, n1=128, cmem=256, kmem_cols=27, kprev_cols=256),            # [latent, gamma(dir)]
            _pl(W='rgb', in_ch=128, n1=3, kprev_cols=128)]
    if prog == 2:
        out = [_pl(W='bwfc', in_ch=256, W2='bwfc', in_ch2=256, kmem_cols=24, oa=256)]            # bw_fc^T: d logits
        for i in range(1, 9):
            l = 8 - i
            if l == 5:
                out.append(_pl(W='bw5', in_ch=447, kprev_cols=256, oc0=191, oa=256, oc1=0, nb=63, ob_b0=256))
            else:
                out.append(_pl(W=f'bw{l}', in_ch=BW_IN[l], kprev_cols=256, oa=63 if l == 0 else 256))
        return out
    out = [_pl(W='rgb', in_ch=128, W2='rgb', in_ch2=128, kmem_cols=3, oa=128),                   # rgb_fc^T: d rgb
           _pl(W='view', in_ch=283, kprev_cols=128, oa=256),                                     # -> d latent
           _pl(W='latent', in_ch=384, kprev_cols=256, oa=256),                                   # -> d feature
           _pl(W='feature', in_ch=256, kprev_cols=256, oa=256, W2='alpha', in_ch2=256, kmem_cols=1)]
    for i in range(4, 12):
        l = 11 - i
        if l == 5:
            out.append(_pl(W='nf5', in_ch=319, kprev_cols=256, oc0=63, oa=256, oc1=0, nb=63, ob_b0=256))
        else:
            out.append(_pl(W=f'nf{l}', in_ch=NF_IN[l], kprev_cols=256, oa=63 if l == 0 else 256))
    return out


def layer_mats(prog, l, W):
    """(Wm, Wp): layer l's weights in natural order, fp32, rows = the output neurons of the layer's out-blocks
    (nrows; zero rows past the layer's outputs), columns = the memory segment's kmem_cols / the previous layer's kprev_cols inputs."""
    L, d = PROGS[prog][l], pack_desc(prog)[l]
    rows = nrows(L)
    nm, npv = (d['kmem_cols'] if L.kmem else 0), (d['kprev_cols'] if L.kprev else 0)
    if not bwd(prog):
        full = np.zeros((rows, d['in_ch']), np.float32)
        full[:d['n1']] = W[d['W']]
        if d['n2']:
            full[d['n1']:d['n1'] + d['n2']] = W[d['W2']]
        return full[:, d['cmem']:d['cmem'] + nm].copy(), full[:, d['cprev']:d['cprev'] + npv].copy()
    # transposed: output neuron m is forward input column oc0 + m (m < oa) or oc1 + m - ob_b0; k = forward output
    col = np.full(rows, -1)
    col[:d['oa']] = d['oc0'] + np.arange(d['oa'])
    col[d['ob_b0']:d['ob_b0'] + d['nb']] = d['oc1'] + np.arange(d['nb'])
    live = col >= 0
    Wm, Wp = np.zeros((rows, nm), np.float32), np.zeros((rows, npv), np.float32)
    if nm:
        Wm[live] = W[d['W2']][:nm, col[live]].T
    if npv:
        Wp[live] = W[d['W']][:npv, col[live]].T
    return Wm, Wp


# ---- the packed image --------------------------------------------------------------------------------------
def nrn(o, m):
    """tc_nrn: the output neuron of row m of out-block o."""
    return 32 * (o >> 1) + 8 * (m >> 2) + 4 * (o & 1) + (m & 3)


def _slices(L):
    """(is memory k-step, k-step index within its segment) per slice of a layer, in image / MFMA order."""
    order = [(True, s) for s in range(L.kmem)] + [(False, s) for s in range(L.kprev)]
    if not L.mem_first:
        order = order[L.kmem:] + order[:L.kmem]
    return order


def restate_image(prog, W):
    """The weight image from the layout comments: per slice [out-block][lane 64][8 bf16], lane L holding
    A[m = L & 15][k = 8 (L >> 4) + j] of neuron row tc_nrn(o, m); 0 past a layer's outputs or a segment's
    columns. uint16 bit patterns."""
    lane, j = np.arange(64), np.arange(8)
    parts = []
    for l, L in enumerate(PROGS[prog]):
        Wm, Wp = layer_mats(prog, l, W)
        for mem, s in _slices(L):
            src = Wm if mem else Wp
            pad = np.zeros((nrows(L), 32 * (L.kmem if mem else L.kprev)), np.float32)
            pad[:, :src.shape[1]] = src
            for o in range(L.ob):
                r = nrn(o, lane & 15)                                        # (64,)
                k = 32 * s + 8 * (lane >> 4)[:, None] + j[None, :]           # (64, 8)
                parts.append(R.bf16_bits(pad[r[:, None], k]).reshape(-1))
    return np.concatenate(parts)


def decode_image(prog, img):
    """Back to dense per-layer matrices: [(Dm, Dp)], rows = natural neuron, columns = natural k over the
    whole k-steps (32 kmem / 32 kprev wide), float32 values of the stored bf16."""
    lane, j = np.arange(64), np.arange(8)
    out, e = [], 0
    v = R.bits_f32(img)
    for L in PROGS[prog]:
        Dm = np.full((nrows(L), 32 * L.kmem), np.nan, np.float32)
        Dp = np.full((nrows(L), 32 * L.kprev), np.nan, np.float32)
        for mem, s in _slices(L):
            for o in range(L.ob):
                r = nrn(o, lane & 15)
                k = 32 * s + 8 * (lane >> 4)[:, None] + j[None, :]
                D = Dm if mem else Dp
                assert np.isnan(D[r[:, None], k]).all()       # no matrix element is held twice
                D[r[:, None], k] = v[e:e + 512].reshape(64, 8)
                e += 512
        # rows no out-block holds (the second half of an odd last block's pair) have no weights
        out.append((np.nan_to_num(Dm), np.nan_to_num(Dp)))
    assert e == img.size
    return out


# ---- mask bits (TcArgs::bits) ------------------------------------------------------------------------------
def _bit_pos():
    n = np.arange(256)
    s, h, jj, e = n >> 5, (n >> 3) & 3, (n >> 1) & 3, n & 1
    i = 4 * s + jj
    return h * 8 + 4 * (i >> 4) + (((i & 15) + 16 * e) >> 3), ((i & 15) + 16 * e) & 7   # byte in the row, bit in it


_BYTE, _BIT = _bit_pos()


def encode_bits(mask):
    """(rows, 256) bool -> (rows, 32) uint8: neuron 32 s + 8 h + 2 j + e is bit ((4 s + j) & 15) + 16 e of
    dword (4 s + j) >> 4 (little-endian) in the 8 bytes at row * 32 + h * 8."""
    mask = np.asarray(mask, bool)
    out = np.zeros((mask.shape[0], 32), np.uint8)
    for n in range(256):
        out[:, _BYTE[n]] |= (mask[:, n].astype(np.uint8) << _BIT[n]).astype(np.uint8)
    return out


def decode_bits(rows):
    rows = np.asarray(rows, np.uint8)
    return ((rows[:, _BYTE] >> _BIT) & 1).astype(bool)


# ---- cases ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    prog: int
    M: int
    cap: int = -1               # -1: = M
    cus: int = 0                # 0: the device's CU count
    mem_f32: int = -1           # -1: the executor's format (forward bf16 rows, backward fp32 rows)
    mem2_f32: int = 0
    bits: str = 'set'           # forward: 'set' | 'null'; backward: 'random' | 'forward' (written by program prog - 2)
    aux: str = 'store'          # backward: 'store' | 'acc' | 'null'
    exact: bool = False
    seed: int = 1

    @property
    def name(self):
        t = f'p{self.prog}-M{self.M}-cap{self.cap_eff}-cus{self.cus or "all"}'
        if self.mem_f32 >= 0:
            t += f'-memf32_{self.mem_f32}{self.mem2_f32}'
        if self.bits not in ('set', 'random'):
            t += '-bits_' + self.bits
        if bwd(self.prog) and self.aux != 'store':
            t += '-aux_' + self.aux
        return t + ('-exact' if self.exact else '')

    @property
    def cap_eff(self):
        return self.M if self.cap < 0 else self.cap

    @property
    def memf(self):
        return (1 if bwd(self.prog) else 0) if self.mem_f32 < 0 else self.mem_f32


# layouts as the executor's: (ld, columns) of the memory operands, the aux rows, per-layer (format, ld, nout)
MEM = {0: (64, 63), 1: (64, 63), 2: (32, 24), 3: (4, 3)}
MEM2 = {1: (64, 27), 3: (64, 1)}
AUX_LD, AUX_COLS = 64, 63


def out_layout(prog, l):
    """(ld, defined columns, nout argument) of out[l], or None (aux-only layer)."""
    L = PROGS[prog][l]
    if L.out == AUX:
        return None
    if L.out == F32:
        n = {(0, 8): 24, (1, 10): 128, (1, 11): 3, (3, 0): 128}[(prog, l)]
        return {24: 32, 128: 128, 3: 4}[n], n, n
    return 256, 256, 256


def gen_weights(prog, rng, exact):
    """Zero-mean uniform weights with the He scale sqrt(6 / fan_in); the exact cases' layer-0 weights are
    integers in {-2..2}."""
    W = {}
    for k in PROG_WEIGHTS[prog]:
        n, fan = WEIGHT_SHAPES[k]
        a = np.sqrt(6.0 / fan)
        W[k] = rng.uniform(-a, a, (n, fan)).astype(np.float32)
    if exact:
        for k in {0: ['bw0'], 1: ['nf0'], 2: ['bwfc'], 3: ['rgb']}[prog]:
            W[k] = rng.integers(-2, 3, W[k].shape).astype(np.float32)
    return W


class CaseData:
    pass


@functools.lru_cache(maxsize=64)
def case_data(cs):
    """Weights, biases, inputs (logical, with NaN where the contract says nothing is consumed)."""
    rng = np.random.default_rng(1000 * cs.prog + cs.seed)
    d = CaseData()
    d.cs, prog, M = cs, cs.prog, cs.M
    d.W = gen_weights(prog, rng, cs.exact)
    nl = len(PROGS[prog])
    d.bias = [None] * nl
    d.bias2 = None
    if not bwd(prog):
        for l, L in enumerate(PROGS[prog]):
            n = pack_desc(prog)[l]['n1']
            d.bias[l] = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        d.bias2 = rng.uniform(-0.1, 0.1, 1).astype(np.float32)
        if cs.exact:
            d.bias[0] = (rng.integers(-8, 9, 256) * 0.5).astype(np.float32)

    def operand(ld, cols, f32, exact):
        """Rows of ld columns, the pad columns NaN: zero-mean values in [-1, 1] (gamma rows are sin / cos
        features; gradients are zero-mean), bf16 rows already rounded, fp32 rows left for the kernel to round;
        exact: 8-bit integers scaled by 2^-4 (in [-8, 8], bf16-exact)."""
        a = np.full((M, ld), np.nan, np.float32)
        if exact:
            a[:, :cols] = rng.integers(-128, 129, (M, cols)) / 16.0
        else:
            v = rng.uniform(-1, 1, (M, cols)).astype(np.float32)
            a[:, :cols] = v if f32 else R.rne_bf16(v)
        return a
    d.mem = operand(*MEM[prog], cs.memf, cs.exact)
    d.mem2 = None
    if prog in MEM2:   # (feeds a later layer: ordinary values in the exact cases too)
        d.mem2 = operand(*MEM2[prog], cs.mem2_f32, False)
    d.aux0 = rng.uniform(-1, 1, (M, AUX_COLS)).astype(np.float32)
    d.bits_rows = max(bits_rows_read(M), 128)
    d.bits_in = {}
    if bwd(prog) and cs.bits == 'random':
        for l, L in enumerate(PROGS[prog]):
            if L.mask:
                d.bits_in[l] = rng.integers(0, 256, (d.bits_rows, 32)).astype(np.uint8)
    return d


def forward_case(cs):
    """The forward case whose mask bits a bits='forward' backward case reads."""
    return Case(cs.prog - 2, cs.M, cap=cs.cap, cus=cs.cus, seed=cs.seed)


def bits_from_forward(d, fwd_bits):
    """The backward case's mask rows from the forward program's buffers (layer -> (rows, 32) uint8, every row
    of the buffer: the DMA reads past M)."""
    return {l: fwd_bits[fl] for l, fl in handoff(d.cs.prog).items()}


def simulated_handoff_bits(d):
    """CPU stand-in of the hand-off: the self-fed forward reference's bits, the sentinel in rows >= M."""
    st = simulate(case_data(forward_case(d.cs)))
    full = {}
    for fl in handoff(d.cs.prog).values():
        a = np.full((d.bits_rows, 32), BITS_SENTINEL, np.uint8)
        a[:d.cs.M] = st[f'bits{fl}']
        full[fl] = a
    return bits_from_forward(d, full)


def seen(a, cols):
    """A memory operand as the kernel sees it: columns < cols, rounded RNE to bf16, float64."""
    return R.rne_bf16(a[:, :cols]).astype(np.float64)


# ---- the per-layer reference --------------------------------------------------------------------------------
def prev_operand(prog, l, stored):
    """The previous layer's stored output as the next operand: bf16 rows as stored, fp32 rows rounded RNE."""
    P = PROGS[prog][l - 1]
    v = stored[f'out{l - 1}']
    if P.out == F32:
        return R.rne_bf16(v).astype(np.float64)
    return R.bits_f32(v).astype(np.float64)


LayerRef = collections.namedtuple('LayerRef', 'ref bnd')


def layer_ref(d, l, stored):
    """ref and bound of all nrows(L) output neurons of layer l (rows x neurons) from the stored output of layer
    l - 1 and the memory operands."""
    cs, prog = d.cs, d.cs.prog
    L, pd = PROGS[prog][l], pack_desc(prog)[l]
    Wm, Wp = layer_mats(prog, l, d.W)
    Wm, Wp = R.rne_bf16(Wm).astype(np.float64), R.rne_bf16(Wp).astype(np.float64)
    n = nrows(L)
    ref = np.zeros((cs.M, n))
    S = np.zeros((cs.M, n))
    K = 0
    if not bwd(prog):
        b = np.zeros(n)
        b[:d.bias[l].size] = d.bias[l]
        if L.out == FA:
            b[256] = d.bias2[0]
        ref += b[None, :]
        S += np.abs(b)[None, :]
    if L.kmem:
        x = seen(d.mem2 if L.mem2 else d.mem, pd['kmem_cols'])
        ref += x @ Wm.T
        S += np.abs(x) @ np.abs(Wm).T
        K += pd['kmem_cols']
    if L.kprev:
        x = prev_operand(prog, l, stored)[:, :pd['kprev_cols']]
        ref += x @ Wp.T
        S += np.abs(x) @ np.abs(Wp).T
        K += pd['kprev_cols']
    bnd = gamma(K + 2) * S
    if cs.exact and l == 0:
        bnd = np.zeros_like(S)
    return LayerRef(ref, bnd)


def bf16_interval(ref, bnd, relu):
    lo, hi = R.rne_bf16_f64(ref - bnd), R.rne_bf16_f64(ref + bnd)
    if relu:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    return lo, hi


def is_tie(v):
    """v lies exactly midway between two neighbouring bf16 values."""
    m, _ = np.frexp(np.asarray(v, np.float64))
    t = np.abs(m) * 256.0
    return (t - np.floor(t)) == 0.5


def masks_of(d, stored):
    """Per masked layer: (rows, 256) bool from the bits the backward program reads."""
    return {l: decode_bits(b[:d.cs.M]) for l, b in stored['bits_in'].items()}


def aux_ref(d, g5, g0):
    """aux rows: reference and bound from the two products (LayerRef slices, rows x 63)."""
    acc = d.cs.aux == 'acc'
    r1 = (d.aux0.astype(np.float64) if acc else 0.0) + g5.ref
    r2 = r1 + g0.ref
    e1 = g5.bnd + (U * (np.abs(r1) + g5.bnd) if acc else 0.0)
    e2 = e1 + g0.bnd
    return r2, e2 + U * (np.abs(r2) + e2)


def simulate(d, via_f32=False):
    """The self-fed reference: every stored buffer as a device that computes each layer exactly would leave
    it (float64 sums, one RNE rounding; via_f32: rounded to fp32 first, as the oracle's fp32 tensors are)."""
    cs, prog, M = d.cs, d.cs.prog, d.cs.M
    st = {'bits_in': simulated_handoff_bits(d) if (bwd(prog) and cs.bits == 'forward') else dict(d.bits_in)}
    masks = masks_of(d, st) if bwd(prog) else {}
    g5 = None
    for l, L in enumerate(PROGS[prog]):
        lr = layer_ref(d, l, st)
        v = lr.ref.astype(np.float32).astype(np.float64) if via_f32 else lr.ref
        if L.relu:
            v = np.maximum(v, 0.0) + 0.0
        if L.out in (BF16, FA, SPLIT):
            h = R.rne_bf16_f64(v[:, :256])
            if L.mask:
                h = np.where(masks[l], h, 0.0)
            st[f'out{l}'] = R.bf16_bits(h.astype(np.float32)).reshape(M, 256)
            if L.out == FA:
                st['alpha'] = v[:, 256].astype(np.float32)
            if L.relu and cs.bits == 'set':
                st[f'bits{l}'] = encode_bits(h > 0)
        elif L.out == F32:
            _, cols, _ = out_layout(prog, l)
            o = v[:, :16 * L.ob].astype(np.float32)
            if L.mask:
                o = np.where(masks[l][:, :o.shape[1]], o, np.float32(0))
            st[f'out{l}'] = o[:, :cols] if cols < o.shape[1] else o
            if L.relu and cs.bits == 'set':
                m = np.zeros((M, 256), bool)
                m[:, :o.shape[1]] = o > 0
                st[f'bits{l}'] = encode_bits(m)
        if L.out == SPLIT:
            g5 = LayerRef(lr.ref[:, 256:256 + AUX_COLS], lr.bnd[:, 256:256 + AUX_COLS])
        if L.out == AUX and cs.aux != 'null':
            g0 = LayerRef(lr.ref[:, :AUX_COLS], lr.bnd[:, :AUX_COLS])
            st['aux'] = aux_ref(d, g5, g0)[0].astype(np.float32)
        st[f'ref{l}'] = lr
    return st


class Report:
    def __init__(self):
        self.checked = self.multi = self.ties = 0
        self.relu_pos = {}


def check_layers(d, st):
    """Every stored layer output of `st` (logical arrays, as simulate() names them) against its own reference
    from the stored output of the layer before. Raises AssertionError naming program, layer, row, neuron."""
    cs, prog, M = d.cs, d.cs.prog, d.cs.M
    who = PROG_NAMES[prog]
    rep = Report()
    if M == 0:
        return rep
    masks = masks_of(d, st) if bwd(prog) else {}
    g5 = None

    def fail(l, bad, msg, got, lo, hi):
        r, n = np.argwhere(bad)[0]
        raise AssertionError(f'{who} [{cs.name}] layer {l} row {r} neuron {n}: {msg}: stored {got[r, n]!r}, allowed '
                             f'[{lo[r, n]!r}, {hi[r, n]!r}] ({int(bad.sum())} elements of the layer)')

    for l, L in enumerate(PROGS[prog]):
        lr = layer_ref(d, l, st)
        if not np.isfinite(lr.ref).all():
            r, n = np.argwhere(~np.isfinite(lr.ref))[0]
            raise AssertionError(f'{who} [{cs.name}] layer {l}: the stored input of row {r} is not finite '
                                 f'(reference of neuron {n})')
        if L.out in (BF16, FA, SPLIT):
            got = R.bits_f32(st[f'out{l}']).astype(np.float64)
            lo, hi = bf16_interval(lr.ref[:, :256], lr.bnd[:, :256], L.relu)
            live = np.ones_like(got, bool)
            if L.mask:
                live = masks[l]
                z = ~live & (st[f'out{l}'] != 0)
                if z.any():
                    fail(l, z, 'mask bit 0 but not +0', got, np.zeros_like(got), np.zeros_like(got))
            bad = live & ~((got >= lo) & (got <= hi))     # NaN compares false
            if bad.any():
                fail(l, bad, 'outside [rne(ref - b), rne(ref + b)]', got, lo, hi)
            rep.checked += got.size
            rep.multi += int((live & (lo != hi)).sum())
            if cs.exact and l == 0:
                rep.ties += int((live & is_tie(lr.ref[:, :256]) & (~np.bool_(L.relu) | (lr.ref[:, :256] > 0))).sum())
            if L.relu:
                rep.relu_pos[l] = float((got > 0).mean())
            if L.out == FA:
                a, ra, ba = st['alpha'].astype(np.float64), lr.ref[:, 256], lr.bnd[:, 256]
                bad = ~(np.abs(a - ra) <= ba + U * np.abs(ra))
                if bad.any():
                    fail(l, bad[:, None], 'alpha outside the bound', a[:, None], (ra - ba)[:, None], (ra + ba)[:, None])
                rep.checked += a.size
        elif L.out == F32:
            got = st[f'out{l}'].astype(np.float64)
            n = got.shape[1]
            ref, bnd = lr.ref[:, :n], lr.bnd[:, :n]
            if L.relu:
                ref = np.maximum(ref, 0.0)
            tol = bnd + (0.0 if (cs.exact and l == 0) else U * np.abs(ref))
            live = np.ones_like(got, bool)
            if L.mask:
                live = masks[l][:, :n]
                z = ~live & (st[f'out{l}'].view(np.uint32) != 0)
                if z.any():
                    fail(l, z, 'mask bit 0 but not +0', got, np.zeros_like(got), np.zeros_like(got))
            bad = live & ~(np.abs(got - ref) <= tol)
            if bad.any():
                fail(l, bad, 'fp32 output outside the bound', got, ref - tol, ref + tol)
            rep.checked += got.size
            if cs.exact and l == 0:
                rep.ties += int((live & is_tie(lr.ref[:, :n])).sum())
            if L.relu:
                rep.relu_pos[l] = float((got > 0).mean())
        if L.out == SPLIT:
            g5 = LayerRef(lr.ref[:, 256:256 + AUX_COLS], lr.bnd[:, 256:256 + AUX_COLS])
        if L.out == AUX and cs.aux != 'null':
            ref, tol = aux_ref(d, g5, LayerRef(lr.ref[:, :AUX_COLS], lr.bnd[:, :AUX_COLS]))
            got = st['aux'].astype(np.float64)
            bad = ~(np.abs(got - ref) <= tol)
            if bad.any():
                fail(l, bad, 'aux outside the bound', got, ref - tol, ref + tol)
            rep.checked += got.size
        # forward mask bits: (stored value > 0), bit for bit
        if not bwd(prog) and L.relu and cs.bits == 'set':
            val = R.bits_f32(st[f'out{l}']) if L.out != F32 else st[f'out{l}']
            m = np.zeros((M, 256), bool)
            m[:, :val.shape[1]] = val > 0
            want = encode_bits(m)
            if not np.array_equal(want, st[f'bits{l}']):
                diff = decode_bits(want) != decode_bits(st[f'bits{l}'])
                r, n = np.argwhere(diff)[0] if diff.any() else (np.argwhere(want != st[f'bits{l}'])[0][0], -1)
                raise AssertionError(f'{who} [{cs.name}] layer {l} row {r} neuron {n}: mask bit differs from '
                                     f'(stored value > 0)')
    return rep


# ---- buffers -----------------------------------------------------------------------------------------------
def _rows_alloc(M):
    return M + 3


def buffers(d):
    """gemm_ref.Buf allocations of a case: NaN-guarded inputs, sentinel-filled outputs whose defined elements
    start as NaN. Returns (bufs, shape) with shape[name] = (rows, cols) of the defined block."""
    cs, prog, M = d.cs, d.cs.prog, d.cs.M
    bufs, shape = {}, {}
    ra = _rows_alloc(M)

    def inp(name, a, f32):
        ld = a.shape[1]
        if f32:
            bufs[name] = R.in_buf(a, ld, 1, True, np.float32, extent=ra * ld)
        else:
            bits = np.where(np.isnan(a), NAN16, R.bf16_bits(np.nan_to_num(a))).astype(np.uint16)
            bufs[name] = R.in_buf(bits, ld, 1, True, np.uint16, fill=NAN16, extent=ra * ld)
    inp('mem', d.mem, cs.memf)
    if d.mem2 is not None:
        inp('mem2', d.mem2, cs.mem2_f32)

    def outp(name, ld, cols, dtype, init=None):
        defined = np.zeros((ra, ld), bool)
        defined[:M, :cols] = True
        z = np.zeros((ra, ld))
        full = None
        if init is not None:
            full = np.full((ra, ld), R.SENTINEL, np.float32)
            full[:M, :cols] = init
        bufs[name] = R.out_buf(ra, ld, ld, 1, True, defined, z, z, init=full, dtype=dtype)
        shape[name] = (M, cols)
    for l, L in enumerate(PROGS[prog]):
        lay = out_layout(prog, l)
        if lay:
            outp(f'out{l}', lay[0], lay[1], np.float32 if L.out == F32 else np.uint16)
        if not bwd(prog) and L.relu:     # forward mask bits: written for rows < M (when passed)
            flat = np.full(R.GUARD + d.bits_rows * 32 + R.GUARD, BITS_SENTINEL, np.uint8)
            idx = R.GUARD + np.arange(M * 32, dtype=np.int64)
            bufs[f'bits{l}'] = R.Buf(flat, R.GUARD, idx if cs.bits == 'set' else idx[:0], out=True)
            shape[f'bits{l}'] = (M, 32)
        if bwd(prog) and L.mask and cs.bits == 'random':
            flat = np.full(R.GUARD + d.bits_rows * 32 + R.GUARD, BITS_SENTINEL, np.uint8)
            flat[R.GUARD:R.GUARD + d.bits_rows * 32] = d.bits_in[l].reshape(-1)
            bufs[f'bits{l}'] = R.Buf(flat, R.GUARD)
    if prog == 1:
        outp('alpha', 1, 1, np.float32)
    if bwd(prog):
        outp('aux', AUX_LD, AUX_COLS, np.float32, init=d.aux0)
        if cs.aux == 'null':
            bufs['aux'].idx = bufs['aux'].idx[:0]
    return bufs, shape


def untouched(name, buf, got_flat, who=''):
    """Everything outside the defined elements is bit-identical to what was uploaded."""
    keep = np.ones(buf.flat.size, bool)
    keep[buf.idx] = False
    a = np.asarray(got_flat)[keep].view(np.uint8)
    b = buf.flat[keep].view(np.uint8)
    if not np.array_equal(a, b):
        k = int(np.flatnonzero(keep)[np.flatnonzero(a != b)[0] // buf.flat.dtype.itemsize]) - buf.off
        raise AssertionError(f'{who}{name}: an element the contract leaves alone changed (first at element {k} '
                             f'from the base: guard bands, rows >= M and pad columns must keep their content)')


def logical(bufs, shape, got):
    """The defined blocks of the downloaded allocations, under simulate()'s names."""
    st = {}
    for name, (r, c) in shape.items():
        b = bufs[name]
        if b.idx.size:
            a = np.asarray(got[name])[b.idx].reshape(r, c)
            st[name] = a[:, 0] if name == 'alpha' else a
    return st


# mask-bit hand-off of the executor: backward layer -> the forward layer whose bits it reads
def handoff(prog):
    if prog == 2:
        return {i: 7 - i for i in range(8)}
    return {0: 10, **{i: 10 - i for i in range(3, 11)}}


# ---- the case lists ------------------------------------------------------------------------------------------
def shape_cases():
    out = []
    for p in range(4):
        kw = dict(bits='random') if bwd(p) else {}
        for M in (1, 17, 111, 112, 113):
            out.append(Case(p, M, **kw))
        out += [Case(p, 113, cap=1024, **kw), Case(p, 341, cus=1, **kw), Case(p, 341, cus=3, **kw),
                Case(p, 0, cap=224, **kw)]
    return out


def variant_cases():
    out = []
    for M in (113, 341):
        for f in (0, 1):
            out.append(Case(0, M, cus=1, mem_f32=f, seed=2))
            for f2 in (0, 1):
                out.append(Case(1, M, cus=1, mem_f32=f, mem2_f32=f2, seed=2))
        for p in (0, 1):
            out.append(Case(p, M, cus=1, bits='null', seed=3))
        for p in (2, 3):
            out += [Case(p, M, cus=1, bits='random', aux='acc', seed=2), Case(p, M, cus=1, bits='random', aux='null', seed=2),
                    Case(p, M, cus=1, bits='forward', seed=4)]
    return out


def exact_cases():
    return [Case(p, 113, cus=1, exact=True, bits='random' if bwd(p) else 'set', seed=5) for p in range(4)]


def all_cases():
    return shape_cases() + variant_cases() + exact_cases()
