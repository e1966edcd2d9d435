"""Float64 references and derived error bounds for the training GEMM engines (anr_gemm.hip, anr_tgemm.hip,
anr_lgemm.hip), shared by test_gemm_ref.py (CPU) and the test_gpu_{gemm,rgemm,wgrad,lgemm}.py files. Not a
test file.

Reference
---------
The product is computed in float64 from the operands the kernel sees by contract, with the descriptor's own
strides, segments and device counts:
  * fp32 kernels: the stored fp32 values;
  * bf16 kernels: every fp32 operand rounded to bf16, round-to-nearest-even (anr_gemm.hip f2bf, anr_tgemm.hip
    f2bf_rne / the compiler's (__bf16) conversion: all RNE); operands stored as bf16 are used as stored;
  * split-bf16 (x3): hi = rne_bf16(x), lo = rne_bf16(x - hi) (x - hi is exact in fp32); the kernel adds
    hi*hi + lo*hi + hi*lo. The reference is the product of the UNSPLIT fp32 operands, and the split's
    residual and the dropped lo*lo term go into the bound, so "fp32-level" is what is asserted.
Then the epilogue in float64 in the kernel's order: bias, accumulate, div_pre, relu, softplus (+ deriv),
spd, mask, div_post (anr_gemm.hip epilogue / epilogue_sw). Atomic (split-K) launches add bias once and the
partials into the pre-existing C and apply nothing else.

Bound
-----
u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u). With S = |A| |B| in float64 (the operands as
the kernel sees them), componentwise:
  * fp32 accumulation of K_total exact-or-fp32 products in any order: |fl(sum) - sum| <= gamma(K_total) S
    (Higham, Accuracy and Stability, 3.1; an fp32 product costs one more rounding, inside gamma(K + 1) —
    gamma(K_total + 1) is what is used). bf16 x bf16 products are exact in fp32.
  * x3: bf16 keeps 8 significant bits, unit roundoff 2^-8. x = hi + lo + r, |x - hi| <= 2^-8 |x|,
    |r| <= 2^-8 |x - hi| <= 2^-16 |x| (the "~2^-16 relative" of anr_gemm.hip's store_tile16). a b -
    (ah bh + al bh + ah bl) = al bl + ra b + a rb - ra rb, in magnitude <= 3 2^-16 (1 + 2^-8) |a b| per
    product (X3_TERM); the three partial products are accumulated in fp32: gamma(3 K_total) (|ah bh| +
    |al bh| + |ah bl|) <= gamma(3 K_total) (1 + 2^-5) S (X3_ACC; (1 + 2^-8)^2 + 2^-7 (1 + 2^-8) < 1 + 2^-5).
  * every fp32 operation of the epilogue adds one rounding of its result, u |result|, to the bound carried
    so far; a division by a constant d scales the carried bound by 1 / |d|; relu, the mask and softplus
    (Lipschitz 1) carry it unchanged.
  * spd factors: f = d / (d + 1) is computed as d * rcp(d + 1): two roundings and a 1-ulp reciprocal, then
    v * f: 5 u relative; f = 1 - exp2(-144.27 h s): the argument carries 3 roundings (h s, the constant, the
    product), exp2 is a 1-ulp instruction, x exp(-x) <= 0.368, so |df| <= (0.368 * 3 + 2 + 1) u <= 4.2 u,
    plus the final product. Both are covered by b f + 6 u |v| (f <= 1).
  * atomic split-K / slab reductions: the partials, the bias and the pre-existing C are added in an
    arbitrary order: gamma(K_total + nsplit + 2) (S + |bias| + |C0|).
  * row sums / column sums: gamma(K_total + nparts + 2) (sum |a| + |r0|).
  * bf16 outputs (row GEMM cbf): no tolerance of their own; the stored value must lie in
    [rne_bf16(ref - b), rne_bf16(ref + b)] (RNE is monotone).

Softplus
--------
The kernel's fast_exp / fast_log1p compose a handful of 1-ulp hardware transcendentals where torch's are
correctly rounded to within its own library's error; the code does not state their error. The bound adds
16 x the error of torch's own fp32 softplus(beta=100, threshold=20) against float64 on the same
pre-activations (softplus_ref_error), measured on the CPU per case. Over the 18 softplus cases of REF_CASES
the measured error is at most 1.602e-8 absolute (test_gemm_ref.py::test_softplus_reference_error prints
and bounds it), so the kernel is allowed 2.6e-7 on top of the propagated product bound. deriv = exp(100 v)
is relative: 16 x the relative error of torch's fp32 exp(100 v) (measured <= 1.963e-6, dominated by the
rounding of 100 v at |100 v| <= 50) plus 100 b_pre for the pre-activation's own bound. deriv jumps to -1 at 100 v = 20: the inputs
are generated so that no pre-activation lies within its bound of the threshold (gemm_data redraws one
element of every row that holds one; asserted on the CPU and before every GPU launch, zero elements).
"""
import dataclasses
import functools

import numpy as np

U = 2.0 ** -24
X3_TERM = 3.0 * 2.0 ** -16 * (1.0 + 2.0 ** -8)
X3_ACC = 1.0 + 2.0 ** -5
SENTINEL = np.float32(-1234.5677)       # output guards and unused output elements (fp32)
SENTINEL16 = np.uint16(0xC49A)          # the same for bf16 outputs (-1232.0)
GUARD = 64                              # guard band, elements, before and after every buffer
SOFTPLUS_MARGIN = 16.0


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- bf16 --------------------------------------------------------------------------------------------
def bf16_bits(x):
    """RNE fp32 -> bf16 bit patterns (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def bits_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rne_bf16(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32."""
    x = np.asarray(x, np.float32)
    return bits_f32(bf16_bits(x)).reshape(x.shape)


def split_bf16(x):
    x = np.asarray(x, np.float32)
    hi = rne_bf16(x)
    lo = rne_bf16(x - hi)
    return hi, lo


def rne_bf16_f64(x):
    """float64 -> nearest bf16 (ties to even) as float64: through fp32 is not double-rounding-safe, so round
    the float64 directly on the bf16 grid."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                   # x = m 2^e, 0.5 <= |m| < 1; bf16 keeps 8 significant bits
    return np.ldexp(np.rint(m * 256.0), e - 8)   # np.rint: half to even


# ---- buffers -----------------------------------------------------------------------------------------
class Buf:
    """One operand or output inside a larger allocation with guard bands.

    flat: the whole allocation as first uploaded (guards included); off: element offset of the pointer the
    kernel gets; idx: flat indices of the logical elements (inputs: where the data went; outputs: the
    elements the kernel must define), exp / bnd: float64 expectation and bound at idx (outputs)."""

    def __init__(self, flat, off, idx=None, exp=None, bnd=None, out=False):
        self.flat, self.off, self.idx, self.exp, self.bnd, self.out = flat, off, idx, exp, bnd, out


def _alloc(span, fill, aligned, dtype=np.float32, skew=1):
    """(flat, off): span elements after the base; the base 16-B aligned, or skew elements past alignment."""
    off = GUARD + (0 if aligned else skew)
    flat = np.full(off + span + GUARD, fill, dtype)
    return flat, off


def _grid(off, rows, cols, rs, cs):
    return off + np.arange(rows, dtype=np.int64)[:, None] * rs + np.arange(cols, dtype=np.int64)[None, :] * cs


def in_buf(logical, rs, cs, aligned, dtype=np.float32, fill=np.nan, extent=None, skew=1):
    """An input: `logical` (rows x cols; NaN where the contract says the kernel consumes nothing) placed
    at strides (rs, cs); everything else in the allocation, guards included, holds `fill` (NaN)."""
    rows, cols = logical.shape
    span = (rows - 1) * rs + (cols - 1) * cs + 1 if rows and cols else 1
    if extent:
        span = max(span, extent)
    flat, off = _alloc(span, fill, aligned, dtype, skew)
    idx = _grid(off, rows, cols, rs, cs)
    flat[idx] = logical
    return Buf(flat, off, idx)


def out_buf(rows, cols, rs, cs, aligned, defined, exp, bnd, init=None, dtype=np.float32, skew=1):
    """An output of rows x cols at strides (rs, cs). `defined` (bool, rows x cols): the elements the kernel
    must write. init (rows x cols or None): pre-existing content where it matters (accumulation targets);
    otherwise defined elements start as NaN (an element nobody wrote shows) and everything else, guards
    included, is the sentinel and must come back bit-identical."""
    span = (rows - 1) * rs + (cols - 1) * cs + 1 if rows and cols else 1
    sent = SENTINEL if dtype == np.float32 else SENTINEL16
    flat, off = _alloc(span, sent, aligned, dtype, skew)
    g = _grid(off, rows, cols, rs, cs)
    if init is not None:
        flat[g] = init
    elif dtype == np.float32:
        flat[g[defined]] = np.nan
    else:
        flat[g[defined]] = 0x7FC0  # bf16 NaN
    return Buf(flat, off, g[defined], np.asarray(exp, np.float64)[defined], np.asarray(bnd, np.float64)[defined], out=True)


def check_out(name, buf, got_flat):
    """The output allocation after the call: untouched outside the defined elements (bit-identical), finite
    and inside the bound on them. Returns (worst error / bound, worst error) for reporting."""
    got_flat = np.asarray(got_flat)
    keep = np.ones(buf.flat.size, bool)
    keep[buf.idx] = False
    a, b = got_flat[keep], buf.flat[keep]
    same = a.view(np.uint32 if a.dtype == np.float32 else np.uint16) == b.view(np.uint32 if b.dtype == np.float32 else np.uint16)
    assert same.all(), f'{name}: {int((~same).sum())} elements outside the defined output changed ' \
                       f'(first at flat index {int(np.flatnonzero(keep)[np.flatnonzero(~same)[0]]) - buf.off} from the base)'
    if buf.idx.size == 0:
        return 0.0, 0.0
    if got_flat.dtype == np.uint16:
        v = bits_f32(got_flat[buf.idx]).astype(np.float64)
        assert np.isfinite(v).all(), f'{name}: non-finite bf16 output'
        lo, hi = rne_bf16_f64(buf.exp - buf.bnd), rne_bf16_f64(buf.exp + buf.bnd)
        ok = (v >= lo) & (v <= hi)
        assert ok.all(), f'{name}: {int((~ok).sum())} bf16 outputs outside [rne(ref - b), rne(ref + b)]; first ' \
                         f'{v[~ok][0]!r} vs [{lo[~ok][0]!r}, {hi[~ok][0]!r}]'
        return 0.0, float(np.abs(v - buf.exp).max())
    v = got_flat[buf.idx].astype(np.float64)
    fin = np.isfinite(v)
    assert fin.all(), f'{name}: {int((~fin).sum())} of {v.size} defined outputs are not finite'
    err = np.abs(v - buf.exp)
    ok = err <= buf.bnd
    if not ok.all():
        k = int(np.argmax(err - buf.bnd))
        raise AssertionError(f'{name}: {int((~ok).sum())} of {v.size} outputs outside the bound; worst {v[k]!r} vs '
                             f'{buf.exp[k]!r}: error {err[k]:.3e} > bound {buf.bnd[k]:.3e}')
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(buf.bnd > 0, err / buf.bnd, 0.0)
    return float(ratio.max()), float(err.max())


def rup(v, m):
    return (v + m - 1) // m * m


def _ld(n, aligned):
    """A row stride past n: a multiple of 4 with padding (16-B rows), or an odd one."""
    return rup(n, 4) + 4 if aligned else (n + 3) | 1


def mask_pattern(rows, cols):
    """Fixed ReLU-mask pattern, about 40 % not positive: exact 0.0, -0.0 and a negative value among them."""
    m, n = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    q = (m * 7 + n * 3 + (m * n) % 5) % 10
    out = (0.25 + 0.05 * q).astype(np.float32)
    out[q == 0] = 0.0
    out[q == 1] = -0.0
    out[q == 2] = -0.5
    out[q == 3] = 0.0
    return out


def softplus64(v):
    z = 100.0 * v
    return np.where(z > 20.0, v, np.log1p(np.exp(np.minimum(z, 20.0))) / 100.0)


def softplus_ref_error(v32):
    """(absolute error of torch's fp32 softplus(beta=100, threshold=20), relative error of its fp32
    exp(100 v)) against float64 on the fp32 pre-activations v32: what the 16x margin is applied to."""
    import torch
    v32 = np.ascontiguousarray(v32, np.float32)
    if v32.size == 0:
        return 0.0, 0.0
    t = torch.from_numpy(v32.reshape(-1))
    sp = torch.nn.functional.softplus(t, beta=100, threshold=20).numpy().astype(np.float64)
    e_abs = float(np.abs(sp - softplus64(v32.reshape(-1).astype(np.float64))).max())
    ex = torch.exp(t * 100.0).numpy().astype(np.float64)
    ref = np.exp(100.0 * v32.reshape(-1).astype(np.float64))
    e_rel = float((np.abs(ex - ref) / ref).max())
    return e_abs, e_rel


# ======================================================================================================
# generic strided GEMM (launch_gemm / launch_gemm_det)
# ======================================================================================================
@dataclasses.dataclass(frozen=True)
class GemmCase:
    name: str
    M: int                       # host M: the grid's M
    N: int
    K: tuple                     # per segment
    prec: str = 'fp32'           # fp32 | bf16 | x3
    a_k: bool = True             # A contiguous in k (else in m)
    b_k: bool = True             # B contiguous in k (else in n)
    aligned: bool = True         # 16-B bases and strides % 4 == 0; else one float off and odd strides
    one_row: bool = False        # the one-row A: a_rs == a_cs == 1
    M_dev: int = None
    K_dev: int = None
    bias: bool = False
    relu: bool = False
    mask: bool = False
    accumulate: bool = False
    atomic: bool = False
    ksplit: int = 1
    kper: int = 0
    div_pre: float = 0.0
    div_post: float = 0.0
    softplus: bool = False
    deriv: bool = False
    spd: str = ''                # '' | 'd' (factors d) | 'h' (softplus outputs h)
    spd_n: int = 0
    spd_scale: float = 0.0
    rowsum: bool = False
    rowsum2: bool = False
    det: bool = False
    seed: int = 1
    parts: int = 0               # > 0: the number of partial sums a slab reduction adds (bound only)
    atr: bool = False            # k_lgemm: A holds softplus factors d, used as w[k] d / (d + 1) (d >= 0) or w[k]
    head_n: int = 0              # k_lgemm: the fused head, head_out = head_w relu(.) + head_b, C not written
    a_unal: bool = False         # A alone off the 16-B boundary with an odd stride (k_lgemm's 4-B load variant)
    a_stored: bool = False       # A / B are stored as bf16: the logical values are bf16 already
    b_stored: bool = False

    @property
    def M_eff(self):
        return self.M if self.M_dev is None else self.M_dev

    @property
    def K_eff(self):
        return tuple((self.K_dev if (i == 0 and self.K_dev is not None) else k) for i, k in enumerate(self.K))

    def live_splits(self):
        if self.parts > 0:
            return self.parts
        if self.ksplit <= 1:
            return 1
        k0 = self.K_eff[0]
        tile = 32 if self.prec == 'fp32' else 64
        per = self.kper if self.kper > 0 else rup((k0 + self.ksplit - 1) // self.ksplit, tile)
        return min(self.ksplit, (k0 + per - 1) // per)


class GemmData:
    pass


def _gemm_operands(c, rng):
    """Logical fp32 operands at host capacity: A_s (M x K_s), B_s (K_s x N), and the epilogue inputs."""
    A = [rng.uniform(-1, 1, (c.M, k)).astype(np.float32) for k in c.K]
    B = [rng.uniform(-1, 1, (k, c.N)).astype(np.float32) for k in c.K]
    if c.a_stored:
        A = [rne_bf16(a) for a in A]
    if c.atr:   # softplus factors exp(100 v) >= 0, or -1 above the threshold (spd_h: softplus outputs h)
        if c.spd == 'h':
            A = [rng.uniform(0, 0.06, a.shape).astype(np.float32) for a in A]
        else:
            A = [np.where(rng.uniform(0, 1, a.shape) < 0.3, -1.0, rng.uniform(0, 4, a.shape)).astype(np.float32) for a in A]
    if c.b_stored:
        B = [rne_bf16(b) for b in B]
    bias = rng.uniform(-1, 1, c.N).astype(np.float32)
    c0 = rng.uniform(-1, 1, (c.M, c.N)).astype(np.float32)
    rs0 = rng.uniform(-1, 1, (2, c.M)).astype(np.float32)
    if c.spd == 'h':
        spd = rng.uniform(0, 0.06, (c.M, c.N)).astype(np.float32)
    else:  # softplus factors exp(100 v) >= 0, or -1 above the threshold
        spd = rng.uniform(0, 4, (c.M, c.N)).astype(np.float32)
        spd[rng.uniform(0, 1, (c.M, c.N)) < 0.3] = -1.0
    return A, B, bias, c0, rs0, spd


def gemm_seen(c, A, B):
    """The operands the kernel sees by contract, as float64."""
    if c.prec == 'bf16':
        return [rne_bf16(a).astype(np.float64) for a in A], [rne_bf16(b).astype(np.float64) for b in B]
    return [a.astype(np.float64) for a in A], [b.astype(np.float64) for b in B]


def gemm_eval(c, A, B, bias, c0, rs0, spd, mask, mut=None, e_sp=(0.0, 0.0)):
    """Float64 result of the launch on the logical operands: dict of (value, bound) arrays over the M_eff
    (or mutated) rows: C, deriv, rowsum, rowsum2. mut: a mutation of the REFERENCE (test_gemm_ref's teeth):
    'drop_last_k', 'drop_first_k_seg1', 'ignore_seg1', 'rows_plus_1', 'no_bias', 'bias_per_split',
    'swap_k_b', 'unrounded'."""
    Me = c.M_eff + (1 if (mut == 'rows_plus_1' and c.M_dev is not None) else 0)
    Ke = list(c.K_eff)
    if mut == 'rows_plus_1' and c.M_dev is None:   # the device SAMPLE count of a weight gradient
        Ke[0] += 1
    cc = dataclasses.replace(c, prec='fp32') if mut == 'unrounded' else c
    atr_b = 0.0
    if c.atr:   # A(m, k) = w[k] f(d), f as the spd factors: 6 u relative on every element (see the bound notes)
        w = atr_weights(c)[None, :].astype(np.float64)
        dd = A[0].astype(np.float64)
        if c.spd == 'h':
            fa = 1.0 - np.exp(-100.0 * dd)
        else:
            fa = np.where(dd >= 0.0, dd / np.where(dd >= 0.0, dd + 1.0, 1.0), 1.0)
        A = [(w * fa)] + list(A[1:])
        atr_b = 6 * U
    As, Bs = gemm_seen(cc, A, B)
    As = [a[:Me, :k] for a, k in zip(As, Ke)]
    Bs = [b[:k] for b, k in zip(Bs, Ke)]
    Araw = [a.astype(np.float64)[:Me, :k] for a, k in zip(A, Ke)]
    if mut == 'drop_last_k':
        s = len(As) - 1
        As[s], Bs[s], Araw[s] = As[s][:, :-1], Bs[s][:-1], Araw[s][:, :-1]
    if mut == 'drop_first_k_seg1':
        As[1], Bs[1], Araw[1] = As[1][:, 1:], Bs[1][1:], Araw[1][:, 1:]
    if mut == 'ignore_seg1':
        As, Bs, Araw = As[:1], Bs[:1], Araw[:1]
    if mut == 'swap_k_b':
        # the adjacent pair whose A columns differ most (a one-row A can hold two nearly equal neighbours,
        # and swapping their B rows is then no fault at all)
        k = int(np.argmax(np.abs(As[0][:, 1:] - As[0][:, :-1]).max(0)))
        b = Bs[0].copy()
        b[[k, k + 1]] = b[[k + 1, k]]
        Bs[0] = b
    acc = np.zeros((Me, c.N))
    S = np.zeros((Me, c.N))
    for a, b in zip(As, Bs):
        acc += a @ b
        S += np.abs(a) @ np.abs(b)
    Kt = sum(Ke)
    if c.prec == 'x3':
        bnd = (X3_TERM + gamma(3 * Kt) * X3_ACC) * S
    else:
        bnd = gamma(Kt + 1) * S
    bnd = bnd + atr_b * S
    out = {}
    nsplit = c.live_splits()
    if c.rowsum:
        rsum = sum(a.sum(1) for a in Araw)
        rabs = sum(np.abs(a).sum(1) for a in Araw)
        for i, nm in enumerate(('rowsum', 'rowsum2')[:2 if c.rowsum2 else 1]):
            r0 = rs0[i, :Me].astype(np.float64)
            out[nm] = (r0 + rsum, gamma(Kt + 4 * nsplit + 2) * (rabs + np.abs(r0)))
    bv = bias.astype(np.float64)[None, :] if (c.bias and mut != 'no_bias') else None
    if c.atomic:
        v = c0[:Me].astype(np.float64) + acc
        tot = S + np.abs(c0[:Me])
        if bv is not None:
            v = v + bv * (nsplit if mut == 'bias_per_split' else 1)
            tot = tot + np.abs(bv)
        extra = (X3_TERM * S) if c.prec == 'x3' else 0.0
        g = gamma((3 if c.prec == 'x3' else 1) * Kt + nsplit + 2) * (X3_ACC if c.prec == 'x3' else 1.0)
        out['C'] = (v, extra + g * tot)
        return out
    v, b = acc, bnd
    if bv is not None:
        v = v + bv
        b = b + U * np.abs(v)
    if c.accumulate:
        v = v + c0[:Me]
        b = b + U * np.abs(v)
    if c.div_pre:
        d = float(np.float32(c.div_pre))
        v = v / d
        b = b / abs(d) + U * np.abs(v)
    if c.relu:
        v = np.maximum(v, 0.0)
    if c.softplus:
        z = 100.0 * v
        out['pre'] = (v, b)
        if c.deriv:
            ez = np.exp(np.minimum(z, 20.0))
            out['deriv'] = (np.where(z > 20.0, -1.0, ez), np.where(z > 20.0, 0.0, ez * (SOFTPLUS_MARGIN * e_sp[1] + 100.0 * b)))
        v = softplus64(v)
        b = b + SOFTPLUS_MARGIN * e_sp[0] + U * np.abs(v)
    if c.spd:
        d = spd[:Me, :c.spd_n].astype(np.float64)
        if c.spd == 'h':
            sc = float(np.float32(c.spd_scale)) if c.spd_scale else 1.0
            f = 1.0 - np.exp(-100.0 * d * sc)
        else:
            f = np.where(d >= 0.0, d / np.where(d >= 0.0, d + 1.0, 1.0), 1.0)
        f = np.concatenate([f, np.ones((Me, c.N - c.spd_n))], 1)
        b = b * f + 6 * U * np.abs(v)
        v = v * f
    if c.mask:
        keep = mask[:Me] > 0
        v = np.where(keep, v, 0.0)
        b = np.where(keep, b, 0.0)
    if c.div_post:
        d = float(np.float32(c.div_post))
        v = v / d
        b = b / abs(d) + U * np.abs(v)
    out['C'] = (v, b)
    if c.head_n:   # head_out[m][o] = sum_n head_w[o][n] h[m][n] + head_b[o]: fmas over the columns, two atomics
        hw, hb = head_weights(c)
        hw64 = hw.astype(np.float64)
        out['head'] = (v @ hw64.T + hb[None, :], b @ np.abs(hw64).T + gamma(c.N + 8) * (np.abs(v) @ np.abs(hw64).T + np.abs(hb)[None, :]))
    return out


def atr_weights(c):
    return np.random.default_rng(7000 + c.seed).uniform(-1, 1, c.K[0]).astype(np.float32)


def head_weights(c):
    rng = np.random.default_rng(8000 + c.seed)
    return rng.uniform(-1, 1, (c.head_n, c.N)).astype(np.float32), rng.uniform(-1, 1, c.head_n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gemm_data(c):
    """Operands, device buffers and expectations of a case: computed once, shared by the CPU and GPU tests."""
    d = GemmData()
    d.case = c
    rng = np.random.default_rng(1000 * c.seed)
    A, B, bias, c0, rs0, spd = _gemm_operands(c, rng)
    mask = mask_pattern(c.M, c.N)
    e_sp = (0.0, 0.0)
    if c.softplus:
        # scale the weights (and the bias) so that the pre-activations lie in [-0.5, 0.5]
        probe = gemm_eval(dataclasses.replace(c, softplus=False, spd='', mask=False, div_post=0.0), A, B, bias, c0, rs0,
                          spd, mask)['C'][0]
        s = np.float32(0.49 / max(1e-30, np.abs(probe).max())) if probe.size else np.float32(1)
        B = [(b * s).astype(np.float32) for b in B]
        bias = (bias * s).astype(np.float32)
        c0 = (c0 * s).astype(np.float32)
        # no pre-activation within its bound of the deriv threshold (100 v = 20): redraw one element of
        # every row that holds such a pre-activation until none is left
        for _ in range(64):
            pre = gemm_eval(dataclasses.replace(c, spd='', mask=False, div_post=0.0), A, B, bias, c0, rs0, spd, mask)['pre']
            bad = np.abs(100.0 * pre[0] - 20.0) <= 100.0 * pre[1]
            if not (c.deriv and bad.any()):
                break
            for m in np.unique(np.nonzero(bad)[0]):
                A[0][m, rng.integers(A[0].shape[1])] = np.float32(rng.uniform(-1, 1))
        e_sp = softplus_ref_error(pre[0].astype(np.float32))
    d.A, d.B, d.bias, d.c0, d.rs0, d.spd, d.mask, d.e_sp = A, B, bias, c0, rs0, spd, mask, e_sp
    d.ref = gemm_eval(c, A, B, bias, c0, rs0, spd, mask, e_sp=e_sp)
    return d


def gemm_threshold_violations(d):
    """Elements whose reference pre-activation lies within its bound of the deriv threshold (must be 0)."""
    if not (d.case.softplus and d.case.deriv):
        return 0
    v, b = d.ref['pre']
    return int((np.abs(100.0 * v - 20.0) <= 100.0 * b).sum())


def gemm_buffers(d):
    """The device allocations of a case (Buf per descriptor pointer) and the strides.

    NaN placement (what the kernel must not consume), by the contract lines of anr_train.h GemmArgs:
      * "M_dev: if set, M is read from device memory": A / mask / spd rows and C / deriv rows >= M_dev;
      * "K_dev: if set, segment 0's K is read from device memory": segment 0's k >= K_dev in A and B;
      * the strided layouts carry no K padding (A(m,k) = A[m a_rs + k a_cs], k < K): every element between
        the rows, and the guard bands, are NaN;
      * spd "n < spd_n": columns >= spd_n of spd.
    """
    c = d.case
    Me, Ke, al = c.M_eff, c.K_eff, c.aligned
    bufs, st = {}, {}
    for s, K in enumerate(c.K):
        a = d.A[s].copy()
        b = d.B[s].copy()
        a[Me:] = np.nan
        a[:, Ke[s]:] = np.nan
        b[Ke[s]:] = np.nan
        if c.one_row:
            a_rs, a_cs = 1, 1
        elif c.a_k:
            a_rs, a_cs = _ld(K, al), 1
        else:
            a_rs, a_cs = 1, _ld(c.M, al)
        if c.b_k:
            b_rs, b_cs = 1, _ld(K, al)
        else:
            b_rs, b_cs = _ld(c.N, al), 1
        if c.a_unal:
            a_rs = (K + 3) | 1
        bufs[f'A{s}'] = in_buf(a, a_rs, a_cs, al and not c.a_unal)
        bufs[f'B{s}'] = in_buf(b, b_rs, b_cs, al)
        st[f'a{s}'] = (a_rs, a_cs)
        st[f'b{s}'] = (b_rs, b_cs)
    ldc = _ld(c.N, al)
    defined = np.zeros((c.M, c.N), bool)
    defined[:Me] = True

    def full(x, fill=0.0):
        o = np.full((c.M, c.N), fill)
        o[:Me] = x
        return o
    v, b = d.ref['C']
    keep_init = c.accumulate or c.atomic
    if c.head_n:   # "C is then not written and head_out (ld ldh, zeroed by the caller) receives the result"
        hv, hb_ = d.ref['head']
        st['ldh'] = 4
        hdef = np.zeros((c.M, 4), bool)
        hdef[:, :c.head_n] = True
        e, bb = np.zeros((c.M, 4)), np.zeros((c.M, 4))
        e[:, :c.head_n], bb[:, :c.head_n] = hv, hb_
        bufs['head_out'] = out_buf(c.M, 4, 4, 1, True, hdef, e, bb, init=np.zeros((c.M, 4), np.float32))
        hw, hb = head_weights(c)
        bufs['head_w'] = in_buf(hw, c.N, 1, True)
        bufs['head_b'] = in_buf(hb[None, :], c.head_n, 1, True)
        defined = np.zeros((c.M, c.N), bool)
    if c.atr:
        bufs['atr'] = in_buf(atr_weights(c)[None, :], c.K[0], 1, True)
    bufs['C'] = out_buf(c.M, c.N, ldc, 1, al, defined, full(v), full(b), init=d.c0 if keep_init else None)
    st['ldc'] = ldc
    if c.bias:
        bufs['bias'] = in_buf(d.bias[None, :], c.N, 1, al)
    if c.mask:
        m = d.mask.copy()
        m[Me:] = np.nan
        st['ldm'] = _ld(c.N, al) + 4   # ldm > N, and not ldc
        bufs['mask'] = in_buf(m, st['ldm'], 1, al)
    if c.softplus and c.deriv:
        v, b = d.ref['deriv']
        st['ldd'] = _ld(c.N, al) + 8
        bufs['deriv'] = out_buf(c.M, c.N, st['ldd'], 1, al, defined, full(v), full(b))
    if c.spd:
        sp = d.spd.copy()
        sp[Me:] = np.nan
        sp[:, c.spd_n:] = np.nan
        st['ldsd'] = _ld(c.N, al) + 12
        bufs['spd'] = in_buf(sp, st['ldsd'], 1, al)
    for i, nm in enumerate(('rowsum', 'rowsum2')):
        if nm in d.ref:
            v, b = d.ref[nm]
            dm = np.zeros((1, c.M), bool)
            dm[0, :Me] = True
            e = np.zeros((1, c.M))
            e[0, :Me] = v
            bb = np.zeros((1, c.M))
            bb[0, :Me] = b
            bufs[nm] = out_buf(1, c.M, c.M, 1, True, dm, e, bb, init=d.rs0[i][None, :])
    return bufs, st


# ---- the cases ---------------------------------------------------------------------------------------
# M in {1, 63, 64, 65, 130}, N in {1, 3, 24, 63, 64, 68, 132}, K in {1, 3, 31, 32, 33, 63, 64, 65, 100}: the
# smallest shapes that cross each edge of the 64 x 64 tile and of the K tile (32 fp32, 64 bf16 / x3)
GEMM_SHAPES = [(1, 1, 1), (63, 3, 3), (64, 24, 31), (65, 63, 32), (130, 64, 33), (1, 68, 63), (63, 132, 64),
               (64, 1, 65), (65, 3, 100), (130, 132, 100), (64, 64, 64), (65, 68, 1)]
SQRT2 = 1.41421356237309515


def _gemm_cases():
    out = []
    # layouts x precision x alignment at every shape
    for prec in ('fp32', 'bf16', 'x3'):
        for a_k in (True, False):
            if prec == 'x3' and not a_k:
                continue  # split-bf16: A k-contiguous only (launch_gemm_sw)
            for b_k in (True, False):
                for al in (True, False):
                    for (M, N, K) in GEMM_SHAPES:
                        out.append(GemmCase(f'lay-{prec}-a{"k" if a_k else "m"}-b{"k" if b_k else "n"}-{"al" if al else "un"}-'
                                            f'{M}x{N}x{K}', M, N, (K,), prec=prec, a_k=a_k, b_k=b_k, aligned=al, bias=True,
                                            seed=len(out) + 1))
    # two segments of odd width; the one-row A with and without row sums
    for prec in ('fp32', 'bf16', 'x3'):
        for K in ((39, 64), (63, 33)):
            for al in (True, False):
                for b_k in (True, False):
                    out.append(GemmCase(f'seg2-{prec}-b{"k" if b_k else "n"}-{"al" if al else "un"}-{K[0]}+{K[1]}', 65, 68, K,
                                        prec=prec, b_k=b_k, aligned=al, bias=True, relu=True, seed=len(out) + 1))
                if prec != 'x3':
                    for rs in (False, True):
                        out.append(GemmCase(f'seg2-{prec}-onerow-{"al" if al else "un"}-{K[0]}+{K[1]}{"-rowsum" if rs else ""}',
                                            1, 68, K, prec=prec, b_k=False, aligned=al, one_row=True, rowsum=rs,
                                            seed=len(out) + 1))
    # epilogues, each with vec_out on (aligned, N % 4 == 0) and off
    epi = {
        'bias': dict(bias=True),
        'bias-relu': dict(bias=True, relu=True),
        'mask': dict(mask=True),
        'accumulate': dict(accumulate=True),
        'divpre': dict(div_pre=SQRT2),
        'divpost-relu': dict(div_post=SQRT2, relu=True),
        'softplus-deriv': dict(bias=True, softplus=True, deriv=True),
        'softplus': dict(bias=True, softplus=True),
        'spd-d': dict(spd='d', spd_n=41),
        'spd-h': dict(spd='h', spd_n=41, spd_scale=SQRT2),
        # the combinations the sdf executors issue (anr_sdf_train.hip SGemm::fwd / xgrad / sdf_input_grad /
        # sdf_tangent / resd_forward, anr_sdf_capi.hip fwd / fwd_sp / bwd):
        'sdf-lin3': dict(bias=True, softplus=True, deriv=True, div_post=SQRT2),           # sdf_forward, l == 3
        'sdf-tangent': dict(spd='d', spd_n=68, div_post=SQRT2),                          # sdf_tangent, l == 3
        'sdf-bwd': dict(b_k=False, spd='d', spd_n=41, div_pre=SQRT2),                    # sdf_input_grad, lin4 -> lin3
        'sdf-bwd-h': dict(b_k=False, spd='h', spd_n=41, spd_scale=SQRT2, div_pre=SQRT2),  # anr_sdf_capi.hip bwd, spd_h
        'sdf-bwd-h0': dict(b_k=False, spd='h', spd_n=68),                                 # ... spd_scale 0
        'sdf-xgrad': dict(b_k=False, mask=True, accumulate=True),                         # SGemm::xgrad
        'sdf-xgrad-mask': dict(b_k=False, mask=True),
        'sdf-resd-tangent': dict(mask=True),                                              # fwd with Epi::mask, no bias
    }
    for prec in ('fp32', 'x3'):
        for nm, kw in epi.items():
            for al in (True, False):
                out.append(GemmCase(f'epi-{prec}-{nm}-{"al" if al else "un"}', 65, 68, (33,), prec=prec, aligned=al,
                                    seed=len(out) + 1, **kw))
        for al in (True, False):  # resd_forward's layer 5: two segments, bias + relu
            out.append(GemmCase(f'epi-{prec}-sdf-resd5-{"al" if al else "un"}', 65, 68, (63, 64), prec=prec, aligned=al,
                                bias=True, relu=True, seed=len(out) + 1))
    # device counts: M_dev one below the grid's M, a whole tile below, and 0
    for prec in ('fp32', 'bf16', 'x3'):
        for md in (129, 66, 0):
            for b_k in (True, False):
                out.append(GemmCase(f'mdev-{prec}-b{"k" if b_k else "n"}-{md}', 130, 68, (33,), prec=prec, b_k=b_k, M_dev=md,
                                    bias=True, relu=True, mask=True, seed=len(out) + 1))
    # the weight-gradient launch: A(m, k) = dY[k][m], B = X rows, split-K over the samples with a device
    # sample count, atomics into a non-zero C with the bias once, row sums
    for prec in ('fp32', 'bf16'):
        for al in (True, False):
            for kd in (256, 130, 100, 1):   # every split live / the last live split partial / splits past K
                out.append(GemmCase(f'wg-{prec}-{"al" if al else "un"}-kdev{kd}', 65, 68, (256,), prec=prec, a_k=False, b_k=False,
                                    aligned=al, K_dev=kd, atomic=True, ksplit=4, kper=64, bias=True, rowsum=True,
                                    rowsum2=(kd != 130), seed=len(out) + 1))
            # kper == 0 (the sdf executor's split): K / ksplit rounded up to the K tile
            out.append(GemmCase(f'wg-{prec}-{"al" if al else "un"}-kper0', 65, 68, (100,), prec=prec, a_k=False, b_k=False,
                                aligned=al, atomic=True, ksplit=3, rowsum=True, seed=len(out) + 1))
            # one-output layer: the one-row A
            out.append(GemmCase(f'wg-{prec}-{"al" if al else "un"}-onerow', 1, 68, (100,), prec=prec, b_k=False, aligned=al,
                                one_row=True, atomic=True, ksplit=2, kper=64, rowsum=True, seed=len(out) + 1))
    # the atomic epilogue in every other operand layout (no executor issues these; the launcher takes them):
    # the non-swapped instantiations of every kernel, two splits with the last one partial, the bias once
    for prec in ('fp32', 'bf16', 'x3'):
        for a_k in (True, False):
            if prec == 'x3' and not a_k:
                continue
            for b_k in (True, False):
                for al in (True, False):
                    out.append(GemmCase(f'atomic-{prec}-a{"k" if a_k else "m"}-b{"k" if b_k else "n"}-{"al" if al else "un"}', 65, 68,
                                        (100,), prec=prec, a_k=a_k, b_k=b_k, aligned=al, atomic=True, ksplit=2, kper=64,
                                        bias=True, seed=len(out) + 1))
    # launch_gemm_det: the same launches on the fixed-order route (no bias, no M_dev: its own conditions)
    for prec in ('fp32', 'bf16'):
        for al in (True, False):
            for kd in (256, 130, 100):
                out.append(GemmCase(f'det-{prec}-{"al" if al else "un"}-kdev{kd}', 65, 68, (256,), prec=prec, a_k=False, b_k=False,
                                    aligned=al, K_dev=kd, atomic=True, ksplit=4, kper=64, rowsum=True, rowsum2=(kd == 256),
                                    det=True, seed=len(out) + 1))
            out.append(GemmCase(f'det-{prec}-{"al" if al else "un"}-onerow', 1, 3, (100,), prec=prec, b_k=False, aligned=al,
                                one_row=True, atomic=True, ksplit=2, kper=64, rowsum=True, det=True, seed=len(out) + 1))
    return out


GEMM_CASES = _gemm_cases()

MUTATIONS = ('drop_last_k', 'drop_first_k_seg1', 'ignore_seg1', 'rows_plus_1', 'no_bias', 'bias_per_split', 'swap_k_b',
             'unrounded')


def gemm_mutation_applies(c, mut):
    Me, Ke = c.M_eff, c.K_eff
    if mut == 'rows_plus_1':
        return (c.M_dev is not None and c.M_dev < c.M) or (c.M_dev is None and c.K_dev is not None and c.K_dev < c.K[0])
    if Me == 0:
        return False
    if mut in ('drop_first_k_seg1', 'ignore_seg1'):
        return len(c.K) == 2
    if mut == 'no_bias':
        return c.bias
    if mut == 'bias_per_split':
        return c.bias and c.atomic and c.live_splits() > 1
    if mut == 'swap_k_b':
        return Ke[0] >= 2
    if mut == 'unrounded':
        return c.prec == 'bf16' and not (c.a_stored and c.b_stored) and sum(Ke) >= 1
    return Ke[-1] >= 1  # drop_last_k


def outside(ref, mutated, names=('C', 'deriv', 'rowsum', 'rowsum2')):
    """Would the mutated result fail the GPU test's check against ref: some element defined by one and not
    the other, or a common element further from ref than its bound."""
    for nm in names:
        if nm not in ref:
            continue
        (v, b), (w, _) = ref[nm], mutated[nm]
        if v.shape != w.shape:
            return True
        if (np.abs(w - v) > b).any():
            return True
    return False


# ======================================================================================================
# bf16 row GEMM (launch_rgemm): C[M][N] = epi(sum_s A_s[M][K_s] W_s[N][K_s]^T), W_s a bf16 weight image
# ======================================================================================================
NAN16 = np.uint16(0x7FC0)
RG_VARIANTS = ('f32', 'abf', 'abf_mbf', 'mbf', 'x3')   # the hook's out_variant index


@dataclasses.dataclass(frozen=True)
class RCase:
    name: str
    M: int                 # M_host: the grid's rows
    M_dev: int
    N: int
    K: tuple
    rows: tuple            # valid image rows per segment (>= N)
    bcol: tuple            # chunk-aligned column offset into the image
    variant: str = 'f32'
    bias: bool = False
    relu: bool = False
    mask: bool = False
    accumulate: bool = False
    cbf: bool = False
    ldc_kind: str = 'v16'  # 'v16': ldc % 8 == 0; 'v4': ldc % 8 == 4; 'odd': odd ldc, skewed bases (vec_out off)
    seed: int = 1

    @property
    def x3(self):
        return self.variant == 'x3'

    @property
    def abf(self):
        return self.variant in ('abf', 'abf_mbf')

    @property
    def mbf(self):
        return self.variant in ('abf_mbf', 'mbf')

    def gemm_case(self):
        """The same product as a GemmCase: A k-contiguous, B = W^T, bf16 (or split) operands."""
        return GemmCase(self.name, self.M, self.N, self.K, prec='x3' if self.x3 else 'bf16', M_dev=self.M_dev,
                        bias=self.bias, relu=self.relu, mask=self.mask, accumulate=self.accumulate, a_stored=self.abf,
                        b_stored=not self.x3, seed=self.seed)


def _bits_or_nan(x):
    b = bf16_bits(np.nan_to_num(x, nan=0.0))
    b[np.isnan(x)] = NAN16
    return b


def rgemm_image(W, rows, ldb, bcol, K, x3):
    """The weight image of W (N x K, fp32) as plain bf16 rows (RGemmSeg's comment in anr_train.h: "bf16 image
    rows (k-contiguous, stride ldb, chunk-aligned column offset bcol, `rows` valid rows)"), hi image and, x3,
    the lo image lo_off elements further. Columns [K, K rounded to 64) of the segment are zero, as wimg_pack
    pads them ("segments padded to 64"); rows >= N (outputs nobody asked for) and every other column are NaN."""
    N = W.shape[0]
    lo_off = rup(rows * ldb, 8) + 64
    flat = np.full(GUARD + lo_off + rows * ldb + GUARD, NAN16, np.uint16)
    hi, lo = split_bf16(W)
    for img, base in ((hi, GUARD), (lo, GUARD + lo_off)):
        v = flat[base:base + rows * ldb].reshape(rows, ldb)
        v[:N, bcol:bcol + rup(K, 64)] = 0
        v[:N, bcol:bcol + K] = bf16_bits(img)
        if not x3:
            break
    return Buf(flat, GUARD), lo_off


def rgemm_buffers(rc, d):
    """NaN placement: rows >= M_dev of A / mask ("M_dev"), columns >= K of A (anr_tgemm.hip k_rgemm: "the
    last, partial chunk of a segment: columns past K read as zero": read and discarded), image rows >= N."""
    Me = rc.M if rc.M_dev is None else rc.M_dev
    al = rc.ldc_kind != 'odd'
    bufs, st = {}, {}
    for s, K in enumerate(rc.K):
        a = d.A[s].copy()
        a[Me:] = np.nan
        lda = rup(K, 64) + (64 if s else 0)
        if rc.abf:
            bufs[f'A{s}'] = in_buf(_bits_or_nan(a), lda, 1, True, np.uint16, NAN16, extent=rc.M * lda)
        else:
            bufs[f'A{s}'] = in_buf(a, lda, 1, True, extent=rc.M * lda)
        ldb = rc.bcol[s] + rup(K, 64) + 8 * s
        bufs[f'B{s}'], lo_off = rgemm_image(np.ascontiguousarray(d.B[s].T), rc.rows[s], ldb, rc.bcol[s], K, rc.x3)
        st[f'lda{s}'], st[f'ldb{s}'], st[f'lo_off{s}'] = lda, ldb, lo_off
    ldc = {'v16': rup(rc.N, 8) + 8, 'v4': rup(rc.N, 8) + 4, 'odd': (rc.N + 3) | 1}[rc.ldc_kind]
    defined = np.zeros((rc.M, rc.N), bool)
    defined[:Me] = True
    v, b = d.ref['C']
    e = np.zeros((rc.M, rc.N))
    bb = np.zeros((rc.M, rc.N))
    e[:Me], bb[:Me] = v, b
    bufs['C'] = out_buf(rc.M, rc.N, ldc, 1, al, defined, e, bb, init=d.c0 if rc.accumulate else None,
                        dtype=np.uint16 if rc.cbf else np.float32)
    st['ldc'] = ldc
    if rc.bias:
        bufs['bias'] = in_buf(d.bias[None, :], rc.N, 1, al)
    if rc.mask:
        m = d.mask.copy()
        m[Me:] = np.nan
        st['ldm'] = rup(rc.N, 4) + 8 if al else (rc.N + 5) | 1
        if rc.mbf:
            bufs['mask'] = in_buf(_bits_or_nan(m), st['ldm'], 1, al, np.uint16, NAN16)
        else:
            bufs['mask'] = in_buf(m, st['ldm'], 1, al)
    return bufs, st


RG_SHAPES = [  # M_host, M_dev, N, K, rows, bcol
    (1, None, 3, (39,), (3,), (0,)),
    (127, 126, 4, (64,), (7,), (64,)),
    (128, None, 24, (100,), (24,), (0,)),
    (129, 128, 128, (128,), (130,), (64,)),
    (300, None, 256, (256,), (256,), (0,)),
    (300, 0, 24, (64,), (24,), (0,)),
    (129, None, 4, (39, 64), (4, 200), (0, 64)),
    (128, 127, 256, (100, 39), (256, 256), (64, 0)),
    (1, None, 128, (256,), (128,), (0,)),
    (127, None, 3, (128,), (5,), (64,)),
    (300, 299, 24, (39,), (255,), (64,)),
]
RG_EPILOGUES = [  # bias, relu, mask, accumulate, cbf, ldc_kind
    (1, 1, 0, 0, 0, 'v16'), (0, 0, 1, 0, 0, 'v4'), (0, 0, 0, 1, 0, 'v16'), (1, 1, 0, 0, 1, 'v16'), (1, 0, 0, 0, 1, 'v4'),
    (1, 1, 1, 0, 0, 'odd'), (0, 0, 1, 0, 1, 'odd'), (1, 0, 1, 1, 0, 'v4'),
]


def _rgemm_cases():
    out = []
    for vi, var in enumerate(RG_VARIANTS):
        shapes = list(RG_SHAPES)
        if var == 'x3':
            shapes.append((129, None, 24, (32,), (24,), (32,)))   # the 32-deep chunk: K = 32, bcol = 32
            shapes.append((128, 127, 4, (32, 39), (4, 4), (32, 0)))
        for i, (M, Md, N, K, rows, bcol) in enumerate(shapes):
            bias, relu, mask, acc, cbf, kind = RG_EPILOGUES[(i + 3 * vi) % len(RG_EPILOGUES)]
            if var == 'x3':
                cbf = 0                      # "Not with x3"
            if var in ('abf_mbf', 'mbf'):
                mask = 1                     # the bf16 mask variants are dispatched with a mask only
            if cbf:
                acc = 0                      # "C bf16 excludes accumulate"
            out.append(RCase(f'rg-{var}-{M}({Md})x{N}x{"+".join(map(str, K))}-{"b" if bias else ""}{"r" if relu else ""}'
                             f'{"m" if mask else ""}{"a" if acc else ""}{"c" if cbf else ""}-{kind}', M, Md, N, K, rows, bcol,
                             variant=var, bias=bool(bias), relu=bool(relu), mask=bool(mask), accumulate=bool(acc),
                             cbf=bool(cbf), ldc_kind=kind, seed=500 + len(out)))
    return out


RG_CASES = _rgemm_cases()


# ======================================================================================================
# weight gradients (launch_wgrad / launch_wgrad_f32 / launch_wgrad_group):
# dW[i][c0 + j] += sum_s dY[s][i] X[s][j], bsum[i] (+ bsum2[i]) += sum_s dY[s][i], s < the device count
# ======================================================================================================
WG_FORMATS = ('x3', 'bb', 'yb', 'xb', 'ff')   # launch_wgrad's out_format index; 'f32': launch_wgrad_f32
WG_MAX_Z = 64


@dataclasses.dataclass(frozen=True)
class WCase:
    name: str
    n: int                 # n_host: the capacity the launch is sized for
    M_dev: int             # device sample count (None: n)
    nout: int
    K: int
    fmt: str = 'bb'        # x3 | bb (bf16 x bf16) | yb (bf16 dY) | xb (bf16 X) | ff (fp32 rows, bf16 product) | f32
    c0: int = 3            # column offset of the product inside the wider dW
    bsum: bool = True
    bsum2: bool = False
    j0: int = 0            # f32 only: X starts j0 columns early, those columns of dW are not written
    det: bool = False
    seed: int = 1

    def gemm_case(self):
        """The same product as an atomic GemmCase: M = nout, N = K, the reduction over the samples."""
        prec = {'x3': 'x3', 'f32': 'fp32'}.get(self.fmt, 'bf16')
        return GemmCase(self.name, self.nout, self.K, (self.n,), prec=prec, a_k=False, b_k=False, K_dev=self.M_dev,
                        atomic=True, rowsum=self.bsum, rowsum2=self.bsum2, parts=WG_MAX_Z + 2,
                        a_stored=self.fmt in ('bb', 'yb'), b_stored=self.fmt in ('bb', 'xb'), seed=self.seed)

    @property
    def ybf(self):
        return self.fmt in ('bb', 'yb')

    @property
    def xbf(self):
        return self.fmt in ('bb', 'xb')


def wgrad_buffers(wc, d, shared=None):
    """NaN placement: rows >= the device count of dY / X (WGrad::M_dev; test_grouped_wgrad_from_legacy_
    default_stream shows they can hold arbitrary bits), columns >= nout / K of the rows (wg_widen / wg_put_bf
    mask them; k_wgrad_dma and k_wgrad_f32 read them into outputs nobody reduces: "chunks past the columns:
    any in-bounds bytes (discarded)"). dW is a window [c0, c0 + K) of a wider non-zero tensor that is
    accumulated into; every other element of it must come back bit-identical.
    shared: the (dW, bsum, bsum2) Bufs of an earlier descriptor with the same target (expectations add)."""
    Me = wc.n if wc.M_dev is None else wc.M_dev
    bufs, st = {}, {}
    y = np.ascontiguousarray(d.A[0].T).copy()   # (n, nout)
    x = d.B[0].copy()                           # (n, K)
    y[Me:] = np.nan
    x[Me:] = np.nan
    st['ldY'], st['ldX'] = rup(wc.nout, 8) + 8, rup(wc.K, 8) + 8
    for nm, a, ld, bf in (('dY', y, st['ldY'], wc.ybf), ('X', x, st['ldX'], wc.xbf)):
        if bf:
            bufs[nm] = in_buf(_bits_or_nan(a), ld, 1, True, np.uint16, NAN16, extent=wc.n * ld)
        else:
            bufs[nm] = in_buf(a, ld, 1, True, extent=wc.n * ld)
    v, b = d.ref['C']
    st['ldw'], st['c0'] = wc.c0 + wc.K + 5, wc.c0
    if shared is not None:
        # a second product into the same target: its own sum on top, the bounds add (one more addition)
        for nm, key, cols in (('dW', 'C', slice(wc.j0, None)), ('bsum', 'rowsum', None), ('bsum2', 'rowsum2', None)):
            if nm in shared and key in d.ref:
                sb = shared[nm]
                v2, b2 = d.ref[key]
                base = d.c0.astype(np.float64) if key == 'C' else d.rs0[0 if key == 'rowsum' else 1, :wc.nout].astype(np.float64)
                add, bb = (v2 - base), b2
                if key == 'C':
                    add, bb = add[:, wc.j0:].reshape(-1), bb[:, wc.j0:].reshape(-1)
                sb.exp = sb.exp + add
                sb.bnd = sb.bnd + bb + U * np.abs(sb.exp)
        return bufs, st
    rng = np.random.default_rng(wc.seed + 99)
    wide = rng.uniform(-1, 1, (wc.nout, st['ldw'])).astype(np.float32)
    wide[:, wc.c0:wc.c0 + wc.K] = d.c0
    defined = np.zeros(wide.shape, bool)
    defined[:, wc.c0 + wc.j0:wc.c0 + wc.K] = True
    e = np.zeros(wide.shape)
    bb = np.zeros(wide.shape)
    e[:, wc.c0:wc.c0 + wc.K], bb[:, wc.c0:wc.c0 + wc.K] = v, b
    bufs['dW'] = out_buf(wc.nout, st['ldw'], st['ldw'], 1, wc.c0 % 2 == 0, defined, e, bb, init=wide)
    for i, (nm, key) in enumerate((('bsum', 'rowsum'), ('bsum2', 'rowsum2'))):
        if key in d.ref:
            v, b = d.ref[key]
            bufs[nm] = out_buf(1, wc.nout, wc.nout, 1, True, np.ones((1, wc.nout), bool), v[None, :], b[None, :],
                               init=d.rs0[i][None, :wc.nout])
    return bufs, st


def _wgrad_cases():
    out = []
    # n in {1, 31, 32, 33, 64, 65, 383, 385, 1000}, M_dev in {n, n - 1, n - 33, 0}, nout in {1, 3, 24, 128, 129, 256},
    # K in {3, 63, 128, 129, 256}: samples across the 32-sample stage and the 384-sample range, outputs across
    # the 128 x 128 tile
    shapes = [(1, None, 1, 3), (31, 30, 3, 63), (32, None, 24, 128), (33, 0, 128, 129), (64, 31, 129, 256),
              (65, 64, 256, 3), (383, 350, 24, 63), (385, 384, 129, 129), (1000, 967, 256, 256), (1000, None, 3, 128),
              (385, 0, 128, 3)]
    for fi, fmt in enumerate(WG_FORMATS):
        for i, (n, md, nout, K) in enumerate(shapes):
            for det in (False, True):
                if det and i % 2 == (fi % 2):
                    continue   # the fixed-order route at every other shape of each format
                out.append(WCase(f'wg-{fmt}-{n}({md})x{nout}x{K}{"-det" if det else ""}', n, md, nout, K, fmt=fmt,
                                 c0=(3, 0, 8)[i % 3], bsum=(i % 4 != 3), bsum2=(i % 3 == 0 and i % 4 != 3), det=det,
                                 seed=900 + len(out)))
    for i, (n, md, nout, K) in enumerate(shapes):   # launch_wgrad_f32, j0 > 0 at every other shape
        j0 = (0, 1, 3)[i % 3] if K > 3 else 0
        out.append(WCase(f'wg-f32-{n}({md})x{nout}x{K}-j{j0}', n, md, nout, K, fmt='f32', c0=(3, 0, 8)[i % 3],
                         bsum=(i % 4 != 3), bsum2=(i % 3 == 0 and i % 4 != 3), j0=j0, seed=900 + len(out)))
    return out


WG_CASES = _wgrad_cases()


def wgrad_group_cases(nz_seed=0):
    """17 descriptors of mixed formats and shapes at one sample count (a second group is issued past
    WG_GROUP_MAX = 16); descriptors 3 and 4 share one dW and one bsum."""
    n, md = 385, 352
    spec = [('bb', 256, 256), ('bb', 24, 256), ('x3', 129, 63), ('yb', 128, 129), ('yb', 128, 129), ('xb', 3, 128),
            ('ff', 256, 3), ('bb', 1, 3), ('x3', 24, 24), ('ff', 129, 129), ('bb', 128, 63), ('xb', 256, 129),
            ('yb', 3, 256), ('bb', 129, 256), ('x3', 1, 128), ('ff', 24, 63), ('bb', 256, 24)]
    flag = lambda k: 3 if k == 4 else k   # descriptor 4 shares descriptor 3's target: the same window and sums
    return [WCase(f'grp{nz_seed}-{k}-{fmt}-{nout}x{K}', n, md, nout, K, fmt=fmt, c0=(0, 3, 8)[flag(k) % 3],
                  bsum=(flag(k) % 5 != 4), bsum2=(flag(k) % 4 == 1 and flag(k) % 5 != 4), seed=1300 + k)
            for k, (fmt, nout, K) in enumerate(spec)]


WG_GROUP_SHARED = (3, 4)

# every case whose reference and bound test_gemm_ref.py checks against itself (the row GEMM and the weight
# gradients through their GemmCase forms)
REF_CASES = GEMM_CASES + [c.gemm_case() for c in RG_CASES] + [c.gemm_case() for c in WG_CASES] + \
    [c.gemm_case() for c in wgrad_group_cases()]


# ======================================================================================================
# LDS-resident layer GEMM (lgemm_*): the shapes lg_dispatch instantiates, from M in {1, 127, 129, 700},
# N in {1, 4, 39, 256, 264}, K in {3, 39, 217, 256} and the two-segment skip layer (63 + 256). The smallest
# launch (cus = 2) has 64 wave slots of 16 rows: M <= 256 runs the half-tile tail, M = 700 whole tiles, and
# M = 1100 (69 tiles) is the smallest listed size at which a wave takes a second tile (the loop wraps).
# ======================================================================================================
def _lgemm_cases():
    out = []

    def add(nm, M, N, K, **kw):
        for prec in kw.pop('precs', ('fp32', 'x3')):
            out.append(GemmCase(f'lg-{prec}-{nm}-{M}x{N}x{"+".join(map(str, K))}', M, N, K, prec=prec, seed=2000 + len(out), **kw))
    add('bias-relu', 1, 1, (256,), bias=True, relu=True)
    add('softplus-deriv', 127, 4, (256,), bias=True, softplus=True, deriv=True, b_k=False)
    add('divpost', 129, 39, (256,), bias=True, div_post=SQRT2)
    add('bias-relu', 700, 256, (39,), bias=True, relu=True, b_k=False)
    add('mask', 700, 256, (39,), mask=True, precs=('fp32',))
    add('spd-d', 129, 256, (39,), spd='d', spd_n=217, precs=('fp32',))
    add('mask', 129, 256, (3,), mask=True, precs=('fp32',))
    add('spd-d-divpost', 127, 256, (217,), spd='d', spd_n=217, div_post=SQRT2, b_k=False)
    add('spd-h', 700, 256, (217,), spd='h', spd_n=256, spd_scale=SQRT2, div_pre=SQRT2)
    add('bias-relu', 129, 256, (217,), bias=True, relu=True, precs=('fp32',))
    add('bias-relu', 1100, 256, (256,), bias=True, relu=True)
    add('softplus-deriv', 700, 256, (256,), bias=True, softplus=True, deriv=True)
    add('softplus', 129, 256, (256,), bias=True, softplus=True, div_post=SQRT2)
    add('spd-h0', 129, 256, (256,), spd='h', spd_n=256, b_k=False)
    add('spd-d', 1, 256, (256,), spd='d', spd_n=217, div_pre=SQRT2, b_k=False)
    add('mask', 127, 256, (256,), mask=True, precs=('fp32',))
    add('atr', 129, 256, (256,), atr=True, spd='d', spd_n=256, b_k=False)
    add('atr-h', 127, 256, (256,), atr=True, spd='h', spd_n=217, b_k=False)
    for M, hn in ((127, 1), (129, 3), (700, 4)):
        add(f'head{hn}', M, 256, (256,), bias=True, relu=True, head_n=hn)
    add('seg2-bias-relu', 129, 256, (63, 256), bias=True, relu=True)
    add('seg2-unal', 127, 256, (63, 256), bias=True, relu=True, a_unal=True)
    add('seg2-mask', 1, 256, (63, 256), mask=True, precs=('fp32',))
    add('bias', 129, 264, (256,), bias=True)
    add('seg2', 1, 264, (63, 256), bias=True, b_k=False)
    return out


LG_CASES = _lgemm_cases()
REF_CASES = REF_CASES + LG_CASES
