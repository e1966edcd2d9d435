"""Float64 / integer numpy references, input sets and error measures for the helper probes and the small render
kernels (tests/test_gpu_math_helpers.py, tests/test_gpu_small_kernels.py); checked themselves on the CPU by
tests/test_small_ref.py. Not a test file.

Error measures. Every reference is float64 evaluated at the fp32 input. `ulp_err` counts fp32 ulps of the
float64 value: ulp(r) = 2^(floor(log2 |r|) - 23), with |r| floored at 2^-126 (so every value below the normal
range, 0 included, is measured in units of 2^-149). `rel_units` is |got - r| / max(|r|, 2^-126) in units of 2^-24.

embed_d (anr_sdf_train.hip) bound. The three kernels contract the first and second derivatives of gamma's
features with adjoints / tangents: out = sum_f t_f, t_f = (omega_f cos | -omega_f sin | -omega_f^2 sin | ...) *
inputs. In the kernels the argument x * omega_f is exact (omega_f is a power of two), sinf / cosf are within ~2
ulp, the scalings by omega_f are exact and each term takes at most three more roundings (products, the rev6
adjoint sum), so a correct implementation stays within (N + 4) 2^-24 sum|t_f| for N summed features (N - 1
additions). The issue's bar multiplies this by max omega^2 over the summed features, which also admits an
implementation that rounds the argument (an absolute argument error |x| omega 2^-24 is amplified by omega in the
first and omega^2 in the second derivative): bound = (N + 4) 2^-24 max(omega_f)^2 sum|t_f|. The feature value v
that embed_d also returns is dead in all three kernels, so only the derivative contractions can be checked.

inv33 bound. The adjugate inverse in fp32 is held to the standard forward bound with a small constant,
max|dRi| <= 16 * 2^-24 * cond_2(A) * max|A^-1|; `inv33_f32` (the same operations in numpy float32) must meet it
on the chosen matrices (test_small_ref). The bound is linear in cond_2, which the adjugate formula meets while one
singular value is small (its determinant and cofactors then lose cond_2 * 2^-24 relative). With TWO small singular
values s (a blend of exactly two near-opposite rotations: a conjugate pair) the determinant ~ s^2 is a cancelling
sum of O(1) products and the error grows like 2^-24 cond_2^2: the float32 restatement reached 1.8 x the bound at
cond_2 = 807 on such a matrix. The near-singular case of the linear bound is therefore built from three rotations
with one small singular value (LBS blends of neighbouring bones stay near cond_2 = 1), and the two-rotation blends
are held to a quadratic bound derived from the formula itself. With u = 2^-24 and entries |a| <= 1: a cofactor
p1 - p2 errs by at most u (|p1| + |p2| + |p1 - p2|) <= 4 u; the determinant sum a_i c_i by at most sum |a_i| 4 u +
3 u sum |a_i c_i| <= 21 u; Ri = c / det by 4 u / |det| + |Ri| (21 u / |det| + 2 u). With |det| = s1 s2 s3 >=
s1^3 / cond_2^2 and max|A^-1| >= 1 / (sqrt3 s1) this is within 32 u cond_2^2 max|A^-1| / s1^3.

k_composite bound. A weight is alpha_i * prod_{j<i} (1 - alpha_j + 1e-10): at most 63 factors of 3 roundings each
(the subtraction, the addition, the product) = 189, the final product and, for the maps, the product with the
colour / depth and the 6 levels of the lane reduction: 200 * 2^-24 relative to sum|terms| (|w_i| itself for a
weight). Weights that fall below the normal range (a ray of alpha = 1: factors of 1e-10) lose relative precision
or flush in any fp32 evaluation, so sum|terms| is floored at 2^-126 as for the helpers.
"""
import numpy as np

TINY = 2.0 ** -126
U24 = 2.0 ** -24
F32 = np.float32


# ---- float sets --------------------------------------------------------------------------------------------
def _bits(v):
    return int(np.array([v], F32).view(np.uint32)[0])


def _key(v):
    """The position of float32(v) in the order of all floats: bits for v >= +0, -(bits of |v|) - 1 below (-0.0 = -1)."""
    b = _bits(v)
    return b if b < 0x80000000 else -(b - 0x80000000) - 1


def f32_range(lo, hi, stride=1):
    """Every stride-th float32 of the closed interval [lo, hi], counted in increasing order from the first float
    >= lo (across -0.0, +0.0 as two floats). Counting from lo, not from bit pattern 0, matters for even strides: a
    sweep whose floats all end in zero bits makes products such as 100 x exact and hides their rounding."""
    lo, hi = float(lo), float(hi)
    assert lo <= hi
    k0, k1 = _key(lo), _key(hi)
    if float(F32(lo)) < lo:
        k0 += 1
    if float(F32(hi)) > hi:
        k1 -= 1
    k = np.arange(k0, k1 + 1, stride, dtype=np.int64)
    return np.where(k >= 0, k, 0x80000000 - k - 1).astype(np.uint32).view(F32)


def around(v, k):
    """The 2k + 1 floats around float32(v) (v > 0)."""
    b = _bits(v)
    return np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32).view(F32)


def ulp_of(ref):
    a = np.maximum(np.abs(np.asarray(ref, np.float64)), TINY)
    _, e = np.frexp(a)
    return np.ldexp(1.0, e - 1 - 23)


def ulp_err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref) / ulp_of(ref)


def rel_units(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / (U24 * np.maximum(np.abs(ref), TINY))


def sincos_inputs():
    """The sincos_fast set: every float of [32768, 65536] (both signs), every 37th of [1e-6, 32768], the two
    floats bracketing k pi / 2 for k <= 41,722, and +-0."""
    k = np.arange(1, 41723, dtype=np.float64) * (np.pi / 2)
    f = k.astype(F32)
    below = np.where(f.astype(np.float64) <= k, f, np.nextafter(f, F32(0)))
    return np.concatenate([f32_range(32768, 65536), -f32_range(32768, 65536), f32_range(1e-6, 32768, 37),
                           below, np.nextafter(below, F32(np.inf)), np.array([0.0, -0.0], F32)])


def softplus_inputs():
    """The softplus set: every 64th float of [-1.2, 0.5], every float with 100 x in [16, 21], the floats with
    100 x in [-0.01, 0.01] (every one of the top binade 2^-14 <= |x| <= 1e-4; the binades below hold 1.9e9
    floats on which softplus is the constant ln2 / 100 to fp32 precision: every 64th of them is in the first
    sweep), +-0, 0.4 and its neighbours, 10 and -10."""
    top = f32_range(2.0 ** -14, 1e-4)
    return np.concatenate([f32_range(-1.2, 0.5, 64), f32_range(0.16, 0.21), top, -top,
                           np.array([0.0, -0.0, 10.0, -10.0], F32), around(0.4, 1)])


# ---- scalar truths -----------------------------------------------------------------------------------------
def softplus100_f64(x32):
    """torch's softplus(beta=100, threshold=20) and its backward factor sigmoid(100 x), in float64."""
    x = np.asarray(x32, np.float64)
    t = 100.0 * x
    e = np.exp(np.minimum(t, 50.0))
    h = np.where(t > 20.0, x, np.log1p(e) / 100.0)
    en = np.exp(-np.abs(t))
    fac = np.where(t >= 0, 1.0 / (1.0 + en), en / (1.0 + en))
    return h, fac


# ---- positional encoding -----------------------------------------------------------------------------------
def gamma64(x32, nfreq):
    """gamma(x) (embedder.py:5-54) in float64 at the fp32 points: (n, 3 + 6 nfreq)."""
    x = np.asarray(x32, np.float64)
    out = [x]
    for k in range(nfreq):
        out += [np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)]
    return np.concatenate(out, -1)


def want_embed_feature(x32, nfreq):
    """k_probe_embed_feature's (n, 64): features 0..63, exactly 0 from frequency nfreq on."""
    g = gamma64(x32, nfreq)
    w = np.zeros((len(g), 64))
    w[:, :min(64, g.shape[1])] = g[:, :64]
    return w


def want_embed(x32, nfreq, NS):
    """embed<NS>'s layout: [i][g][s] = feature 4 s + g."""
    w = np.zeros((len(x32), 4 * NS))
    g = gamma64(x32, nfreq)
    k = min(4 * NS, g.shape[1])
    w[:, :k] = g[:, :k]
    return w.reshape(len(x32), NS, 4).transpose(0, 2, 1).copy()


def want_embed_b(x32, nfreq, NS):
    """embed_b<NS>'s layout: [i][h][8 s + 2 p + j] = (sin, cos)[j] of pair P = 4 NS h + 4 s + p - 2 = 3 freq +
    comp (0 from 3 nfreq on); the two slots before pair 0 (lane group 0) hold x, y | z, 0."""
    x = np.asarray(x32, np.float64)
    w = np.zeros((len(x), 4, 8 * NS))
    for h in range(4):
        for s in range(NS):
            for p in range(4):
                P = 4 * NS * h + 4 * s + p - 2
                j = 8 * s + 2 * p
                if P == -2:
                    w[:, h, j], w[:, h, j + 1] = x[:, 0], x[:, 1]
                elif P == -1:
                    w[:, h, j] = x[:, 2]
                elif P < 3 * nfreq:
                    a = x[:, P % 3] * 2.0 ** (P // 3)
                    w[:, h, j], w[:, h, j + 1] = np.sin(a), np.cos(a)
    return w


def gamma_d64(x32, nf):
    """Per feature of gamma_nf: its component, omega, first and second derivative along that component."""
    x = np.asarray(x32, np.float64)
    F = 3 + 6 * nf
    comp = np.zeros(F, int)
    om = np.ones(F)
    d1 = np.zeros((len(x), F))
    d2 = np.zeros((len(x), F))
    for f in range(F):
        if f < 3:
            comp[f], d1[:, f] = f, 1.0
            continue
        fr, w = divmod(f - 3, 6)
        comp[f], om[f] = w % 3, 2.0 ** fr
        a = x[:, comp[f]] * om[f]
        if w < 3:
            d1[:, f], d2[:, f] = om[f] * np.cos(a), -om[f] ** 2 * np.sin(a)
        else:
            d1[:, f], d2[:, f] = -om[f] * np.sin(a), -om[f] ** 2 * np.cos(a)
    return comp, om, d1, d2


def embed_d_bound(nfeat, om_max, abs_terms):
    return (nfeat + 4) * U24 * om_max ** 2 * abs_terms


def embed_tan_ref(x32, xd32, nf, scale):
    """k_st_embed_tan: (value, bound), each (n, F)."""
    comp, om, d1, _ = gamma_d64(x32, nf)
    v = np.float64(F32(scale)) * d1 * np.asarray(xd32, np.float64)[:, comp]
    return v, embed_d_bound(1, om[None, :], np.abs(v))


def embed_bwd10_ref(x32, G32):
    """k_st_embed_bwd10: (value, bound), each (n, 3)."""
    comp, om, d1, _ = gamma_d64(x32, 10)
    t = d1 * np.asarray(G32, np.float64)[:, :63]
    v = np.stack([t[:, comp == c].sum(1) for c in range(3)], 1)
    a = np.stack([np.abs(t[:, comp == c]).sum(1) for c in range(3)], 1)
    return v, embed_d_bound(21, om.max(), a)


def embed_rev6_ref(t32, td32, A0, A4, tbar0):
    """k_st_embed_rev6 on A0 (2n, 40), A4 (2n, 256), tbar0 (n, 4): (tbar, bound, ttbar, bound), each (n, 3)."""
    n = len(t32)
    comp, om, d1, d2 = gamma_d64(t32, 6)
    rs2 = np.float64(F32(0.70710678118654752))
    A0, A4 = np.asarray(A0, np.float64), np.asarray(A4, np.float64)
    ab = A0[:n, :39] + A4[:n, 217:256] * rs2
    atb = A0[n:, :39] + A4[n:, 217:256] * rs2
    pd = np.asarray(td32, np.float64)[:, comp]
    t1, t2, t3 = d1 * ab, d2 * pd * atb, d1 * atb
    t0 = np.asarray(tbar0, np.float64)[:, :3]
    tb = t0 + np.stack([(t1 + t2)[:, comp == c].sum(1) for c in range(3)], 1)
    tba = np.abs(t0) + np.stack([(np.abs(t1) + np.abs(t2))[:, comp == c].sum(1) for c in range(3)], 1)
    ttb = np.stack([t3[:, comp == c].sum(1) for c in range(3)], 1)
    ttba = np.stack([np.abs(t3)[:, comp == c].sum(1) for c in range(3)], 1)
    return tb, embed_d_bound(13, om.max(), tba), ttb, embed_d_bound(13, om.max(), ttba)


# ---- inv33 -------------------------------------------------------------------------------------------------
def _rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def inv33_cases(n=4096, seed=11):
    """{name: (n, 16) float32 row-major 4x4 transforms}: rotations; convex blends of 24 rotations near one pose
    (as LBS produces); blends of near-opposite rotations (cond_2 up to ~1e4)."""
    rng = np.random.default_rng(seed)

    def pack(R3):
        A = np.zeros((len(R3), 4, 4))
        A[:, :3, :3] = R3
        A[:, :3, 3] = rng.uniform(-1, 1, (len(R3), 3))
        A[:, 3, 3] = 1
        return A.reshape(-1, 16).astype(F32)

    rot = _rotations(rng, n)
    base = _rotations(rng, n)
    joint = np.einsum('nij,nkjl->nkil', base, _small_rotations(rng, n, 24, 0.6))
    w = rng.dirichlet(np.full(24, 0.3), n)
    lbs = np.einsum('nk,nkij->nij', w, joint)
    # near-opposite rotations: R, R rot_x(pi - e1), R rot_y(pi - e2) with weights a = b + c + d, b, c (normalised):
    # close to R diag(2 b + d, 2 c + d, d), ONE small singular value, cond_2 ~ 0.5 / d up to ~1e4. (A blend of only
    # two near-opposite rotations has a conjugate PAIR of small singular values s; there the adjugate's error
    # grows like 2^-24 / s^2 = 2^-24 cond_2^2, which no bound linear in cond_2 holds: see the module docstring.)
    ex, ey = np.zeros((n, 3)), np.zeros((n, 3))
    ex[:, 0], ey[:, 1] = 1, 1
    rx = _axis_rotations(rng, n, np.pi - rng.uniform(0, 0.01, n), ex)
    ry = _axis_rotations(rng, n, np.pi - rng.uniform(0, 0.01, n), ey)
    b, c = rng.uniform(0.1, 0.3, n), rng.uniform(0.1, 0.3, n)
    d = 10.0 ** rng.uniform(-4.3, -0.5, n)
    w3 = np.stack([b + c + d, b, c], 1)
    w3 /= w3.sum(1, keepdims=True)
    opp = np.einsum('nij,njk->nik', base, w3[:, 0, None, None] * np.eye(3)[None] + w3[:, 1, None, None] * rx +
                    w3[:, 2, None, None] * ry)
    out = {'rotations': pack(rot), 'lbs_blends': pack(lbs), 'near_opposite': pack(opp)}
    # the two-bone case: (1 - t) R + t R rot(axis, pi - eps), t near 1/2: the pair of small singular values, held
    # to the quadratic bound of inv33_ref (drawn last, so that the cases above keep their matrices)
    # (both small singular values ~ max(|1 - 2 t|, eps / 2): cond_2 up to ~1e3)
    ax_rot = _axis_rotations(rng, n, np.pi - 10.0 ** rng.uniform(-2.7, -0.5, n))
    t = 0.5 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, -0.7, n)
    out['two_opposite'] = pack((1 - t)[:, None, None] * base + t[:, None, None] * np.einsum('nij,njk->nik', base, ax_rot))
    return out


def _axis_rotations(rng, n, ang, ax=None):
    ax = rng.standard_normal((n, 3)) if ax is None else ax
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    s, c = np.sin(ang)[:, None, None], np.cos(ang)[:, None, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def _small_rotations(rng, n, k, max_ang):
    return _axis_rotations(rng, n * k, rng.uniform(0, max_ang, n * k)).reshape(n, k, 3, 3)


def inv33_ref(A16, quadratic=False):
    """(float64 inverse (n, 9), bound (n,)) of the 3x3 blocks of (n, 16) float32 transforms: the linear bound of
    the module docstring, or the quadratic one for matrices with two small singular values."""
    A = np.asarray(A16, np.float64).reshape(-1, 4, 4)[:, :3, :3]
    inv = np.linalg.inv(A)
    sv = np.linalg.svd(A, compute_uv=False)
    cond, amax = sv[:, 0] / sv[:, 2], np.abs(inv).max((1, 2))
    if quadratic:
        return inv.reshape(-1, 9), 32 * U24 * cond ** 2 * amax / sv[:, 0] ** 3
    return inv.reshape(-1, 9), 16 * U24 * cond * amax


def inv33_f32(A16):
    """anr_lbs.h inv33 in numpy float32 (uncontracted, the same operation order)."""
    A = np.asarray(A16, F32).reshape(-1, 16)
    a, b, c, d, e, f, g, h, k = (A[:, i] for i in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    c00, c01, c02 = e * k - f * h, c * h - b * k, b * f - c * e
    c10, c11, c12 = f * g - d * k, a * k - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    rd = F32(1.0) / (a * c00 + b * c10 + c * c20)
    return np.stack([c00 * rd, c01 * rd, c02 * rd, c10 * rd, c11 * rd, c12 * rd, c20 * rd, c21 * rd, c22 * rd], 1)


# ---- compaction and alpha_ind ------------------------------------------------------------------------------
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def compact_ref(mask, chunk_min, chunk, ray_offset=0):
    """The ordered compaction: (mask with the chunks' forced bits, ray_off (R + 1), list, total)."""
    mask = np.asarray(mask, np.uint64).copy()
    R = len(mask)
    ray = np.arange(R)
    idx = (np.asarray(chunk_min, np.uint64)[ray // chunk] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    forced = (idx >> 6) == (ray + ray_offset) % chunk
    mask[forced] |= np.uint64(1) << (idx[forced] & 63).astype(np.uint64)
    bits = np.unpackbits(mask.view(np.uint8).reshape(R, 8), axis=1, bitorder='little')
    lst = np.nonzero(bits.reshape(-1))[0].astype(np.int32)
    ray_off = np.concatenate([[0], np.cumsum(bits.sum(1, dtype=np.int64))]).astype(np.int32)
    return mask, ray_off, lst, int(ray_off[-1])


def compact_naive(mask, chunk_min, chunk, ray_offset=0):
    """compact_ref as a plain loop over rays and samples."""
    out_mask, ray_off, lst = [], [0], []
    for ray, m in enumerate(int(v) for v in mask):
        idx = int(chunk_min[ray // chunk]) & 0xFFFFFFFF
        if idx >> 6 == (ray + ray_offset) % chunk:
            m |= 1 << (idx & 63)
        for s in range(64):
            if (m >> s) & 1:
                lst.append(ray * 64 + s)
        out_mask.append(m)
        ray_off.append(len(lst))
    return np.array(out_mask, np.uint64), np.array(ray_off, np.int32), np.array(lst, np.int32), len(lst)


def alpha_ref(sigma, ray_off, chunk, train_th):
    """alpha_ind rows (tpose_nerf_network.py:186-196): sigma' > train_th plus every chunk's argmax (the first index
    of the maximum, -0.0 == +0.0 as torch.argmax compares): (out_row (n'), total)."""
    sigma = np.asarray(sigma, F32)
    flag = sigma > F32(train_th)
    R = len(ray_off) - 1
    for r0 in range(0, R, chunk):
        s0, s1 = int(ray_off[r0]), int(ray_off[min(R, r0 + chunk)])
        if s1 > s0:
            flag[s0 + int(np.argmax(sigma[s0:s1]))] = True
    row = np.where(flag, np.cumsum(flag) - 1, -1).astype(np.int32)
    return row, int(flag.sum())


# ---- compositing -------------------------------------------------------------------------------------------
def composite_ref(raw32, z32):
    """raw2outputs (nerf_net_utils.py:6-36) in float64 on the fp32 raw (R, 64, 4) and z (R, 64): values and
    sum|terms| of (weights, rgb, depth, acc)."""
    raw, z = np.asarray(raw32, np.float64), np.asarray(z32, np.float64)
    al = raw[..., 3]
    T = np.cumprod(np.concatenate([np.ones((len(al), 1)), 1.0 - al + 1e-10], 1), 1)[:, :-1]
    w = al * T
    val = (w, (w[..., None] * raw[..., :3]).sum(1), (w * z).sum(1), w.sum(1))
    mag = (np.abs(w), np.abs(w[..., None] * raw[..., :3]).sum(1), np.abs(w * z).sum(1), np.abs(w).sum(1))
    return val, mag


def composite_bound(mag):
    return 200 * U24 * np.maximum(mag, TINY)


def composite_f32(raw32, z32):
    """The same in numpy float32 (sequential products and sums)."""
    raw, z = np.asarray(raw32, F32), np.asarray(z32, F32)
    al = raw[..., 3]
    p = (F32(1.0) - al) + F32(1e-10)
    T = np.cumprod(np.concatenate([np.ones((len(al), 1), F32), p], 1), 1, dtype=F32)[:, :-1]
    w = al * T
    return (w, (w[..., None] * raw[..., :3]).sum(1, dtype=F32), (w * z).sum(1, dtype=F32), w.sum(1, dtype=F32))


def composite_alphas(R, seed):
    """{name: raw (R, 64, 4) float32}: the alpha cases of the compositing tests, colours random in [0, 1]."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in ('random', 'zeros', 'one_at_0', 'one_at_63', 'almost_one', 'all_ones'):
        raw = rng.uniform(0, 1, (R, 64, 4)).astype(F32)
        if name == 'zeros':
            raw[..., 3] = 0
        elif name == 'one_at_0':
            raw[:, 0, 3] = 1
        elif name == 'one_at_63':
            raw[:, 63, 3] = 1
        elif name == 'almost_one':
            raw[np.arange(R), rng.integers(0, 64, R), 3] = F32(1 - 2.0 ** -24)
            raw[0, :, 3] = F32(1 - 2.0 ** -24)
        elif name == 'all_ones':
            raw[R // 2, :, 3] = 1
        out[name] = raw
    return out
