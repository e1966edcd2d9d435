// anr_testapi_small.hip — test-only C entries to the per-sample math helpers and the small integer / compositing
// kernels of the render path, linked into tests/libanr_testapi.so beside anr_testapi.hip and
// anr_testapi_tchain.hip.
//
// Two groups (mirrored by tests/_small_hooks.py, descriptor sizes checked through anr_test_small_sizeof):
//
//   Helper probes. One elementwise kernel per __device__ helper of anr_common.h (fast_exp, fast_log1p, div_const,
//   softplus_factor_h, embed_feature), anr_mlp_body.h (sincos_fast, softplus100, softplus100_fac, embed<NS>,
//   embed_b<NS>) and anr_lbs.h (inv33): each thread applies the helper to one input and stores what it returns.
//   This file is compiled with the library's CXXFLAGS, so a probe pins the helper AS WRITTEN under the project's
//   flags (contraction pragmas, builtins, -O3). It does not pin each instance the compiler inlined into a fused
//   kernel, whose surrounding code may be scheduled, contracted or vectorised differently; those stay with the
//   parity tests of the fused programs. embed_d (file-local in anr_sdf_train.hip) is reached through its three
//   kernels k_st_embed_tan / k_st_embed_rev6 / k_st_embed_bwd10, launched as the sdf_pdf training step does.
//
//   Small kernels. k_scan_blocks alone, the ordered compaction (k_compact1, or k_count + k_scan_blocks +
//   k_compact), the alpha_ind rows (k_alpha_count1 + k_alpha_scatter1, or k_chunk_argmax + k_flag_count +
//   k_flag_force + k_scan_blocks + k_flag_scatter) and k_composite, with the grids, blocks and path selection of
//   anr_capi.hip (stage_frontend, stage_alpha_ind, stage_composite); `path` may also force either side.
//
// The conventions are anr_testapi.hip's: a precondition that does not hold returns its own negative code and
// launches nothing. Nothing here is part of the shipped library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../animatable_nerf_amd/csrc/anr_mlp_body.h"
#include "../../animatable_nerf_amd/csrc/anr_lbs.h"

namespace anr {
// the embed_d kernels of anr_sdf_train.hip (declared here as anr_kernels.h declares the render kernels)
__global__ void k_st_embed_tan(const float* __restrict__ x, long ldx, const float* __restrict__ xd, long ldxd, int nf,
                               int n, float* out, long ldo, int col0, float scale);
__global__ void k_st_embed_rev6(const float* __restrict__ t, long ldt, const float* __restrict__ td, long ldtd,
                                const float* __restrict__ A0, const float* __restrict__ A4, int n, float* tbar,
                                float* ttbar);
__global__ void k_st_embed_bwd10(const float* __restrict__ x, long ldx, const float* __restrict__ G, long ldg, int n,
                                 float* xbar, long ldxb);
}  // namespace anr

using namespace anr;

namespace {

enum { P_SINCOS = 0, P_SP_FAC = 1, P_SP = 2, P_EXP = 3, P_LOG1P = 4, P_SPF_H = 5, P_DIV = 6, P_COUNT = 7 };

// o0[i] (and o1[i] for the helpers with two results) = helper(x[i]); p0, p1: div_const's b and rb
template <int WHICH>
__global__ __launch_bounds__(256) void k_probe1(const float* __restrict__ x, float* __restrict__ o0,
                                                float* __restrict__ o1, long n, float p0, float p1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  if constexpr (WHICH == P_SINCOS) {
    float s, c;
    sincos_fast(v, s, c);
    o0[i] = s;
    o1[i] = c;
  } else if constexpr (WHICH == P_SP_FAC) {
    float fac;
    o0[i] = softplus100_fac(v, fac);
    o1[i] = fac;
  } else if constexpr (WHICH == P_SP) {
    o0[i] = softplus100(v);
  } else if constexpr (WHICH == P_EXP) {
    o0[i] = fast_exp(v);
  } else if constexpr (WHICH == P_LOG1P) {
    o0[i] = fast_log1p(v);
  } else if constexpr (WHICH == P_SPF_H) {
    o0[i] = softplus_factor_h(v);
  } else {
    o0[i] = div_const(v, p0, p1);
  }
}

// A (n, 16) row-major blended transforms -> Ri (n, 9)
__global__ __launch_bounds__(256) void k_probe_inv33(const float* __restrict__ A, float* __restrict__ Ri, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float Ab[16], R[9];
  for (int m = 0; m < 16; ++m) Ab[m] = A[i * 16 + m];
  inv33(Ab, R);
  for (int m = 0; m < 9; ++m) Ri[i * 9 + m] = R[m];
}

// out (n, 64): feature f of gamma_nfreq(x_i), f = 0..63 (features past 3 + 6 nfreq included)
__global__ __launch_bounds__(256) void k_probe_embed_feature(const float* __restrict__ x, int nfreq,
                                                             float* __restrict__ out, long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * 64) return;
  const long i = e >> 6;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  out[e] = embed_feature(p, (int)(e & 63), nfreq);
}

// the fused kernels' lane layout: 16 points per wave, g = lane >> 4; out (n, 4, NS), [i][g][s] = e[s]
template <int NS>
__global__ __launch_bounds__(256) void k_probe_embed(const float* __restrict__ x, int nfreq, float* __restrict__ out,
                                                     long n) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int g = (int)(t & 63) >> 4;
  const long i = (t >> 6) * 16 + (t & 15);
  if (i >= n) return;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  float e[NS];
  embed<NS>(p, g, nfreq, e);
  for (int s = 0; s < NS; ++s) out[(i * 4 + g) * NS + s] = e[s];
}

// the same layout for the bf16 fragment order: out (n, 4, 8 NS), [i][h][j] = e[j]. embed_b holds a wave-wide
// ballot, so whole waves only (n is a multiple of 16, checked by the entry) and no early return
template <int NS>
__global__ __launch_bounds__(256) void k_probe_embed_b(const float* __restrict__ x, int nfreq, float* __restrict__ out,
                                                       long n) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int h = (int)(t & 63) >> 4;
  const long i = (t >> 6) * 16 + (t & 15);
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  float e[8 * NS];
  embed_b<NS>(p, h, nfreq, e);
  for (int j = 0; j < 8 * NS; ++j) out[(i * 4 + h) * (8 * NS) + j] = e[j];
}

}  // namespace

extern "C" {

// the codes of anr_testapi.hip that these entries return
enum {
  ANR_T_OK = 0,
  ANR_T_NULL = -100,   // a required pointer is NULL
  ANR_T_SHAPE = -101,  // counts / selectors out of range
  ANR_T_SLAB = -107,   // a buffer holds too few elements
  ANR_T_HIP = -109,    // a HIP error at the launch
};

static int launched() { return hipGetLastError() == hipSuccess ? ANR_T_OK : ANR_T_HIP; }
static const long kMaxElems = 1L << 28;  // keeps every grid and every int index of the probes in range

// ---------------------------------------------------------------------------------------------------
// helper probes
// ---------------------------------------------------------------------------------------------------
// which: 0 sincos_fast (o0 sin, o1 cos), 1 softplus100_fac (o0 h, o1 fac), 2 softplus100, 3 fast_exp,
// 4 fast_log1p, 5 softplus_factor_h, 6 div_const(x, p0 = b, p1 = rb)
int anr_test_probe1(int which, const float* x, float* o0, float* o1, long n, float p0, float p1, hipStream_t s) {
  if (which < 0 || which >= P_COUNT || n < 1 || n > kMaxElems) return ANR_T_SHAPE;
  if (!x || !o0 || ((which == P_SINCOS || which == P_SP_FAC) && !o1)) return ANR_T_NULL;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (which) {
    case P_SINCOS: hipLaunchKernelGGL(k_probe1<P_SINCOS>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    case P_SP_FAC: hipLaunchKernelGGL(k_probe1<P_SP_FAC>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    case P_SP: hipLaunchKernelGGL(k_probe1<P_SP>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    case P_EXP: hipLaunchKernelGGL(k_probe1<P_EXP>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    case P_LOG1P: hipLaunchKernelGGL(k_probe1<P_LOG1P>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    case P_SPF_H: hipLaunchKernelGGL(k_probe1<P_SPF_H>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
    default: hipLaunchKernelGGL(k_probe1<P_DIV>, grid, block, 0, s, x, o0, o1, n, p0, p1); break;
  }
  return launched();
}

int anr_test_probe_inv33(const float* A, float* Ri, long n, hipStream_t s) {
  if (n < 1 || n > kMaxElems / 16) return ANR_T_SHAPE;
  if (!A || !Ri) return ANR_T_NULL;
  hipLaunchKernelGGL(k_probe_inv33, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, Ri, n);
  return launched();
}

// which: 0 embed_feature (out (n, 64); nfreq 4, 6, 10), 1 embed<NS> (nfreq 10 -> NS 16, 4 -> NS 8; out
// (n, 4, NS)), 2 embed_b<NS> (nfreq 10 and 6 -> NS 2, 4 -> NS 1; out (n, 4, 8 NS); n a multiple of 16). The
// (NS, nfreq) pairs are the ones the kernels instantiate.
int anr_test_probe_embed(int which, const float* x, int nfreq, float* out, long n, hipStream_t s) {
  if (which < 0 || which > 2 || n < 1 || n > kMaxElems / 64) return ANR_T_SHAPE;
  if (!x || !out) return ANR_T_NULL;
  const dim3 block(256);
  if (which == 0) {
    if (nfreq != 4 && nfreq != 6 && nfreq != 10) return ANR_T_SHAPE;
    hipLaunchKernelGGL(k_probe_embed_feature, dim3((unsigned)((n * 64 + 255) / 256)), block, 0, s, x, nfreq, out, n);
    return launched();
  }
  const dim3 grid((unsigned)(((n + 15) / 16 * 64 + 255) / 256));  // a wave per 16 points
  if (which == 1) {
    if (nfreq == 10) hipLaunchKernelGGL(k_probe_embed<16>, grid, block, 0, s, x, nfreq, out, n);
    else if (nfreq == 4) hipLaunchKernelGGL(k_probe_embed<8>, grid, block, 0, s, x, nfreq, out, n);
    else return ANR_T_SHAPE;
    return launched();
  }
  if (n % 64 != 0) return ANR_T_SHAPE;  // whole 256-thread blocks: every lane of every wave holds a point
  if (nfreq == 10 || nfreq == 6) hipLaunchKernelGGL(k_probe_embed_b<2>, grid, block, 0, s, x, nfreq, out, n);
  else if (nfreq == 4) hipLaunchKernelGGL(k_probe_embed_b<1>, grid, block, 0, s, x, nfreq, out, n);
  else return ANR_T_SHAPE;
  return launched();
}

// embed_d through its kernels, launched as anr_sdf_train.hip launches them (256-thread blocks)
int anr_test_embed_tan(const float* x, long ldx, const float* xd, long ldxd, int nf, int n, float* out, long ldo,
                       int col0, float scale, hipStream_t s) {
  if ((nf != 6 && nf != 10) || n < 1 || n > (1 << 20) || col0 < 0) return ANR_T_SHAPE;
  if (!x || !xd || !out) return ANR_T_NULL;
  if (ldx < 3 || ldxd < 3 || ldo < col0 + 3 + 6 * nf) return ANR_T_SLAB;
  const int F = 3 + 6 * nf;
  hipLaunchKernelGGL(k_st_embed_tan, dim3((unsigned)(((long)n * F + 255) / 256)), dim3(256), 0, s, x, ldx, xd, ldxd, nf,
                     n, out, ldo, col0, scale);
  return launched();
}

// A0 (2n, 40), A4 (2n, 256), tbar (n, 4) accumulated into, ttbar (n, 4) or NULL
int anr_test_embed_rev6(const float* t, long ldt, const float* td, long ldtd, const float* A0, const float* A4, int n,
                        float* tbar, float* ttbar, hipStream_t s) {
  if (n < 1 || n > (1 << 20)) return ANR_T_SHAPE;
  if (!t || !td || !A0 || !A4 || !tbar) return ANR_T_NULL;
  if (ldt < 3 || ldtd < 3) return ANR_T_SLAB;
  hipLaunchKernelGGL(k_st_embed_rev6, dim3((n + 255) / 256), dim3(256), 0, s, t, ldt, td, ldtd, A0, A4, n, tbar, ttbar);
  return launched();
}

int anr_test_embed_bwd10(const float* x, long ldx, const float* G, long ldg, int n, float* xbar, long ldxb,
                         hipStream_t s) {
  if (n < 1 || n > (1 << 20)) return ANR_T_SHAPE;
  if (!x || !G || !xbar) return ANR_T_NULL;
  if (ldx < 3 || ldg < 63 || ldxb < 3) return ANR_T_SLAB;
  hipLaunchKernelGGL(k_st_embed_bwd10, dim3((n + 255) / 256), dim3(256), 0, s, x, ldx, G, ldg, n, xbar, ldxb);
  return launched();
}

// ---------------------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------------------
// sums (nb) -> exclusive offsets in place, *total = the sum
int anr_test_scan_blocks(int* sums, int nb, int* total, hipStream_t s) {
  if (nb < 1) return ANR_T_SHAPE;
  if (!sums || !total) return ANR_T_NULL;
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, sums, nb, total);
  return launched();
}

// path: 0 as stage_frontend selects (n_rays <= 1024: k_compact1), 1 k_count + k_scan_blocks + k_compact,
// 2 k_compact1 (n_rays <= 1024)
struct anr_test_compact {
  int n_rays, chunk, ray_offset, path;
  unsigned long long* mask;             // (n_rays) in / out
  const unsigned long long* chunk_min;  // (ceil(n_rays / chunk))
  int* ray_off;                         // (n_rays + 1)
  int* block_sum;                       // (ceil(n_rays / 256))
  int* list;                            // (list_cap >= 64 n_rays)
  int* total;
  long list_cap;
};

int anr_test_compact_run(const anr_test_compact* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  if (d->n_rays < 1 || d->n_rays > (1 << 24) || d->chunk < 1 || d->ray_offset < 0 || d->path < 0 || d->path > 2)
    return ANR_T_SHAPE;
  if (d->path == 2 && d->n_rays > 1024) return ANR_T_SHAPE;
  if (!d->mask || !d->chunk_min || !d->ray_off || !d->block_sum || !d->list || !d->total) return ANR_T_NULL;
  if (d->list_cap < 64L * d->n_rays) return ANR_T_SLAB;
  const int R = d->n_rays;
  CompactArgs ca{};
  ca.n_rays = R; ca.chunk = d->chunk; ca.ray_offset = d->ray_offset;
  ca.mask = (uint64_t*)d->mask; ca.chunk_min = (const uint64_t*)d->chunk_min;
  ca.ray_off = d->ray_off; ca.block_sum = d->block_sum; ca.list = d->list;
  if (d->path == 2 || (d->path == 0 && R <= 1024)) {
    hipLaunchKernelGGL(k_compact1, dim3(1), dim3(1024), 0, s, ca, d->total);
    return launched();
  }
  const int nb = (R + 255) / 256;
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(256), 0, s, ca);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, ca.block_sum, nb, d->total);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_compact, dim3((R + 3) / 4), dim3(256), 0, s, ca);
  return launched();
}

// path: 0 as stage_alpha_ind selects without a ray split (one chunk and <= 64 blocks of 1024 sample slots: the
// two-launch path), 1 the general path, 2 the two-launch path (its conditions hold, ray_offset 0). chunk_max is
// preset to 0 by the caller (k_prep in the library).
struct anr_test_alpha {
  int n_rays, chunk, ray_offset, path;
  float train_th;
  int pad0;
  const int* ray_off;             // (n_rays + 1), global
  const int* n_kept;              // device: n'
  const float* sigma;             // (n')
  unsigned long long* chunk_max;  // (nchunks), 0
  unsigned char* flags;           // (64 n_rays)
  int* block_sum;                 // (ceil(64 n_rays / 1024))
  int* out_row;                   // (64 n_rays)
  const int* list;
  const unsigned long long* mask;
  int* total;
};

int anr_test_alpha_run(const anr_test_alpha* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  if (d->n_rays < 1 || d->n_rays > (1 << 24) || d->chunk < 1 || d->ray_offset < 0 || d->path < 0 || d->path > 2)
    return ANR_T_SHAPE;
  const int R = d->n_rays;
  const int nch = (R + d->chunk - 1) / d->chunk;
  const int nb2 = (int)(((long)R * 64 + 1023) / 1024);
  const bool one = nch == 1 && nb2 <= 64 && d->ray_offset == 0;
  if (d->path == 2 && !one) return ANR_T_SHAPE;
  if (!d->ray_off || !d->n_kept || !d->sigma || !d->chunk_max || !d->flags || !d->block_sum || !d->out_row ||
      !d->list || !d->mask || !d->total)
    return ANR_T_NULL;
  AlphaArgs aa{};
  aa.n_rays = R; aa.chunk = d->chunk;
  aa.ray_off = d->ray_off; aa.n_kept = d->n_kept; aa.sigma = d->sigma;
  aa.chunk_max = (uint64_t*)d->chunk_max;
  aa.train_th = d->train_th;
  aa.flags = d->flags; aa.block_sum = d->block_sum; aa.out_row = d->out_row;
  aa.list = d->list; aa.mask = (const uint64_t*)d->mask;
  aa.ray_offset = d->ray_offset;
  if (d->path == 2 || (d->path == 0 && one)) {
    hipLaunchKernelGGL(k_alpha_count1, dim3(nb2), dim3(256), 0, s, aa);
    if (launched() != ANR_T_OK) return ANR_T_HIP;
    hipLaunchKernelGGL(k_alpha_scatter1, dim3(nb2), dim3(256), 0, s, aa, d->total);
    return launched();
  }
  hipLaunchKernelGGL(k_chunk_argmax, dim3(nch, 16), dim3(256), 0, s, aa);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_flag_count, dim3(nb2), dim3(256), 0, s, aa);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_flag_force, dim3((nch + 255) / 256), dim3(256), 0, s, aa, nch);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, aa.block_sum, nb2, d->total);
  if (launched() != ANR_T_OK) return ANR_T_HIP;
  hipLaunchKernelGGL(k_flag_scatter, dim3(nb2), dim3(256), 0, s, aa);
  return launched();
}

struct anr_test_composite {
  int n_rays, pad0;
  const float* raw;     // (n_rays, 64, 4), 16-B aligned
  const float* near_;   // (n_rays)
  const float* far_;    // (n_rays)
  const float* t_rand;  // (n_rays, 64) or NULL
  float* rgb;           // (n_rays, 3)
  float* acc;           // (n_rays)
  float* depth;         // (n_rays)
  float* weights;       // (n_rays, 64) or NULL
};

int anr_test_composite_run(const anr_test_composite* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  if (d->n_rays < 1 || d->n_rays > (1 << 24)) return ANR_T_SHAPE;
  if (!d->raw || !d->near_ || !d->far_ || !d->rgb || !d->acc || !d->depth) return ANR_T_NULL;
  if (((uintptr_t)d->raw & 15) != 0) return ANR_T_SHAPE;
  CompositeArgs co{};
  co.raw = (const float4*)d->raw; co.near_ = d->near_; co.far_ = d->far_; co.t_rand = d->t_rand;
  co.n_rays = d->n_rays;
  co.rgb = d->rgb; co.acc = d->acc; co.depth = d->depth; co.weights = d->weights;
  hipLaunchKernelGGL(k_composite, dim3((d->n_rays + 3) / 4), dim3(256), 0, s, co);
  return launched();
}

// sizeof of the descriptors, numbered on from anr_test_tchain_sizeof's 5..6: 7 compaction, 8 alpha_ind,
// 9 composite
int anr_test_small_sizeof(int which) {
  switch (which) {
    case 7: return (int)sizeof(anr_test_compact);
    case 8: return (int)sizeof(anr_test_alpha);
    case 9: return (int)sizeof(anr_test_composite);
    default: return -1;
  }
}

}  // extern "C"
