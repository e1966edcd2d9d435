// anr_lbw.hip — per-sample kernels of the aligned_aninerf_lbw render path
// (aligned_aninerf_lbw_network.py:90-147 under tpose_renderer.py:159-186).
//
//   k_lbw_wnorm   effective weights v * (g / |v|_row) of the 14 weight-normed layers (9 density, 5 colour)
//   k_lbw_fold    per-frame folded biases: bw_latent into bw_linears.0/.5 (pose and T-pose pass), color_latent
//                 into the colour net's lin3
//   k_lbw_gather  kept sample -> pose point / direction / dist, init_pbw from the front-end's KNN record,
//                 gamma_10(pose point) rows
//   k_lbw_warp    pbw = softmax(log(init_pbw + 1e-9) + y), LBS pose -> T -> big pose for the point and the
//                 direction, the inputs of the density / colour nets, the second search's queries
//   k_lbw_tbw_in  init_tbw from the second search's KNN records
//   k_lbw_tbw     tbw = softmax(log(init_tbw + 1e-9) + y)
//   k_lbw_raw     alpha = 1 - exp(-relu(y0) dist), sigmoid rgb, the per-chunk tbounds mask, scatter, and the
//                 masked alpha in compact order for the alpha_ind stage
// The searches are k_sdf_front (anr_sdf.hip), the GEMMs between the kernels run on anr_gemm.hip / anr_lgemm.hip
// (anr_lbw_capi.hip drives the sequence).
#include "anr_common.h"
#include "anr_lbs.h"
#include "anr_lbw.h"

#pragma clang fp contract(off)

namespace anr {

// weight norm (nn.utils.weight_norm, dim 0): one block per output row of the 14 layers
__global__ __launch_bounds__(256) void k_lbw_wnorm(LbwTensors T, float* wimg) {
  const float* const* t = T.t;
  int row = blockIdx.x, L = 0;
  while (L < LBW_NUM_WN - 1 && row >= lbw_wn_layer(L).out) { row -= lbw_wn_layer(L).out; ++L; }
  const LbwWnLayer d = lbw_wn_layer(L);
  const float* v = t[d.v] + (size_t)row * d.in;
  float s = 0.f;
  for (int k = threadIdx.x; k < d.in; k += 256) s += v[k] * v[k];
  __shared__ float sh[256];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  const float scale = t[d.g][row] / sqrtf(sh[0]);
  float* o = wimg + d.off + (size_t)row * d.in;
  for (int k = threadIdx.x; k < d.in; k += 256) o[k] = v[k] * scale;
}

// fold[w * 256 + n], w = 0, 1, 3, 4: bias of bw_linears.{0, 5} + W[:, 63:191] bw_latent[row], row = latent_index + 1
// (w < 2, the pose pass) or 0 (w > 2, the T-pose pass); w = 2: colour lin3 bias + W3[:, 256:384] color_latent[latent_index]
__global__ __launch_bounds__(256) void k_lbw_fold(LbwTensors T, const float* wimg, const int64_t* li, float* fold) {
  const float* const* t = T.t;
  const int which = blockIdx.x, n = threadIdx.x;
  float acc;
  if (which != 2) {
    const int l = (which == 1 || which == 4) ? 5 : 0;
    const int in_ch = l == 0 ? 191 : 447;
    const float* W = t[LBW_BWLIN0 + 2 * l] + (size_t)n * in_ch;
    const float* lat = t[LBW_BW_LAT] + (size_t)(which < 2 ? li[0] + 1 : 0) * 128;
    acc = t[LBW_BWLIN0 + 2 * l + 1][n];
    for (int q = 0; q < 128; ++q) acc = fmaf(W[63 + q], lat[q], acc);
  } else {
    const LbwWnLayer d = lbw_wn_layer(12);
    const float* W = wimg + d.off + (size_t)n * 384;
    const float* lat = t[LBW_COLOR_LAT] + (size_t)li[0] * 128;
    acc = t[d.v - 2][n];
    for (int q = 0; q < 128; ++q) acc = fmaf(W[256 + q], lat[q], acc);
  }
  fold[which * 256 + n] = acc;
}

// sample_blend_closest_points' blend of one KNN record (k_sdf_prep's summation order)
__device__ __forceinline__ void lbw_knn_blend(const uint32_t* __restrict__ knn, size_t rec_i,
                                              const float* __restrict__ weights, float* __restrict__ out) {
  const uint4* rec = (const uint4*)(knn + rec_i * 8);
  const uint4 r0 = rec[0], r1 = rec[1];
  const float w[5] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w),
                      __uint_as_float(r1.x)};
  const int idx[5] = {(int)(r1.y & 0xffff), (int)(r1.y >> 16), (int)(r1.z & 0xffff), (int)(r1.z >> 16), (int)r1.w};
  for (int l = 0; l < 24; ++l) {
    float acc = weights[idx[0] * 24 + l] * w[0];
    for (int k = 1; k < 5; ++k) acc = acc + weights[idx[k] * 24 + l] * w[k];
    out[l] = acc;
  }
}

// softmax(log(init + 1e-9) + y) over the 24 joints (calculate_neural_blend_weights :55-58)
__device__ __forceinline__ void lbw_softmax(const float* __restrict__ init, const float* __restrict__ y, float bw[24]) {
  float m = -INFINITY;
  for (int j = 0; j < 24; ++j) {
    bw[j] = logf(init[j] + 1e-9f) + y[j];
    m = fmaxf(m, bw[j]);
  }
  float s = 0.f;
  for (int j = 0; j < 24; ++j) {
    bw[j] = expf(bw[j] - m);
    s = s + bw[j];
  }
  for (int j = 0; j < 24; ++j) bw[j] = bw[j] / s;
}

// thread per kept sample, then the gamma_10 rows written coalesced
__global__ __launch_bounds__(256) void k_lbw_gather(LbwPointArgs a) {
  __shared__ float sp[256][4];
  const int i0 = blockIdx.x * 256, i = i0 + threadIdx.x;
  if (i < a.cnt) {
    const int pid = a.list[a.b0 + i];
    const int ray = pid >> 6, s = pid & 63;
    float z, dist, pts[3], p[3], pd[3];
    sample_point(a.ray_o, a.ray_d, a.near_, a.far_, a.t_rand, ray, s, 64, z, dist, pts);
    world_to_pose(pts, a.R, a.Th, p);
    const float* d = a.ray_d + 3 * ray;  // world_dirs_to_pose_dirs: d @ R
    for (int j = 0; j < 3; ++j) pd[j] = fmaf(d[2], a.R[6 + j], fmaf(d[1], a.R[3 + j], d[0] * a.R[j]));
    float* pt = a.ptp + (size_t)i * 8;
    pt[0] = p[0]; pt[1] = p[1]; pt[2] = p[2];
    pt[3] = pd[0]; pt[4] = pd[1]; pt[5] = pd[2];
    pt[6] = dist; pt[7] = 0.f;
    sp[threadIdx.x][0] = p[0]; sp[threadIdx.x][1] = p[1]; sp[threadIdx.x][2] = p[2];
    lbw_knn_blend(a.knn, (size_t)pid, a.weights, a.ibw + (size_t)i * 24);
  }
  __syncthreads();
  if (!a.fused) sdf_rows_store<64>(a.Gx, i0, a.cnt, [&](int r, int c) { return c < 63 ? embed_feature(sp[r], c, 10) : 0.f; });
}

// thread per kept sample for pbw and the LBS, then the network inputs written coalesced
__global__ __launch_bounds__(256) void k_lbw_warp(LbwPointArgs a) {
  __shared__ float sp[256][8];  // tpose xyz, -, tpose_dir xyz, -
  const int i0 = blockIdx.x * 256, i = i0 + threadIdx.x;
  if (i < a.cnt) {
    float bw[24];
    if (a.fused) {
      for (int j = 0; j < 24; ++j) bw[j] = a.Ybw[(size_t)i * 24 + j];
    } else {
      lbw_softmax(a.ibw + (size_t)i * 24, a.Ybw + (size_t)i * 24, bw);
    }
    if (a.pbw_rows) {  // NULL in an image-only call: no rows are kept
      float* prow = a.pbw_rows + (size_t)(a.b0 + i) * 24;
      for (int j = 0; j < 24; ++j) prow[j] = bw[j];
    }
    const float* pt = a.ptp + (size_t)i * 8;
    float Ab[16], Bb[16], Ri[9];
    blend16(bw, a.A, Ab);
    blend16(bw, a.bigA, Bb);
    inv33(Ab, Ri);
    const float y[3] = {pt[0] - Ab[3], pt[1] - Ab[7], pt[2] - Ab[11]};
    float tp[3], td[3], bp[3], bd[3];
    for (int r = 0; r < 3; ++r) {
      tp[r] = (Ri[3 * r] * y[0] + Ri[3 * r + 1] * y[1]) + Ri[3 * r + 2] * y[2];
      td[r] = (Ri[3 * r] * pt[3] + Ri[3 * r + 1] * pt[4]) + Ri[3 * r + 2] * pt[5];
    }
    for (int r = 0; r < 3; ++r) {
      bp[r] = ((Bb[4 * r] * tp[0] + Bb[4 * r + 1] * tp[1]) + Bb[4 * r + 2] * tp[2]) + Bb[4 * r + 3];
      bd[r] = (Bb[4 * r] * td[0] + Bb[4 * r + 1] * td[1]) + Bb[4 * r + 2] * td[2];
    }
    for (int r = 0; r < 3; ++r) {
      a.tp3[(size_t)i * 3 + r] = bp[r];
      sp[threadIdx.x][r] = bp[r];
      sp[threadIdx.x][4 + r] = bd[r];
    }
  }
  __syncthreads();
  const float sqrt2 = 1.41421356237309515f;
  const int rows = min(256, a.cnt - i0);
  if (!a.fused) {
    sdf_rows_store<40>(a.Xs0, i0, a.cnt, [&](int r, int c) { return c < 39 ? embed_feature(sp[r], c, 6) : 0.f; });
    for (int f = threadIdx.x; f < rows * 39; f += 256) {
      const int r = f / 39, c = f - r * 39;
      a.X4[(size_t)(i0 + r) * 256 + 217 + c] = embed_feature(sp[r], c, 6) / sqrt2;
    }
  }
  // C0: tpose (0..2), gamma_4(tpose_dir) (3..29)
  sdf_rows_store<40>(a.C0, i0, a.cnt,
                     [&](int r, int c) { return c < 3 ? sp[r][c] : c < 30 ? embed_feature(sp[r] + 4, c - 3, 4) : 0.f; });
  if (a.full && !a.fused) sdf_rows_store<64>(a.Gx, i0, a.cnt, [&](int r, int c) { return c < 63 ? embed_feature(sp[r], c, 10) : 0.f; });
}

__global__ __launch_bounds__(256) void k_lbw_tbw_in(LbwPointArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cnt) return;
  lbw_knn_blend(a.knn2, (size_t)i, a.weights, a.ibw + (size_t)i * 24);
}

__global__ __launch_bounds__(256) void k_lbw_tbw(LbwPointArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cnt) return;
  float bw[24];
  if (a.fused) {
    for (int j = 0; j < 24; ++j) bw[j] = a.Ybw[(size_t)i * 24 + j];
  } else {
    lbw_softmax(a.ibw + (size_t)i * 24, a.Ybw + (size_t)i * 24, bw);
  }
  float* trow = a.tbw_rows + (size_t)(a.b0 + i) * 24;
  for (int j = 0; j < 24; ++j) trow[j] = bw[j];
}

// raw2alpha (TPoseHuman.forward :249-251), sigmoid rgb, raw zeroed outside the chunk's widened tbounds (:124-130)
__global__ __launch_bounds__(256) void k_lbw_raw(LbwPointArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.cnt) return;
  const int pid = a.list[a.b0 + i];
  const int ray = pid >> 6;
  const float dens = a.Y8[(size_t)i * 264];
  const float dist = a.ptp[(size_t)i * 8 + 6];
  const float alpha = 1.0f - expf(-fmaxf(dens, 0.f) * dist);
  const float* yc = a.Yc + (size_t)i * 4;
  float4 raw = make_float4(1.0f / (1.0f + expf(-yc[0])), 1.0f / (1.0f + expf(-yc[1])), 1.0f / (1.0f + expf(-yc[2])),
                           alpha);
  const float* tb = a.tbtab + (size_t)(ray / a.chunk) * 6;
  const float* c = a.C0 + (size_t)i * 40;
  bool inside = true;
  for (int r = 0; r < 3; ++r) inside = inside && c[r] > tb[r] && c[r] < tb[3 + r];
  if (!inside) raw = make_float4(0.f, 0.f, 0.f, 0.f);
  a.raw[pid] = raw;
  if (a.sigma) a.sigma[a.b0 + i] = raw.w;
}

}  // namespace anr
