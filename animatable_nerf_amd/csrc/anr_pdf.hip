// anr_pdf.hip — per-sample kernels of the aligned_aninerf_pdf render path
// (aligned_aninerf_pdf_network.py:97-138 under tpose_renderer.py:159-186).
//
//   k_pdf_fold  per-frame folded biases: poses into resd_linears.0/.5, color_latent into the colour net's lin3
//   k_pdf_warp  kept sample -> pose point / direction / dist, pbw from the front-end's KNN record, LBS pose -> T ->
//               big pose for the point and the direction (:66-90): the displacement program's point row and the
//               direction part of the colour input row
//   k_pdf_alpha_out  get_alpha's scatter of the raw density
//   k_pdf_mid   exact-fp32 path only: resd = 0.05 tanh(y), tpose = init_bigpose + resd, the density net's input
//               rows (the fused displacement program does this in its epilogue, anr_mlp_body.h V = 23 / 33)
// The weight norm is k_lbw_wnorm (the tensor table of tpose_human is aligned_aninerf_lbw's), the search is
// k_sdf_front, the raw assembly k_lbw_raw (anr_pdf_capi.hip drives the sequence).
#include "anr_common.h"
#include "anr_lbs.h"
#include "anr_pdf.h"

#pragma clang fp contract(off)

namespace anr {

// fold[0:256] = resd_linears.0 bias + W0[:, 63:135] poses; fold[256:512] = same for .5 (391 inputs);
// fold[512:768] = colour lin3 bias + W3[:, 256:384] color_latent[latent_index]
__global__ __launch_bounds__(256) void k_pdf_fold(LbwTensors T, const float* wimg, const float* poses, const int64_t* li,
                                                  float* fold) {
  const float* const* t = T.t;
  const int which = blockIdx.x, n = threadIdx.x;
  float acc;
  if (which < 2) {
    const int l = which == 0 ? 0 : 5;
    const int in_ch = which == 0 ? 135 : 391;
    const float* W = t[PDF_RLIN0 + 2 * l] + (size_t)n * in_ch;
    acc = t[PDF_RLIN0 + 2 * l + 1][n];
    for (int q = 0; q < 72; ++q) acc = fmaf(W[63 + q], poses[q], acc);
  } else {
    const LbwWnLayer d = lbw_wn_layer(12);
    const float* W = wimg + d.off + (size_t)n * 384;
    const float* lat = t[PDF_COLOR_LAT] + (size_t)li[0] * 128;
    acc = t[d.v - 2][n];
    for (int q = 0; q < 128; ++q) acc = fmaf(W[256 + q], lat[q], acc);
  }
  fold[which * 256 + n] = acc;
}

// thread per kept sample (k_sdf_prep's arithmetic, plus dist), then the rows written coalesced
__global__ __launch_bounds__(256) void k_pdf_warp(PdfPointArgs a) {
  __shared__ float sp[256][8];  // init_bigpose xyz, -, big-pose dir xyz, -
  const int i0 = blockIdx.x * 256, i = i0 + threadIdx.x;
  if (i < a.cnt) {
    const int pid = a.list[a.b0 + i];
    const int ray = pid >> 6, s = pid & 63;
    float z, dist = 0.f, pts[3], p[3], pd[3] = {0.f, 0.f, 0.f};
    if (a.wpts) {  // get_alpha: pose_pts of the chunk's (n_pts, 3) product, no direction
      world_to_pose_pt(a.wpts, pid, a.n_pts, a.n_pts, a.R, a.Th, p);
    } else {
      sample_point(a.ray_o, a.ray_d, a.near_, a.far_, a.t_rand, ray, s, 64, z, dist, pts);
      world_to_pose(pts, a.R, a.Th, p);
      const float* d = a.ray_d + 3 * ray;  // world_dirs_to_pose_dirs: d @ R
      for (int j = 0; j < 3; ++j) pd[j] = fmaf(d[2], a.R[6 + j], fmaf(d[1], a.R[3 + j], d[0] * a.R[j]));
    }
    // sample_blend_closest_points' blend of the KNN record (k_sdf_prep's summation order)
    const uint4* rec = (const uint4*)(a.knn + (size_t)pid * 8);
    const uint4 r0 = rec[0], r1 = rec[1];
    const float w[5] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w),
                        __uint_as_float(r1.x)};
    const int idx[5] = {(int)(r1.y & 0xffff), (int)(r1.y >> 16), (int)(r1.z & 0xffff), (int)(r1.z >> 16), (int)r1.w};
    float bw[24];
    for (int l = 0; l < 24; ++l) {
      float acc = a.weights[idx[0] * 24 + l] * w[0];
      for (int k = 1; k < 5; ++k) acc = acc + a.weights[idx[k] * 24 + l] * w[k];
      bw[l] = acc;
    }
    float Ab[16], Bb[16], Ri[9];
    blend16(bw, a.A, Ab);
    blend16(bw, a.bigA, Bb);
    inv33(Ab, Ri);
    const float y[3] = {p[0] - Ab[3], p[1] - Ab[7], p[2] - Ab[11]};
    float tp[3], td[3], bp[3], bd[3];
    for (int r = 0; r < 3; ++r) {
      tp[r] = (Ri[3 * r] * y[0] + Ri[3 * r + 1] * y[1]) + Ri[3 * r + 2] * y[2];
      td[r] = (Ri[3 * r] * pd[0] + Ri[3 * r + 1] * pd[1]) + Ri[3 * r + 2] * pd[2];
    }
    for (int r = 0; r < 3; ++r) {
      bp[r] = ((Bb[4 * r] * tp[0] + Bb[4 * r + 1] * tp[1]) + Bb[4 * r + 2] * tp[2]) + Bb[4 * r + 3];
      bd[r] = (Bb[4 * r] * td[0] + Bb[4 * r + 1] * td[1]) + Bb[4 * r + 2] * td[2];
    }
    float* pt = a.ptp + (size_t)i * 8;
    pt[0] = bp[0]; pt[1] = bp[1]; pt[2] = bp[2];
    pt[3] = bd[0]; pt[4] = bd[1]; pt[5] = bd[2];
    pt[6] = dist; pt[7] = 0.f;
    for (int r = 0; r < 3; ++r) {
      sp[threadIdx.x][r] = bp[r];
      sp[threadIdx.x][4 + r] = bd[r];
    }
  }
  __syncthreads();
  // C0: 0..2 init_bigpose until the displacement step writes tpose there, gamma_4(big-pose dir) (3..29)
  sdf_rows_store<40>(a.C0, i0, a.cnt,
                     [&](int r, int c) { return c < 3 ? sp[r][c] : c < 30 ? embed_feature(sp[r] + 4, c - 3, 4) : 0.f; });
  // gamma_10 rows for the layer-GEMM displacement MLP (the fused program forms them on chip: Gr NULL)
  if (a.Gr) sdf_rows_store<64>(a.Gr, i0, a.cnt, [&](int r, int c) { return c < 63 ? embed_feature(sp[r], c, 10) : 0.f; });
}

// resd = 0.05 tanh(y); tpose = init_bigpose + resd -> C0 columns 0..2; gamma_6(tpose) -> Xs0 and X4[:, 217:] / sqrt(2)
__global__ __launch_bounds__(256) void k_pdf_mid(PdfPointArgs a) {
  __shared__ float sp[256][4];
  const int i0 = blockIdx.x * 256, i = i0 + threadIdx.x;
  if (i < a.cnt) {
    const float* pt = a.ptp + (size_t)i * 8;
    const float* y = a.Yr + (size_t)i * 4;
    for (int r = 0; r < 3; ++r) {
      const float rs = 0.05f * tanhf(y[r]);
      if (a.resd_rows) a.resd_rows[(size_t)(a.b0 + i) * 3 + r] = rs;
      const float t = pt[r] + rs;
      sp[threadIdx.x][r] = t;
      a.C0[(size_t)i * 40 + r] = t;
    }
  }
  __syncthreads();
  const float sqrt2 = 1.41421356237309515f;
  const int rows = min(256, a.cnt - i0);
  sdf_rows_store<40>(a.Xs0, i0, a.cnt, [&](int r, int c) { return c < 39 ? embed_feature(sp[r], c, 6) : 0.f; });
  for (int f = threadIdx.x; f < rows * 39; f += 256) {
    const int r = f / 39, c = f - r * 39;
    a.X4[(size_t)(i0 + r) * 256 + 217 + c] = embed_feature(sp[r], c, 6) / sqrt2;
  }
}

// get_alpha (:166-172): the density net's raw output 0 at the kept points of one chunk (alpha: the chunk's rows of
// the caller's output, zero elsewhere)
__global__ __launch_bounds__(256) void k_pdf_alpha_out(const int* list, int b0, int cnt, const float* Y8, float* alpha) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt) return;
  alpha[list[b0 + i]] = Y8[(size_t)i * 264];
}

}  // namespace anr
