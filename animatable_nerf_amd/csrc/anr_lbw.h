// anr_lbw.h — internal structures of the aligned_aninerf_lbw render path (aligned_aninerf_lbw_network.py:90-147).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anr {

// state_dict order of aligned_aninerf_lbw_network.Network (include/aninerf.h, anr_lbw_params)
enum : int {
  LBW_LIN0 = 0,        // tpose_human.nerf_network.lin{l}: bias 3l, weight_g 3l+1, weight_v 3l+2 (l = 0..8)
  LBW_COLOR_LAT = 27,  // tpose_human.color_network.color_latent.weight (num_latent_code, 128)
  LBW_CLIN0 = 28,      // tpose_human.color_network.lin{l}: bias 28+3l, weight_g 29+3l, weight_v 30+3l (l = 0..4)
  LBW_BW_LAT = 43,     // bw_latent.weight (num_train_frame + 1, 128)
  LBW_BWLIN0 = 44,     // bw_linears.{l}: weight 44+2l, bias 45+2l (l = 0..7)
  LBW_BWFC_W = 60,
  LBW_BWFC_B = 61,
  LBW_NUM_TENSORS = 62,
};

// weight-normed layers: 9 density + 5 colour, effective weights v * (g / |v|_row) packed back to back
struct LbwWnLayer {
  int v, g, in, out;
  long off;  // float offset in the effective-weight image
};
constexpr int LBW_NUM_WN = 14;
__host__ __device__ constexpr LbwWnLayer lbw_wn_layer(int i) {
  constexpr int ins[14] = {39, 256, 256, 256, 256, 256, 256, 256, 256, 286, 256, 256, 384, 256};
  constexpr int outs[14] = {256, 256, 256, 217, 256, 256, 256, 256, 257, 256, 256, 256, 256, 3};
  long off = 0;
  for (int k = 0; k < i; ++k) off += (long)ins[k] * outs[k];
  const int base = i < 9 ? 3 * i : LBW_CLIN0 + 3 * (i - 9);
  return LbwWnLayer{base + 2, base + 1, ins[i], outs[i], off};
}
constexpr long LBW_WN_FLOATS = lbw_wn_layer(13).off + 256L * 3;
__host__ __device__ constexpr int lbw_wn_rows() {
  int r = 0;
  for (int i = 0; i < LBW_NUM_WN; ++i) r += lbw_wn_layer(i).out;
  return r;
}

// folded biases (k_lbw_fold): [0] bw_linears.0 and [1] bw_linears.5 with bw_latent[latent_index + 1] (pose
// pass), [2] colour lin3 with color_latent[latent_index] (fold + 512, where the colour programs read it), [3] / [4]
// bw_linears.0 / .5 with bw_latent[0] (T-pose pass)
constexpr int LBW_FOLD_FLOATS = 5 * 256;

struct LbwTensors {
  const float* t[LBW_NUM_TENSORS];  // kernel argument by value (496 B)
};

// per-point kernels over one batch [b0, b0 + cnt) of the compact kept-sample list
struct LbwPointArgs {
  const int* list;
  int b0, cnt;
  const float *ray_o, *ray_d, *near_, *far_, *t_rand;
  int chunk;
  const float *R, *Th, *A, *bigA;
  const float* weights;   // (nv, 24)
  const uint32_t* knn;    // first search: records of every sample (R*64, 8)
  const uint32_t* knn2;   // second search: records of this batch's warped points (cnt, 8)
  const float* tbtab;     // (nchunks, 6) tbounds after this chunk's widening
  float* ptp;             // [P][8]: pose xyz, pose dir xyz, dist
  float* Gx;              // [P][64] gamma_10 of the blend-weight MLP's point (pose, then warped)
  float* ibw;             // [P][24] init_pbw, then init_tbw
  const float* Ybw;       // [P][24] bw_fc output
  float* tp3;             // [P][3] warped points (the second search's queries)
  float* Xs0;             // [P][40] gamma_6(tpose)
  float* X4;              // [P][256] lin4 input: cols 217..255 = gamma_6 / sqrt(2)
  float* C0;              // [P][40] colour input: tpose, gamma_4(tpose_dir)
  const float* Y8;        // [P][264] lin8 output: density, feature
  const float* Yc;        // [P][4] colour logits
  int full;               // the T-pose blend-weight pass follows: k_lbw_warp also writes gamma_10(tpose)
  int fused;              // the networks run as fused programs (anr_lbw_b16.hip): they form gamma themselves (no Gx /
                          // Xs0 / X4 rows) and the blend-weight program has applied the softmax (Ybw holds weights)
  float* pbw_rows;        // (n', 24) compact; NULL in an image-only call, as tbw_rows and sigma
  float* tbw_rows;        // (n', 24)
  float* sigma;           // (n') alpha after the box mask, compact (the alpha_ind stage's input)
  float4* raw;            // (R*64)
};

__global__ void k_lbw_wnorm(LbwTensors T, float* wimg);
__global__ void k_lbw_fold(LbwTensors T, const float* wimg, const int64_t* li, float* fold);
__global__ void k_lbw_gather(LbwPointArgs a);
__global__ void k_lbw_warp(LbwPointArgs a);
__global__ void k_lbw_tbw_in(LbwPointArgs a);
__global__ void k_lbw_tbw(LbwPointArgs a);
__global__ void k_lbw_raw(LbwPointArgs a);

}  // namespace anr
