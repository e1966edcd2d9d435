// anr_pdf.h — internal structures of the aligned_aninerf_pdf render path (aligned_aninerf_pdf_network.py:97-138).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "anr_lbw.h"

namespace anr {

// state_dict order of aligned_aninerf_pdf_network.Network (include/aninerf.h, anr_pdf_params). Entries 0..42
// (tpose_human: the density net, color_latent, the colour net) are aligned_aninerf_lbw's tensor for tensor, so
// k_lbw_wnorm and lbw_wn_layer() serve this network through an LbwTensors copy of the table.
enum : int {
  PDF_COLOR_LAT = LBW_COLOR_LAT,  // 27
  PDF_CLIN0 = LBW_CLIN0,          // 28
  PDF_RESD_LAT = 43,              // resd_latent.weight (unused by the forward)
  PDF_RLIN0 = 44,                 // resd_linears.{l}: weight 44+2l, bias 45+2l (l = 0..7)
  PDF_RFC_W = 60,
  PDF_RFC_B = 61,
  PDF_NUM_TENSORS = 62,
};
static_assert(PDF_NUM_TENSORS == LBW_NUM_TENSORS, "the weight-norm table is shared through LbwTensors");

// folded biases (k_pdf_fold): [0] resd_linears.0 and [1] resd_linears.5 with poses (72), [2] colour lin3 with
// color_latent[latent_index] (fold + 512, where the colour programs read it)
constexpr int PDF_FOLD_FLOATS = 3 * 256;

// per-point kernels over one batch [b0, b0 + cnt) of the compact kept-sample list
struct PdfPointArgs {
  const int* list;
  int b0, cnt;
  const float *ray_o, *ray_d, *near_, *far_, *t_rand;
  const float* wpts;     // free points of one get_alpha chunk (SdfFrontArgs' free-sample mode) or NULL: ids index
  int n_pts;             // them, no view direction and no dist
  const float *R, *Th, *A, *bigA;
  const float* weights;  // (nv, 24)
  const uint32_t* knn;   // the search's records of every sample (R*64, 8)
  float* ptp;            // [P][8]: init_bigpose xyz, big-pose dir xyz, dist, 0 (LbwPointArgs::ptp for k_lbw_raw)
  float* Gr;             // [P][64] gamma_10(init_bigpose), exact-fp32 path (NULL: the fused program forms it)
  const float* Yr;       // [P][4] resd_fc output (exact-fp32 path)
  float* Xs0;            // [P][40] gamma_6(tpose)                          (exact-fp32 path)
  float* X4;             // [P][256] lin4 input: cols 217..255 = gamma_6 / sqrt(2)  (exact-fp32 path)
  float* C0;             // [P][40] colour input: tpose (0..2), gamma_4(big-pose dir) (3..29)
  float* resd_rows;      // (n', 3) compact output, or NULL (image-only call)
};

__global__ void k_pdf_fold(LbwTensors T, const float* wimg, const float* poses, const int64_t* li, float* fold);
__global__ void k_pdf_warp(PdfPointArgs a);
__global__ void k_pdf_mid(PdfPointArgs a);
__global__ void k_pdf_alpha_out(const int* list, int b0, int cnt, const float* Y8, float* alpha);

}  // namespace anr
