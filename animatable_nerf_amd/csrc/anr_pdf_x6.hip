// anr_pdf_x6.hip — the aligned_aninerf_pdf render's fused displacement program in render precision ANR_BF16X6
// (every weight and activation as hi/mid/lo bf16, six MFMA products per multiply-add with fp32 accumulation):
// program 33 = the bf16x3 program 23 of anr_pdf_b16.hip (own TU: the two instantiations build in parallel).
// Launched through anr_pdf_b16.hip's launch_pdf_resd (x6).
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_pdf_resd_x6(MlpArgs a) { ANR_STAMPED(pdf_resd_body<true>(a);); }

}  // namespace anr
