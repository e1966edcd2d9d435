// anr_lbw_x6.hip — the aligned_aninerf_lbw render's fused MLP programs in render precision ANR_BF16X6 (every
// weight and activation as hi/mid/lo bf16, six MFMA products per multiply-add with fp32 accumulation: fp32-level
// products; softplus at libm accuracy): programs 30, 31, 32 = the bf16x3 programs 20, 21, 22 of anr_lbw_b16.hip
// (own TU: the two instantiation sets build in parallel). Launched through anr_lbw_b16.hip's launch_lbw_* (x6).
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_lbw_bw_x6(MlpArgs a) { ANR_STAMPED(lbw_bw_body<true>(a);); }
__global__ __launch_bounds__(512) void k_lbw_density_x6(MlpArgs a) { ANR_STAMPED(lbw_density_body<true>(a);); }
__global__ __launch_bounds__(512) void k_lbw_color_x6(MlpArgs a) { ANR_STAMPED(lbw_color_body<true>(a);); }

}  // namespace anr
