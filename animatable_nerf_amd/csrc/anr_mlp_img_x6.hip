// anr_mlp_img_x6.hip — k_mlp_img_x6: the image render program with every layer in bf16x6 (render
// precision ANR_BF16X6; anr_mlp_body.h V = 19, the arithmetic of k_mlp_x6).
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_mlp_img_x6(MlpArgs a) { ANR_STAMPED(mlp_body<true, 19, true>(a);); }

}  // namespace anr
