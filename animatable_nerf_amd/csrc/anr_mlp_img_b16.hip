// anr_mlp_img_b16.hip — k_mlp_img_b16: the image render program (anr_mlp_body.h V = 9) in hi/lo-split
// bf16 MFMA (render precision ANR_BF16X3; the pose pass per ANR_POSE_MODE).
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_mlp_img_b16(MlpArgs a) { ANR_STAMPED(mlp_body<true, 9, true>(a);); }

}  // namespace anr
