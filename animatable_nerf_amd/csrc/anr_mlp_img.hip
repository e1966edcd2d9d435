// anr_mlp_img.hip — k_mlp_img: the image render program (anr_mlp_body.h V = 9: the render program
// without its T-pose BW pass) with exact fp32 MFMA everywhere.
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_mlp_img(MlpArgs a) { ANR_STAMPED(mlp_body<false, 9, true>(a);); }

}  // namespace anr
