// anr_mlp_img_x6_ns.hip — k_mlp_img_x6_ns: the image render program k_mlp_img_x6 (render precision ANR_BF16X6; anr_mlp_body.h V = 19) at
// N_samples = 64 * nseg (anr_render_ns_fwd): the same layers, the kept ids decoded as row * 64 + lane.
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_mlp_img_x6_ns(MlpArgs a, int nseg) { ANR_STAMPED(mlp_body<true, 19, true, true>(a, nseg);); }

}  // namespace anr
