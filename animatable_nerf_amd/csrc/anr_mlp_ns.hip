// anr_mlp_ns.hip — k_mlp_ns: the fused render kernel k_mlp (exact fp32 MFMA; anr_mlp_body.h V = 2) at
// N_samples = 64 * nseg (anr_render_ns_fwd): the same layers, the kept ids decoded as row * 64 + lane.
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_mlp_ns(MlpArgs a, int nseg) { ANR_STAMPED(mlp_body<false, 2, false, true>(a, nseg);); }

}  // namespace anr
