// anr_lbw_b16.hip — the aligned_aninerf_lbw render's fused MLP launches, one per batch each, on the render
// kernel's machinery (anr_mlp_body.h): activations in registers, split-bf16 weights streamed through the LDS
// ring. Render precision ANR_BF16X3 (hi/lo, 3 products per multiply-add):
//   k_lbw_bw_b16       blend-weight MLP + log-softmax epilogue (aligned_aninerf_lbw_network.py:48-58), program V = 20
//   k_lbw_density_b16  density network forward, no per-layer stores (:336-352), program V = 21
//   k_lbw_color_b16    colour network with the 286-wide first layer (:403-436), program V = 22
// and ANR_BF16X6 (hi/mid/lo, 6 products, fp32-level; anr_lbw_x6.hip): k_lbw_*_x6, programs V + 10.
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_lbw_bw_b16(MlpArgs a) { ANR_STAMPED(lbw_bw_body<false>(a);); }
__global__ __launch_bounds__(512) void k_lbw_density_b16(MlpArgs a) { ANR_STAMPED(lbw_density_body<false>(a);); }
__global__ __launch_bounds__(512) void k_lbw_color_b16(MlpArgs a) { ANR_STAMPED(lbw_color_body<false>(a);); }

namespace {
// one persistent launch of a fused program over the batch's rows (grid <= one workgroup per 128-row tile), as
// anr_resd_b16.hip launches the sdf_pdf programs
int launch_prog(const void* kernel, bool& attr, const MlpArgs& a, int grid, hipStream_t s) {
  if (!attr) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, mlp_lds_bytes<true>()) != hipSuccess)
      return -1;
    attr = true;
  }
  if (a.n_rows <= 0) return 0;
  const int ntiles = (a.n_rows + 127) / 128;
  MlpArgs args = a;
  const int g = grid < ntiles ? grid : ntiles;
  ProfSlot* ps = prof_begin(s, g);  // the network time and clock of a profiled call (anr_profile_*)
  args.clk = ps ? ps->clk : nullptr;
  void* kargs[] = {&args};
  if (hipLaunchKernel(kernel, dim3(g), dim3(512), kargs, mlp_lds_bytes<true>(), s) != hipSuccess) return -1;
  if (hipGetLastError() != hipSuccess) return -1;
  return prof_end(ps, s) == 0 ? 0 : -1;
}
bool attr_b16[3], attr_x6[3];
}  // namespace

int launch_lbw_bw(const MlpArgs& a, int grid, hipStream_t s, bool x6) {
  return x6 ? launch_prog((const void*)k_lbw_bw_x6, attr_x6[0], a, grid, s)
            : launch_prog((const void*)k_lbw_bw_b16, attr_b16[0], a, grid, s);
}
int launch_lbw_density(const MlpArgs& a, int grid, hipStream_t s, bool x6) {
  return x6 ? launch_prog((const void*)k_lbw_density_x6, attr_x6[1], a, grid, s)
            : launch_prog((const void*)k_lbw_density_b16, attr_b16[1], a, grid, s);
}
int launch_lbw_color(const MlpArgs& a, int grid, hipStream_t s, bool x6) {
  return x6 ? launch_prog((const void*)k_lbw_color_x6, attr_x6[2], a, grid, s)
            : launch_prog((const void*)k_lbw_color_b16, attr_b16[2], a, grid, s);
}

}  // namespace anr
