// anr_pdf_b16.hip — the aligned_aninerf_pdf render's fused displacement launch, one per batch, on the render
// kernel's machinery (anr_mlp_body.h): activations in registers, split-bf16 weights streamed through the LDS ring.
//   k_pdf_resd_b16  displacement MLP + 0.05 tanh + tpose = x + resd epilogue (aligned_aninerf_pdf_network.py:49-64,
//                   :79-80), program V = 23, render precision ANR_BF16X3
//   k_pdf_resd_x6   the same in ANR_BF16X6 (anr_pdf_x6.hip), program V = 33
// Density and colour run on aligned_aninerf_lbw's programs (anr_lbw_b16.hip), unchanged.
#include "anr_mlp_body.h"

namespace anr {

__global__ __launch_bounds__(512) void k_pdf_resd_b16(MlpArgs a) { ANR_STAMPED(pdf_resd_body<false>(a);); }

namespace {
// one persistent launch over the batch's rows (grid <= one workgroup per 128-row tile), as anr_lbw_b16.hip's
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
bool attr_b16, attr_x6;
}  // namespace

int launch_pdf_resd(const MlpArgs& a, int grid, hipStream_t s, bool x6) {
  return x6 ? launch_prog((const void*)k_pdf_resd_x6, attr_x6, a, grid, s)
            : launch_prog((const void*)k_pdf_resd_b16, attr_b16, a, grid, s);
}

}  // namespace anr
