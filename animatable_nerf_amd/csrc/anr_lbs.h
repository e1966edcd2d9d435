// anr_lbs.h — per-sample linear-blend-skinning helpers shared by the sdf_pdf and aligned_aninerf_lbw
// per-point kernels (anr_sdf.hip, anr_lbw.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace anr {

__device__ __forceinline__ void blend16(const float bw[24], const float* __restrict__ A, float Ab[16]) {
#pragma clang fp contract(fast)
  for (int m = 0; m < 16; ++m) Ab[m] = 0.f;
  for (int j = 0; j < 24; ++j)
    for (int m = 0; m < 16; ++m) Ab[m] += bw[j] * A[j * 16 + m];
}

__device__ __forceinline__ void inv33(const float Ab[16], float Ri[9]) {
#pragma clang fp contract(off)
  const float a = Ab[0], b = Ab[1], c = Ab[2], d = Ab[4], e = Ab[5], f = Ab[6], g = Ab[8], h = Ab[9], k = Ab[10];
  const float c00 = e * k - f * h, c01 = c * h - b * k, c02 = b * f - c * e;
  const float c10 = f * g - d * k, c11 = a * k - c * g, c12 = c * d - a * f;
  const float c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
  const float rd = 1.0f / (a * c00 + b * c10 + c * c20);
  Ri[0] = c00 * rd; Ri[1] = c01 * rd; Ri[2] = c02 * rd;
  Ri[3] = c10 * rd; Ri[4] = c11 * rd; Ri[5] = c12 * rd;
  Ri[6] = c20 * rd; Ri[7] = c21 * rd; Ri[8] = c22 * rd;
}

// the workgroup's 256 rows of a [P][W] block, written column-fastest by all threads (coalesced):
// value(row, col) from the per-row values staged in LDS by the thread-per-sample phase
template <int W, typename F>
__device__ __forceinline__ void sdf_rows_store(float* base, int i0, int cnt, F value) {
  const int rows = min(256, cnt - i0);
  for (int f = threadIdx.x; f < rows * W; f += 256) {
    const int r = f / W, c = f - r * W;
    base[(size_t)(i0 + r) * W + c] = value(r, c);
  }
}

}  // namespace anr
