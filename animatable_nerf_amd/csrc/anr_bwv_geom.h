// anr_bwv_geom.h — the point-triangle geometry shared by the blend-weight volumes (anr_bwvol.hip) and the
// mesh evaluator (anr_meshdist.hip): the 64-byte triangle record and cell box of the float32 search, the
// float32 squared distances with their pruning bound, and the float64 closest point of the finish. Each
// translation unit gets its own copy (unnamed namespace), as when the code lived in anr_bwvol.hip.
#pragma once
#include "anr_common.h"

namespace {

constexpr int BWV_CELL = 64;           // primitives per cell (one bounding box each)
constexpr float BWV_REL = 1e-5f;       // relative part of the pruning margin

struct BwvTri {  // 64 bytes: read whole by one scalar load
  float a[3], e0[3], e1[3];
  float d00, d01, d11;       // e0.e0, e0.e1, e1.e1
  float r00, r11, r22;       // 1 / |e0|^2, 1 / |e1|^2, 1 / |e1 - e0|^2 (0 for a zero-length edge)
  float rdet;                // 1 / (d00 d11 - d01^2), 0 for a zero-area triangle
};
struct BwvBox {  // 64 bytes
  float lo[3], hi[3];
  float mabs;    // absolute part of the pruning margin: 32 eps diag^2
  float rep[3];  // a point of the cell's first primitive: |p - rep|^2 bounds the answer from above
  float pad[6];
};

__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 10 bits -> every third bit
__device__ __forceinline__ uint32_t spread3(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

__device__ __forceinline__ float sq3(float x, float y, float z) { return fmaf(z, z, fmaf(y, y, x * x)); }

// float32 squared distance from p to the triangle: the smallest over the three edge segments and, when
// the projection falls inside, the plane. Every candidate is |p - q|^2 for a point q of the triangle
// (clamped parameters), so the result is never below the true distance by more than the rounding of
// that one expression — what the pruning margin of k_bwv_search covers.
__device__ __forceinline__ float tri_d2(const float p[3], const BwvTri& t) {
  const float ax = p[0] - t.a[0], ay = p[1] - t.a[1], az = p[2] - t.a[2];
  const float d1 = fmaf(az, t.e0[2], fmaf(ay, t.e0[1], ax * t.e0[0]));
  const float d2 = fmaf(az, t.e1[2], fmaf(ay, t.e1[1], ax * t.e1[0]));
  // edge a -> b
  const float t0 = fminf(fmaxf(d1 * t.r00, 0.f), 1.f);
  float best = sq3(fmaf(-t0, t.e0[0], ax), fmaf(-t0, t.e0[1], ay), fmaf(-t0, t.e0[2], az));
  // edge a -> c
  const float t1 = fminf(fmaxf(d2 * t.r11, 0.f), 1.f);
  best = fminf(best, sq3(fmaf(-t1, t.e1[0], ax), fmaf(-t1, t.e1[1], ay), fmaf(-t1, t.e1[2], az)));
  // edge b -> c: (p - b).(c - b) = d2 - d1 - d01 + d00
  const float t2 = fminf(fmaxf(((d2 - d1) + (t.d00 - t.d01)) * t.r22, 0.f), 1.f);
  {
    const float u = 1.f - t2;  // q = a + u e0 + t2 e1
    best = fminf(best, sq3(fmaf(-t2, t.e1[0], fmaf(-u, t.e0[0], ax)), fmaf(-t2, t.e1[1], fmaf(-u, t.e0[1], ay)),
                           fmaf(-t2, t.e1[2], fmaf(-u, t.e0[2], az))));
  }
  // the plane
  const float s = (t.d11 * d1 - t.d01 * d2) * t.rdet, r = (t.d00 * d2 - t.d01 * d1) * t.rdet;
  const float dp = sq3(fmaf(-r, t.e1[0], fmaf(-s, t.e0[0], ax)), fmaf(-r, t.e1[1], fmaf(-s, t.e0[1], ay)),
                       fmaf(-r, t.e1[2], fmaf(-s, t.e0[2], az)));
  const bool in = s >= 0.f && r >= 0.f && s + r <= 1.f && t.rdet != 0.f;
  best = fminf(best, in ? dp : __builtin_inff());
  return best;
}

__device__ __forceinline__ float box_d2(const float p[3], const BwvBox& b) {
  const float dx = fmaxf(fmaxf(b.lo[0] - p[0], p[0] - b.hi[0]), 0.f);
  const float dy = fmaxf(fmaxf(b.lo[1] - p[1], p[1] - b.hi[1]), 0.f);
  const float dz = fmaxf(fmaxf(b.lo[2] - p[2], p[2] - b.hi[2]), 0.f);
  return sq3(dx, dy, dz);
}

// closest point of segment o + t e, t in [0, 1], to the point at offset ap from o (e = 0: the point o)
__device__ __forceinline__ double seg_t(const double ap[3], const double e[3]) {
#pragma clang fp contract(off)
  const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
  if (!(ee > 0.0)) return 0.0;
  const double t = (ap[0] * e[0] + ap[1] * e[1] + ap[2] * e[2]) / ee;
  return fmin(fmax(t, 0.0), 1.0);
}

// float64 closest point of triangle (a, b, c) to p as barycentrics w (w[0] a + w[1] b + w[2] c): the
// projection when it lies inside, else the closest of the three edge segments (lowest edge on a tie)
__device__ void tri_closest_f64(const double p[3], const double a[3], const double b[3], const double c[3],
                                double w[3], double& dist) {
#pragma clang fp contract(off)
  double e0[3], e1[3], e2[3], ap[3], bp[3];
  for (int k = 0; k < 3; ++k) {
    e0[k] = b[k] - a[k]; e1[k] = c[k] - a[k]; e2[k] = c[k] - b[k];
    ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k];
  }
  const double d00 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
  const double d01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
  const double d11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
  const double d1 = ap[0] * e0[0] + ap[1] * e0[1] + ap[2] * e0[2];
  const double d2 = ap[0] * e1[0] + ap[1] * e1[1] + ap[2] * e1[2];
  const double det = d00 * d11 - d01 * d01;
  double cand[4][3];
  int n = 0;
  if (det > 1e-10 * d00 * d11) {
    const double s = (d11 * d1 - d01 * d2) / det, r = (d00 * d2 - d01 * d1) / det;
    if (s >= 0.0 && r >= 0.0 && s + r <= 1.0) {
      cand[n][0] = 1.0 - s - r; cand[n][1] = s; cand[n][2] = r;
      ++n;
    }
  }
  if (n == 0) {
    const double t0 = seg_t(ap, e0), t1 = seg_t(ap, e1), t2 = seg_t(bp, e2);
    cand[0][0] = 1.0 - t0; cand[0][1] = t0; cand[0][2] = 0.0;
    cand[1][0] = 1.0 - t1; cand[1][1] = 0.0; cand[1][2] = t1;
    cand[2][0] = 0.0; cand[2][1] = 1.0 - t2; cand[2][2] = t2;
    n = 3;
  }
  double bd = __builtin_inf();
  for (int k = 0; k < n; ++k) {
    double dd = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double q = cand[k][0] * a[j] + cand[k][1] * b[j] + cand[k][2] * c[j];
      dd += (p[j] - q) * (p[j] - q);
    }
    if (dd < bd) {
      bd = dd;
      w[0] = cand[k][0]; w[1] = cand[k][1]; w[2] = cand[k][2];
    }
  }
  dist = sqrt(bd);
}

}  // namespace
