// anr_rays_ns.hip — the ray-side kernels of the render path at N_samples = 64 * nseg (nseg = 1..4;
// anr_render_ns_fwd). A ray is nseg segments of 64 samples and a row is ray * nseg + seg: one wave per
// row with lane = sample within the segment, so row * 64 + lane == ray * N_samples + s and the keep
// ballots are one 64-bit word per row. The compaction and alpha_ind kernels of anr_rays.hip work on
// "rays of 64" and run over rows unchanged (chunk and ray_offset given in rows); only the two kernels
// that evaluate the ray march itself need the segment:
//
//   k_frontend_ns    k_frontend with s = seg * 64 + lane of N_samples; FrontArgs::n_rays, chunk and
//                    ray_offset in rows
//   k_composite_ns   k_composite looping over a ray's segments, the transmittance carried across
#include "anr_common.h"
#include "anr_kernels.h"

#pragma clang fp contract(off)

namespace anr {

// One wave per row, 16 rows per 1024-thread block. The chunk's argmin key index is row_in_chunk * 64 +
// lane == (ray in chunk) * N_samples + s, the reference's flattened index (first index on ties); it
// fits 32 bits (chunk * N_samples <= 2^31 is checked by the entry).
__global__ __launch_bounds__(1024) void k_frontend_ns(FrontArgs a, int nseg) {
  __shared__ uint64_t skey[16];
  __shared__ int schunk[16];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int row = blockIdx.x * 16 + w;
  const bool live = row < a.n_rays;
  uint64_t key = ~0ull;
  if (live) {
    const int ray = ns_ray_of_row(row, nseg);
    const int s = (row - ray * nseg) * 64 + lane;
    float z, dist, pts[3], pose[3];
    sample_point(a.ray_o, a.ray_d, a.near_, a.far_, a.t_rand, ray, s, nseg * 64, z, dist, pts);
    world_to_pose(pts, a.R, a.Th, pose);
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = a.pbounds[c]; hi[c] = a.pbounds[3 + c]; }
    TriCell cell;
    tri_cell(pose, lo, hi, a.X, a.Y, a.Z, cell);
    const float pn = a.pn24 ? tri_channel(a.pn24, 1, 0, cell) : tri_channel(a.pbw, 25, 24, cell);
    // the novel-view filter is per sample (k_frontend)
    const bool vis = visible_in_views(pts, a.n_views, a.Ks, a.RT, a.msks, a.img_h, a.img_w);
    const bool keep = vis && pn < a.norm_th;
    const uint64_t m = __ballot(keep);
    if (lane == 0) a.mask[row] = m;
    if (a.raw != nullptr && !keep) a.raw[(size_t)row * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int rc = (row + a.ray_offset) % a.chunk;
    key = vis ? (((uint64_t)__float_as_uint(pn) << 32) | (uint32_t)(rc * 64 + lane)) : ~0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(key, off);
      key = o < key ? o : key;
    }
  }
  if (lane == 0) {
    skey[w] = key;
    schunk[w] = live ? row / a.chunk : -1;
  }
  __syncthreads();
  // one thread per run of equal chunk ids: min over the run, one atomic
  if (threadIdx.x < 16) {
    const int c = schunk[threadIdx.x];
    if (c >= 0 && (threadIdx.x == 0 || schunk[threadIdx.x - 1] != c)) {
      uint64_t k = skey[threadIdx.x];
      for (int j = threadIdx.x + 1; j < 16 && schunk[j] == c; ++j) k = skey[j] < k ? skey[j] : k;
      if (k != ~0ull) atomicMin((unsigned long long*)&a.chunk_min[c], (unsigned long long)k);
    }
  }
}

// A12 compositing, one wave per ray over its nseg segments. Within a segment the product scan of
// k_composite; the running transmittance (the inclusive product at lane 63) goes into the next segment,
// and each lane sums its nseg terms before the one wave reduction. With nseg == 1 every operation is
// k_composite's on the same operands (the carried transmittance is exactly 1).
__global__ __launch_bounds__(256) void k_composite_ns(CompositeArgs a, int nseg) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n_rays) return;
  const int n = nseg * 64;
  const float nr = a.near_[ray], fr = a.far_[ray];
  const float* trow = a.t_rand ? a.t_rand + (size_t)ray * n : nullptr;
  float carry = 1.0f;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, sd = 0.f, sa = 0.f;
  for (int seg = 0; seg < nseg; ++seg) {
    const size_t id = ((size_t)ray * nseg + seg) * 64 + lane;
    const float4 r = a.raw[id];
    const float z = z_sample(nr, fr, trow, seg * 64 + lane, n);
    const float p = (1.0f - r.w) + 1e-10f;
    float incl = p;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float y = __shfl_up(incl, off);
      if (lane >= off) incl = incl * y;
    }
    float T = __shfl_up(incl, 1);
    if (lane == 0) T = 1.0f;
    T = carry * T;
    carry = carry * __shfl(incl, 63);
    const float w = r.w * T;
    if (seg == 0) {
      s0 = w * r.x; s1 = w * r.y; s2 = w * r.z; sd = w * z; sa = w;
    } else {
      s0 += w * r.x; s1 += w * r.y; s2 += w * r.z; sd += w * z; sa += w;
    }
    if (a.weights) a.weights[id] = w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off);
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
    sd += __shfl_xor(sd, off);
    sa += __shfl_xor(sa, off);
  }
  if (lane == 0) {
    a.rgb[3 * ray] = s0;
    a.rgb[3 * ray + 1] = s1;
    a.rgb[3 * ray + 2] = s2;
    a.depth[ray] = sd;
    a.acc[ray] = sa;
  }
}

}  // namespace anr
