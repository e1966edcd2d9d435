// anr_bwvol.hip — blend-weight volumes on the device (tools/custom_dataset/prepare_blend_weights.py:156-211,
// 229-283): for every voxel of an 'ij' grid the closest vertex (per-frame bweights/{i}.npy) or the closest
// point of the triangle mesh (tbw.npy, bigpose_bw.npy), the skinning weights there and the distance.
//
// Launch sequence of anr_bw_volume (all on the caller's stream, no kernel waits on another workgroup):
//   k_bwv_code    a 30-bit Morton code per primitive (triangle centroid or vertex) over the grid's box
//   k_bwv_rank    the permutation that sorts (code, index): each key counts the smaller ones
//   k_bwv_prep    one wave per cell of 64 primitives consecutive in Morton order: a 16-float record per
//                 triangle (origin, two edge vectors, their dot products, reciprocals; zero where an edge
//                 or the area vanishes) or a float4 per vertex, the original indices, and the cell's
//                 float32 bounding box
//   k_bwv_search  float32: a wave owns a 4x4x4 brick of voxels, one voxel per lane; primitives are read
//                 through a wave-uniform index (every lane reads the same record, a scalar broadcast
//                 load) and replace the lane's best under the lexicographic (d^2, original index) order,
//                 so among equal float32 squared distances the lowest index wins. The pruned variant
//                 skips a cell when its box bound exceeds every lane's best by a margin that covers the
//                 float32 rounding; no atomics, no split of the primitive range: the result does not
//                 depend on launch geometry
//   k_bwv_finish  float64: for each voxel's winner the closest point, barycentrics, interpolated weights
//                 and distance, cast to float32 once; 256 voxels per block staged in LDS, then the
//                 (nb + 1)-float rows are written with consecutive lanes on consecutive floats
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/aninerf.h"
#include "anr_bwv_geom.h"  // BwvTri, BwvBox, tri_d2, box_d2, seg_t, tri_closest_f64 (shared with anr_meshdist.hip)
#include "anr_common.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr int BWV_BRICK = 4;           // a wave's brick is 4 x 4 x 4 voxels
constexpr int BWV_MAX_NB = 64;
constexpr long BWV_MAX_VOX = 1L << 28;
constexpr bool BWV_DEFAULT_PRUNED = true;  // what opts.exhaustive == 0 selects (tools/bwvol_ab.py decides)

struct BwvLayout { size_t key, perm, orig, rec, box, win, total; int ncell; };

BwvLayout bwv_layout(int nv, int nf, long nvox) {
  BwvLayout L{};
  const int nprim = std::max(nv, nf);
  L.ncell = (nprim + BWV_CELL - 1) / BWV_CELL;
  const size_t slots = (size_t)L.ncell * BWV_CELL;
  Carve c;
  L.key = c.bytes(slots * sizeof(uint64_t));
  L.perm = c.bytes(slots * sizeof(int32_t));
  L.orig = c.bytes(slots * sizeof(int32_t));
  L.rec = c.bytes(slots * sizeof(BwvTri));
  L.box = c.bytes((size_t)L.ncell * sizeof(BwvBox));
  L.win = c.bytes((size_t)nvox * sizeof(int32_t));
  L.total = c.o;
  return L;
}

// key[i] = (30-bit Morton code of primitive i's centroid over the grid's box) << 32 | i: distinct keys,
// so their order is a permutation whatever the geometry (a face index outside [0, nv) is the caller's
// contract; it is clamped here and below so that no read leaves the vertex array)
template <int MODE>
__global__ __launch_bounds__(256) void k_bwv_code(const float* __restrict__ verts, int nv,
                                                  const int32_t* __restrict__ faces, int nprim, float lx, float ly,
                                                  float lz, float sx, float sy, float sz,
                                                  uint64_t* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nprim) return;
  float c[3] = {0.f, 0.f, 0.f};
  if (MODE == 0) {
    for (int k = 0; k < 3; ++k) c[k] = verts[3 * (size_t)i + k];
  } else {
    for (int j = 0; j < 3; ++j) {
      const int vi = clampi(faces[3 * (size_t)i + j], 0, nv - 1);
      for (int k = 0; k < 3; ++k) c[k] += verts[3 * (size_t)vi + k] * (1.f / 3.f);
    }
  }
  const float q[3] = {(c[0] - lx) * sx, (c[1] - ly) * sy, (c[2] - lz) * sz};
  uint32_t code = 0;
  for (int k = 0; k < 3; ++k) {
    const int qi = q[k] > 0.f ? (q[k] < 1023.f ? (int)q[k] : 1023) : 0;  // NaN -> 0
    code |= spread3((uint32_t)qi) << k;
  }
  key[i] = ((uint64_t)code << 32) | (uint32_t)i;
}

// perm[rank of key i] = i by counting the smaller keys (tiles of 256 keys broadcast from LDS): a fixed,
// allocation-free sort of a few 10^4 keys
__global__ __launch_bounds__(256) void k_bwv_rank(const uint64_t* __restrict__ key, int nprim,
                                                  int32_t* __restrict__ perm) {
  __shared__ uint64_t s_k[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const uint64_t mine = i < nprim ? key[i] : 0;
  int cnt = 0;
  for (int j0 = 0; j0 < nprim; j0 += 256) {
    const int j = j0 + threadIdx.x;
    s_k[threadIdx.x] = j < nprim ? key[j] : ~(uint64_t)0;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) cnt += s_k[k] < mine ? 1 : 0;
    __syncthreads();
  }
  if (i < nprim) perm[cnt] = i;  // cnt < nprim: at most nprim - 1 keys are smaller
}

// one wave per cell of 64 primitives consecutive in Morton order: their records, original indices and
// the cell's box
template <int MODE>
__global__ __launch_bounds__(64) void k_bwv_prep(const float* __restrict__ verts, int nv,
                                                 const int32_t* __restrict__ faces, int nprim,
                                                 const int32_t* __restrict__ perm, void* __restrict__ rec,
                                                 int32_t* __restrict__ orig, BwvBox* __restrict__ box) {
  const int s = blockIdx.x * BWV_CELL + threadIdx.x;  // slot; the arrays hold whole cells
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, rep[3] = {0.f, 0.f, 0.f};
  // slots past the last primitive repeat it: an equal (d^2, index) never replaces the lane's best
  const int i = clampi(perm[min(s, nprim - 1)], 0, nprim - 1);
  orig[s] = i;
  if (MODE == 0) {
    float4 v;
    v.x = verts[3 * (size_t)i]; v.y = verts[3 * (size_t)i + 1]; v.z = verts[3 * (size_t)i + 2];
    lo[0] = hi[0] = rep[0] = v.x; lo[1] = hi[1] = rep[1] = v.y; lo[2] = hi[2] = rep[2] = v.z;
    v.w = __int_as_float(i);  // the original index rides in the record
    ((float4*)rec)[s] = v;
  } else {
    BwvTri t;
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
      const int vi = clampi(faces[3 * (size_t)i + k], 0, nv - 1);
      for (int c = 0; c < 3; ++c) {
        const float x = verts[3 * (size_t)vi + c];
        p[k][c] = (double)x;
        lo[c] = fminf(lo[c], x);
        hi[c] = fmaxf(hi[c], x);
      }
    }
    double e0[3], e1[3], d00 = 0.0, d01 = 0.0, d11 = 0.0;
    for (int c = 0; c < 3; ++c) {
      e0[c] = p[1][c] - p[0][c];
      e1[c] = p[2][c] - p[0][c];
      d00 += e0[c] * e0[c]; d01 += e0[c] * e1[c]; d11 += e1[c] * e1[c];
      t.a[c] = rep[c] = (float)p[0][c]; t.e0[c] = (float)e0[c]; t.e1[c] = (float)e1[c];
    }
    const double d22 = d00 - 2.0 * d01 + d11, det = d00 * d11 - d01 * d01;
    t.d00 = (float)d00; t.d01 = (float)d01; t.d11 = (float)d11;
    t.r00 = d00 > 0.0 ? (float)(1.0 / d00) : 0.f;
    t.r11 = d11 > 0.0 ? (float)(1.0 / d11) : 0.f;
    t.r22 = d22 > 0.0 ? (float)(1.0 / d22) : 0.f;
    // sin^2 of the corner angle at or below 1e-10: the triangle counts as its edges
    t.rdet = det > 1e-10 * d00 * d11 ? (float)(1.0 / det) : 0.f;
    if (!(t.r00 < inf)) t.r00 = 0.f;
    if (!(t.r11 < inf)) t.r11 = 0.f;
    if (!(t.r22 < inf)) t.r22 = 0.f;
    if (!(t.rdet < inf)) t.rdet = 0.f;
    ((BwvTri*)rec)[s] = t;
  }
  BwvBox b = {};
  for (int c = 0; c < 3; ++c) {
    b.lo[c] = wave_minf(lo[c]);
    b.hi[c] = wave_maxf(hi[c]);
    b.rep[c] = rep[c];  // lane 0's primitive
  }
  const float ex = b.hi[0] - b.lo[0], ey = b.hi[1] - b.lo[1], ez = b.hi[2] - b.lo[2];
  b.mabs = 32.f * 5.9604644775390625e-08f * (ex * ex + ey * ey + ez * ez);
  if (threadIdx.x == 0) box[blockIdx.x] = b;
}

// Cells are visited in storage (Morton) order; a better candidate replaces the lane's best when it is
// strictly closer or equally close with a lower original index, so the visiting order does not matter.
// Pruned: thr = min(best, ub), ub = min over cells of |p - rep|^2 (1 + BWV_REL) + 32 eps diag^2; a cell is skipped when box_d2 > thr (1 + BWV_REL)
// + 32 eps diag^2 for every lane (diag: the diagonal of the cell's box). DESIGN.md §2 "Blend-weight
// volumes" derives both terms from the float32 rounding of tri_d2 / box_d2; tests/test_bwvol_ref.py
// restates the rule on the CPU.
template <int MODE, bool PRUNE>
__global__ __launch_bounds__(256) void k_bwv_search(const void* __restrict__ rec, const int32_t* __restrict__ orig,
                                                    const BwvBox* __restrict__ box, int nprim, double ox, double oy,
                                                    double oz, double vsize, int X, int Y, int Z, int bx_n, int by_n,
                                                    int bz_n, int32_t* __restrict__ win) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (wave >= bx_n * by_n * bz_n) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int bz = wave % bz_n, by = (wave / bz_n) % by_n, bx = wave / (bz_n * by_n);
  const int x = bx * BWV_BRICK + (lane >> 4), y = by * BWV_BRICK + ((lane >> 2) & 3), z = bz * BWV_BRICK + (lane & 3);
  const bool inside = x < X && y < Y && z < Z;
  // lanes past the grid search the nearest grid voxel again and write nothing
  const int cx = min(x, X - 1), cy = min(y, Y - 1), cz = min(z, Z - 1);
  const float p[3] = {(float)(ox + (double)cx * vsize), (float)(oy + (double)cy * vsize),
                      (float)(oz + (double)cz * vsize)};
  const int ncell = (nprim + BWV_CELL - 1) / BWV_CELL;
  float ub = __builtin_inff();
  if (PRUNE)
    for (int c = 0; c < ncell; ++c) {
      const BwvBox b = box[c];
      // the float32 distance to rep's own primitive may exceed |p - rep|^2 by that primitive's rounding
      const float u = sq3(p[0] - b.rep[0], p[1] - b.rep[1], p[2] - b.rep[2]);
      ub = fminf(ub, fmaf(u, BWV_REL, u) + b.mabs);
    }
  float best = __builtin_inff();
  int besto = 0x7fffffff;
  for (int c = 0; c < ncell; ++c) {
    if (PRUNE) {
      const BwvBox b = box[c];
      const float thr = fminf(best, ub);
      if (__all(box_d2(p, b) > fmaf(thr, BWV_REL, thr) + b.mabs)) continue;
    }
    // whole cells: the last one is padded with copies of the last primitive, which can never replace it
    const int i0 = c * BWV_CELL;
    if (MODE == 0) {
      constexpr int N = 8;  // eight float4 records per step: two 64-byte scalar loads in flight together
      for (int i = i0; i < i0 + BWV_CELL; i += N) {
        float4 v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = ((const float4*)rec)[i + k];
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const int o = __float_as_int(v[k].w);
          const float d = sq3(p[0] - v[k].x, p[1] - v[k].y, p[2] - v[k].z);
          if (d < best || (d == best && o < besto)) {
            best = d;
            besto = o;
          }
        }
      }
    } else {
      // one 64-byte record per step (the compiler keeps a second record's load next to its use anyway)
#pragma unroll 2
      for (int i = i0; i < i0 + BWV_CELL; ++i) {
        const BwvTri t = ((const BwvTri*)rec)[i];
        const int o = orig[i];
        const float d = tri_d2(p, t);
        if (d < best || (d == best && o < besto)) {
          best = d;
          besto = o;
        }
      }
    }
  }
  // besto keeps its initial value only when every distance is NaN: still a valid index for k_bwv_finish
  if (inside) win[((size_t)x * Y + y) * Z + z] = min(besto, nprim - 1);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_bwv_finish(const float* __restrict__ verts, int nv,
                                                    const int32_t* __restrict__ faces, const float* __restrict__ skin,
                                                    int nb, const int32_t* __restrict__ win, double ox, double oy,
                                                    double oz, double vsize, int Y, int Z, long nvox,
                                                    float* __restrict__ volume, int32_t* __restrict__ index) {
#pragma clang fp contract(off)
  __shared__ double s_w[256][3];
  __shared__ float s_d[256];
  __shared__ int s_v[256][3];
  const long n0 = (long)blockIdx.x * 256;
  const long n = n0 + threadIdx.x;
  if (n < nvox) {
    const int k = win[n];
    const int z = (int)(n % Z), y = (int)((n / Z) % Y), x = (int)(n / ((long)Z * Y));
    const double p[3] = {ox + (double)x * vsize, oy + (double)y * vsize, oz + (double)z * vsize};
    double w[3] = {1.0, 0.0, 0.0}, dist;
    int vi[3];
    if (MODE == 0) {
      vi[0] = vi[1] = vi[2] = k;
      const double dx = p[0] - (double)verts[3 * (size_t)k], dy = p[1] - (double)verts[3 * (size_t)k + 1],
                   dz = p[2] - (double)verts[3 * (size_t)k + 2];
      dist = sqrt((dx * dx + dy * dy) + dz * dz);
    } else {
      double q[3][3];
      for (int j = 0; j < 3; ++j) {
        vi[j] = clampi(faces[3 * (size_t)k + j], 0, nv - 1);
        for (int c = 0; c < 3; ++c) q[j][c] = (double)verts[3 * (size_t)vi[j] + c];
      }
      tri_closest_f64(p, q[0], q[1], q[2], w, dist);
    }
    for (int j = 0; j < 3; ++j) {
      s_w[threadIdx.x][j] = w[j];
      s_v[threadIdx.x][j] = vi[j];
    }
    s_d[threadIdx.x] = (float)dist;
    if (index) index[n] = k;
  }
  __syncthreads();
  const int C = nb + 1;
  const long cnt = min((long)256, nvox - n0) * C;
  float* out = volume + (size_t)n0 * C;
  for (long e = threadIdx.x; e < cnt; e += 256) {
    const int v = (int)(e / C), c = (int)(e - (long)v * C);
    float r;
    if (c == nb) {
      r = s_d[v];
    } else if (MODE == 0) {
      r = skin[(size_t)s_v[v][0] * nb + c];
    } else {
      const double a = (double)skin[(size_t)s_v[v][0] * nb + c], b = (double)skin[(size_t)s_v[v][1] * nb + c],
                   g = (double)skin[(size_t)s_v[v][2] * nb + c];
      r = (float)((s_w[v][0] * a + s_w[v][1] * b) + s_w[v][2] * g);
    }
    out[e] = r;
  }
}

}  // namespace

extern "C" {

size_t anr_bw_volume_workspace_bytes(int nv, int nf, int X, int Y, int Z) {
  if (nv <= 0 || nf < 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
  const long nvox = (long)X * (long)Y * (long)Z;
  if (nvox > BWV_MAX_VOX) return 0;
  return bwv_layout(nv, nf, nvox).total;
}

int anr_bw_volume(const float* verts, int nv, const int32_t* faces, int nf, const float* skin, int nb,
                  const double* origin, double vsize, int X, int Y, int Z, const anr_bwv_opts* o, float* volume,
                  int32_t* index, void* workspace, size_t ws_bytes, void* stream) {
  if (!verts || !skin || !origin || !volume || !workspace) return fail(ANR_E_ARG, "anr_bw_volume: NULL argument");
  int mode = 0, search = 0;
  if (o) {
    if (o->struct_size != sizeof(anr_bwv_opts))
      return fail(ANR_E_ARG, "anr_bw_volume: opts.struct_size is not sizeof(anr_bwv_opts)");
    mode = o->mode;
    search = o->exhaustive;
  }
  if (mode != 0 && mode != 1) return fail(ANR_E_ARG, "anr_bw_volume: mode must be 0 (vertex) or 1 (surface)");
  if (search < 0 || search > 2) return fail(ANR_E_ARG, "anr_bw_volume: exhaustive must be 0, 1 or 2");
  if (nb < 1 || nb > BWV_MAX_NB) return fail(ANR_E_ARG, "anr_bw_volume: nb outside 1..64");
  if (nv <= 0) return fail(ANR_E_ARG, "anr_bw_volume: nv must be positive");
  if (mode == 1 && (!faces || nf <= 0)) return fail(ANR_E_ARG, "anr_bw_volume: surface mode needs faces (nf > 0)");
  if (nf < 0) return fail(ANR_E_ARG, "anr_bw_volume: nf must not be negative");
  if (X <= 0 || Y <= 0 || Z <= 0 || (long)X * (long)Y * (long)Z > BWV_MAX_VOX)
    return fail(ANR_E_ARG, "anr_bw_volume: X, Y, Z must be positive with X * Y * Z at most 2^28");
  if (!(vsize > 0.0) || !std::isfinite(vsize) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) ||
      !std::isfinite(origin[2]))
    return fail(ANR_E_ARG, "anr_bw_volume: vsize must be positive, vsize and origin finite");
  const long nvox = (long)X * (long)Y * (long)Z;
  const BwvLayout L = bwv_layout(nv, nf, nvox);
  if (ws_bytes < L.total) return fail(ANR_E_WORKSPACE, "anr_bw_volume: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint64_t* key = (uint64_t*)(ws + L.key);
  int32_t* perm = (int32_t*)(ws + L.perm);
  int32_t* orig = (int32_t*)(ws + L.orig);
  void* rec = ws + L.rec;
  BwvBox* box = (BwvBox*)(ws + L.box);
  int32_t* win = (int32_t*)(ws + L.win);
  const int nprim = mode == 0 ? nv : nf;
  const int ncell = (nprim + BWV_CELL - 1) / BWV_CELL;
  const bool prune = search == 2 || (search == 0 && BWV_DEFAULT_PRUNED);
  const int bx = (X + BWV_BRICK - 1) / BWV_BRICK, by = (Y + BWV_BRICK - 1) / BWV_BRICK,
            bz = (Z + BWV_BRICK - 1) / BWV_BRICK;
  const unsigned sblocks = (unsigned)(((long)bx * by * bz + 3) / 4);
  const unsigned fblocks = (unsigned)((nvox + 255) / 256);
  const unsigned pblocks = (unsigned)((nprim + 255) / 256);
  const double ox = origin[0], oy = origin[1], oz = origin[2];
  // Morton quantisation over the grid's box (primitives outside it clamp to its faces)
  float msc[3];
  const int dims[3] = {X, Y, Z};
  for (int c = 0; c < 3; ++c) {
    const double ext = vsize * (double)(dims[c] - 1);
    msc[c] = ext > 0.0 ? (float)(1023.0 / ext) : 0.f;
  }
#define BWV_SEARCH(M, P)                                                                                       \
  hipLaunchKernelGGL((k_bwv_search<M, P>), dim3(sblocks), dim3(256), 0, s, (const void*)rec,                   \
                     (const int32_t*)orig, (const BwvBox*)box, nprim, ox, oy, oz, vsize, X, Y, Z, bx, by, bz, win)
#define BWV_RUN(M)                                                                                             \
  do {                                                                                                         \
    hipLaunchKernelGGL(k_bwv_code<M>, dim3(pblocks), dim3(256), 0, s, verts, nv, faces, nprim, (float)ox,      \
                       (float)oy, (float)oz, msc[0], msc[1], msc[2], key);                                     \
    ANR_TRY(check_launch("k_bwv_code"));                                                                       \
    hipLaunchKernelGGL(k_bwv_rank, dim3(pblocks), dim3(256), 0, s, (const uint64_t*)key, nprim, perm);         \
    ANR_TRY(check_launch("k_bwv_rank"));                                                                       \
    hipLaunchKernelGGL(k_bwv_prep<M>, dim3(ncell), dim3(64), 0, s, verts, nv, faces, nprim,                    \
                       (const int32_t*)perm, rec, orig, box);                                                  \
    ANR_TRY(check_launch("k_bwv_prep"));                                                                       \
    if (prune) BWV_SEARCH(M, true);                                                                            \
    else BWV_SEARCH(M, false);                                                                                 \
    ANR_TRY(check_launch("k_bwv_search"));                                                                     \
    hipLaunchKernelGGL(k_bwv_finish<M>, dim3(fblocks), dim3(256), 0, s, verts, nv, faces, skin, nb,            \
                       (const int32_t*)win, ox, oy, oz, vsize, Y, Z, nvox, volume, index);                     \
  } while (0)
  if (mode == 0) BWV_RUN(0);
  else BWV_RUN(1);
#undef BWV_RUN
#undef BWV_SEARCH
  return check_launch("k_bwv_finish");
}

}  // extern "C"
