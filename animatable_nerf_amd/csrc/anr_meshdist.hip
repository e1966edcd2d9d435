// anr_meshdist.hip — the mesh evaluator on the device (lib/evaluators/mesh_evaluator.py:19-136): area-weighted
// surface samples (trimesh.sample.sample_surface), closest-point distances from a point list to a triangle
// mesh (trimesh.proximity.closest_point), and the Chamfer / point-to-surface means of one frame.
//
// Everything runs on the caller's stream; every loop has a bound known at launch; no kernel waits on another
// workgroup (the scans are reduce-then-scan passes). The point-triangle geometry is anr_bwv_geom.h, shared
// with anr_bwvol.hip.
//
// Sampling (anr_mesh_sample)
//   k_md_area        float64 face areas and, per tile of 1024 faces, their inclusive prefix inside the tile
//   k_md_dscan_top   the exclusive prefix of the tile totals (one block)
//   k_md_dscan_apply cum[i] = tile prefix + prefix inside the tile. cum is non-decreasing and a zero-area
//                    face repeats its predecessor's value exactly (every level adds a running sum to the
//                    carry that is the last value of the level below), so searchsorted never lands on one
//   k_md_sample      face = searchsorted(cum, u0 cum[-1], 'left'); point = a + (e0 u1 + e1 u2), float64
// Structure over a mesh (md_build)
//   k_md_bounds1/2   the mesh's box: Morton frame and the float64 centre every record is taken about
//   k_md_code_tri    (30-bit Morton code of the centroid) << 32 | face
//   md_sort          LSD radix sort, four 8-bit digits of the code: per-wave histograms (k_md_hist), their
//                    exclusive scan (k_md_iscan_*), a stable scatter that ranks the keys of a wave by
//                    ballots (k_md_scatter). Linear in n, and a fixed order: (code, index)
//   k_md_prep        per cell of 64 faces consecutive in that order: BwvTri records about the centre, the
//                    original indices, the cell's BwvBox
//   k_md_group       a second level: one BwvBox per 64 consecutive cells
// Query (md_query): k_md_code_pts + md_sort over the points, then
//   k_md_search      64 Morton-consecutive queries per wave, one per lane, float32 about the centre; the loop
//                    of k_bwv_search: lexicographic (d^2, original index) winner, cells pruned by their box
//                    with the margins BWV_REL and 32 eps diag^2, and whole groups of cells by the group's box
//                    under the same rule (on a 3 M-face mesh a wave otherwise reads 48,305 cell boxes twice)
//   k_md_finish      tri_closest_f64 on the winner with the float64 query and the original vertices
//   k_md_mean / k_md_row   float64 means in a fixed order (256 strided partial sums, then a tree), NaN as 0
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/aninerf.h"
#include "anr_bwv_geom.h"
#include "anr_common.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr int MD_MAX_NF = 1 << 26;
constexpr int MD_MAX_PTS = 1 << 24;
constexpr int MD_TILE = 1024;             // elements per block of a scan, keys per wave of the sort
constexpr int MD_SORT_ITERS = MD_TILE / 64;
constexpr int MD_N_CHAMFER = 1000;        // mesh_evaluator.py:100
constexpr int MD_N_P2S = 10000;           // :124
constexpr int MD_GROUP = 64;              // cells per box of the second level
constexpr int MD_DEFAULT_SEARCH = 2;       // what opts.exhaustive == 0 selects: 1 exhaustive, 2 two levels of boxes,
                                          // 3 cell boxes only (tools/mesh_eval_ab.py decides)

struct MdFrame {  // made on the device by k_md_bounds2
  double ctr[3];  // records and queries are taken about this point in float64 before the cast to float32
  float lo[3];    // Morton quantisation: q = (x - lo) * sc, clamped to 0..1023
  float sc[3];
};

struct MdLayout {
  size_t cum, bsum, part, frame, keyA, keyB, hist, hsum, orig, rec, box, gbox, win, pts, sface, dist, kface, status, total;
  int ncell, nwaves;
};

inline int md_tiles(long n) { return (int)((n + MD_TILE - 1) / MD_TILE); }

MdLayout md_layout(int nf, int npts) {
  MdLayout L{};
  const int nkeys = std::max(nf, npts);
  L.ncell = (nf + BWV_CELL - 1) / BWV_CELL;
  L.nwaves = md_tiles(nkeys);
  const size_t slots = (size_t)L.ncell * BWV_CELL;
  Carve c;
  L.cum = c.bytes((size_t)nf * sizeof(double));
  L.bsum = c.bytes((size_t)md_tiles(nf) * sizeof(double));
  L.part = c.bytes((size_t)md_tiles(nf) * 6 * sizeof(float));
  L.frame = c.bytes(sizeof(MdFrame));
  L.keyA = c.bytes((size_t)nkeys * sizeof(uint64_t));
  L.keyB = c.bytes((size_t)nkeys * sizeof(uint64_t));
  L.hist = c.bytes((size_t)L.nwaves * 256 * sizeof(int32_t));
  L.hsum = c.bytes((size_t)md_tiles((long)L.nwaves * 256) * sizeof(int32_t));
  L.orig = c.bytes(slots * sizeof(int32_t));
  L.rec = c.bytes(slots * sizeof(BwvTri));
  L.box = c.bytes((size_t)L.ncell * sizeof(BwvBox));
  L.gbox = c.bytes((size_t)((L.ncell + MD_GROUP - 1) / MD_GROUP) * sizeof(BwvBox));
  L.win = c.bytes((size_t)npts * sizeof(int32_t));
  // the composite's own buffers: its samples, their faces, distances and winners
  L.pts = c.bytes((size_t)npts * 3 * sizeof(double));
  L.sface = c.bytes((size_t)npts * sizeof(int32_t));
  L.dist = c.bytes((size_t)npts * sizeof(double));
  L.kface = c.bytes((size_t)npts * sizeof(int32_t));
  L.status = c.bytes(4 * sizeof(int32_t));
  L.total = c.o;
  return L;
}

// ---- sampling ------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_tri_f64(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                             size_t f, double p[3][3]) {
  for (int k = 0; k < 3; ++k) {
    const int vi = clampi(faces[3 * f + k], 0, nv - 1);
    for (int c = 0; c < 3; ++c) p[k][c] = (double)verts[3 * (size_t)vi + c];
  }
}

// one wave per tile of 1024 faces, 16 consecutive faces per lane: area = 0.5 |e0 x e1| in float64;
// cum[i] = P + (running sum inside the lane), P = the exclusive prefix of the lanes' totals (lane 0 adds
// them in order), bsum[tile] = the tile's total
__global__ __launch_bounds__(64) void k_md_area(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                int nf, double* __restrict__ cum, double* __restrict__ bsum) {
#pragma clang fp contract(off)
  __shared__ double s_p[64];
  constexpr int PER = MD_TILE / 64;
  const long f0 = (long)blockIdx.x * MD_TILE + (long)threadIdx.x * PER;
  double run[PER];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    double area = 0.0;
    if (f0 + j < nf) {
      double p[3][3];
      load_tri_f64(verts, nv, faces, (size_t)(f0 + j), p);
      const double e0[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
      const double e1[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
      const double cx = e0[1] * e1[2] - e0[2] * e1[1];
      const double cy = e0[2] * e1[0] - e0[0] * e1[2];
      const double cz = e0[0] * e1[1] - e0[1] * e1[0];
      area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    }
    acc = acc + area;
    run[j] = acc;
  }
  s_p[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int k = 0; k < 64; ++k) {
      const double t = s_p[k];
      s_p[k] = a;
      a = a + t;
    }
    bsum[blockIdx.x] = a;
  }
  __syncthreads();
  const double P = s_p[threadIdx.x];
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (f0 + j < nf) cum[f0 + j] = P + run[j];
}

// bsum[b] <- sum of bsum[0..b-1], added in order by one thread (tiles of 256 staged in LDS)
__global__ __launch_bounds__(256) void k_md_dscan_top(double* __restrict__ bsum, int nb) {
#pragma clang fp contract(off)
  __shared__ double s_v[256];
  double acc = 0.0;  // thread 0's
  for (int t0 = 0; t0 < nb; t0 += 256) {
    const int i = t0 + threadIdx.x;
    s_v[threadIdx.x] = i < nb ? bsum[i] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = min(256, nb - t0);
      for (int k = 0; k < cnt; ++k) {
        const double t = s_v[k];
        s_v[k] = acc;
        acc = acc + t;
      }
    }
    __syncthreads();
    if (i < nb) bsum[i] = s_v[threadIdx.x];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_md_dscan_apply(double* __restrict__ cum, int nf, const double* __restrict__ bsum) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < nf) cum[i] = bsum[i / MD_TILE] + cum[i];
}

// u (n,3): u0 picks the face, (u1, u2) the point on it. status (one int32): 1 when the total area is zero
// or not finite; then no face is drawn (points 0, face -1)
__global__ __launch_bounds__(256) void k_md_sample(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                   int nf, const double* __restrict__ cum, const double* __restrict__ u,
                                                   int n, double* __restrict__ points, int32_t* __restrict__ face,
                                                   int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const double total = cum[nf - 1];
  const bool ok = total > 0.0 && total < __builtin_inf();
  if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = ok ? 0 : 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!ok) {
    points[3 * (size_t)i] = points[3 * (size_t)i + 1] = points[3 * (size_t)i + 2] = 0.0;
    face[i] = -1;
    return;
  }
  const double x = u[3 * (size_t)i] * total;
  int lo = 0, hi = nf - 1;  // the first index with cum >= x, the last face when there is none
  for (int it = 0; it < 27 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  double p[3][3];
  load_tri_f64(verts, nv, faces, (size_t)lo, p);
  double u1 = u[3 * (size_t)i + 1], u2 = u[3 * (size_t)i + 2];
  if (u1 + u2 > 1.0) {
    u1 = fabs(u1 - 1.0);
    u2 = fabs(u2 - 1.0);
  }
  for (int c = 0; c < 3; ++c) {
    const double e0 = p[1][c] - p[0][c], e1 = p[2][c] - p[0][c];
    points[3 * (size_t)i + c] = p[0][c] + (e0 * u1 + e1 * u2);
  }
  face[i] = lo;
}

// a mesh without faces: nothing to draw from
__global__ __launch_bounds__(256) void k_md_nomesh(int n, double* __restrict__ points, int32_t* __restrict__ face,
                                                   int32_t* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) status[0] = 1;
  if (i >= n) return;
  points[3 * (size_t)i] = points[3 * (size_t)i + 1] = points[3 * (size_t)i + 2] = 0.0;
  face[i] = -1;
}

// ---- the mesh's box -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_md_bounds1(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                    int nf, float* __restrict__ part) {
  __shared__ float s_r[4][6];
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int j = 0; j < MD_TILE / 256; ++j) {
    const long f = (long)blockIdx.x * MD_TILE + j * 256 + threadIdx.x;
    if (f < nf)
      for (int k = 0; k < 3; ++k) {
        const int vi = clampi(faces[3 * (size_t)f + k], 0, nv - 1);
        for (int c = 0; c < 3; ++c) {
          const float x = verts[3 * (size_t)vi + c];  // fminf / fmaxf drop a NaN
          lo[c] = fminf(lo[c], x);
          hi[c] = fmaxf(hi[c], x);
        }
      }
  }
  for (int c = 0; c < 3; ++c) {
    lo[c] = wave_minf(lo[c]);
    hi[c] = wave_maxf(hi[c]);
  }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) {
      s_r[threadIdx.x >> 6][c] = lo[c];
      s_r[threadIdx.x >> 6][3 + c] = hi[c];
    }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    float r = s_r[0][c];
    for (int w = 1; w < 4; ++w) r = c < 3 ? fminf(r, s_r[w][c]) : fmaxf(r, s_r[w][c]);
    part[(size_t)blockIdx.x * 6 + c] = r;
  }
}

__global__ __launch_bounds__(256) void k_md_bounds2(const float* __restrict__ part, int nb, MdFrame* __restrict__ frame) {
  __shared__ float s_r[4][6];
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int b = threadIdx.x; b < nb; b += 256)
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], part[(size_t)b * 6 + c]);
      hi[c] = fmaxf(hi[c], part[(size_t)b * 6 + 3 + c]);
    }
  for (int c = 0; c < 3; ++c) {
    lo[c] = wave_minf(lo[c]);
    hi[c] = wave_maxf(hi[c]);
  }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) {
      s_r[threadIdx.x >> 6][c] = lo[c];
      s_r[threadIdx.x >> 6][3 + c] = hi[c];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    float l = s_r[0][c], h = s_r[0][3 + c];
    for (int w = 1; w < 4; ++w) {
      l = fminf(l, s_r[w][c]);
      h = fmaxf(h, s_r[w][3 + c]);
    }
    if (!(l <= h) || !(l > -inf) || !(h < inf)) l = h = 0.f;  // no finite vertex: every code is 0
    const double ext = (double)h - (double)l;
    frame->ctr[c] = 0.5 * ((double)l + (double)h);
    frame->lo[c] = l;
    frame->sc[c] = ext > 0.0 ? (float)(1023.0 / ext) : 0.f;
  }
}

__device__ __forceinline__ uint32_t morton30(const float q[3]) {
  uint32_t code = 0;
  for (int k = 0; k < 3; ++k) {
    const int qi = q[k] > 0.f ? (q[k] < 1023.f ? (int)q[k] : 1023) : 0;  // NaN -> 0
    code |= spread3((uint32_t)qi) << k;
  }
  return code;
}

__global__ __launch_bounds__(256) void k_md_code_tri(const float* __restrict__ verts, int nv,
                                                     const int32_t* __restrict__ faces, int nf,
                                                     const MdFrame* __restrict__ frame, uint64_t* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nf) return;
  float c[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < 3; ++j) {
    const int vi = clampi(faces[3 * (size_t)i + j], 0, nv - 1);
    for (int k = 0; k < 3; ++k) c[k] += verts[3 * (size_t)vi + k] * (1.f / 3.f);
  }
  const float q[3] = {(c[0] - frame->lo[0]) * frame->sc[0], (c[1] - frame->lo[1]) * frame->sc[1],
                      (c[2] - frame->lo[2]) * frame->sc[2]};
  key[i] = ((uint64_t)morton30(q) << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_md_code_pts(const double* __restrict__ points, int n,
                                                     const MdFrame* __restrict__ frame, uint64_t* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float q[3];
  for (int c = 0; c < 3; ++c) q[c] = (float)(points[3 * (size_t)i + c] - (double)frame->lo[c]) * frame->sc[c];
  key[i] = ((uint64_t)morton30(q) << 32) | (uint32_t)i;
}

// ---- LSD radix sort of the keys by one 8-bit digit --------------------------------------------------------
// wave w owns keys [1024 w, 1024 w + 1024); hist[d * nwaves + w] = how many of them carry digit d
__global__ __launch_bounds__(256) void k_md_hist(const uint64_t* __restrict__ key, int n, int shift, int nwaves,
                                                 int32_t* __restrict__ hist) {
  __shared__ int s_h[4][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + w;
  for (int d = lane; d < 256; d += 64) s_h[w][d] = 0;
  __syncthreads();
  for (int it = 0; it < MD_SORT_ITERS; ++it) {
    const long i = (long)wave * MD_TILE + it * 64 + lane;
    if (wave < nwaves && i < n) atomicAdd(&s_h[w][(int)((key[i] >> shift) & 255)], 1);
  }
  __syncthreads();
  if (wave < nwaves)
    for (int d = lane; d < 256; d += 64) hist[(size_t)d * nwaves + wave] = s_h[w][d];
}

// exclusive scan of m int32 in place: tile sums, their scan by one block, then the tiles
__global__ __launch_bounds__(256) void k_md_iscan_reduce(const int32_t* __restrict__ v, int m, int32_t* __restrict__ hsum) {
  __shared__ int sh[4];
  int s = 0;
  for (int j = 0; j < 4; ++j) {
    const long i = (long)blockIdx.x * MD_TILE + threadIdx.x * 4 + j;
    if (i < m) s += v[i];
  }
  int total;
  block_excl_scan_256(s, sh, total);
  if (threadIdx.x == 0) hsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_md_iscan_top(int32_t* __restrict__ hsum, int nb) {
  __shared__ int sh[4];
  int running = 0;
  for (int t0 = 0; t0 < nb; t0 += 256) {
    const int i = t0 + threadIdx.x;
    const int v = i < nb ? hsum[i] : 0;
    int total;
    const int ex = block_excl_scan_256(v, sh, total);
    if (i < nb) hsum[i] = running + ex;
    running += total;
  }
}

__global__ __launch_bounds__(256) void k_md_iscan_apply(int32_t* __restrict__ v, int m, const int32_t* __restrict__ hsum) {
  __shared__ int sh[4];
  int x[4], s = 0;
  for (int j = 0; j < 4; ++j) {
    const long i = (long)blockIdx.x * MD_TILE + threadIdx.x * 4 + j;
    x[j] = i < m ? v[i] : 0;
    s += x[j];
  }
  int total;
  int ex = block_excl_scan_256(s, sh, total) + hsum[blockIdx.x];
  for (int j = 0; j < 4; ++j) {
    const long i = (long)blockIdx.x * MD_TILE + threadIdx.x * 4 + j;
    if (i < m) v[i] = ex;
    ex += x[j];
  }
}

// stable scatter: a key goes to (scanned hist of its digit and wave) + (keys of that digit earlier in the
// wave's range). Inside a step of 64 keys the lanes sharing a digit are found with eight ballots and ranked
// by lane; the step's lowest such lane then advances the digit's counter
__global__ __launch_bounds__(256) void k_md_scatter(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int n,
                                                    int shift, int nwaves, const int32_t* __restrict__ hist) {
  __shared__ int s_b[4][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + w;
  for (int d = lane; d < 256; d += 64) s_b[w][d] = wave < nwaves ? hist[(size_t)d * nwaves + wave] : 0;
  __syncthreads();
  for (int it = 0; it < MD_SORT_ITERS; ++it) {
    const long i = (long)wave * MD_TILE + it * 64 + lane;
    const bool valid = wave < nwaves && i < n;
    const uint64_t k = valid ? in[i] : 0;
    const int d = (int)((k >> shift) & 255);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const int base = s_b[w][d];
    __syncthreads();
    if (valid) {
      const unsigned pos = (unsigned)(base + rank);
      if (pos < (unsigned)n) out[pos] = k;  // always, when hist is this input's
      if (rank == 0) s_b[w][d] = base + __popcll(peers);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_md_perm(const uint64_t* __restrict__ key, int n, int32_t* __restrict__ perm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) perm[i] = (int32_t)(uint32_t)key[i];
}

// ---- the structure: records about the centre ----------------------------------------------------------
__global__ __launch_bounds__(64) void k_md_prep(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                int nf, const uint64_t* __restrict__ key, const MdFrame* __restrict__ frame,
                                                BwvTri* __restrict__ rec, int32_t* __restrict__ orig,
                                                BwvBox* __restrict__ box) {
  const int s = blockIdx.x * BWV_CELL + threadIdx.x;  // slot; the arrays hold whole cells
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, rep[3] = {0.f, 0.f, 0.f};
  // slots past the last face repeat it: an equal (d^2, index) never replaces the lane's best
  const int i = clampi((int)(uint32_t)key[min(s, nf - 1)], 0, nf - 1);
  orig[s] = i;
  BwvTri t;
  double p[3][3];
  for (int k = 0; k < 3; ++k) {
    const int vi = clampi(faces[3 * (size_t)i + k], 0, nv - 1);
    for (int c = 0; c < 3; ++c) {
      p[k][c] = (double)verts[3 * (size_t)vi + c] - frame->ctr[c];
      const float x = (float)p[k][c];
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
  rec[s] = t;
  BwvBox b = {};
  for (int c = 0; c < 3; ++c) {
    b.lo[c] = wave_minf(lo[c]);
    b.hi[c] = wave_maxf(hi[c]);
    b.rep[c] = rep[c];  // lane 0's face
  }
  const float ex = b.hi[0] - b.lo[0], ey = b.hi[1] - b.lo[1], ez = b.hi[2] - b.lo[2];
  b.mabs = 32.f * 5.9604644775390625e-08f * (ex * ex + ey * ey + ez * ez);
  if (threadIdx.x == 0) box[blockIdx.x] = b;
}

// the second level: one box over each group of MD_GROUP consecutive cells (rep: the first cell's; the margin
// from the group's own diagonal, which is at least any of its cells')
__global__ __launch_bounds__(64) void k_md_group(const BwvBox* __restrict__ box, int ncell, BwvBox* __restrict__ gbox) {
  const int c0 = blockIdx.x * MD_GROUP;
  const BwvBox b = box[min(c0 + (int)threadIdx.x, ncell - 1)];  // lanes past the last cell repeat it
  BwvBox g = {};
  for (int c = 0; c < 3; ++c) {
    g.lo[c] = wave_minf(b.lo[c]);
    g.hi[c] = wave_maxf(b.hi[c]);
    g.rep[c] = __shfl(b.rep[c], 0);
  }
  const float ex = g.hi[0] - g.lo[0], ey = g.hi[1] - g.lo[1], ez = g.hi[2] - g.lo[2];
  g.mabs = 32.f * 5.9604644775390625e-08f * (ex * ex + ey * ey + ez * ez);
  if (threadIdx.x == 0) gbox[blockIdx.x] = g;
}

// ---- the search: k_bwv_search's loop over a point list ----------------------------------------------------
// qkey: the queries' sorted keys; the wave takes 64 consecutive ones. A lane whose query is not finite takes
// no part in the pruning vote (its every distance is NaN or infinite, whatever is visited).
// PRUNE 0: every face. 1: cells skipped by their boxes, every box read. 2: groups of MD_GROUP cells skipped by
// the group's box first, under the same rule; the upper bound ub comes from the groups' representatives and
// then from the cells' of the groups that bound leaves (any subset of the faces gives a valid bound).
template <int PRUNE>
__global__ __launch_bounds__(256) void k_md_search(const BwvTri* __restrict__ rec, const int32_t* __restrict__ orig,
                                                   const BwvBox* __restrict__ box, const BwvBox* __restrict__ gbox, int nf,
                                                   const MdFrame* __restrict__ frame, const double* __restrict__ points,
                                                   int n, const uint64_t* __restrict__ qkey, int32_t* __restrict__ win) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if ((long)wave * 64 >= n) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int s = wave * 64 + lane;
  // lanes past the list search the last query again and write nothing
  const int qi = clampi((int)(uint32_t)qkey[min(s, n - 1)], 0, n - 1);
  const float p[3] = {(float)(points[3 * (size_t)qi] - frame->ctr[0]), (float)(points[3 * (size_t)qi + 1] - frame->ctr[1]),
                      (float)(points[3 * (size_t)qi + 2] - frame->ctr[2])};
  const float inf = __builtin_inff();
  const bool dead = !(fabsf(p[0]) < inf && fabsf(p[1]) < inf && fabsf(p[2]) < inf);
  const int ncell = (nf + BWV_CELL - 1) / BWV_CELL;
  const int ngroup = PRUNE == 2 ? (ncell + MD_GROUP - 1) / MD_GROUP : 1;
  const int gcells = PRUNE == 2 ? MD_GROUP : ncell;  // cells per step of the outer loops
  float ub = inf;
  if (PRUNE == 2)
    for (int g = 0; g < ngroup; ++g) {
      const BwvBox b = gbox[g];
      const float u = sq3(p[0] - b.rep[0], p[1] - b.rep[1], p[2] - b.rep[2]);
      ub = fminf(ub, fmaf(u, BWV_REL, u) + b.mabs);
    }
  if (PRUNE)
    for (int g = 0; g < ngroup; ++g) {
      if (PRUNE == 2) {
        const BwvBox b = gbox[g];
        if (__all(dead || box_d2(p, b) > fmaf(ub, BWV_REL, ub) + b.mabs)) continue;
      }
      const int c1 = min(ncell, (g + 1) * gcells);
      for (int c = g * gcells; c < c1; ++c) {
        const BwvBox b = box[c];
        // the float32 distance to rep's own primitive may exceed |p - rep|^2 by that primitive's rounding
        const float u = sq3(p[0] - b.rep[0], p[1] - b.rep[1], p[2] - b.rep[2]);
        ub = fminf(ub, fmaf(u, BWV_REL, u) + b.mabs);
      }
    }
  float best = inf;
  int besto = 0x7fffffff;
  for (int g = 0; g < ngroup; ++g) {
    if (PRUNE == 2) {
      const BwvBox b = gbox[g];
      const float thr = fminf(best, ub);
      if (__all(dead || box_d2(p, b) > fmaf(thr, BWV_REL, thr) + b.mabs)) continue;
    }
    const int c1 = min(ncell, (g + 1) * gcells);
    for (int c = g * gcells; c < c1; ++c) {
      if (PRUNE) {
        const BwvBox b = box[c];
        const float thr = fminf(best, ub);
        if (__all(dead || box_d2(p, b) > fmaf(thr, BWV_REL, thr) + b.mabs)) continue;
      }
      // whole cells: the last one is padded with copies of the last face, which can never replace it
      const int i0 = c * BWV_CELL;
#pragma unroll 2
      for (int i = i0; i < i0 + BWV_CELL; ++i) {
        const BwvTri t = rec[i];
        const int o = orig[i];
        const float d = tri_d2(p, t);
        if (d < best || (d == best && o < besto)) {
          best = d;
          besto = o;
        }
      }
    }
  }
  // besto keeps its initial value only when every distance is NaN: still a valid face for k_md_finish
  if (s < n) win[qi] = min(besto, nf - 1);
}

__global__ __launch_bounds__(256) void k_md_finish(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces,
                                                   int nf, const double* __restrict__ points, const int32_t* __restrict__ win,
                                                   int n, double* __restrict__ dist, int32_t* __restrict__ face) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = clampi(win[i], 0, nf - 1);
  const double p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
  double q[3][3], w[3] = {1.0, 0.0, 0.0}, d;
  load_tri_f64(verts, nv, faces, (size_t)k, q);
  tri_closest_f64(p, q[0], q[1], q[2], w, d);
  // a NaN in the query or in the face compares with nothing (tri_closest_f64 leaves +inf): the distance is
  // NaN, as the reference's closest_point gives, and the means count it as 0
  bool nan = false;
  for (int c = 0; c < 3; ++c) nan = nan || p[c] != p[c] || q[0][c] != q[0][c] || q[1][c] != q[1][c] || q[2][c] != q[2][c];
  if (nan) d = __builtin_nan("");
  dist[i] = d;
  if (face) face[i] = k;
}

// ---- means -------------------------------------------------------------------------------------------------
// sum of d[0..n) with a NaN counted as 0 (mesh_evaluator.py:114-115): thread t adds d[t], d[t + 256], ... in
// order, then a fixed tree over the 256 partial sums; always one block of 256 threads
__device__ double block_sum_nan0(const double* __restrict__ d, int n, double* sh) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = d[i];
    acc = acc + (v != v ? 0.0 : v);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + off];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_md_mean(const double* __restrict__ dist, int n, double* __restrict__ mean) {
  __shared__ double sh[256];
  const double s = block_sum_nan0(dist, n, sh);
  if (threadIdx.x == 0) mean[0] = s / (double)n;
}

// dist_a: source samples against the target, n_c for Chamfer then n_p for P2S; dist_b: n_c target samples
// against the source; status2: the two samplers' words
__global__ __launch_bounds__(256) void k_md_row(const double* __restrict__ dist_a, const double* __restrict__ dist_b, int n_c,
                                                int n_p, const int32_t* __restrict__ status2, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  const double st = block_sum_nan0(dist_a, n_c, sh) / (double)n_c;
  const double p2s = block_sum_nan0(dist_a + n_c, n_p, sh) / (double)n_p;
  const double ts = block_sum_nan0(dist_b, n_c, sh) / (double)n_c;
  if (threadIdx.x == 0) {
    const int status = (status2[0] ? 1 : 0) | (status2[1] ? 2 : 0);
    const double nan = __builtin_nan("");
    out[0] = status ? nan : (st + ts) / 2.0;
    out[1] = status ? nan : p2s;
    out[2] = status ? nan : st;
    out[3] = status ? nan : ts;
    out[4] = (double)status;
    out[5] = out[6] = out[7] = 0.0;
  }
}

__global__ void k_md_badrow(int status, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const double nan = __builtin_nan("");
    out[0] = out[1] = out[2] = out[3] = nan;
    out[4] = (double)status;
    out[5] = out[6] = out[7] = 0.0;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------
struct MdWs {
  char* ws;
  MdLayout L;
  template <class T> T* at(size_t off) const { return (T*)(ws + off); }
};

inline unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }

int md_sample(hipStream_t s, const MdWs& W, const float* verts, int nv, const int32_t* faces, int nf, const double* u,
              int n, double* points, int32_t* face, int32_t* status) {
  if (nf <= 0) {
    hipLaunchKernelGGL(k_md_nomesh, dim3(blocks256(n)), dim3(256), 0, s, n, points, face, status);
    return check_launch("k_md_nomesh");
  }
  double* cum = W.at<double>(W.L.cum);
  double* bsum = W.at<double>(W.L.bsum);
  const int nb = md_tiles(nf);
  hipLaunchKernelGGL(k_md_area, dim3(nb), dim3(64), 0, s, verts, nv, faces, nf, cum, bsum);
  ANR_TRY(check_launch("k_md_area"));
  hipLaunchKernelGGL(k_md_dscan_top, dim3(1), dim3(256), 0, s, bsum, nb);
  ANR_TRY(check_launch("k_md_dscan_top"));
  hipLaunchKernelGGL(k_md_dscan_apply, dim3(blocks256(nf)), dim3(256), 0, s, cum, nf, (const double*)bsum);
  ANR_TRY(check_launch("k_md_dscan_apply"));
  hipLaunchKernelGGL(k_md_sample, dim3(blocks256(n)), dim3(256), 0, s, verts, nv, faces, nf, (const double*)cum, u, n,
                     points, face, status);
  return check_launch("k_md_sample");
}

// keys in W.keyA, sorted by their 30-bit code (ties by index: the initial order) back into W.keyA
int md_sort(hipStream_t s, const MdWs& W, int n) {
  uint64_t* a = W.at<uint64_t>(W.L.keyA);
  uint64_t* b = W.at<uint64_t>(W.L.keyB);
  int32_t* hist = W.at<int32_t>(W.L.hist);
  int32_t* hsum = W.at<int32_t>(W.L.hsum);
  const int nwaves = md_tiles(n);
  const int m = nwaves * 256, mb = md_tiles(m);
  const unsigned sb = (unsigned)((nwaves + 3) / 4);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 32 + 8 * pass;
    hipLaunchKernelGGL(k_md_hist, dim3(sb), dim3(256), 0, s, (const uint64_t*)a, n, shift, nwaves, hist);
    ANR_TRY(check_launch("k_md_hist"));
    hipLaunchKernelGGL(k_md_iscan_reduce, dim3(mb), dim3(256), 0, s, (const int32_t*)hist, m, hsum);
    ANR_TRY(check_launch("k_md_iscan_reduce"));
    hipLaunchKernelGGL(k_md_iscan_top, dim3(1), dim3(256), 0, s, hsum, mb);
    ANR_TRY(check_launch("k_md_iscan_top"));
    hipLaunchKernelGGL(k_md_iscan_apply, dim3(mb), dim3(256), 0, s, hist, m, (const int32_t*)hsum);
    ANR_TRY(check_launch("k_md_iscan_apply"));
    hipLaunchKernelGGL(k_md_scatter, dim3(sb), dim3(256), 0, s, (const uint64_t*)a, b, n, shift, nwaves,
                       (const int32_t*)hist);
    ANR_TRY(check_launch("k_md_scatter"));
    std::swap(a, b);
  }
  return ANR_OK;
}

int md_build(hipStream_t s, const MdWs& W, const float* verts, int nv, const int32_t* faces, int nf,
             int32_t* order_only = nullptr) {
  const int nb = md_tiles(nf);
  float* part = W.at<float>(W.L.part);
  MdFrame* frame = W.at<MdFrame>(W.L.frame);
  uint64_t* key = W.at<uint64_t>(W.L.keyA);
  hipLaunchKernelGGL(k_md_bounds1, dim3(nb), dim3(256), 0, s, verts, nv, faces, nf, part);
  ANR_TRY(check_launch("k_md_bounds1"));
  hipLaunchKernelGGL(k_md_bounds2, dim3(1), dim3(256), 0, s, (const float*)part, nb, frame);
  ANR_TRY(check_launch("k_md_bounds2"));
  hipLaunchKernelGGL(k_md_code_tri, dim3(blocks256(nf)), dim3(256), 0, s, verts, nv, faces, nf, (const MdFrame*)frame, key);
  ANR_TRY(check_launch("k_md_code_tri"));
  ANR_TRY(md_sort(s, W, nf));
  if (order_only) {
    hipLaunchKernelGGL(k_md_perm, dim3(blocks256(nf)), dim3(256), 0, s, (const uint64_t*)key, nf, order_only);
    return check_launch("k_md_perm");
  }
  const int ncell = (nf + BWV_CELL - 1) / BWV_CELL;
  hipLaunchKernelGGL(k_md_prep, dim3(ncell), dim3(64), 0, s, verts, nv, faces, nf, (const uint64_t*)key,
                     (const MdFrame*)frame, W.at<BwvTri>(W.L.rec), W.at<int32_t>(W.L.orig), W.at<BwvBox>(W.L.box));
  ANR_TRY(check_launch("k_md_prep"));
  hipLaunchKernelGGL(k_md_group, dim3((ncell + MD_GROUP - 1) / MD_GROUP), dim3(64), 0, s,
                     (const BwvBox*)W.at<BwvBox>(W.L.box), ncell, W.at<BwvBox>(W.L.gbox));
  return check_launch("k_md_group");
}

// after md_build of the same mesh: distances and faces of n points
int md_query(hipStream_t s, const MdWs& W, const float* verts, int nv, const int32_t* faces, int nf, const double* points,
             int n, int search, double* dist, int32_t* face) {
  const MdFrame* frame = W.at<MdFrame>(W.L.frame);
  uint64_t* key = W.at<uint64_t>(W.L.keyA);
  int32_t* win = W.at<int32_t>(W.L.win);
  hipLaunchKernelGGL(k_md_code_pts, dim3(blocks256(n)), dim3(256), 0, s, points, n, frame, key);
  ANR_TRY(check_launch("k_md_code_pts"));
  ANR_TRY(md_sort(s, W, n));
  const unsigned sblocks = (unsigned)(((long)(n + 63) / 64 + 3) / 4);
#define MD_SEARCH(P)                                                                                              \
  hipLaunchKernelGGL((k_md_search<P>), dim3(sblocks), dim3(256), 0, s, (const BwvTri*)W.at<BwvTri>(W.L.rec),      \
                     (const int32_t*)W.at<int32_t>(W.L.orig), (const BwvBox*)W.at<BwvBox>(W.L.box),                 \
                     (const BwvBox*)W.at<BwvBox>(W.L.gbox), nf, frame, points, n,                                  \
                     (const uint64_t*)key, win)
  if (search == 2) MD_SEARCH(2);
  else if (search == 3) MD_SEARCH(1);
  else MD_SEARCH(0);
#undef MD_SEARCH
  ANR_TRY(check_launch("k_md_search"));
  hipLaunchKernelGGL(k_md_finish, dim3(blocks256(n)), dim3(256), 0, s, verts, nv, faces, nf, points, (const int32_t*)win, n,
                     dist, face);
  return check_launch("k_md_finish");
}

// the options: 0 on success with the fields resolved
int md_opts(const char* who, const anr_meshdist_opts* o, int* search_out, int* n_c, int* n_p) {
  int search = 0;
  *n_c = MD_N_CHAMFER;
  *n_p = MD_N_P2S;
  if (o) {
    if (o->struct_size != sizeof(anr_meshdist_opts))
      return fail(ANR_E_ARG, std::string(who) + ": opts.struct_size is not sizeof(anr_meshdist_opts)");
    search = o->exhaustive;
    if (o->n_chamfer < 0 || o->n_p2s < 0) return fail(ANR_E_ARG, std::string(who) + ": n_chamfer / n_p2s must not be negative");
    if (o->n_chamfer) *n_c = o->n_chamfer;
    if (o->n_p2s) *n_p = o->n_p2s;
  }
  if (search < 0 || search > 3) return fail(ANR_E_ARG, std::string(who) + ": exhaustive must be 0, 1, 2 or 3");
  *search_out = search == 0 ? MD_DEFAULT_SEARCH : search;
  return ANR_OK;
}

}  // namespace

extern "C" {

size_t anr_mesh_dist_workspace_bytes(int nf, int n_pts) {
  if (nf <= 0 || nf > MD_MAX_NF || n_pts <= 0 || n_pts > MD_MAX_PTS) return 0;
  return md_layout(nf, n_pts).total;
}

int anr_mesh_sample(const float* verts, int nv, const int32_t* faces, int nf, const double* u, int n, double* points,
                    int32_t* face, int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
  if (!u || !points || !face || !status || !workspace) return fail(ANR_E_ARG, "anr_mesh_sample: NULL argument");
  if (nf > 0 && (!verts || !faces)) return fail(ANR_E_ARG, "anr_mesh_sample: NULL argument (a mesh with faces needs verts and faces)");
  if (nf > 0 && nv <= 0) return fail(ANR_E_ARG, "anr_mesh_sample: nv must be positive");
  if (nf > MD_MAX_NF) return fail(ANR_E_ARG, "anr_mesh_sample: nf above 2^26");
  if (n <= 0 || n > MD_MAX_PTS) return fail(ANR_E_ARG, "anr_mesh_sample: n must lie in 1..2^24");
  const MdWs W{(char*)workspace, md_layout(std::max(nf, 1), n)};
  if (ws_bytes < W.L.total) return fail(ANR_E_WORKSPACE, "anr_mesh_sample: workspace too small");
  return md_sample((hipStream_t)stream, W, verts, nv, faces, nf, u, n, points, face, status);
}

int anr_mesh_order(const float* verts, int nv, const int32_t* faces, int nf, int32_t* perm, void* workspace,
                   size_t ws_bytes, void* stream) {
  if (!verts || !faces || !perm || !workspace) return fail(ANR_E_ARG, "anr_mesh_order: NULL argument");
  if (nv <= 0) return fail(ANR_E_ARG, "anr_mesh_order: nv must be positive");
  if (nf <= 0 || nf > MD_MAX_NF) return fail(ANR_E_ARG, "anr_mesh_order: nf must lie in 1..2^26");
  const MdWs W{(char*)workspace, md_layout(nf, 1)};
  if (ws_bytes < W.L.total) return fail(ANR_E_WORKSPACE, "anr_mesh_order: workspace too small");
  return md_build((hipStream_t)stream, W, verts, nv, faces, nf, perm);
}

int anr_mesh_point_dist(const float* verts, int nv, const int32_t* faces, int nf, const double* points, int n,
                        const anr_meshdist_opts* o, double* dist, int32_t* face, double* mean, void* workspace,
                        size_t ws_bytes, void* stream) {
  if (!verts || !faces || !points || !dist || !workspace) return fail(ANR_E_ARG, "anr_mesh_point_dist: NULL argument");
  int search;
  int n_c, n_p;
  ANR_TRY(md_opts("anr_mesh_point_dist", o, &search, &n_c, &n_p));
  if (nv <= 0) return fail(ANR_E_ARG, "anr_mesh_point_dist: nv must be positive");
  if (nf <= 0 || nf > MD_MAX_NF) return fail(ANR_E_ARG, "anr_mesh_point_dist: nf must lie in 1..2^26");
  if (n <= 0 || n > MD_MAX_PTS) return fail(ANR_E_ARG, "anr_mesh_point_dist: n must lie in 1..2^24");
  const MdWs W{(char*)workspace, md_layout(nf, n)};
  if (ws_bytes < W.L.total) return fail(ANR_E_WORKSPACE, "anr_mesh_point_dist: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ANR_TRY(md_build(s, W, verts, nv, faces, nf));
  ANR_TRY(md_query(s, W, verts, nv, faces, nf, points, n, search, dist, face));
  if (mean) {
    hipLaunchKernelGGL(k_md_mean, dim3(1), dim3(256), 0, s, (const double*)dist, n, mean);
    return check_launch("k_md_mean");
  }
  return ANR_OK;
}

int anr_mesh_metrics(const float* src_verts, int src_nv, const int32_t* src_faces, int src_nf, const float* tgt_verts,
                     int tgt_nv, const int32_t* tgt_faces, int tgt_nf, const double* u, const anr_meshdist_opts* o,
                     double* out, void* workspace, size_t ws_bytes, void* stream) {
  if (!u || !out || !workspace) return fail(ANR_E_ARG, "anr_mesh_metrics: NULL argument");
  if ((src_nf > 0 && (!src_verts || !src_faces)) || (tgt_nf > 0 && (!tgt_verts || !tgt_faces)))
    return fail(ANR_E_ARG, "anr_mesh_metrics: NULL argument (a mesh with faces needs verts and faces)");
  int search;
  int n_c, n_p;
  ANR_TRY(md_opts("anr_mesh_metrics", o, &search, &n_c, &n_p));
  if ((src_nf > 0 && src_nv <= 0) || (tgt_nf > 0 && tgt_nv <= 0))
    return fail(ANR_E_ARG, "anr_mesh_metrics: nv must be positive");
  if (src_nf > MD_MAX_NF || tgt_nf > MD_MAX_NF) return fail(ANR_E_ARG, "anr_mesh_metrics: nf above 2^26");
  if ((long)n_c * 2 + n_p > MD_MAX_PTS) return fail(ANR_E_ARG, "anr_mesh_metrics: 2 n_chamfer + n_p2s above 2^24");
  const int npts = 2 * n_c + n_p, na = n_c + n_p;
  const MdWs W{(char*)workspace, md_layout(std::max(std::max(src_nf, tgt_nf), 1), npts)};
  if (ws_bytes < W.L.total) return fail(ANR_E_WORKSPACE, "anr_mesh_metrics: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (src_nf <= 0 || tgt_nf <= 0) {  // a mesh without faces: the row carries the status alone
    hipLaunchKernelGGL(k_md_badrow, dim3(1), dim3(64), 0, s, (src_nf <= 0 ? 1 : 0) | (tgt_nf <= 0 ? 2 : 0), out);
    return check_launch("k_md_badrow");
  }
  // samples: [source Chamfer n_c | source P2S n_p | target Chamfer n_c]; u rows in the reference's draw
  // order: source Chamfer, target Chamfer, source P2S
  double* pts = W.at<double>(W.L.pts);
  int32_t* sface = W.at<int32_t>(W.L.sface);
  double* dist = W.at<double>(W.L.dist);
  int32_t* kface = W.at<int32_t>(W.L.kface);
  int32_t* status = W.at<int32_t>(W.L.status);
  ANR_TRY(md_sample(s, W, src_verts, src_nv, src_faces, src_nf, u, n_c, pts, sface, status));
  ANR_TRY(md_sample(s, W, src_verts, src_nv, src_faces, src_nf, u + 6 * (size_t)n_c, n_p, pts + 3 * (size_t)n_c,
                    sface + n_c, status));
  ANR_TRY(md_sample(s, W, tgt_verts, tgt_nv, tgt_faces, tgt_nf, u + 3 * (size_t)n_c, n_c, pts + 3 * (size_t)na, sface + na,
                    status + 1));
  ANR_TRY(md_build(s, W, tgt_verts, tgt_nv, tgt_faces, tgt_nf));
  ANR_TRY(md_query(s, W, tgt_verts, tgt_nv, tgt_faces, tgt_nf, pts, na, search, dist, kface));
  ANR_TRY(md_build(s, W, src_verts, src_nv, src_faces, src_nf));
  ANR_TRY(md_query(s, W, src_verts, src_nv, src_faces, src_nf, pts + 3 * (size_t)na, n_c, search, dist + na, kface + na));
  hipLaunchKernelGGL(k_md_row, dim3(1), dim3(256), 0, s, (const double*)dist, (const double*)(dist + na), n_c, n_p,
                     (const int32_t*)status, out);
  return check_launch("k_md_row");
}

}  // extern "C"
