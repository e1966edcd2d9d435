// anr_meshcc.hip — the largest watertight component of a triangle mesh, on the device: the split of
// lib/networks/renderer/sdf_mesh_renderer.py:77-78, max(trimesh.Trimesh(v, t).split(), key=lambda m:
// len(m.vertices)), with the semantics of the host renderer_sdf_mesh.largest_component (trimesh is
// not installed: parity with it is unpinned, parity with the host pass is exact).
//
// Faces are joined through shared undirected edges only (a shared vertex joins nothing); an edge's
// multiplicity is the number of face sides that carry its vertex pair, all three sides of every face
// counted (so a degenerate face (a, a, b) carries the pair (a, b) twice and the pair (a, a) once); a
// component's label is its lowest face index; it is watertight when every one of its edges has
// multiplicity 2; the watertight component with the most distinct vertices is kept, the lowest label
// on a tie. Output faces keep their order, output vertices are the sorted distinct ids of the kept faces.
//
// Launch sequence of anr_mesh_cc_count (all on the caller's stream, one memset in front; S = 3 nt sides):
//   k_cc_validate  every index against [0, nv): a status word, and the indices as int32. Every later
//                  kernel reads the status first and returns when it is set: no index is dereferenced
//                  before this launch has passed
//   k_cc_hist      integer atomicAdd histograms of the sides by their lower endpoint and of the corners
//                  by their vertex; parent[f] = f
//   scans          exclusive scans of both histograms (block scan + the scan of the block sums)
//   k_cc_fill      records through an atomic cursor: (other endpoint, face) per side, the corner id
//                  3 f + k per corner. The order inside a bucket is arbitrary; nothing below depends on it
//   k_cc_union     a thread per face walks the bucket of each of its sides: the records with the same
//                  other endpoint are the edge (their count its multiplicity), and the face is united
//                  with the lowest face among them. Union-find over faces: a root is hooked by atomicCAS
//                  onto a LOWER root only and paths are shortened by atomicMin, so parent[] only ever
//                  decreases; parent[] is read by agent-scope atomic loads (a plain load can be stale
//                  across XCDs)
//   k_cc_flatten   root[f] = find(f) (parent[] is constant in this launch); a face with a side of
//                  multiplicity != 2 marks its root bad; roots are counted
//   k_cc_nverts    a thread per corner: it counts for its root when no record of its vertex's bucket has
//                  the same root and a lower corner id; the counts are summed per wave and block before
//                  the integer atomicAdd into nverts[root]
//   k_cc_select    atomicMax of (nverts << 32) | (0xFFFFFFFF - label) over the roots that are not bad
//   k_cc_flags     keep flags of the faces and vertices of the winner
//   scans          exclusive scans of both flag arrays: the output positions
//   k_cc_finish    counts {V', T', n_components, n_watertight, kept_label, status}, labels
// anr_mesh_cc_emit gathers (or copies the inputs when no component is watertight).
//
// No kernel waits on another lane or workgroup: every loop is bounded by a bucket length or by the
// strictly decreasing parent index, and a failed CAS means the root moved to a lower index. Bucket
// walks are O(valence^2) per vertex: marching-cubes valence is small; a pathological fan (one vertex
// in most faces) is slow but bounded. Every reduction is integer: two calls write the same bits.
#include <string>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_kernels.h"
#include "anr_ws.h"

using namespace anr;

namespace {

struct CcState {
  int32_t counts[ANR_MESHCC_NCOUNT];  // as anr_mesh_cc_count returns them (k_cc_finish)
  int32_t status;                     // 0, or 2 once an index is outside [0, nv)
  int32_t ncomp, nwt;
  int32_t vout, tout;                 // totals of the keep-flag scans
  unsigned long long best;            // (nverts << 32) | (0xFFFFFFFF - label), 0: no watertight component
};

struct CcLayout {
  size_t st, ehead, vhead, ecur, vcur, nverts, bad, fkeep, vkeep, zero_end;  // [st, zero_end) is cleared per call
  size_t tri, erec, vrec, parent, root, fbad, bs_e, bs_v, bs_f, bs_k, total;
};

CcLayout cc_layout(long nv, long nt) {
  CcLayout L{};
  const size_t V = (size_t)nv, T = (size_t)nt, S = 3 * T;
  Carve c;
  L.st = c.bytes(sizeof(CcState));
  L.ehead = c.bytes((V + 1) * 4);
  L.vhead = c.bytes((V + 1) * 4);
  L.ecur = c.bytes(V * 4);
  L.vcur = c.bytes(V * 4);
  L.nverts = c.bytes(T * 4);
  L.bad = c.bytes(T * 4);
  L.fkeep = c.bytes((T + 1) * 4);
  L.vkeep = c.bytes((V + 1) * 4);
  L.zero_end = c.o;
  L.tri = c.bytes(S * 4);
  L.erec = c.bytes(S * 8);
  L.vrec = c.bytes(S * 4);
  L.parent = c.bytes(T * 4);
  L.root = c.bytes(T * 4);
  L.fbad = c.bytes(T);
  L.bs_e = c.bytes((V / 256 + 1) * 4);
  L.bs_v = c.bytes((V / 256 + 1) * 4);
  L.bs_f = c.bytes((T / 256 + 1) * 4);
  L.bs_k = c.bytes((V / 256 + 1) * 4);
  L.total = c.o;
  return L;
}

struct CcArgs {
  const int64_t* tris;  // (nt, 3) the caller's
  int nt, nv, S;
  CcState* st;
  int* tri;             // (S) validated indices
  int *ehead, *vhead;   // (nv + 1) histograms -> block-local exclusive offsets (bs_e, bs_v: block offsets)
  int *ecur, *vcur;     // (nv) fill cursors
  int2* erec;           // (S) per side, bucketed by lower endpoint: (other endpoint, face)
  int* vrec;            // (S) per corner, bucketed by vertex: 3 face + corner
  int *parent, *root;   // (nt)
  int *nverts, *bad;    // (nt) per root: distinct vertices, an edge of multiplicity != 2
  uint8_t* fbad;        // (nt) the face has a side of multiplicity != 2
  int *fkeep, *vkeep;   // (nt + 1), (nv + 1) keep flags -> block-local output positions (bs_f, bs_k)
  int *bs_e, *bs_v, *bs_f, *bs_k;
};

CcArgs cc_args(const int64_t* tris, long nt, long nv, char* ws) {
  const CcLayout L = cc_layout(nv, nt);
  CcArgs a{};
  a.tris = tris; a.nt = (int)nt; a.nv = (int)nv; a.S = (int)(3 * nt);
  a.st = (CcState*)(ws + L.st);
  a.tri = (int*)(ws + L.tri);
  a.ehead = (int*)(ws + L.ehead); a.vhead = (int*)(ws + L.vhead);
  a.ecur = (int*)(ws + L.ecur); a.vcur = (int*)(ws + L.vcur);
  a.erec = (int2*)(ws + L.erec); a.vrec = (int*)(ws + L.vrec);
  a.parent = (int*)(ws + L.parent); a.root = (int*)(ws + L.root);
  a.nverts = (int*)(ws + L.nverts); a.bad = (int*)(ws + L.bad);
  a.fbad = (uint8_t*)(ws + L.fbad);
  a.fkeep = (int*)(ws + L.fkeep); a.vkeep = (int*)(ws + L.vkeep);
  a.bs_e = (int*)(ws + L.bs_e); a.bs_v = (int*)(ws + L.bs_v);
  a.bs_f = (int*)(ws + L.bs_f); a.bs_k = (int*)(ws + L.bs_k);
  return a;
}

// the thread's element, or -1 past n (the grid is rounded up to whole blocks; the sum can pass 2^31)
__device__ __forceinline__ int cc_tid(int n) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  return q < n ? (int)q : -1;
}
// global exclusive offset of element i from its block-local offset and its block's offset
__device__ __forceinline__ int cc_off(const int* __restrict__ off, const int* __restrict__ bs, int i) {
  return bs[i >> 8] + off[i];
}
__device__ __forceinline__ int cc_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int cc_max(int a, int b) { return a > b ? a : b; }

__global__ __launch_bounds__(256) void k_cc_validate(CcArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool out = false;
  if (i < a.S) {
    const int64_t x = a.tris[i];
    out = x < 0 || x >= (int64_t)a.nv;
    a.tri[i] = out ? 0 : (int)x;
  }
  const unsigned long long m = __ballot(out);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicOr(&a.st->status, 2);
}

__global__ __launch_bounds__(256) void k_cc_hist(CcArgs a) {
  if (a.st->status) return;
  const int f = cc_tid(a.nt);
  if (f < 0) return;
  const int v[3] = {a.tri[3 * f], a.tri[3 * f + 1], a.tri[3 * f + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicAdd(&a.ehead[cc_min(v[k], v[(k + 1) % 3])], 1);
    atomicAdd(&a.vhead[v[k]], 1);
  }
  a.parent[f] = f;
}

// block-local exclusive scan in place + the block's sum (k_scan_blocks turns the sums into block offsets)
__global__ __launch_bounds__(256) void k_cc_scan(int* __restrict__ data, int n, int* __restrict__ bsum) {
  __shared__ int sh[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int v = i < n ? data[i] : 0;
  int total;
  const int ex = block_excl_scan_256(v, sh, total);
  if (i < n) data[i] = ex;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_cc_fill(CcArgs a) {
  if (a.st->status) return;
  const int f = cc_tid(a.nt);
  if (f < 0) return;
  const int v[3] = {a.tri[3 * f], a.tri[3 * f + 1], a.tri[3 * f + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int x = v[k], y = v[(k + 1) % 3];
    const int lo = cc_min(x, y), hi = cc_max(x, y);
    // the cursors count exactly what k_cc_hist counted, so a slot stays inside its bucket
    const int pe = cc_off(a.ehead, a.bs_e, lo) + atomicAdd(&a.ecur[lo], 1);
    a.erec[pe] = make_int2(hi, f);
    const int pv = cc_off(a.vhead, a.bs_v, x) + atomicAdd(&a.vcur[x], 1);
    a.vrec[pv] = 3 * f + k;
  }
}

__device__ __forceinline__ int cc_parent(const int* p, int x) {
  return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x while other workgroups hook and shorten: parent[] only decreases, so the walk is bounded by x.
// The second walk points the path at the root found where it does not point there already (atomicMin:
// never raises a parent, and the new parent is an ancestor, so every chain still ends at its component's root).
__device__ __forceinline__ int cc_find(int* parent, int x) {
  int r = x;
  for (int p = cc_parent(parent, r); p != r; p = cc_parent(parent, r)) r = p;
  while (x > r) {
    const int p = cc_parent(parent, x);
    if (p > r) atomicMin(&parent[x], r);
    x = p;
  }
  return r;
}

__device__ __forceinline__ void cc_union(int* parent, int x, int y) {
  x = cc_find(parent, x);
  y = cc_find(parent, y);
  while (x != y) {
    if (x < y) {
      const int t = x;
      x = y;
      y = t;
    }
    // hook the larger root x onto the smaller root y; a failed CAS returns x's new parent, which is lower
    const int old = atomicCAS(&parent[x], x, y);
    if (old == x) return;
    x = cc_find(parent, old);
    y = cc_find(parent, y);
  }
}

__global__ __launch_bounds__(256) void k_cc_union(CcArgs a) {
  if (a.st->status) return;
  const int f = cc_tid(a.nt);
  if (f < 0) return;
  const int v[3] = {a.tri[3 * f], a.tri[3 * f + 1], a.tri[3 * f + 2]};
  int bad = 0;
  for (int k = 0; k < 3; ++k) {
    const int x = v[k], y = v[(k + 1) % 3];
    const int lo = cc_min(x, y), hi = cc_max(x, y);
    const int b0 = cc_off(a.ehead, a.bs_e, lo), b1 = cc_off(a.ehead, a.bs_e, lo + 1);
    int mult = 0, low = f;
    for (int j = b0; j < b1; ++j) {
      const int2 r = a.erec[j];
      if (r.x == hi) {
        ++mult;
        low = cc_min(low, r.y);
      }
    }
    bad |= mult != 2;
    if (low < f) cc_union(a.parent, f, low);
  }
  a.fbad[f] = (uint8_t)bad;
}

__global__ __launch_bounds__(256) void k_cc_flatten(CcArgs a) {
  if (a.st->status) return;
  const int f = cc_tid(a.nt);
  if (f < 0) return;
  int r = f;
  for (int p = a.parent[r]; p != r; p = a.parent[r]) r = p;  // p < r: bounded by f
  a.root[f] = r;
  if (a.fbad[f]) a.bad[r] = 1;
  if (r == f) atomicAdd(&a.st->ncomp, 1);
}

// One add per (wave, root) instead of one per corner: a large component would otherwise serialise a
// million adds on its one counter. The lanes of a wave that count for the root of the first such lane are
// summed by ballot, and the block's four waves merge those sums through LDS; lanes with another root (a
// wave that spans components) follow in at most 63 further rounds, each of which retires a lane.
__global__ __launch_bounds__(256) void k_cc_nverts(CcArgs a) {
  __shared__ int s_root[4], s_cnt[4];
  if (a.st->status) return;
  const int i = cc_tid(a.S);
  int r = -1;
  bool pending = false;  // this corner is the first of its vertex in its component
  if (i >= 0) {
    const int v = a.tri[i];
    r = a.root[i / 3];
    const int b0 = cc_off(a.vhead, a.bs_v, v), b1 = cc_off(a.vhead, a.bs_v, v + 1);
    pending = true;
    for (int j = b0; j < b1 && pending; ++j) {
      const int id = a.vrec[j];
      if (id < i && a.root[id / 3] == r) pending = false;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long m = __ballot(pending);
  int rl = -1, cnt = 0;
  if (m) {
    rl = __shfl(r, __ffsll((long long)m) - 1);
    const bool mine = pending && r == rl;
    cnt = __popcll(__ballot(mine));
    if (mine) pending = false;
  }
  if (lane == 0) {
    s_root[w] = rl;
    s_cnt[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_root[threadIdx.x] >= 0) {
    // the lowest wave with this root adds for all of them
    const int mr = s_root[threadIdx.x];
    int total = 0;
    bool owner = true;
    for (int k = 0; k < 4; ++k)
      if (s_root[k] == mr) {
        owner = owner && k >= (int)threadIdx.x;
        total += s_cnt[k];
      }
    if (owner) atomicAdd(&a.nverts[mr], total);
  }
  for (int round = 0; round < 63; ++round) {
    m = __ballot(pending);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    rl = __shfl(r, leader);
    const bool mine = pending && r == rl;
    cnt = __popcll(__ballot(mine));
    if (lane == leader) atomicAdd(&a.nverts[rl], cnt);
    if (mine) pending = false;
  }
}

__global__ __launch_bounds__(256) void k_cc_select(CcArgs a) {
  if (a.st->status) return;
  const int f = cc_tid(a.nt);
  if (f < 0 || a.root[f] != f || a.bad[f]) return;
  atomicAdd(&a.st->nwt, 1);
  atomicMax(&a.st->best, ((unsigned long long)(unsigned)a.nverts[f] << 32) | (0xFFFFFFFFu - (unsigned)f));
}

__global__ __launch_bounds__(256) void k_cc_flags(CcArgs a) {
  if (a.st->status) return;
  const unsigned long long best = a.st->best;
  if (!best) return;
  const int f = cc_tid(a.nt);
  if (f < 0 || a.root[f] != (int)(0xFFFFFFFFu - (unsigned)best)) return;
  a.fkeep[f] = 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.vkeep[a.tri[3 * f + k]] = 1;  // every writer stores the same 1
}

__global__ __launch_bounds__(256) void k_cc_finish(CcArgs a, int32_t* __restrict__ counts, int32_t* __restrict__ labels) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  const int status = a.st->status;
  const unsigned long long best = a.st->best;
  if (f == 0) {
    int32_t c[ANR_MESHCC_NCOUNT];
    if (status) {
      c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 0; c[4] = -1; c[5] = 2;
    } else if (!best) {
      c[0] = a.nv; c[1] = a.nt; c[2] = a.st->ncomp; c[3] = 0; c[4] = -1; c[5] = 1;
    } else {
      c[0] = a.st->vout; c[1] = a.st->tout; c[2] = a.st->ncomp; c[3] = a.st->nwt;
      c[4] = (int32_t)(0xFFFFFFFFu - (unsigned)best); c[5] = 0;
    }
    for (int k = 0; k < ANR_MESHCC_NCOUNT; ++k) {
      a.st->counts[k] = c[k];
      counts[k] = c[k];
    }
  }
  if (labels && f < a.nt) labels[f] = status ? -1 : a.root[f];
}

__global__ __launch_bounds__(256) void k_cc_emit_faces(CcArgs a, int64_t* __restrict__ out) {
  const int status = a.st->counts[5];
  if (status == 2) return;
  const int f = cc_tid(a.nt);
  if (f < 0) return;
  if (status == 1) {
    for (int k = 0; k < 3; ++k) out[3 * (size_t)f + k] = a.tris[3 * (size_t)f + k];
    return;
  }
  if (a.root[f] != a.st->counts[4]) return;
  const size_t o = (size_t)cc_off(a.fkeep, a.bs_f, f);
  for (int k = 0; k < 3; ++k) out[3 * o + k] = (int64_t)cc_off(a.vkeep, a.bs_k, a.tri[3 * f + k]);
}

__global__ __launch_bounds__(256) void k_cc_emit_verts(CcArgs a, const double* __restrict__ verts, double* __restrict__ out) {
  const int status = a.st->counts[5];
  if (status == 2) return;
  const int v = cc_tid(a.nv);
  if (v < 0) return;
  size_t o = (size_t)v;
  if (status == 0) {
    const int o0 = cc_off(a.vkeep, a.bs_k, v), o1 = cc_off(a.vkeep, a.bs_k, v + 1);
    if (o1 == o0) return;
    o = (size_t)o0;
  }
  for (int k = 0; k < 3; ++k) out[3 * o + k] = verts[3 * (size_t)v + k];
}

bool cc_sizes_ok(long nv, long nt) { return nv >= 0 && nt >= 0 && 3 * nt < (1L << 31) && nv < (1L << 31) - 1; }

int cc_check(const char* who, long nt, long nv, const void* ws, size_t ws_bytes) {
  if (nt < 0 || nv < 0) return fail(ANR_E_ARG, std::string(who) + ": nt and nv must not be negative");
  if (!cc_sizes_ok(nv, nt)) return fail(ANR_E_ARG, std::string(who) + ": 3 nt and nv + 1 must be below 2^31");
  if (!ws) return fail(ANR_E_ARG, std::string(who) + ": NULL workspace");
  if (ws_bytes < cc_layout(nv, nt).total) return fail(ANR_E_WORKSPACE, std::string(who) + ": workspace too small");
  return ANR_OK;
}

unsigned cc_blocks(long n) { return (unsigned)(n > 0 ? (n + 255) / 256 : 1); }

// data (n) -> exclusive offsets (block-local in data, per block in bsum), the total to *total
int cc_scan(int* data, long n, int* bsum, int* total, hipStream_t s) {
  const unsigned nb = cc_blocks(n);
  hipLaunchKernelGGL(k_cc_scan, dim3(nb), dim3(256), 0, s, data, (int)n, bsum);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, bsum, (int)nb, total);
  return check_launch("k_cc_scan");
}

}  // namespace

extern "C" {

size_t anr_mesh_cc_workspace_bytes(long nv, long nt) {
  if (!cc_sizes_ok(nv, nt)) return 0;
  return cc_layout(nv, nt).total;
}

int anr_mesh_cc_count(const int64_t* triangles, long nt, long nv, int32_t* counts, int32_t* labels, void* workspace,
                      size_t ws_bytes, void* stream) {
  ANR_TRY(cc_check("anr_mesh_cc_count", nt, nv, workspace, ws_bytes));
  if (!counts) return fail(ANR_E_ARG, "anr_mesh_cc_count: NULL counts");
  if (!triangles && nt > 0) return fail(ANR_E_ARG, "anr_mesh_cc_count: NULL triangles");
  const CcLayout L = cc_layout(nv, nt);
  CcArgs a = cc_args(triangles, nt, nv, (char*)workspace);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync((char*)workspace + L.st, 0, L.zero_end - L.st, s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_mesh_cc_count: hipMemsetAsync failed");
  const unsigned fb = cc_blocks(nt), sb = cc_blocks(3 * nt);
  hipLaunchKernelGGL(k_cc_validate, dim3(sb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_validate"));
  hipLaunchKernelGGL(k_cc_hist, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_hist"));
  // (the histogram totals land in vout / tout and are overwritten by the flag scans below)
  ANR_TRY(cc_scan(a.ehead, nv + 1, a.bs_e, &a.st->vout, s));
  ANR_TRY(cc_scan(a.vhead, nv + 1, a.bs_v, &a.st->tout, s));
  hipLaunchKernelGGL(k_cc_fill, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_fill"));
  hipLaunchKernelGGL(k_cc_union, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_union"));
  hipLaunchKernelGGL(k_cc_flatten, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_flatten"));
  hipLaunchKernelGGL(k_cc_nverts, dim3(sb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_nverts"));
  hipLaunchKernelGGL(k_cc_select, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_select"));
  hipLaunchKernelGGL(k_cc_flags, dim3(fb), dim3(256), 0, s, a);
  ANR_TRY(check_launch("k_cc_flags"));
  ANR_TRY(cc_scan(a.vkeep, nv + 1, a.bs_k, &a.st->vout, s));
  ANR_TRY(cc_scan(a.fkeep, nt + 1, a.bs_f, &a.st->tout, s));
  hipLaunchKernelGGL(k_cc_finish, dim3(fb), dim3(256), 0, s, a, counts, labels);
  return check_launch("k_cc_finish");
}

int anr_mesh_cc_emit(const double* vertices, const int64_t* triangles, long nt, long nv, double* out_vertices,
                     int64_t* out_triangles, void* workspace, size_t ws_bytes, void* stream) {
  ANR_TRY(cc_check("anr_mesh_cc_emit", nt, nv, workspace, ws_bytes));
  if ((!vertices || !out_vertices) && nv > 0) return fail(ANR_E_ARG, "anr_mesh_cc_emit: NULL vertices");
  if ((!triangles || !out_triangles) && nt > 0) return fail(ANR_E_ARG, "anr_mesh_cc_emit: NULL triangles");
  CcArgs a = cc_args(triangles, nt, nv, (char*)workspace);
  hipStream_t s = (hipStream_t)stream;
  if (nt > 0) {
    hipLaunchKernelGGL(k_cc_emit_faces, dim3(cc_blocks(nt)), dim3(256), 0, s, a, out_triangles);
    ANR_TRY(check_launch("k_cc_emit_faces"));
  }
  if (nv > 0) {
    hipLaunchKernelGGL(k_cc_emit_verts, dim3(cc_blocks(nv)), dim3(256), 0, s, a, vertices, out_vertices);
    ANR_TRY(check_launch("k_cc_emit_verts"));
  }
  return ANR_OK;
}

}  // extern "C"
