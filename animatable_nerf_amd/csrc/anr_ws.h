// anr_ws.h — render workspace layout (shared by the render and training entry points).
#pragma once
#include <stddef.h>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/aninerf.h"
#include "anr_kernels.h"
#include "anr_layers.h"

namespace anr {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Carves a workspace into 256-B aligned regions, in call order: each call returns the offset of its
// region; `o` is then the total so far. A layout that continues another's starts at that one's total.
struct Carve {
  size_t o = 0;
  size_t bytes(size_t n) {
    const size_t at = o;
    o = align256(o + n);
    return at;
  }
  size_t floats(size_t n) { return bytes(n * 4); }
};

// Workspace layout. Fields up to `tbw_rows` depend only on n_rays (anr_render_counts/bw_rows).
struct Layout {
  size_t counts, mask, ray_off, block_sum, list, sigma, flags, block_sum2, out_row, pbw_rows, tbw_rows;
  size_t chunk_min, chunk_max, raw, pbw32, tbw32, pn24, fold, total;
};

inline Layout layout(int n_rays, int chunk, long np, long nt, bool need_raw) {
  Layout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  Carve c;
  L.counts = c.bytes(16);
  L.mask = c.bytes(R * 8);
  L.ray_off = c.bytes((R + 1) * 4);
  L.block_sum = c.bytes(((R + 255) / 256) * 4);
  L.list = c.bytes(N * 4);
  L.sigma = c.bytes(N * 4);
  L.flags = c.bytes(N);
  L.block_sum2 = c.bytes(((N + 1023) / 1024) * 4);
  L.out_row = c.bytes(N * 4);
  L.pbw_rows = c.bytes(N * 24 * 4);
  L.tbw_rows = c.bytes(N * 24 * 4);
  const size_t nch = (R + chunk - 1) / (chunk > 0 ? chunk : 1);
  L.chunk_min = c.bytes(nch * 8);
  L.chunk_max = c.bytes(nch * 8);
  L.raw = need_raw ? c.bytes(N * 16) : 0;
  L.pbw32 = c.bytes((size_t)np * 32 * 4);
  L.tbw32 = c.bytes((size_t)nt * 32 * 4);
  L.pn24 = c.bytes((size_t)np * 4);
  L.fold = c.bytes(ANR_FOLD_FLOATS * 4);
  L.total = c.o;
  return L;
}

// Image-only render (anr_render_image_fwd): what the front-end, the image program and the compositing
// touch. No sigma, flags, block_sum2, out_row, pbw_rows, tbw_rows, chunk_max, tbw32: those fields stay 0
// and nothing of an image render may read them. counts is at offset 0 as in layout() (anr_render_counts).
inline Layout layout_image(int n_rays, int chunk, long np, bool need_raw) {
  Layout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  Carve c;
  L.counts = c.bytes(16);
  L.mask = c.bytes(R * 8);
  L.ray_off = c.bytes((R + 1) * 4);
  L.block_sum = c.bytes(((R + 255) / 256) * 4);
  L.list = c.bytes(N * 4);
  const size_t nch = (R + chunk - 1) / (chunk > 0 ? chunk : 1);
  L.chunk_min = c.bytes(nch * 8);
  L.raw = need_raw ? c.bytes(N * 16) : 0;
  L.pbw32 = c.bytes((size_t)np * 32 * 4);
  L.pn24 = c.bytes((size_t)np * 4);
  L.fold = c.bytes(ANR_FOLD_FLOATS * 4);
  L.total = c.o;
  return L;
}

int fail(int code, const std::string& msg);
int check_launch(const char* what);
// compute units of the current device, cached per device (256 where the query fails)
int num_cus();
#define ANR_TRY(x)                  \
  do {                              \
    const int _rc = (x);            \
    if (_rc != ANR_OK) return _rc;  \
  } while (0)

// ray split of one reference chunk over ranks (anr_train_hooks): ray offset + the host reduction hook
struct RaySplit {
  int ray_offset;
  anr_reduce_fn reduce;
  void* user;
  int run(void* buf, int count, int op, hipStream_t s) const;
};

// One call of the blend-volume path, filled once per entry and read by every stage. It owns nothing: every
// pointer is the caller's, nothing is allocated, and the stages only enqueue on `s`.
//   R, o.chunk, L  in rows. A row is 64 samples: a ray (nseg == 0, the 64-sample kernels), one of the nseg
//                  rows of a ray (nseg > 0, anr_render_ns_fwd: N_samples = 64 * nseg, the `_ns` kernels, also
//                  at nseg == 1), or a group of 64 free samples (x, Network.forward: o.chunk = R, the whole
//                  call is one reference chunk, no t_rand, ray pointers unused). The compaction and alpha_ind
//                  kernels run over rows as over rays.
//   image          the image-only render on a layout_image() workspace (no T-pose volume, rows or alpha_ind
//                  state); anr_alpha_points' workspace (alpha_layout) has the same front-end fields
//   split          ray split of the reference chunk over ranks (training), or NULL
// A caller of stage_alpha_ind or stage_composite alone (the KNN-skinned renders) fills what that stage reads.
struct VolCall {
  const anr_params* p;
  const anr_frame* f;
  const float *ray_o, *ray_d, *near_, *far_;
  int R;
  anr_render_opts o;
  char* ws;
  Layout L;
  float4* raw;
  hipStream_t s;
  const anr_samples* x;
  const RaySplit* split;
  bool image;
  int nseg;
};

// ---- argument checks of the blend-volume entries (anr_capi.hip) ----
// what an entry needs checked; `who` prefixes every message
struct VolCheck {
  const char* who;
  bool samples;  // free samples x and the caller's raw (anr_network_fwd); else rays, outputs, chunk, N_samples
  bool tbw;      // the T-pose volume (not the image-only renders)
  bool ns;       // N_samples 64, 128, 192 or 256 (anr_render_ns_fwd); else 64 alone
};
int check_vol_call(const VolCheck& k, const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d,
                   const float* near_, const float* far_, int n_rays, const anr_render_opts* o, const anr_render_out* out,
                   const anr_samples* x, const float* raw, const void* ws);
int check_novel(const std::string& who, const anr_params* p, const anr_frame* f);  // o->novel_pose: its tensors
int check_views(const std::string& who, const anr_frame* f);  // the visibility filter's views (n_views == 0: off)

// ---- stages (anr_capi.hip) ----
// parts of stage_frontend and stage_mlp that anr_alpha_points (anr_mesh.hip) runs with its own front-end launch:
// k_prep's arguments for the pose volume, the folded biases and the novel-pose tensors; the ordered compaction
// (one_launch: k_compact1, for R <= 1024; else k_count, k_scan_blocks, k_compact); the fused programs' arguments
// that every program reads (weights, folds, transforms, pose volume, kept list, pose-pass offsets)
PrepArgs prep_args(const VolCall& c);
int compact_rows(const VolCall& c, bool one_launch);
MlpArgs mlp_args(const VolCall& c);
// launch of one fused program: grid min(tiles, num_cus()), 512 threads, the program's LDS bytes; its
// dynamic-LDS attribute is set before its first launch in the process
int launch_alpha_program(const VolCall& c, MlpArgs& ma, long tiles);  // k_alpha* by c.o.precision

int stage_frontend(const VolCall& c);   // k_prep, front-end, [ray-split reduction], compaction: counts[0] = n'
int stage_mlp(const VolCall& c);        // the fused program by (c.image, c.nseg, c.o.precision)
int stage_alpha_ind(const VolCall& c);  // reads R, o.chunk, o.train_th, ws, L, s, split: counts[1] = m
// reads near_, far_, o.t_rand, raw, s, nseg; n_rays in rays (c.R / nseg under nseg > 0)
int stage_composite(const VolCall& c, int n_rays, const anr_render_out* out);

}  // namespace anr
