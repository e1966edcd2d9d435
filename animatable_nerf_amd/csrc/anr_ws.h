// anr_ws.h — render workspace layout (shared by the render and training entry points).
#pragma once
#include <stddef.h>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/aninerf.h"
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

// image: the image-only render on a layout_image() workspace (no T-pose volume, rows or alpha_ind state)
// x != NULL: free samples (Network.forward): R = ceil(n_pts / 64) groups of 64 samples, the caller's
// opts with chunk = R (the whole call is one reference chunk) and no t_rand; ray pointers unused
// nseg > 0 (anr_render_ns_fwd): N_samples = 64 * nseg. R, o->chunk and the layout are then in rows (a ray is
// nseg rows of 64 samples: R = n_rays * nseg, chunk = rays per chunk * nseg) for stage_frontend, stage_mlp and
// stage_alpha_ind, whose compaction and alpha_ind kernels run over rows as over rays; stage_composite takes rays.
// nseg == 0: the 64-sample kernels.
int stage_frontend(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d, const float* near_,
                   const float* far_, int R, const anr_render_opts* o, char* ws, const Layout& L, float4* raw,
                   hipStream_t s, const anr_samples* x = nullptr, const RaySplit* split = nullptr, bool image = false,
                   int nseg = 0);
int stage_mlp(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d, const float* near_,
              const float* far_, int R, const anr_render_opts* o, char* ws, const Layout& L, float4* raw,
              hipStream_t s, const anr_samples* x = nullptr, bool image = false, int nseg = 0);
int stage_alpha_ind(int R, const anr_render_opts* o, char* ws, const Layout& L, hipStream_t s,
                    const RaySplit* split = nullptr);
int stage_composite(const float* near_, const float* far_, int R, const anr_render_opts* o, const float4* raw,
                    const anr_render_out* out, float* weights, hipStream_t s, int nseg = 0);

}  // namespace anr
