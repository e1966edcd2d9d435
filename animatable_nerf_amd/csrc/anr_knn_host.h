// anr_knn_host.h — host side shared by the KNN-skinned render paths (sdf_pdf, aligned_aninerf_lbw,
// aligned_aninerf_pdf: anr_sdf_capi.hip, anr_lbw_capi.hip, anr_pdf_capi.hip) and the sdf_pdf training front-end
// (anr_sdf_train.hip): the workspace prefix of the front-end, the front-end + ordered compaction stage, the
// free-point KNN search, the packing and binding of the fused programs' images, and the argument checks the three
// C-ABI files have in common. Helpers take data (offsets, pointers, thresholds, layer-table ids), never the network.
// Definitions: anr_knn_host.hip. Host code only.
#pragma once
#include <algorithm>

#include "anr_kernels.h"
#include "anr_sdf.h"
#include "anr_ws.h"

namespace anr {

// the regions every KNN front-end call carves first, counts at offset 0 (the *_render_counts accessors)
struct KnnFrontLayout {
  size_t counts, mask, chunk_min, ray_off, block_sum, list, knn, tbtab;
  void carve(Carve& c, size_t R, int chunk) {
    const size_t nch = (R + chunk - 1) / (size_t)std::max(chunk, 1);
    counts = c.bytes(16);
    mask = c.bytes(R * 8);
    chunk_min = c.bytes(nch * 8);
    ray_off = c.bytes((R + 1) * 4);
    block_sum = c.bytes(((R + 255) / 256) * 4);
    list = c.bytes(R * 64 * 4);
    knn = c.bytes(R * 64 * 32);
    tbtab = c.bytes(nch * 6 * 4);
  }
};

// a fused program's image: bf16x3 (k_pack_seq) or bf16x6 (k_pack_seq_x6), sized for the larger
inline size_t carve_seq_image(Carve& c, int L0, int nl) {
  return c.bytes((size_t)std::max(seq_image_bytes(L0, nl), x6seq_image_bytes(L0, nl)));
}

// The front-end + ordered compaction over fa's rays or free-point groups. Sets fa.mask / chunk_min / knn from L,
// presets counts and chunk_min, runs k_sdf_tbtab (tbounds NULL: none) before the front-end, or, with the
// visibility filter (filt: the widening depends on which chunks keep a sample), after it over chunk_min, then
// k_sdf_front on min(cus, ceil(R / 16)) workgroups and k_count / k_scan_blocks / k_compact. n_kept != NULL: the
// stream-synchronised host read of n'. `who` prefixes the error texts.
int knn_front_compact(SdfFrontArgs& fa, char* ws, const KnnFrontLayout& L, const float* tbounds, float* tbounds_out,
                      bool filt, const char* who, hipStream_t s, int* n_kept);

// KNN search of free points against a vertex set (sample_blend_closest_points): k_sdf_front in free-sample mode over
// G = ceil(n / 64) groups that form one chunk, world -> pose with R = I, Th = 0 (the identity in fp32:
// x * 1 + y * 0 + z * 0)
struct KnnFreeLayout {
  size_t ident, mask, cmin, knn, raw, sdf;  // R | Th (12 floats), (G x 8), 8, (64 G x 32), (64 G x 16), (64 G x 4)
  void carve(Carve& c, size_t G) {
    ident = c.bytes(64);
    mask = c.bytes(G * 8);
    cmin = c.bytes(8);
    knn = c.bytes(G * 64 * 32);
    raw = c.bytes(G * 64 * 16);
    sdf = c.bytes(G * 64 * 4);
  }
};
// once per call: the identity upload and the chunk_min preset
int knn_free_setup(char* ws, const KnnFreeLayout& L, const char* who, hipStream_t s);
int knn_free_points(char* ws, const KnnFreeLayout& L, const float* pts, int n, const float* verts, int nv,
                    float norm_th, const char* who, hipStream_t s);

// the fused programs' layer-sequence images of one render call (who: the error texts' suffix)
struct SeqImages {
  hipStream_t s;
  bool x6;
  const char* who;
  // the image of layers L0 .. L0 + nl - 1 from pa (layer L0 + skip_layer scaled by scale; -1: none)
  int pack(const PackArgs& pa, int L0, int nl, int skip_layer, float scale) const;
  // the image's weight bytes (the bias section follows them)
  size_t wbytes(int L0, int nl) const { return x6 ? x6seq_wbytes(L0, nl) : seq_wbytes(L0, nl); }
  void bind(MlpArgs& a, unsigned char* img, int L0, int nl) const {
    a.wimg = img;
    a.bias = (const float*)(img + wbytes(L0, nl));
  }
  // the density / SDF net: 9 weight-normed layers WN[0..8], biases tp[3 l], the skip at entry 4 with 1 / sqrt2
  int pack_density(const float* const* WN, const float* const* tp, unsigned char* out) const;
  // a colour net: 5 weight-normed layers WN[9..13], biases tp[clin0 + 3 l]; lin3's bias is the latent fold
  int pack_colour(const float* const* WN, const float* const* tp, int clin0, int L0, int nl, unsigned char* out) const;
  // an 8-layer-plus-fc skip MLP: weights tp[lin0 + 2 l], biases tp[lin0 + 2 l + 1]; layers 0 / 5: folded biases
  int pack_skip8(const float* const* tp, int lin0, int fc_w, int fc_b, int L0, int nl, unsigned char* out) const;
};

// the fused density and colour programs of aligned_aninerf_lbw / _pdf over cnt rows (cimg NULL: no colour net)
int launch_density_colour(const SeqImages& im, unsigned char* dimg, unsigned char* cimg, const float* fold,
                          const float* C0, float* Y8, float* Yc, int cnt, int cus);

// kept samples per batch: cap, or the test override in `env` (a multiple of 256 in [256, cap]); read per call
long batch_rows(const char* env, long cap);

inline bool opts_ok(int n_rays, const anr_render_opts* o) { return n_rays > 0 && o && o->chunk > 0; }
inline bool precision_ok(int p) { return p == ANR_FP32 || p == ANR_BF16X3 || p == ANR_BF16X6; }
inline bool n_verts_ok(int nv) { return nv > 0 && nv <= 6912; }

// the argument checks of a render call, in the order of the C-ABI files: NULL arguments (structs_ok: the caller's
// params / frame / out), N_samples, chunk / ray range (max_samples 0: no upper bound), novel_pose (novel_msg),
// the precision set (check_precision)
int check_knn_common(const char* who, bool structs_ok, const float* ray_o, const float* ray_d, const float* near_,
                     const float* far_, int R, const anr_render_opts* o, const void* ws, long max_samples,
                     const char* novel_msg, bool check_precision);
// ... and after the caller's tensor checks: n_verts, the outputs, the visibility-filter views
int check_knn_frame(const char* who, int n_verts, bool outputs_ok, int n_views, const float* Ks, const float* RT,
                    const uint8_t* msks, int img_h, int img_w);

}  // namespace anr
