// anr_knn_host.hip — the shared host stage of the KNN-skinned render paths (anr_knn_host.h). The only launch sites of
// k_sdf_front, the three-launch compaction of these paths and k_pack_seq / k_pack_seq_x6. Host code only.
#include "anr_knn_host.h"

#include <cstdlib>
#include <string>

namespace anr {

namespace {

int launch_front(const SdfFrontArgs& fa, const char* who, hipStream_t s) {
  hipLaunchKernelGGL(k_sdf_front, dim3(std::min(num_cus(), (fa.n_rays + 15) / 16)), dim3(1024), 0, s, fa);
  return check_launch((std::string("k_sdf_front (") + who + ")").c_str());
}

}  // namespace

int knn_front_compact(SdfFrontArgs& fa, char* ws, const KnnFrontLayout& L, const float* tbounds, float* tbounds_out,
                      bool filt, const char* who, hipStream_t s, int* n_kept) {
  const int R = fa.n_rays, nch = (R + fa.chunk - 1) / fa.chunk;
  const std::string w(who);
  int* counts = (int*)(ws + L.counts);
  fa.mask = (uint64_t*)(ws + L.mask);
  fa.chunk_min = (uint64_t*)(ws + L.chunk_min);
  fa.knn = (uint32_t*)(ws + L.knn);
  if (hipMemsetAsync(counts, 0, 16, s) != hipSuccess ||
      hipMemsetAsync(fa.chunk_min, 0xff, (size_t)nch * 8, s) != hipSuccess)
    return fail(ANR_E_HIP, w + ": memset");
  float* tbtab = (float*)(ws + L.tbtab);
  if (tbounds && !filt) {
    hipLaunchKernelGGL(k_sdf_tbtab, dim3(1), dim3(64), 0, s, tbounds, nch, tbtab, tbounds_out, nullptr);
    ANR_TRY(check_launch(("k_sdf_tbtab (" + w + ")").c_str()));
  }
  ANR_TRY(launch_front(fa, who, s));
  if (tbounds && filt) {
    hipLaunchKernelGGL(k_sdf_tbtab, dim3(1), dim3(64), 0, s, tbounds, nch, tbtab, tbounds_out,
                       (const uint64_t*)fa.chunk_min);
    ANR_TRY(check_launch(("k_sdf_tbtab (" + w + ", visible chunks)").c_str()));
  }
  CompactArgs ca{};
  ca.n_rays = R; ca.chunk = fa.chunk; ca.mask = fa.mask; ca.chunk_min = fa.chunk_min;
  ca.ray_off = (int*)(ws + L.ray_off); ca.block_sum = (int*)(ws + L.block_sum); ca.list = (int*)(ws + L.list);
  const int nb = (R + 255) / 256;
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(256), 0, s, ca);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, ca.block_sum, nb, counts);
  hipLaunchKernelGGL(k_compact, dim3((R + 3) / 4), dim3(256), 0, s, ca);
  ANR_TRY(check_launch(("k_compact (" + w + ")").c_str()));
  if (n_kept &&
      (hipMemcpyAsync(n_kept, counts, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
    return fail(ANR_E_HIP, w + ": kept-count readback");
  return ANR_OK;
}

int knn_free_setup(char* ws, const KnnFreeLayout& L, const char* who, hipStream_t s) {
  static const float ident[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  if (hipMemcpyAsync(ws + L.ident, ident, sizeof(ident), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemsetAsync(ws + L.cmin, 0xff, 8, s) != hipSuccess)
    return fail(ANR_E_HIP, std::string(who) + ": free-point search setup");
  return ANR_OK;
}

int knn_free_points(char* ws, const KnnFreeLayout& L, const float* pts, int n, const float* verts, int nv,
                    float norm_th, const char* who, hipStream_t s) {
  const float* rt = (const float*)(ws + L.ident);
  SdfFrontArgs fa{};
  fa.wpts = pts; fa.n_pts = n; fa.n_rays = fa.chunk = (n + 63) / 64;
  fa.R = rt; fa.Th = rt + 9;
  fa.verts = verts; fa.nv = nv; fa.norm_th = norm_th;
  fa.mask = (uint64_t*)(ws + L.mask); fa.chunk_min = (uint64_t*)(ws + L.cmin);
  fa.knn = (uint32_t*)(ws + L.knn); fa.raw = (float4*)(ws + L.raw); fa.sdf = (float*)(ws + L.sdf);
  return launch_front(fa, who, s);
}

int SeqImages::pack(const PackArgs& pa, int L0, int nl, int skip_layer, float scale) const {
  const int nt = x6 ? seq_x6_pack_threads(L0, nl) : seq_pack_threads(L0, nl);
  if (x6) hipLaunchKernelGGL(k_pack_seq_x6, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, skip_layer, scale);
  else hipLaunchKernelGGL(k_pack_seq, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, skip_layer, scale);
  return check_launch((std::string(x6 ? "k_pack_seq_x6 (" : "k_pack_seq (") + who + ")").c_str());
}

int SeqImages::pack_density(const float* const* WN, const float* const* tp, unsigned char* out) const {
  PackArgs pa{};
  for (int l = 0; l < 9; ++l) {
    pa.t[l] = WN[l];
    pa.t[9 + l] = tp[3 * l];
  }
  pa.out = out;
  return pack(pa, ANR_L_SDF0, ANR_SDF_LAYERS, 4, 1.0f / 1.41421356237309515f);
}

int SeqImages::pack_colour(const float* const* WN, const float* const* tp, int clin0, int L0, int nl,
                           unsigned char* out) const {
  PackArgs pa{};
  for (int l = 0; l < 5; ++l) {
    pa.t[l] = WN[9 + l];
    pa.t[9 + l] = l == 3 ? nullptr : tp[clin0 + 3 * l];
  }
  pa.out = out;
  return pack(pa, L0, nl, -1, 1.0f);
}

int SeqImages::pack_skip8(const float* const* tp, int lin0, int fc_w, int fc_b, int L0, int nl,
                          unsigned char* out) const {
  PackArgs pa{};
  for (int l = 0; l < 8; ++l) {
    pa.t[l] = tp[lin0 + 2 * l];
    pa.t[9 + l] = l == 0 || l == 5 ? nullptr : tp[lin0 + 2 * l + 1];
  }
  pa.t[8] = tp[fc_w];
  pa.t[17] = tp[fc_b];
  pa.out = out;
  return pack(pa, L0, nl, -1, 1.0f);
}

int launch_density_colour(const SeqImages& im, unsigned char* dimg, unsigned char* cimg, const float* fold,
                          const float* C0, float* Y8, float* Yc, int cnt, int cus) {
  MlpArgs da{};
  im.bind(da, dimg, ANR_L_SDF0, ANR_SDF_LAYERS);
  da.ptb = C0;
  da.ptb_ld = 40;
  da.y8 = Y8;
  da.n_rows = cnt;
  if (launch_lbw_density(da, cus, im.s, im.x6) != 0)
    return fail(ANR_E_HIP, std::string("k_lbw_density launch failed (") + im.who + ")");
  if (!cimg) return ANR_OK;
  MlpArgs ca{};
  im.bind(ca, cimg, ANR_L_LCOL0, ANR_LCOL_LAYERS);
  ca.fold = fold;
  ca.ptb = C0;
  ca.ptb_ld = 40;
  ca.y8 = Y8;
  ca.yr = Yc;
  ca.n_rows = cnt;
  if (launch_lbw_color(ca, cus, im.s, im.x6) != 0)
    return fail(ANR_E_HIP, std::string("k_lbw_color launch failed (") + im.who + ")");
  return ANR_OK;
}

long batch_rows(const char* env, long cap) {
  const char* v = getenv(env);
  if (!v || !v[0]) return cap;
  const long b = atol(v);
  return (b >= 256 && b <= cap && b % 256 == 0) ? b : cap;
}

int check_knn_common(const char* who, bool structs_ok, const float* ray_o, const float* ray_d, const float* near_,
                     const float* far_, int R, const anr_render_opts* o, const void* ws, long max_samples,
                     const char* novel_msg, bool check_precision) {
  const std::string w = std::string(who) + ": ";
  if (!structs_ok || !o || !ws || !ray_o || !ray_d || !near_ || !far_) return fail(ANR_E_ARG, w + "NULL argument");
  if (o->n_samples != 64) return fail(ANR_E_ARG, w + "only N_samples == 64 is supported");
  if (o->chunk <= 0 || R <= 0 || (max_samples && (long)R * 64 > max_samples))
    return fail(ANR_E_ARG, w + "bad chunk / n_rays");
  if (o->novel_pose) return fail(ANR_E_ARG, w + novel_msg);
  if (check_precision && !precision_ok(o->precision))
    return fail(ANR_E_ARG, w + "precision must be ANR_FP32, ANR_BF16X3 or ANR_BF16X6");
  return ANR_OK;
}

int check_knn_frame(const char* who, int n_verts, bool outputs_ok, int n_views, const float* Ks, const float* RT,
                    const uint8_t* msks, int img_h, int img_w) {
  const std::string w = std::string(who) + ": ";
  if (!n_verts_ok(n_verts)) return fail(ANR_E_ARG, w + "n_verts must be in [1, 6912]");
  if (!outputs_ok) return fail(ANR_E_ARG, w + "NULL output");
  if (n_views < 0 || (n_views > 0 && (!Ks || !RT || !msks || img_h <= 0 || img_w <= 0)))
    return fail(ANR_E_ARG, w + "bad visibility-filter views");
  return ANR_OK;
}

}  // namespace anr
