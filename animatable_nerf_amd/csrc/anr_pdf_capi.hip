// anr_pdf_capi.hip — C-ABI of the aligned_aninerf_pdf render path (include/aninerf.h, "aligned_aninerf_pdf variant").
//
// Sequence per render call (aligned_aninerf_pdf_network.py:97-138 under tpose_renderer.py:159-186):
//   k_lbw_wnorm / k_pdf_fold / k_sdf_tbtab (per-call weight and bounds preparation)
//   -> k_sdf_front over pvertices (KNN records, keep mask pnorm < 0.1, per-chunk argmin; the visibility filter when
//      the frame carries views) -> ordered compaction -> one host read of n'
//   -> per batch of <= P kept samples: k_pdf_warp (pbw, LBS to the big pose), the displacement MLP (poses folded
//      into layers 0 / 5) with resd = 0.05 tanh, tpose = init_bigpose + resd, the density net, the colour net
//      (color_latent folded into lin3), k_lbw_raw (reused through LbwPointArgs as it stands: it reads list / b0 /
//      cnt, Y8, Yc, ptp's dist column, C0's tpose columns, tbtab / chunk, and writes raw; sigma NULL)
//   -> compositing (k_composite).
// anr_pdf_alpha_points (Network.get_alpha :140-174 under aninerf_mesh_renderer's batchify): per chunk of chunk_pts
// points the same sequence in k_sdf_front's free-sample mode, without directions, colour net, box test and
// compositing; k_pdf_alpha_out scatters the density net's raw output 0.
// ANR_BF16X3 / ANR_BF16X6: each network is one fused launch per batch (anr_pdf_b16.hip / anr_pdf_x6.hip program
// V = 23 (+ 10) of anr_mlp_body.h, whose epilogue writes resd and tpose itself; anr_lbw_b16.hip / anr_lbw_x6.hip
// programs 21, 22 (+ 10)). ANR_FP32: 9 + 9 + 5 layer GEMMs through anr_gemm_seq.h with k_pdf_mid between the
// displacement and the density layers. The front-end + compaction stage, the image packing, the fused density /
// colour pair and the fp32 layer sequences are the KNN family's shared host code (anr_knn_host.h, anr_gemm_seq.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_gemm_seq.h"
#include "anr_kernels.h"
#include "anr_knn_host.h"
#include "anr_lbw.h"
#include "anr_pdf.h"
#include "anr_sdf.h"
#include "anr_train.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr long PDF_BATCH = 1L << 18;          // kept samples per batch
constexpr size_t PDF_LIMG_BYTES = 16u << 20;  // k_lgemm weight images (23 GEMMs, <= 448 KiB each)
constexpr float PDF_NORM_TH = 0.1f;           // aligned_aninerf_pdf_network.py:107 (not cfg.norm_th)

struct PLayout {
  KnnFrontLayout F;
  size_t wimg, fold, limg;
  size_t rimg, dimg, cimg;  // the fused programs' images: bf16x3 (k_pack_seq) or bf16x6 (k_pack_seq_x6)
  size_t resd_rows;         // full call only
  size_t ptp, Gr, Ha, Hb, Yr, Xs0, X4, C0, Y8, Yc;
  long P;
  size_t total;
};

PLayout playout(int n_rays, int chunk, bool image) {
  PLayout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  Carve c;
  L.F.carve(c, R, chunk);
  L.wimg = c.bytes(LBW_WN_FLOATS * 4);
  L.fold = c.bytes(PDF_FOLD_FLOATS * 4);
  L.limg = c.bytes(PDF_LIMG_BYTES);
  L.rimg = carve_seq_image(c, ANR_L_RESD0, ANR_RESD_LAYERS);
  L.dimg = carve_seq_image(c, ANR_L_SDF0, ANR_SDF_LAYERS);
  L.cimg = carve_seq_image(c, ANR_L_LCOL0, ANR_LCOL_LAYERS);
  if (!image) L.resd_rows = c.bytes(N * 3 * 4);
  // the batch size: PDF_BATCH, or the test override ANR_PDF_BATCH
  const long P = (long)std::min<size_t>(N, (size_t)batch_rows("ANR_PDF_BATCH", PDF_BATCH));
  L.P = P;
  auto f = [&](long w) { return c.floats((size_t)P * w); };
  L.ptp = f(8); L.Gr = f(64); L.Ha = f(256); L.Hb = f(256); L.Yr = f(4);
  L.Xs0 = f(40); L.X4 = f(256); L.C0 = f(40); L.Y8 = f(264); L.Yc = f(4);
  L.total = c.o;
  return L;
}

bool alpha_opts_ok(long n_pts, const anr_alpha_opts* o) {
  return n_pts > 0 && n_pts <= (1L << 24) && o && o->chunk_pts > 0 && o->chunk_pts % 64 == 0;
}
// groups of 64 points of the largest chunk of a get_alpha call
int alpha_groups(long n_pts, const anr_alpha_opts* o) { return (int)((std::min<long>(n_pts, o->chunk_pts) + 63) / 64); }

int check(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d, const float* near_,
          const float* far_, int R, const anr_render_opts* o, const anr_pdf_render_out* out, void* ws) {
  ANR_TRY(check_knn_common("pdf render", p && f && out, ray_o, ray_d, near_, far_, R, o, ws, 0x7fffffffL / 24,
                           "cfg.test_novel_pose is not supported", true));
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i)
    if (!p->t[i] && i != PDF_RESD_LAT) return fail(ANR_E_ARG, "pdf render: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->poses || !f->tbounds || !f->latent_index)
    return fail(ANR_E_ARG, "pdf render: NULL frame tensor");
  return check_knn_frame("pdf render", f->n_verts, out->rgb_map && out->acc_map && out->depth_map && out->raw,
                         f->n_views, f->Ks, f->RT, f->msks, f->img_h, f->img_w);
}

// the render sequence over rays (wpts NULL) or over the free points of one get_alpha chunk (wpts: n_pts points in
// R = ceil(n_pts / 64) groups that form one chunk; no directions, no colour net, no box test, no compositing: the raw
// density of the kept points goes to alpha, which the caller zeroed; out->raw is scratch for the front-end)
int pdf_core(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d, const float* near_,
             const float* far_, int R, int chunk, int precision, const float* t_rand, const anr_pdf_render_out* out,
             bool image, const PLayout& L, void* workspace, hipStream_t s, const float* wpts, int n_pts, float* alpha) {
  char* ws = (char*)workspace;
  float4* raw = (float4*)out->raw;

  // per-call weight preparation (weight norm, folds; the per-chunk tbounds: knn_front_compact)
  const float* const* tp = p->t;
  float* wimg = (float*)(ws + L.wimg);
  float* fold = (float*)(ws + L.fold);
  float* tbtab = (float*)(ws + L.F.tbtab);
  LbwTensors T{};
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i) T.t[i] = tp[i];
  hipLaunchKernelGGL(k_lbw_wnorm, dim3(lbw_wn_rows()), dim3(256), 0, s, T, wimg);
  ANR_TRY(check_launch("k_lbw_wnorm (pdf)"));
  hipLaunchKernelGGL(k_pdf_fold, dim3(wpts ? 2 : 3), dim3(256), 0, s, T, (const float*)wimg, f->poses, f->latent_index, fold);
  ANR_TRY(check_launch("k_pdf_fold"));
  const bool filt = !wpts && f->n_views > 0;  // visibility filter: widening depends on the front-end

  // front-end over pvertices + ordered compaction (free points: no box test, no tbounds table). Every sample's raw
  // is written here (zero where dropped) or by k_lbw_raw; the front-end's sdf output has no meaning for this network
  // and goes to the list region, which is free until k_compact.
  const int cus = num_cus();
  auto F = [&](size_t off) { return (float*)(ws + off); };
  SdfFrontArgs fa{};
  fa.ray_o = ray_o; fa.ray_d = ray_d; fa.near_ = near_; fa.far_ = far_; fa.t_rand = t_rand;
  fa.wpts = wpts; fa.n_pts = n_pts;
  fa.n_rays = R; fa.chunk = chunk; fa.R = f->R; fa.Th = f->Th; fa.verts = f->pvertices; fa.nv = f->n_verts;
  fa.norm_th = PDF_NORM_TH; fa.raw = raw;
  fa.sdf = (float*)(ws + L.F.list);
  if (filt) {
    fa.n_views = f->n_views; fa.Ks = f->Ks; fa.RT = f->RT; fa.msks = f->msks; fa.img_h = f->img_h; fa.img_w = f->img_w;
  }
  int n = 0;
  ANR_TRY(knn_front_compact(fa, ws, L.F, wpts ? nullptr : f->tbounds, out->tbounds_out, filt, "pdf render", s, &n));
  const int* list = (const int*)(ws + L.F.list);

  float *Ha = F(L.Ha), *Hb = F(L.Hb);
  const long P = L.P;
  const float* WN[LBW_NUM_WN];
  for (int l = 0; l < LBW_NUM_WN; ++l) WN[l] = wimg + lbw_wn_layer(l).off;
  LImgCache limg;
  limg.base = ws + L.limg;
  limg.cap = PDF_LIMG_BYTES;
  const float *Wr[8], *Br[8];
  for (int l = 0; l < 8; ++l) {
    Wr[l] = tp[PDF_RLIN0 + 2 * l];
    Br[l] = tp[PDF_RLIN0 + 2 * l + 1];
  }

  // split-bf16 precisions: the three networks as one fused launch per batch each, images packed once per call
  const bool x6 = precision == ANR_BF16X6;
  const bool fused = x6 || precision == ANR_BF16X3;
  const SeqImages im{s, x6, "pdf"};
  unsigned char* rimg = (unsigned char*)(ws + L.rimg);
  unsigned char* dimg = (unsigned char*)(ws + L.dimg);
  unsigned char* cimg = wpts ? nullptr : (unsigned char*)(ws + L.cimg);  // get_alpha: no colour net
  if (fused) {  // the displacement MLP's layer 0 / 5 biases: folded with the poses
    ANR_TRY(im.pack_skip8(tp, PDF_RLIN0, PDF_RFC_W, PDF_RFC_B, ANR_L_RESD0, ANR_RESD_LAYERS, rimg));
    ANR_TRY(im.pack_density(WN, tp, dimg));
    if (cimg) ANR_TRY(im.pack_colour(WN, tp, PDF_CLIN0, ANR_L_LCOL0, ANR_LCOL_LAYERS, cimg));
  }

  for (long b0 = 0; b0 < n; b0 += P) {
    const int cnt = (int)std::min<long>(P, n - b0);
    PdfPointArgs a{};
    a.list = list; a.b0 = (int)b0; a.cnt = cnt;
    a.ray_o = ray_o; a.ray_d = ray_d; a.near_ = near_; a.far_ = far_; a.t_rand = t_rand;
    a.wpts = wpts; a.n_pts = n_pts;
    a.R = f->R; a.Th = f->Th; a.A = f->A; a.bigA = f->big_A; a.weights = f->weights; a.knn = fa.knn;
    a.ptp = F(L.ptp); a.Gr = fused ? nullptr : F(L.Gr); a.Yr = F(L.Yr); a.Xs0 = F(L.Xs0); a.X4 = F(L.X4); a.C0 = F(L.C0);
    a.resd_rows = image ? nullptr : F(L.resd_rows);
    const dim3 pg((cnt + 255) / 256), pb(256);
    G g{s, cnt, 0, &limg, cus};  // the layer GEMMs of the exact-fp32 precision

    // pose space -> big pose: pbw, LBS for the point and the direction, dist
    hipLaunchKernelGGL(k_pdf_warp, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_pdf_warp"));

    if (fused) {
      // displacement: resd rows and tpose (C0 columns 0..2) come out of the program's epilogue
      MlpArgs ra{};
      im.bind(ra, rimg, ANR_L_RESD0, ANR_RESD_LAYERS);
      ra.fold = fold;
      ra.ptb = a.ptp;
      ra.ptb_ld = 8;
      ra.yr = image ? nullptr : F(L.resd_rows) + (size_t)b0 * 3;
      ra.gb = a.C0;
      ra.n_rows = cnt;
      if (launch_pdf_resd(ra, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_pdf_resd launch failed");
      ANR_TRY(launch_density_colour(im, dimg, cimg, fold, a.C0, F(L.Y8), F(L.Yc), cnt, cus));
    } else {
      // displacement MLP over gamma_10 in Gr -> Yr (poses folded into the biases of layers 0 / 5)
      ANR_TRY(g.skip8(F(L.Yr), 4, 3, Wr, Br, tp[PDF_RFC_W], tp[PDF_RFC_B], fold, fold + 256, a.Gr, 63, 135, 391, Ha, Hb,
                      false));
      hipLaunchKernelGGL(k_pdf_mid, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_pdf_mid"));
      // the density net, then the colour net over [tpose, gamma_4(tpose_dir)] || feature (color_latent folded into
      // lin3's bias, fold + 512)
      ANR_TRY(g.density_sp(WN, tp, a.Xs0, a.X4, F(L.Y8), Ha, Hb));
      if (!wpts) ANR_TRY(g.colour5(WN, tp, PDF_CLIN0, fold + 512, a.C0, F(L.Y8), F(L.Yc), Ha, Hb));
    }

    if (wpts) {  // get_alpha: the raw density, scattered to the chunk's rows
      hipLaunchKernelGGL(k_pdf_alpha_out, pg, pb, 0, s, list, (int)b0, cnt, (const float*)F(L.Y8), alpha);
      ANR_TRY(check_launch("k_pdf_alpha_out"));
      continue;
    }
    // raw2alpha with the real dists, sigmoid rgb, the per-chunk tbounds mask on tpose, scatter: k_lbw_raw as it is
    LbwPointArgs ra{};
    ra.list = list; ra.b0 = (int)b0; ra.cnt = cnt; ra.chunk = chunk; ra.tbtab = tbtab;
    ra.ptp = a.ptp; ra.C0 = a.C0; ra.Y8 = F(L.Y8); ra.Yc = F(L.Yc); ra.raw = raw; ra.sigma = nullptr;
    hipLaunchKernelGGL(k_lbw_raw, pg, pb, 0, s, ra);
    ANR_TRY(check_launch("k_lbw_raw (pdf)"));
  }

  if (wpts) return ANR_OK;
  VolCall v{};  // what stage_composite reads
  v.near_ = near_; v.far_ = far_; v.o.t_rand = t_rand; v.raw = raw; v.s = s;
  const anr_render_out ro{out->rgb_map, out->acc_map, out->depth_map, out->raw};
  return stage_composite(v, R, &ro);
}

}  // namespace

extern "C" {

size_t anr_pdf_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only) {
  if (!opts_ok(n_rays, o) || (long)n_rays * 64 > 0x7fffffffL / 24) return 0;
  return playout(n_rays, o->chunk, image_only != 0).total;
}

const int32_t* anr_pdf_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).F.counts);
}

const uint32_t* anr_pdf_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const uint32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).F.knn);
}

const int32_t* anr_pdf_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).F.list);
}

const float* anr_pdf_render_points(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const float*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).C0);
}

const float* anr_pdf_render_bigpose(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const float*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).ptp);
}

int anr_pdf_render_rows(const void* workspace, int n_rays, const anr_render_opts* o, float* resd, int32_t* ids,
                        void* stream) {
  if (!workspace || !opts_ok(n_rays, o)) return fail(ANR_E_ARG, "anr_pdf_render_rows: bad arguments");
  const PLayout L = playout(n_rays, o->chunk, false);
  const char* ws = (const char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int n = 0;
  if (hipMemcpyAsync(&n, ws + L.F.counts, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_pdf_render_rows: count readback");
  if (n < 0 || (long)n > (long)n_rays * 64) return fail(ANR_E_ARG, "anr_pdf_render_rows: not the workspace of a render call");
  if (n == 0) return ANR_OK;
  if (resd && hipMemcpyAsync(resd, ws + L.resd_rows, (size_t)n * 12, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_pdf_render_rows: copy");
  if (ids && hipMemcpyAsync(ids, ws + L.F.list, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_pdf_render_rows: copy");
  return ANR_OK;
}

int anr_pdf_render_fwd(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d,
                       const float* near_, const float* far_, int R, const anr_render_opts* o,
                       const anr_pdf_render_out* out, int image_only, void* workspace, size_t ws_bytes, void* stream) {
  const bool image = image_only != 0;
  ANR_TRY(check(p, f, ray_o, ray_d, near_, far_, R, o, out, workspace));
  const PLayout L = playout(R, o->chunk, image);
  if (ws_bytes < L.total) return fail(ANR_E_WORKSPACE, "pdf render: workspace too small");
  return pdf_core(p, f, ray_o, ray_d, near_, far_, R, o->chunk, o->precision, o->t_rand, out, image, L, workspace,
                  (hipStream_t)stream, nullptr, 0, nullptr);
}

// get_alpha: the layout of one chunk's call (G groups of 64 points forming one chunk, image-only: no resd rows)
// followed by the front-end's raw scratch (64 G float4)
size_t anr_pdf_alpha_workspace_bytes(long n_pts, const anr_alpha_opts* o) {
  if (!alpha_opts_ok(n_pts, o)) return 0;
  const int G = alpha_groups(n_pts, o);
  return playout(G, G, true).total + align256((size_t)G * 64 * 16);
}

int anr_pdf_alpha_points(const anr_pdf_params* p, const anr_pdf_frame* f, const float* wpts, long n_pts,
                         const anr_alpha_opts* o, float* alpha, void* workspace, size_t ws_bytes, void* stream) {
  if (!p || !f || !wpts || !o || !alpha || !workspace) return fail(ANR_E_ARG, "pdf alpha: NULL argument");
  if (!alpha_opts_ok(n_pts, o)) return fail(ANR_E_ARG, "pdf alpha: n_pts must be in [1, 2^24] and chunk_pts a positive multiple of 64");
  if (o->novel_pose) return fail(ANR_E_ARG, "pdf alpha: cfg.test_novel_pose is not supported");
  if (!precision_ok(o->precision))
    return fail(ANR_E_ARG, "pdf alpha: precision must be ANR_FP32, ANR_BF16X3 or ANR_BF16X6");
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i)
    if (!p->t[i] && i != PDF_RESD_LAT) return fail(ANR_E_ARG, "pdf alpha: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->poses)
    return fail(ANR_E_ARG, "pdf alpha: NULL frame tensor");
  if (!n_verts_ok(f->n_verts)) return fail(ANR_E_ARG, "pdf alpha: n_verts must be in [1, 6912]");
  if (f->n_views) return fail(ANR_E_ARG, "pdf alpha: the visibility filter is a renderer option (n_views must be 0)");
  if (ws_bytes < anr_pdf_alpha_workspace_bytes(n_pts, o)) return fail(ANR_E_WORKSPACE, "pdf alpha: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(alpha, 0, (size_t)n_pts * 4, s) != hipSuccess) return fail(ANR_E_HIP, "pdf alpha: memset");
  const int G = alpha_groups(n_pts, o);
  const PLayout L = playout(G, G, true);
  anr_pdf_render_out out{};
  out.raw = (float*)((char*)workspace + L.total);
  for (long c0 = 0; c0 < n_pts; c0 += o->chunk_pts) {  // one Network.get_alpha call per chunk (batchify :14-23)
    const int m = (int)std::min<long>(o->chunk_pts, n_pts - c0);
    const int g = (m + 63) / 64;
    ANR_TRY(pdf_core(p, f, nullptr, nullptr, nullptr, nullptr, g, g, o->precision, nullptr, &out, true, L, workspace, s,
                     wpts + 3 * c0, m, alpha + c0));
  }
  return ANR_OK;
}

}  // extern "C"
