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
// displacement and the density layers.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_gemm_seq.h"
#include "anr_kernels.h"
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

// the batch size: PDF_BATCH, or the test override ANR_PDF_BATCH (a multiple of 256 in [256, PDF_BATCH])
long pdf_batch() {
  const char* v = getenv("ANR_PDF_BATCH");
  if (!v || !v[0]) return PDF_BATCH;
  const long b = atol(v);
  return (b >= 256 && b <= PDF_BATCH && b % 256 == 0) ? b : PDF_BATCH;
}

struct PLayout {
  size_t counts, mask, chunk_min, ray_off, block_sum, list, knn, tbtab, wimg, fold, limg;
  size_t rimg, dimg, cimg;  // the fused programs' images: bf16x3 (k_pack_seq) or bf16x6 (k_pack_seq_x6)
  size_t resd_rows;         // full call only
  size_t ptp, Gr, Ha, Hb, Yr, Xs0, X4, C0, Y8, Yc;
  long P;
  size_t total;
};

PLayout playout(int n_rays, int chunk, bool image) {
  PLayout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  const size_t nch = (R + chunk - 1) / (size_t)std::max(chunk, 1);
  Carve c;
  L.counts = c.bytes(16);
  L.mask = c.bytes(R * 8);
  L.chunk_min = c.bytes(nch * 8);
  L.ray_off = c.bytes((R + 1) * 4);
  L.block_sum = c.bytes(((R + 255) / 256) * 4);
  L.list = c.bytes(N * 4);
  L.knn = c.bytes(N * 32);
  L.tbtab = c.bytes(nch * 6 * 4);
  L.wimg = c.bytes(LBW_WN_FLOATS * 4);
  L.fold = c.bytes(PDF_FOLD_FLOATS * 4);
  L.limg = c.bytes(PDF_LIMG_BYTES);
  auto img = [&](int L0, int nl) { return c.bytes((size_t)std::max(seq_image_bytes(L0, nl), x6seq_image_bytes(L0, nl))); };
  L.rimg = img(ANR_L_RESD0, ANR_RESD_LAYERS);
  L.dimg = img(ANR_L_SDF0, ANR_SDF_LAYERS);
  L.cimg = img(ANR_L_LCOL0, ANR_LCOL_LAYERS);
  if (!image) L.resd_rows = c.bytes(N * 3 * 4);
  const long P = (long)std::min<size_t>(N, (size_t)pdf_batch());
  L.P = P;
  auto f = [&](long w) { return c.floats((size_t)P * w); };
  L.ptp = f(8); L.Gr = f(64); L.Ha = f(256); L.Hb = f(256); L.Yr = f(4);
  L.Xs0 = f(40); L.X4 = f(256); L.C0 = f(40); L.Y8 = f(264); L.Yc = f(4);
  L.total = c.o;
  return L;
}

int pdf_cus() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
  return v;
}

bool opts_ok(int n_rays, const anr_render_opts* o) { return n_rays > 0 && o && o->chunk > 0; }
bool alpha_opts_ok(long n_pts, const anr_alpha_opts* o) {
  return n_pts > 0 && n_pts <= (1L << 24) && o && o->chunk_pts > 0 && o->chunk_pts % 64 == 0;
}
// groups of 64 points of the largest chunk of a get_alpha call
int alpha_groups(long n_pts, const anr_alpha_opts* o) { return (int)((std::min<long>(n_pts, o->chunk_pts) + 63) / 64); }

int check(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d, const float* near_,
          const float* far_, int R, const anr_render_opts* o, const anr_pdf_render_out* out, void* ws) {
  if (!p || !f || !o || !out || !ws || !ray_o || !ray_d || !near_ || !far_)
    return fail(ANR_E_ARG, "pdf render: NULL argument");
  if (o->n_samples != 64) return fail(ANR_E_ARG, "pdf render: only N_samples == 64 is supported");
  if (o->chunk <= 0 || R <= 0 || (long)R * 64 > 0x7fffffffL / 24) return fail(ANR_E_ARG, "pdf render: bad chunk / n_rays");
  if (o->novel_pose) return fail(ANR_E_ARG, "pdf render: cfg.test_novel_pose is not supported");
  if (o->precision != ANR_FP32 && o->precision != ANR_BF16X3 && o->precision != ANR_BF16X6)
    return fail(ANR_E_ARG, "pdf render: precision must be ANR_FP32, ANR_BF16X3 or ANR_BF16X6");
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i)
    if (!p->t[i] && i != PDF_RESD_LAT) return fail(ANR_E_ARG, "pdf render: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->poses || !f->tbounds || !f->latent_index)
    return fail(ANR_E_ARG, "pdf render: NULL frame tensor");
  if (f->n_verts <= 0 || f->n_verts > 6912) return fail(ANR_E_ARG, "pdf render: n_verts must be in [1, 6912]");
  if (!out->rgb_map || !out->acc_map || !out->depth_map || !out->raw) return fail(ANR_E_ARG, "pdf render: NULL output");
  if (f->n_views < 0 || (f->n_views > 0 && (!f->Ks || !f->RT || !f->msks || f->img_h <= 0 || f->img_w <= 0)))
    return fail(ANR_E_ARG, "pdf render: bad visibility-filter views");
  return ANR_OK;
}

// the render sequence over rays (wpts NULL) or over the free points of one get_alpha chunk (wpts: n_pts points in
// R = ceil(n_pts / 64) groups that form one chunk; no directions, no colour net, no box test, no compositing: the raw
// density of the kept points goes to alpha, which the caller zeroed; out->raw is scratch for the front-end)
int pdf_core(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d, const float* near_,
             const float* far_, int R, int chunk, int precision, const float* t_rand, const anr_pdf_render_out* out,
             bool image, const PLayout& L, void* workspace, hipStream_t s, const float* wpts, int n_pts, float* alpha) {
  char* ws = (char*)workspace;
  const int nch = (R + chunk - 1) / chunk;
  int* counts = (int*)(ws + L.counts);
  float4* raw = (float4*)out->raw;

  if (hipMemsetAsync(ws + L.counts, 0, 16, s) != hipSuccess ||
      hipMemsetAsync(ws + L.chunk_min, 0xff, (size_t)nch * 8, s) != hipSuccess)
    return fail(ANR_E_HIP, "pdf render: memset");

  // per-call weight preparation (weight norm, folds, per-chunk tbounds)
  const float* const* tp = p->t;
  float* wimg = (float*)(ws + L.wimg);
  float* fold = (float*)(ws + L.fold);
  float* tbtab = (float*)(ws + L.tbtab);
  LbwTensors T{};
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i) T.t[i] = tp[i];
  hipLaunchKernelGGL(k_lbw_wnorm, dim3(lbw_wn_rows()), dim3(256), 0, s, T, wimg);
  ANR_TRY(check_launch("k_lbw_wnorm (pdf)"));
  hipLaunchKernelGGL(k_pdf_fold, dim3(wpts ? 2 : 3), dim3(256), 0, s, T, (const float*)wimg, f->poses, f->latent_index, fold);
  ANR_TRY(check_launch("k_pdf_fold"));
  const bool filt = !wpts && f->n_views > 0;  // visibility filter: widening depends on the front-end
  if (!filt && !wpts) {
    hipLaunchKernelGGL(k_sdf_tbtab, dim3(1), dim3(64), 0, s, f->tbounds, nch, tbtab, out->tbounds_out, nullptr);
    ANR_TRY(check_launch("k_sdf_tbtab (pdf)"));
  }

  // front-end over pvertices + ordered compaction. Every sample's raw is written here (zero where dropped) or by
  // k_lbw_raw; the front-end's sdf output has no meaning for this network and goes to the list region, which is
  // free until k_compact.
  const int cus = pdf_cus();
  auto F = [&](size_t off) { return (float*)(ws + off); };
  SdfFrontArgs fa{};
  fa.ray_o = ray_o; fa.ray_d = ray_d; fa.near_ = near_; fa.far_ = far_; fa.t_rand = t_rand;
  fa.wpts = wpts; fa.n_pts = n_pts;
  fa.n_rays = R; fa.chunk = chunk; fa.R = f->R; fa.Th = f->Th; fa.verts = f->pvertices; fa.nv = f->n_verts;
  fa.norm_th = PDF_NORM_TH; fa.mask = (uint64_t*)(ws + L.mask); fa.chunk_min = (uint64_t*)(ws + L.chunk_min);
  fa.knn = (uint32_t*)(ws + L.knn); fa.raw = raw;
  fa.sdf = (float*)(ws + L.list);
  if (filt) {
    fa.n_views = f->n_views; fa.Ks = f->Ks; fa.RT = f->RT; fa.msks = f->msks; fa.img_h = f->img_h; fa.img_w = f->img_w;
  }
  hipLaunchKernelGGL(k_sdf_front, dim3(std::min(cus, (R + 15) / 16)), dim3(1024), 0, s, fa);
  ANR_TRY(check_launch("k_sdf_front (pdf)"));
  if (filt) {
    hipLaunchKernelGGL(k_sdf_tbtab, dim3(1), dim3(64), 0, s, f->tbounds, nch, tbtab, out->tbounds_out,
                       (const uint64_t*)fa.chunk_min);
    ANR_TRY(check_launch("k_sdf_tbtab (pdf, visible chunks)"));
  }
  CompactArgs ca{};
  ca.n_rays = R; ca.chunk = chunk; ca.mask = fa.mask; ca.chunk_min = fa.chunk_min;
  ca.ray_off = (int*)(ws + L.ray_off); ca.block_sum = (int*)(ws + L.block_sum); ca.list = (int*)(ws + L.list);
  const int nb = (R + 255) / 256;
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(256), 0, s, ca);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, ca.block_sum, nb, counts);
  hipLaunchKernelGGL(k_compact, dim3((R + 3) / 4), dim3(256), 0, s, ca);
  ANR_TRY(check_launch("k_compact (pdf)"));
  int n = 0;
  if (hipMemcpyAsync(&n, counts, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(ANR_E_HIP, "pdf render: kept-count readback");

  float *Ha = F(L.Ha), *Hb = F(L.Hb);
  const long P = L.P;
  auto WN = [&](int l) { return (const float*)wimg + lbw_wn_layer(l).off; };
  const float sqrt2 = 1.41421356237309515f;
  LImgCache limg;
  limg.base = ws + L.limg;
  limg.cap = PDF_LIMG_BYTES;
  const float* Wr[8];
  for (int l = 0; l < 8; ++l) Wr[l] = tp[PDF_RLIN0 + 2 * l];
  auto Br = [&](int l) { return tp[PDF_RLIN0 + 2 * l + 1]; };

  // split-bf16 precisions: the three networks as one fused launch per batch each, images packed once per call
  const bool x6 = precision == ANR_BF16X6;
  const bool fused = x6 || precision == ANR_BF16X3;
  auto wbytes = [&](int L0, int nl) { return x6 ? x6seq_wbytes(L0, nl) : seq_wbytes(L0, nl); };
  unsigned char* rimg = (unsigned char*)(ws + L.rimg);
  unsigned char* dimg = (unsigned char*)(ws + L.dimg);
  unsigned char* cimg = (unsigned char*)(ws + L.cimg);
  if (fused) {
    auto pack = [&](const PackArgs& pa, int L0, int nl, int sl, float sc) {
      const int nt = x6 ? seq_x6_pack_threads(L0, nl) : seq_pack_threads(L0, nl);
      if (x6) hipLaunchKernelGGL(k_pack_seq_x6, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, sl, sc);
      else hipLaunchKernelGGL(k_pack_seq, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, sl, sc);
      return check_launch(x6 ? "k_pack_seq_x6 (pdf)" : "k_pack_seq (pdf)");
    };
    PackArgs pr{};
    for (int l = 0; l < 8; ++l) {
      pr.t[l] = Wr[l];
      pr.t[9 + l] = l == 0 || l == 5 ? nullptr : Br(l);  // folded with the poses
    }
    pr.t[8] = tp[PDF_RFC_W];
    pr.t[17] = tp[PDF_RFC_B];
    pr.out = rimg;
    ANR_TRY(pack(pr, ANR_L_RESD0, ANR_RESD_LAYERS, -1, 1.0f));
    PackArgs pd{};
    for (int l = 0; l < 9; ++l) {
      pd.t[l] = WN(l);
      pd.t[9 + l] = tp[3 * l];
    }
    pd.out = dimg;
    ANR_TRY(pack(pd, ANR_L_SDF0, ANR_SDF_LAYERS, 4, 1.0f / sqrt2));
    if (!wpts) {
    PackArgs pc{};
    for (int l = 0; l < 5; ++l) {
      pc.t[l] = WN(9 + l);
      pc.t[9 + l] = l == 3 ? nullptr : tp[PDF_CLIN0 + 3 * l];  // lin3's bias: the latent fold
    }
    pc.out = cimg;
    ANR_TRY(pack(pc, ANR_L_LCOL0, ANR_LCOL_LAYERS, -1, 1.0f));
    }
  }

  for (long b0 = 0; b0 < n; b0 += P) {
    const int cnt = (int)std::min<long>(P, n - b0);
    PdfPointArgs a{};
    a.list = ca.list; a.b0 = (int)b0; a.cnt = cnt;
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
      ra.wimg = rimg;
      ra.bias = (const float*)(rimg + wbytes(ANR_L_RESD0, ANR_RESD_LAYERS));
      ra.fold = fold;
      ra.ptb = a.ptp;
      ra.ptb_ld = 8;
      ra.yr = image ? nullptr : F(L.resd_rows) + (size_t)b0 * 3;
      ra.gb = a.C0;
      ra.n_rows = cnt;
      if (launch_pdf_resd(ra, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_pdf_resd launch failed");
      MlpArgs da{};
      da.wimg = dimg;
      da.bias = (const float*)(dimg + wbytes(ANR_L_SDF0, ANR_SDF_LAYERS));
      da.ptb = a.C0;
      da.ptb_ld = 40;
      da.y8 = F(L.Y8);
      da.n_rows = cnt;
      if (launch_lbw_density(da, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_lbw_density launch failed (pdf)");
      if (!wpts) {
      MlpArgs ca2{};
      ca2.wimg = cimg;
      ca2.bias = (const float*)(cimg + wbytes(ANR_L_LCOL0, ANR_LCOL_LAYERS));
      ca2.fold = fold;
      ca2.ptb = a.C0;
      ca2.ptb_ld = 40;
      ca2.y8 = F(L.Y8);
      ca2.yr = F(L.Yc);
      ca2.n_rows = cnt;
      if (launch_lbw_color(ca2, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_lbw_color launch failed (pdf)");
      }
    } else {
      // displacement MLP over gamma_10 in Gr -> Yr (poses folded into the biases of layers 0 / 5)
      ANR_TRY(g.fwd(Ha, 256, 256, Wr[0], 135, fold, a.Gr, 64, 63, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wr[1], 256, Br(1), Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(Ha, 256, 256, Wr[2], 256, Br(2), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wr[3], 256, Br(3), Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(Ha, 256, 256, Wr[4], 256, Br(4), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wr[5], 391, fold + 256, a.Gr, 64, 63, 0, true, nullptr, 0.f, false, Ha, 256, 256, 135));
      ANR_TRY(g.fwd(Ha, 256, 256, Wr[6], 256, Br(6), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wr[7], 256, Br(7), Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(F(L.Yr), 4, 3, tp[PDF_RFC_W], 256, tp[PDF_RFC_B], Hb, 256, 256, 0, false));
      hipLaunchKernelGGL(k_pdf_mid, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_pdf_mid"));

      // density net: softplus outputs only (the dummy factor pointer selects the softplus epilogue of lin3)
      const float* hin = nullptr;
      auto sp_fwd = [&](int l, int K, float* outp) -> int {
        const int r = g.fwd_sp(outp, WN(l), K, tp[3 * l], l == 0 ? a.Xs0 : hin, l == 0 ? 40 : 256, nullptr);
        hin = outp;
        return r;
      };
      ANR_TRY(sp_fwd(0, 39, Ha));
      ANR_TRY(sp_fwd(1, 256, Hb));
      ANR_TRY(sp_fwd(2, 256, Ha));
      ANR_TRY(g.fwd(a.X4, 256, 217, WN(3), 256, tp[9], hin, 256, 256, 0, false, Hb, sqrt2, true));
      hin = a.X4;
      ANR_TRY(sp_fwd(4, 256, Ha));
      ANR_TRY(sp_fwd(5, 256, Hb));
      ANR_TRY(sp_fwd(6, 256, Ha));
      ANR_TRY(sp_fwd(7, 256, Hb));
      ANR_TRY(g.fwd(F(L.Y8), 264, 257, WN(8), 256, tp[24], hin, 256, 256, 0, false));

      // colour net: [tpose, gamma_4(tpose_dir)] (30) || feature (256); color_latent folded into lin3's bias
      if (!wpts) {
      const int cb = PDF_CLIN0;
      ANR_TRY(g.fwd(Ha, 256, 256, WN(9), 286, tp[cb], a.C0, 40, 30, 0, true, nullptr, 0.f, false, F(L.Y8) + 1, 264, 256, 30));
      ANR_TRY(g.fwd(Hb, 256, 256, WN(10), 256, tp[cb + 3], Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(Ha, 256, 256, WN(11), 256, tp[cb + 6], Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, WN(12), 384, fold + 512, Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(F(L.Yc), 4, 3, WN(13), 256, tp[cb + 12], Hb, 256, 256, 0, false));
      }
    }

    if (wpts) {  // get_alpha: the raw density, scattered to the chunk's rows
      hipLaunchKernelGGL(k_pdf_alpha_out, pg, pb, 0, s, (const int*)ca.list, (int)b0, cnt, (const float*)F(L.Y8), alpha);
      ANR_TRY(check_launch("k_pdf_alpha_out"));
      continue;
    }
    // raw2alpha with the real dists, sigmoid rgb, the per-chunk tbounds mask on tpose, scatter: k_lbw_raw as it is
    LbwPointArgs ra{};
    ra.list = ca.list; ra.b0 = (int)b0; ra.cnt = cnt; ra.chunk = chunk; ra.tbtab = tbtab;
    ra.ptp = a.ptp; ra.C0 = a.C0; ra.Y8 = F(L.Y8); ra.Yc = F(L.Yc); ra.raw = raw; ra.sigma = nullptr;
    hipLaunchKernelGGL(k_lbw_raw, pg, pb, 0, s, ra);
    ANR_TRY(check_launch("k_lbw_raw (pdf)"));
  }

  if (wpts) return ANR_OK;
  anr_render_opts co{};  // stage_composite reads the sample count and the draws
  co.n_samples = 64; co.chunk = chunk; co.t_rand = t_rand; co.precision = precision;
  const anr_render_out ro{out->rgb_map, out->acc_map, out->depth_map, out->raw};
  return stage_composite(near_, far_, R, &co, raw, &ro, nullptr, s);
}

}  // namespace

extern "C" {

size_t anr_pdf_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only) {
  if (!opts_ok(n_rays, o) || (long)n_rays * 64 > 0x7fffffffL / 24) return 0;
  return playout(n_rays, o->chunk, image_only != 0).total;
}

const int32_t* anr_pdf_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).counts);
}

const uint32_t* anr_pdf_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const uint32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).knn);
}

const int32_t* anr_pdf_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + playout(n_rays, o->chunk, image_only != 0).list);
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
  if (hipMemcpyAsync(&n, ws + L.counts, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_pdf_render_rows: count readback");
  if (n < 0 || (long)n > (long)n_rays * 64) return fail(ANR_E_ARG, "anr_pdf_render_rows: not the workspace of a render call");
  if (n == 0) return ANR_OK;
  if (resd && hipMemcpyAsync(resd, ws + L.resd_rows, (size_t)n * 12, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_pdf_render_rows: copy");
  if (ids && hipMemcpyAsync(ids, ws + L.list, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
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
  if (o->precision != ANR_FP32 && o->precision != ANR_BF16X3 && o->precision != ANR_BF16X6)
    return fail(ANR_E_ARG, "pdf alpha: precision must be ANR_FP32, ANR_BF16X3 or ANR_BF16X6");
  for (int i = 0; i < ANR_PDF_NUM_TENSORS; ++i)
    if (!p->t[i] && i != PDF_RESD_LAT) return fail(ANR_E_ARG, "pdf alpha: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->poses)
    return fail(ANR_E_ARG, "pdf alpha: NULL frame tensor");
  if (f->n_verts <= 0 || f->n_verts > 6912) return fail(ANR_E_ARG, "pdf alpha: n_verts must be in [1, 6912]");
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
