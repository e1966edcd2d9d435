// anr_lbw_capi.hip — C-ABI of the aligned_aninerf_lbw render path (include/aninerf.h, "aligned_aninerf_lbw variant").
//
// Sequence per render call (aligned_aninerf_lbw_network.py:90-147 under tpose_renderer.py:159-186):
//   k_lbw_wnorm / k_lbw_fold / k_sdf_tbtab (per-call weight and bounds preparation)
//   -> k_sdf_front over pvertices (KNN records, keep mask, per-chunk argmin) -> ordered compaction -> one host
//      read of n'
//   -> per batch of <= P kept samples: k_lbw_gather, the blend-weight MLP (bw_latent folded into layers 0 / 5),
//      k_lbw_warp (pbw, LBS to the big pose), [full call: k_sdf_front in free-sample mode over tvertices,
//      k_lbw_tbw_in, the blend-weight MLP again with bw_latent[0], k_lbw_tbw], the density net (weight-normed
//      softplus layers, no stored factors: nothing differentiates here), the colour net (color_latent folded into
//      lin3), k_lbw_raw
//   -> [full call: the alpha_ind row stage] -> compositing (k_composite).
// ANR_BF16X3 / ANR_BF16X6: each network is one fused launch per batch (anr_lbw_b16.hip / anr_lbw_x6.hip, programs
// V = 20, 21, 22 (+ 10) of anr_mlp_body.h; the blend-weight program applies the softmax itself). ANR_FP32: 9 + 9 + 5
// layer GEMMs, anr_gemm.hip's exact fp32 MFMA kernels or anr_lgemm.hip's, driven through anr_gemm_seq.h as the
// sdf_pdf render drives them. The front-end + compaction stage, the free-point search, the image packing and the
// fused density / colour pair are the KNN family's shared host code (anr_knn_host.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_gemm_seq.h"
#include "anr_kernels.h"
#include "anr_knn_host.h"
#include "anr_lbw.h"
#include "anr_sdf.h"
#include "anr_train.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr long LBW_BATCH = 1L << 18;          // kept samples per batch
constexpr size_t LBW_LIMG_BYTES = 16u << 20;  // k_lgemm weight images (25 GEMMs, <= 448 KiB each)

struct LLayout {
  KnnFrontLayout F;
  size_t chunk_max, wimg, fold, limg;
  size_t bimg, dimg, cimg;  // the fused programs' images: bf16x3 (k_pack_seq) or bf16x6 (k_pack_seq_x6)
  size_t sigma, flags, block_sum2, out_row, pbw_rows, tbw_rows;  // full call only
  size_t ptp, Gx, ibw, Ybw, Ha, Hb, tp3, Xs0, X4, C0, Y8, Yc;
  KnnFreeLayout S;                                               // second search (full call only)
  long P;
  size_t total;
};

LLayout llayout(int n_rays, int chunk, bool image) {
  LLayout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  Carve c;
  L.F.carve(c, R, chunk);
  L.chunk_max = c.bytes(((R + chunk - 1) / (size_t)std::max(chunk, 1)) * 8);
  L.wimg = c.bytes(LBW_WN_FLOATS * 4);
  L.fold = c.bytes(LBW_FOLD_FLOATS * 4);
  L.limg = c.bytes(LBW_LIMG_BYTES);
  L.bimg = carve_seq_image(c, ANR_L_LBW0, ANR_LBW_LAYERS);
  L.dimg = carve_seq_image(c, ANR_L_SDF0, ANR_SDF_LAYERS);
  L.cimg = carve_seq_image(c, ANR_L_LCOL0, ANR_LCOL_LAYERS);
  if (!image) {
    L.sigma = c.bytes(N * 4);
    L.flags = c.bytes(N);
    L.block_sum2 = c.bytes(((N + 1023) / 1024) * 4);
    L.out_row = c.bytes(N * 4);
    L.pbw_rows = c.bytes(N * 24 * 4);
    L.tbw_rows = c.bytes(N * 24 * 4);
  }
  // the batch size: LBW_BATCH, or the test override ANR_LBW_BATCH
  const long P = (long)std::min<size_t>(N, (size_t)batch_rows("ANR_LBW_BATCH", LBW_BATCH));
  L.P = P;
  auto f = [&](long w) { return c.floats((size_t)P * w); };
  L.ptp = f(8); L.Gx = f(64); L.ibw = f(24); L.Ybw = f(24); L.Ha = f(256); L.Hb = f(256); L.tp3 = f(3);
  L.Xs0 = f(40); L.X4 = f(256); L.C0 = f(40); L.Y8 = f(264); L.Yc = f(4);
  if (!image) L.S.carve(c, ((size_t)P + 63) / 64);
  L.total = c.o;
  return L;
}

int check(const anr_lbw_params* p, const anr_lbw_frame* f, const float* ray_o, const float* ray_d, const float* near_,
          const float* far_, int R, const anr_render_opts* o, const anr_lbw_render_out* out, int image, void* ws) {
  ANR_TRY(check_knn_common("lbw render", p && f && out, ray_o, ray_d, near_, far_, R, o, ws, 0x7fffffffL / 24,
                           "cfg.test_novel_pose (novel_pose_bw) is not supported", true));
  for (int i = 0; i < ANR_LBW_NUM_TENSORS; ++i)
    if (!p->t[i]) return fail(ANR_E_ARG, "lbw render: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->tbounds || !f->latent_index ||
      (!image && !f->tvertices))
    return fail(ANR_E_ARG, "lbw render: NULL frame tensor");
  return check_knn_frame("lbw render", f->n_verts, out->rgb_map && out->acc_map && out->depth_map && out->raw, 0,
                         nullptr, nullptr, nullptr, 0, 0);
}

}  // namespace

extern "C" {

size_t anr_lbw_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only) {
  if (!opts_ok(n_rays, o)) return 0;
  return llayout(n_rays, o->chunk, image_only != 0).total;
}

const int32_t* anr_lbw_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).F.counts);
}

const uint32_t* anr_lbw_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const uint32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).F.knn);
}

const int32_t* anr_lbw_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).F.list);
}

const float* anr_lbw_render_points(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const float*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).C0);
}

int anr_lbw_render_rows(const void* workspace, int n_rays, const anr_render_opts* o, float* pbw, float* tbw, int32_t* ids,
                        void* stream) {
  if (!workspace || !opts_ok(n_rays, o) || ((pbw == nullptr) != (tbw == nullptr)))
    return fail(ANR_E_ARG, "anr_lbw_render_rows: bad arguments");
  const LLayout L = llayout(n_rays, o->chunk, false);
  const char* ws = (const char*)workspace;
  const long N = (long)n_rays * 64;
  hipStream_t s = (hipStream_t)stream;
  if (pbw) {
    hipLaunchKernelGGL(k_gather_rows, dim3((int)((N * 6 + 255) / 256)), dim3(256), 0, s, (const int*)(ws + L.out_row),
                       (const int*)(ws + L.F.counts), (const float4*)(ws + L.pbw_rows), (const float4*)(ws + L.tbw_rows),
                       (float4*)pbw, (float4*)tbw);
    ANR_TRY(check_launch("k_gather_rows (lbw)"));
  }
  if (ids) {
    hipLaunchKernelGGL(k_row_ids, dim3((int)((N + 255) / 256)), dim3(256), 0, s, (const int*)(ws + L.out_row),
                       (const int*)(ws + L.F.counts), (const int*)(ws + L.F.list), (int*)ids);
    ANR_TRY(check_launch("k_row_ids (lbw)"));
  }
  return ANR_OK;
}

int anr_lbw_render_fwd(const anr_lbw_params* p, const anr_lbw_frame* f, const float* ray_o, const float* ray_d,
                       const float* near_, const float* far_, int R, const anr_render_opts* o,
                       const anr_lbw_render_out* out, int image_only, void* workspace, size_t ws_bytes, void* stream) {
  const bool image = image_only != 0;
  ANR_TRY(check(p, f, ray_o, ray_d, near_, far_, R, o, out, image, workspace));
  const int chunk = o->chunk;
  const LLayout L = llayout(R, chunk, image);
  if (ws_bytes < L.total) return fail(ANR_E_WORKSPACE, "lbw render: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int nch = (R + chunk - 1) / chunk;
  float4* raw = (float4*)out->raw;

  if (hipMemsetAsync(ws + L.chunk_max, 0, (size_t)nch * 8, s) != hipSuccess)
    return fail(ANR_E_HIP, "lbw render: memset");

  // per-call weight preparation (weight norm, latent folds; the per-chunk tbounds: knn_front_compact)
  const float* const* tp = p->t;
  float* wimg = (float*)(ws + L.wimg);
  float* fold = (float*)(ws + L.fold);
  float* tbtab = (float*)(ws + L.F.tbtab);
  LbwTensors T{};
  for (int i = 0; i < ANR_LBW_NUM_TENSORS; ++i) T.t[i] = tp[i];
  hipLaunchKernelGGL(k_lbw_wnorm, dim3(lbw_wn_rows()), dim3(256), 0, s, T, wimg);
  ANR_TRY(check_launch("k_lbw_wnorm"));
  hipLaunchKernelGGL(k_lbw_fold, dim3(5), dim3(256), 0, s, T, (const float*)wimg, f->latent_index, fold);
  ANR_TRY(check_launch("k_lbw_fold"));

  // front-end over pvertices + ordered compaction. Every sample's raw is written here (zero where dropped)
  // or by k_lbw_raw; the front-end's sdf output has no meaning for this network and goes to scratch.
  const int cus = num_cus();
  auto F = [&](size_t off) { return (float*)(ws + off); };
  SdfFrontArgs fa{};
  fa.ray_o = ray_o; fa.ray_d = ray_d; fa.near_ = near_; fa.far_ = far_; fa.t_rand = o->t_rand;
  fa.n_rays = R; fa.chunk = chunk; fa.R = f->R; fa.Th = f->Th; fa.verts = f->pvertices; fa.nv = f->n_verts;
  fa.norm_th = o->norm_th; fa.raw = raw;
  // the dropped samples' "sdf = 10" stores need (R*64) floats: the list region is free until k_compact
  fa.sdf = (float*)(ws + L.F.list);
  int n = 0;
  ANR_TRY(knn_front_compact(fa, ws, L.F, f->tbounds, out->tbounds_out, false, "lbw render", s, &n));
  const int* list = (const int*)(ws + L.F.list);

  if (!image) ANR_TRY(knn_free_setup(ws, L.S, "lbw render", s));

  float *Ha = F(L.Ha), *Hb = F(L.Hb);
  const long P = L.P;
  const float* WN[LBW_NUM_WN];
  for (int l = 0; l < LBW_NUM_WN; ++l) WN[l] = wimg + lbw_wn_layer(l).off;
  LImgCache limg;
  limg.base = ws + L.limg;
  limg.cap = LBW_LIMG_BYTES;
  const float *Wb[8], *Bb[8];
  for (int l = 0; l < 8; ++l) {
    Wb[l] = tp[LBW_BWLIN0 + 2 * l];
    Bb[l] = tp[LBW_BWLIN0 + 2 * l + 1];
  }

  // split-bf16 precisions: the blend-weight MLP, the density net and the colour net as one fused launch per
  // batch each (anr_lbw_b16.hip; ANR_BF16X6: the fp32-level programs of anr_lbw_x6.hip), images packed once per call
  const bool x6 = o->precision == ANR_BF16X6;
  const bool fused = x6 || o->precision == ANR_BF16X3;
  const SeqImages im{s, x6, "lbw"};
  unsigned char* bimg = (unsigned char*)(ws + L.bimg);
  unsigned char* dimg = (unsigned char*)(ws + L.dimg);
  unsigned char* cimg = (unsigned char*)(ws + L.cimg);
  if (fused) {  // the blend-weight MLP's layer 0 / 5 biases: folded with the latent
    ANR_TRY(im.pack_skip8(tp, LBW_BWLIN0, LBW_BWFC_W, LBW_BWFC_B, ANR_L_LBW0, ANR_LBW_LAYERS, bimg));
    ANR_TRY(im.pack_density(WN, tp, dimg));
    ANR_TRY(im.pack_colour(WN, tp, LBW_CLIN0, ANR_L_LCOL0, ANR_LCOL_LAYERS, cimg));
  }

  for (long b0 = 0; b0 < n; b0 += P) {
    const int cnt = (int)std::min<long>(P, n - b0);
    LbwPointArgs a{};
    a.list = list; a.b0 = (int)b0; a.cnt = cnt;
    a.ray_o = ray_o; a.ray_d = ray_d; a.near_ = near_; a.far_ = far_; a.t_rand = o->t_rand; a.chunk = chunk;
    a.R = f->R; a.Th = f->Th; a.A = f->A; a.bigA = f->big_A; a.weights = f->weights; a.knn = fa.knn;
    a.knn2 = image ? nullptr : (const uint32_t*)(ws + L.S.knn);
    a.tbtab = tbtab;
    a.ptp = F(L.ptp); a.Gx = F(L.Gx); a.ibw = F(L.ibw); a.Ybw = F(L.Ybw); a.tp3 = F(L.tp3);
    a.Xs0 = F(L.Xs0); a.X4 = F(L.X4); a.C0 = F(L.C0); a.Y8 = F(L.Y8); a.Yc = F(L.Yc);
    a.full = image ? 0 : 1;
    a.fused = fused ? 1 : 0;
    a.pbw_rows = image ? nullptr : F(L.pbw_rows);
    a.tbw_rows = image ? nullptr : F(L.tbw_rows);
    a.sigma = image ? nullptr : F(L.sigma);
    a.raw = raw;
    const dim3 pg((cnt + 255) / 256), pb(256);
    G g{s, cnt, 0, &limg, cus};  // the layer GEMMs of the exact-fp32 precision

    // the blend-weight MLP over gamma_10 in Gx -> Ybw; fold0 / fold5: layers 0 / 5 biases with the latent folded
    // (fused: one launch over the points at pts, row stride ld, with the softmax applied: Ybw = the weights)
    auto bw_mlp = [&](const float* fold0, const float* fold5, const float* pts, int ld) -> int {
      if (fused) {
        MlpArgs ba{};
        im.bind(ba, bimg, ANR_L_LBW0, ANR_LBW_LAYERS);
        ba.fold = fold0;  // fold5 = fold0 + 256 (k_lbw_fold)
        ba.ptb = pts;
        ba.ptb_ld = ld;
        ba.pbw32 = a.ibw;
        ba.pbw_rows = F(L.Ybw);
        ba.n_rows = cnt;
        return launch_lbw_bw(ba, cus, s, x6) != 0 ? fail(ANR_E_HIP, "k_lbw_bw launch failed") : ANR_OK;
      }
      return g.skip8(F(L.Ybw), 24, 24, Wb, Bb, tp[LBW_BWFC_W], tp[LBW_BWFC_B], fold0, fold5, a.Gx, 63, 191, 447, Ha, Hb,
                     false);
    };

    // pose space: init_pbw, pbw, LBS to the big pose
    hipLaunchKernelGGL(k_lbw_gather, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_gather"));
    ANR_TRY(bw_mlp(fold, fold + 256, a.ptp, 8));
    hipLaunchKernelGGL(k_lbw_warp, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_warp"));

    // T-pose space: the second search over tvertices (free-sample mode, as anr_knn_blend drives it), tbw
    if (!image) {
      // threshold +inf: every record is wanted
      ANR_TRY(knn_free_points(ws, L.S, a.tp3, cnt, f->tvertices, f->n_verts, INFINITY, "lbw, tvertices", s));
      hipLaunchKernelGGL(k_lbw_tbw_in, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_lbw_tbw_in"));
      ANR_TRY(bw_mlp(fold + 768, fold + 1024, a.tp3, 3));
      hipLaunchKernelGGL(k_lbw_tbw, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_lbw_tbw"));
    }

    // the density net, then the colour net over [tpose, gamma_4(tpose_dir)] || feature (color_latent folded into
    // lin3's bias, fold + 512)
    if (fused) {
      ANR_TRY(launch_density_colour(im, dimg, cimg, fold, a.C0, F(L.Y8), F(L.Yc), cnt, cus));
    } else {
      ANR_TRY(g.density_sp(WN, tp, a.Xs0, a.X4, F(L.Y8), Ha, Hb));
      ANR_TRY(g.colour5(WN, tp, LBW_CLIN0, fold + 512, a.C0, F(L.Y8), F(L.Yc), Ha, Hb));
    }

    hipLaunchKernelGGL(k_lbw_raw, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_raw"));
  }

  VolCall v{};  // what stage_alpha_ind and stage_composite read
  v.near_ = near_; v.far_ = far_; v.R = R; v.o = *o; v.ws = ws; v.raw = raw; v.s = s;
  if (!image) {
    Layout& A = v.L;
    A.counts = L.F.counts; A.mask = L.F.mask; A.ray_off = L.F.ray_off; A.list = L.F.list; A.sigma = L.sigma;
    A.chunk_max = L.chunk_max; A.flags = L.flags; A.block_sum2 = L.block_sum2; A.out_row = L.out_row;
    ANR_TRY(stage_alpha_ind(v));
  }
  const anr_render_out ro{out->rgb_map, out->acc_map, out->depth_map, out->raw};
  return stage_composite(v, R, &ro);
}

}  // extern "C"
