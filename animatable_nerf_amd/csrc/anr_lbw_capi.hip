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
// sdf_pdf render drives them.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_gemm_seq.h"
#include "anr_kernels.h"
#include "anr_lbw.h"
#include "anr_sdf.h"
#include "anr_train.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr long LBW_BATCH = 1L << 18;          // kept samples per batch
constexpr size_t LBW_LIMG_BYTES = 16u << 20;  // k_lgemm weight images (25 GEMMs, <= 448 KiB each)

// the batch size: LBW_BATCH, or the test override ANR_LBW_BATCH (a multiple of 256 in [256, LBW_BATCH])
long lbw_batch() {
  const char* v = getenv("ANR_LBW_BATCH");
  if (!v || !v[0]) return LBW_BATCH;
  const long b = atol(v);
  return (b >= 256 && b <= LBW_BATCH && b % 256 == 0) ? b : LBW_BATCH;
}

struct LLayout {
  size_t counts, mask, chunk_min, chunk_max, ray_off, block_sum, list, knn, tbtab, wimg, fold, limg;
  size_t bimg, dimg, cimg;  // the fused programs' images: bf16x3 (k_pack_seq) or bf16x6 (k_pack_seq_x6)
  size_t sigma, flags, block_sum2, out_row, pbw_rows, tbw_rows;  // full call only
  size_t ptp, Gx, ibw, Ybw, Ha, Hb, tp3, Xs0, X4, C0, Y8, Yc;
  size_t ident, mask2, cmin2, knn2, raw2, sdf2;                  // second search (full call only)
  long P;
  size_t total;
};

LLayout llayout(int n_rays, int chunk, bool image) {
  LLayout L{};
  const size_t R = (size_t)n_rays, N = R * 64;
  const size_t nch = (R + chunk - 1) / (size_t)std::max(chunk, 1);
  Carve c;
  L.counts = c.bytes(16);
  L.mask = c.bytes(R * 8);
  L.chunk_min = c.bytes(nch * 8);
  L.chunk_max = c.bytes(nch * 8);
  L.ray_off = c.bytes((R + 1) * 4);
  L.block_sum = c.bytes(((R + 255) / 256) * 4);
  L.list = c.bytes(N * 4);
  L.knn = c.bytes(N * 32);
  L.tbtab = c.bytes(nch * 6 * 4);
  L.wimg = c.bytes(LBW_WN_FLOATS * 4);
  L.fold = c.bytes(LBW_FOLD_FLOATS * 4);
  L.limg = c.bytes(LBW_LIMG_BYTES);
  auto img = [&](int L0, int nl) { return c.bytes((size_t)std::max(seq_image_bytes(L0, nl), x6seq_image_bytes(L0, nl))); };
  L.bimg = img(ANR_L_LBW0, ANR_LBW_LAYERS);
  L.dimg = img(ANR_L_SDF0, ANR_SDF_LAYERS);
  L.cimg = img(ANR_L_LCOL0, ANR_LCOL_LAYERS);
  if (!image) {
    L.sigma = c.bytes(N * 4);
    L.flags = c.bytes(N);
    L.block_sum2 = c.bytes(((N + 1023) / 1024) * 4);
    L.out_row = c.bytes(N * 4);
    L.pbw_rows = c.bytes(N * 24 * 4);
    L.tbw_rows = c.bytes(N * 24 * 4);
  }
  const long P = (long)std::min<size_t>(N, (size_t)lbw_batch());
  L.P = P;
  auto f = [&](long w) { return c.floats((size_t)P * w); };
  L.ptp = f(8); L.Gx = f(64); L.ibw = f(24); L.Ybw = f(24); L.Ha = f(256); L.Hb = f(256); L.tp3 = f(3);
  L.Xs0 = f(40); L.X4 = f(256); L.C0 = f(40); L.Y8 = f(264); L.Yc = f(4);
  if (!image) {
    const size_t G = ((size_t)P + 63) / 64;
    L.ident = c.bytes(64);
    L.mask2 = c.bytes(G * 8);
    L.cmin2 = c.bytes(8);
    L.knn2 = c.bytes(G * 64 * 32);
    L.raw2 = c.bytes(G * 64 * 16);
    L.sdf2 = c.bytes(G * 64 * 4);
  }
  L.total = c.o;
  return L;
}

int lbw_cus() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
  return v;
}

bool opts_ok(int n_rays, const anr_render_opts* o) { return n_rays > 0 && o && o->chunk > 0; }

int check(const anr_lbw_params* p, const anr_lbw_frame* f, const float* ray_o, const float* ray_d, const float* near_,
          const float* far_, int R, const anr_render_opts* o, const anr_lbw_render_out* out, int image, void* ws) {
  if (!p || !f || !o || !out || !ws || !ray_o || !ray_d || !near_ || !far_)
    return fail(ANR_E_ARG, "lbw render: NULL argument");
  if (o->n_samples != 64) return fail(ANR_E_ARG, "lbw render: only N_samples == 64 is supported");
  if (o->chunk <= 0 || R <= 0 || (long)R * 64 > 0x7fffffffL / 24) return fail(ANR_E_ARG, "lbw render: bad chunk / n_rays");
  if (o->novel_pose) return fail(ANR_E_ARG, "lbw render: cfg.test_novel_pose (novel_pose_bw) is not supported");
  if (o->precision != ANR_FP32 && o->precision != ANR_BF16X3 && o->precision != ANR_BF16X6)
    return fail(ANR_E_ARG, "lbw render: precision must be ANR_FP32, ANR_BF16X3 or ANR_BF16X6");
  for (int i = 0; i < ANR_LBW_NUM_TENSORS; ++i)
    if (!p->t[i]) return fail(ANR_E_ARG, "lbw render: NULL parameter tensor");
  if (!f->A || !f->big_A || !f->R || !f->Th || !f->pvertices || !f->weights || !f->tbounds || !f->latent_index ||
      (!image && !f->tvertices))
    return fail(ANR_E_ARG, "lbw render: NULL frame tensor");
  if (f->n_verts <= 0 || f->n_verts > 6912) return fail(ANR_E_ARG, "lbw render: n_verts must be in [1, 6912]");
  if (!out->rgb_map || !out->acc_map || !out->depth_map || !out->raw) return fail(ANR_E_ARG, "lbw render: NULL output");
  return ANR_OK;
}

}  // namespace

extern "C" {

size_t anr_lbw_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only) {
  if (!opts_ok(n_rays, o)) return 0;
  return llayout(n_rays, o->chunk, image_only != 0).total;
}

const int32_t* anr_lbw_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).counts);
}

const uint32_t* anr_lbw_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const uint32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).knn);
}

const int32_t* anr_lbw_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only) {
  if (!workspace || !opts_ok(n_rays, o)) return nullptr;
  return (const int32_t*)((const char*)workspace + llayout(n_rays, o->chunk, image_only != 0).list);
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
                       (const int*)(ws + L.counts), (const float4*)(ws + L.pbw_rows), (const float4*)(ws + L.tbw_rows),
                       (float4*)pbw, (float4*)tbw);
    ANR_TRY(check_launch("k_gather_rows (lbw)"));
  }
  if (ids) {
    hipLaunchKernelGGL(k_row_ids, dim3((int)((N + 255) / 256)), dim3(256), 0, s, (const int*)(ws + L.out_row),
                       (const int*)(ws + L.counts), (const int*)(ws + L.list), (int*)ids);
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
  int* counts = (int*)(ws + L.counts);
  float4* raw = (float4*)out->raw;

  if (hipMemsetAsync(ws + L.counts, 0, 16, s) != hipSuccess ||
      hipMemsetAsync(ws + L.chunk_min, 0xff, (size_t)nch * 8, s) != hipSuccess ||
      hipMemsetAsync(ws + L.chunk_max, 0, (size_t)nch * 8, s) != hipSuccess)
    return fail(ANR_E_HIP, "lbw render: memset");

  // per-call weight preparation (weight norm, latent folds, per-chunk tbounds)
  const float* const* tp = p->t;
  float* wimg = (float*)(ws + L.wimg);
  float* fold = (float*)(ws + L.fold);
  float* tbtab = (float*)(ws + L.tbtab);
  LbwTensors T{};
  for (int i = 0; i < ANR_LBW_NUM_TENSORS; ++i) T.t[i] = tp[i];
  hipLaunchKernelGGL(k_lbw_wnorm, dim3(lbw_wn_rows()), dim3(256), 0, s, T, wimg);
  ANR_TRY(check_launch("k_lbw_wnorm"));
  hipLaunchKernelGGL(k_lbw_fold, dim3(5), dim3(256), 0, s, T, (const float*)wimg, f->latent_index, fold);
  ANR_TRY(check_launch("k_lbw_fold"));
  hipLaunchKernelGGL(k_sdf_tbtab, dim3(1), dim3(64), 0, s, f->tbounds, nch, tbtab, out->tbounds_out, nullptr);
  ANR_TRY(check_launch("k_sdf_tbtab (lbw)"));

  // front-end over pvertices + ordered compaction. Every sample's raw is written here (zero where dropped)
  // or by k_lbw_raw; the front-end's sdf output has no meaning for this network and goes to scratch (Ha).
  const int cus = lbw_cus();
  auto F = [&](size_t off) { return (float*)(ws + off); };
  SdfFrontArgs fa{};
  fa.ray_o = ray_o; fa.ray_d = ray_d; fa.near_ = near_; fa.far_ = far_; fa.t_rand = o->t_rand;
  fa.n_rays = R; fa.chunk = chunk; fa.R = f->R; fa.Th = f->Th; fa.verts = f->pvertices; fa.nv = f->n_verts;
  fa.norm_th = o->norm_th; fa.mask = (uint64_t*)(ws + L.mask); fa.chunk_min = (uint64_t*)(ws + L.chunk_min);
  fa.knn = (uint32_t*)(ws + L.knn); fa.raw = raw;
  // the dropped samples' "sdf = 10" stores need (R*64) floats: the list region is free until k_compact
  fa.sdf = (float*)(ws + L.list);
  hipLaunchKernelGGL(k_sdf_front, dim3(std::min(cus, (R + 15) / 16)), dim3(1024), 0, s, fa);
  ANR_TRY(check_launch("k_sdf_front (lbw, pvertices)"));
  CompactArgs ca{};
  ca.n_rays = R; ca.chunk = chunk; ca.mask = fa.mask; ca.chunk_min = fa.chunk_min;
  ca.ray_off = (int*)(ws + L.ray_off); ca.block_sum = (int*)(ws + L.block_sum); ca.list = (int*)(ws + L.list);
  const int nb = (R + 255) / 256;
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(256), 0, s, ca);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, ca.block_sum, nb, counts);
  hipLaunchKernelGGL(k_compact, dim3((R + 3) / 4), dim3(256), 0, s, ca);
  ANR_TRY(check_launch("k_compact (lbw)"));
  int n = 0;
  if (hipMemcpyAsync(&n, counts, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(ANR_E_HIP, "lbw render: kept-count readback");

  if (!image) {
    static const float ident[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    if (hipMemcpyAsync(ws + L.ident, ident, sizeof(ident), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(ws + L.cmin2, 0xff, 8, s) != hipSuccess)
      return fail(ANR_E_HIP, "lbw render: second-search setup");
  }

  float *Ha = F(L.Ha), *Hb = F(L.Hb);
  const long P = L.P;
  auto WN = [&](int l) { return (const float*)wimg + lbw_wn_layer(l).off; };
  const float sqrt2 = 1.41421356237309515f;
  LImgCache limg;
  limg.base = ws + L.limg;
  limg.cap = LBW_LIMG_BYTES;
  const float* Wb[8];
  for (int l = 0; l < 8; ++l) Wb[l] = tp[LBW_BWLIN0 + 2 * l];
  auto Bb = [&](int l) { return tp[LBW_BWLIN0 + 2 * l + 1]; };

  // split-bf16 precisions: the blend-weight MLP, the density net and the colour net as one fused launch per
  // batch each (anr_lbw_b16.hip; ANR_BF16X6: the fp32-level programs of anr_lbw_x6.hip), images packed once per call
  const bool x6 = o->precision == ANR_BF16X6;
  const bool fused = x6 || o->precision == ANR_BF16X3;
  auto wbytes = [&](int L0, int nl) { return x6 ? x6seq_wbytes(L0, nl) : seq_wbytes(L0, nl); };
  unsigned char* bimg = (unsigned char*)(ws + L.bimg);
  unsigned char* dimg = (unsigned char*)(ws + L.dimg);
  unsigned char* cimg = (unsigned char*)(ws + L.cimg);
  if (fused) {
    auto pack = [&](const PackArgs& pa, int L0, int nl, int sl, float sc) {
      const int nt = x6 ? seq_x6_pack_threads(L0, nl) : seq_pack_threads(L0, nl);
      if (x6) hipLaunchKernelGGL(k_pack_seq_x6, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, sl, sc);
      else hipLaunchKernelGGL(k_pack_seq, dim3((nt + 255) / 256), dim3(256), 0, s, pa, L0, nl, sl, sc);
      return check_launch(x6 ? "k_pack_seq_x6 (lbw)" : "k_pack_seq (lbw)");
    };
    PackArgs pb{};
    for (int l = 0; l < 8; ++l) {
      pb.t[l] = Wb[l];
      pb.t[9 + l] = l == 0 || l == 5 ? nullptr : Bb(l);  // folded with the latent
    }
    pb.t[8] = tp[LBW_BWFC_W];
    pb.t[17] = tp[LBW_BWFC_B];
    pb.out = bimg;
    ANR_TRY(pack(pb, ANR_L_LBW0, ANR_LBW_LAYERS, -1, 1.0f));
    PackArgs pd{};
    for (int l = 0; l < 9; ++l) {
      pd.t[l] = WN(l);
      pd.t[9 + l] = tp[3 * l];
    }
    pd.out = dimg;
    ANR_TRY(pack(pd, ANR_L_SDF0, ANR_SDF_LAYERS, 4, 1.0f / sqrt2));
    PackArgs pc{};
    for (int l = 0; l < 5; ++l) {
      pc.t[l] = WN(9 + l);
      pc.t[9 + l] = l == 3 ? nullptr : tp[LBW_CLIN0 + 3 * l];  // lin3's bias: the latent fold
    }
    pc.out = cimg;
    ANR_TRY(pack(pc, ANR_L_LCOL0, ANR_LCOL_LAYERS, -1, 1.0f));
  }

  for (long b0 = 0; b0 < n; b0 += P) {
    const int cnt = (int)std::min<long>(P, n - b0);
    LbwPointArgs a{};
    a.list = ca.list; a.b0 = (int)b0; a.cnt = cnt;
    a.ray_o = ray_o; a.ray_d = ray_d; a.near_ = near_; a.far_ = far_; a.t_rand = o->t_rand; a.chunk = chunk;
    a.R = f->R; a.Th = f->Th; a.A = f->A; a.bigA = f->big_A; a.weights = f->weights; a.knn = fa.knn;
    a.knn2 = image ? nullptr : (const uint32_t*)(ws + L.knn2);
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
        ba.wimg = bimg;
        ba.bias = (const float*)(bimg + wbytes(ANR_L_LBW0, ANR_LBW_LAYERS));
        ba.fold = fold0;  // fold5 = fold0 + 256 (k_lbw_fold)
        ba.ptb = pts;
        ba.ptb_ld = ld;
        ba.pbw32 = a.ibw;
        ba.pbw_rows = F(L.Ybw);
        ba.n_rows = cnt;
        return launch_lbw_bw(ba, cus, s, x6) != 0 ? fail(ANR_E_HIP, "k_lbw_bw launch failed") : ANR_OK;
      }
      ANR_TRY(g.fwd(Ha, 256, 256, Wb[0], 191, fold0, a.Gx, 64, 63, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wb[1], 256, Bb(1), Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(Ha, 256, 256, Wb[2], 256, Bb(2), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wb[3], 256, Bb(3), Ha, 256, 256, 0, true));
      ANR_TRY(g.fwd(Ha, 256, 256, Wb[4], 256, Bb(4), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wb[5], 447, fold5, a.Gx, 64, 63, 0, true, nullptr, 0.f, false, Ha, 256, 256, 191));
      ANR_TRY(g.fwd(Ha, 256, 256, Wb[6], 256, Bb(6), Hb, 256, 256, 0, true));
      ANR_TRY(g.fwd(Hb, 256, 256, Wb[7], 256, Bb(7), Ha, 256, 256, 0, true));
      return g.fwd(F(L.Ybw), 24, 24, tp[LBW_BWFC_W], 256, tp[LBW_BWFC_B], Hb, 256, 256, 0, false);
    };

    // pose space: init_pbw, pbw, LBS to the big pose
    hipLaunchKernelGGL(k_lbw_gather, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_gather"));
    ANR_TRY(bw_mlp(fold, fold + 256, a.ptp, 8));
    hipLaunchKernelGGL(k_lbw_warp, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_warp"));

    // T-pose space: the second search over tvertices (free-sample mode, as anr_knn_blend drives it), tbw
    if (!image) {
      const int Gq = (cnt + 63) / 64;
      const float* rt = (const float*)(ws + L.ident);
      SdfFrontArgs fb{};
      fb.wpts = a.tp3; fb.n_pts = cnt; fb.n_rays = Gq; fb.chunk = Gq;
      fb.R = rt; fb.Th = rt + 9;  // world -> pose with R = I, Th = 0 is the identity in fp32
      fb.verts = f->tvertices; fb.nv = f->n_verts; fb.norm_th = INFINITY;
      fb.mask = (uint64_t*)(ws + L.mask2); fb.chunk_min = (uint64_t*)(ws + L.cmin2);
      fb.knn = (uint32_t*)(ws + L.knn2); fb.raw = (float4*)(ws + L.raw2); fb.sdf = (float*)(ws + L.sdf2);
      hipLaunchKernelGGL(k_sdf_front, dim3(std::min(cus, (Gq + 15) / 16)), dim3(1024), 0, s, fb);
      ANR_TRY(check_launch("k_sdf_front (lbw, tvertices)"));
      hipLaunchKernelGGL(k_lbw_tbw_in, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_lbw_tbw_in"));
      ANR_TRY(bw_mlp(fold + 768, fold + 1024, a.tp3, 3));
      hipLaunchKernelGGL(k_lbw_tbw, pg, pb, 0, s, a);
      ANR_TRY(check_launch("k_lbw_tbw"));
    }

    if (fused) {
      MlpArgs da{};
      da.wimg = dimg;
      da.bias = (const float*)(dimg + wbytes(ANR_L_SDF0, ANR_SDF_LAYERS));
      da.ptb = a.C0;
      da.ptb_ld = 40;
      da.y8 = F(L.Y8);
      da.n_rows = cnt;
      if (launch_lbw_density(da, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_lbw_density launch failed");
      MlpArgs ca2{};
      ca2.wimg = cimg;
      ca2.bias = (const float*)(cimg + wbytes(ANR_L_LCOL0, ANR_LCOL_LAYERS));
      ca2.fold = fold;
      ca2.ptb = a.C0;
      ca2.ptb_ld = 40;
      ca2.y8 = F(L.Y8);
      ca2.yr = F(L.Yc);
      ca2.n_rows = cnt;
      if (launch_lbw_color(ca2, cus, s, x6) != 0) return fail(ANR_E_HIP, "k_lbw_color launch failed");
    } else {
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
    const int cb = LBW_CLIN0;
    ANR_TRY(g.fwd(Ha, 256, 256, WN(9), 286, tp[cb], a.C0, 40, 30, 0, true, nullptr, 0.f, false, F(L.Y8) + 1, 264, 256, 30));
    ANR_TRY(g.fwd(Hb, 256, 256, WN(10), 256, tp[cb + 3], Ha, 256, 256, 0, true));
    ANR_TRY(g.fwd(Ha, 256, 256, WN(11), 256, tp[cb + 6], Hb, 256, 256, 0, true));
    ANR_TRY(g.fwd(Hb, 256, 256, WN(12), 384, fold + 512, Ha, 256, 256, 0, true));
    ANR_TRY(g.fwd(F(L.Yc), 4, 3, WN(13), 256, tp[cb + 12], Hb, 256, 256, 0, false));
    }

    hipLaunchKernelGGL(k_lbw_raw, pg, pb, 0, s, a);
    ANR_TRY(check_launch("k_lbw_raw"));
  }

  if (!image) {
    Layout A{};
    A.counts = L.counts; A.mask = L.mask; A.ray_off = L.ray_off; A.list = L.list; A.sigma = L.sigma;
    A.chunk_max = L.chunk_max; A.flags = L.flags; A.block_sum2 = L.block_sum2; A.out_row = L.out_row;
    ANR_TRY(stage_alpha_ind(R, o, ws, A, s));
  }
  const anr_render_out ro{out->rgb_map, out->acc_map, out->depth_map, out->raw};
  return stage_composite(near_, far_, R, o, raw, &ro, nullptr, s);
}

}  // extern "C"
