// anr_gemm_seq.h — host side of the layer-wise GEMM sequences of the sdf_pdf, aligned_aninerf_lbw and
// aligned_aninerf_pdf renders (anr_sdf_capi.hip, anr_lbw_capi.hip, anr_pdf_capi.hip): the per-call cache of
// split-bf16 weight images, the launcher that routes one layer to k_lgemm (anr_lgemm.hip) or k_gemm (anr_gemm.hip),
// and the layer sequences those renders share (G::skip8, density_sp, colour5). The front-end, compaction and
// fused-image stage they share is anr_knn_host.h. Host code only.
#pragma once
#include <cstdlib>

#include "anr_train.h"
#include "anr_ws.h"

namespace anr {

// weight (and bias) images of the split-bf16 layer GEMM (anr_lgemm.hip), packed on first use in a render call
// (the weights are fixed for its batches) and reused by every later batch
struct LImgCache {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  struct E {
    const float* B[2];
    const float* bias;
    long rs[2], cs[2];
    int K[2], N;
    size_t off;
  } e[48];
  int n = 0;
  const void* get(const GemmArgs& g, hipStream_t s) {
    E k{};
    for (int i = 0; i < g.nseg; ++i) {
      k.B[i] = g.seg[i].B; k.rs[i] = g.seg[i].b_rs; k.cs[i] = g.seg[i].b_cs; k.K[i] = g.seg[i].K;
    }
    k.N = g.N;
    k.bias = g.bias;
    for (int i = 0; i < n; ++i) {
      const E& c = e[i];
      bool same = c.N == k.N && c.bias == k.bias;
      for (int j = 0; j < 2; ++j) same = same && c.B[j] == k.B[j] && c.rs[j] == k.rs[j] && c.cs[j] == k.cs[j] && c.K[j] == k.K[j];
      if (same) return base + c.off;
    }
    const size_t bytes = lgemm_image_bytes(g);
    if (n == 48 || used + bytes > cap) return nullptr;
    k.off = used;
    if (lgemm_pack(g, base + used, s) != 0) return nullptr;
    used = align256(used + bytes);
    e[n++] = k;
    return base + k.off;
  }
};

struct G {
  hipStream_t s;
  int M;
  int x3;  // render precision ANR_BF16X3: split-bf16 MFMA GEMMs (k_lgemm; k_gemm_b<.., .., true> otherwise)
  LImgCache* limg;
  int cus;
  int spd_h = 0;  // the spd operands of bwd / bwd_top hold softplus outputs h (GemmArgs::spd_h)
  float spd_scale = 0.f;  // ... stored as h / spd_scale (GemmArgs::spd_scale)
  // exact fp32 precision: the layer GEMMs that fit k_lgemm run on its F32 kernels (exact fp32 MFMA,
  // fp32 weight image resident in LDS) instead of k_gemm_t (ANR_SDF_LG32=0: k_gemm_t throughout)
  bool lg() const {
    if (x3) return true;
    const char* v = getenv("ANR_SDF_LG32");
    return !(v && v[0] == '0');
  }
  int run(GemmArgs g) {
    if (M <= 0 || g.N <= 0) return ANR_OK;
    g.M = M;
    g.x3 = x3;
    g.ksplit = 1;
    if (lg() && limg && lgemm_supported(g)) {
      g.prof = !x3;  // the exact render's clock (anr_profile_read_clock) from these launches' stamps
      if (const void* img = limg->get(g, s)) {
        (void)lgemm_run(g, img, cus, s);
        return check_launch("k_lgemm (layer sequence)");
      }
    }
    launch_gemm(g, dim3((g.N + 63) / 64, (M + 63) / 64, 1), s);
    return check_launch("k_gemm (layer sequence)");
  }
  // the first reverse GEMM with d sdf / d z7 = softplus_backward(W8[0], z7) applied to the stored
  // lin7 factors D7 as they are loaded (k_lgemm ATR); false (nothing launched) where k_lgemm does not
  // run, and the caller materialises G7 with k_sdf_gtop instead
  bool bwd_top(float* dX, long ldX, int K, const float* D7, const float* w8, int Nout, const float* W, int in_ch,
               const float* spd, int spd_n) {
    if (!lg() || !limg || M <= 0) return false;
    GemmArgs g{};
    g.M = M; g.N = K; g.nseg = 1; g.x3 = x3; g.ksplit = 1; g.prof = !x3;
    g.seg[0] = GemmSeg{D7, 256, 1, W, in_ch, 1, Nout};
    g.C = dX; g.ldc = ldX;
    g.spd = spd; g.ldsd = 256; g.spd_n = spd_n; g.spd_h = spd_h;
    g.a_softplus_w = w8;
    if (!lgemm_supported(g)) return false;
    const void* img = limg->get(g, s);
    if (!img) return false;
    (void)lgemm_run(g, img, cus, s);
    return true;
  }
  // Y = epi([X0 | X1] [W[:, c0:c0+K0] | W[:, c1:c1+K1]]^T + bias)
  // (sp_out_only: softplus with no factor written — deriv only selects the softplus epilogue)
  int fwd(float* Y, long ldY, int N, const float* W, int in_ch, const float* bias, const float* X0, long ld0, int K0,
          int c0, bool relu, float* deriv = nullptr, float div_post = 0.f, bool sp_out_only = false,
          const float* X1 = nullptr, long ld1 = 0, int K1 = 0, int c1 = 0) {
    GemmArgs g{};
    g.N = N;
    g.nseg = X1 ? 2 : 1;
    g.seg[0] = GemmSeg{X0, ld0, 1, W + c0, 1, in_ch, K0};
    if (X1) g.seg[1] = GemmSeg{X1, ld1, 1, W + c1, 1, in_ch, K1};
    g.C = Y; g.ldc = ldY; g.bias = bias; g.relu = relu ? 1 : 0;
    if (deriv) { g.softplus = 1; g.deriv = sp_out_only ? nullptr : deriv; g.ldd = 256; }
    g.div_post = div_post;
    return run(g);
  }
  // split-bf16 only: Yh = Wh relu(X W^T + bias) + bh with the 256-wide hidden activation never stored
  // (k_lgemm HEAD epilogue, two column groups adding into a zeroed Yh); false: nothing launched, the
  // caller runs the two GEMMs
  bool fwd_head(float* Yh, long ldh, int nh, const float* Wh, const float* bh, const float* W, int in_ch,
                const float* bias, const float* X, long ldX, int K) {
    if (!lg() || !limg || M <= 0) return false;
    GemmArgs g{};
    g.M = M; g.N = 256; g.nseg = 1; g.x3 = x3; g.ksplit = 1; g.prof = !x3;
    g.seg[0] = GemmSeg{X, ldX, 1, W, 1, in_ch, K};
    g.C = Yh; g.ldc = 4;  // not written (HEAD); kept valid for the support checks
    g.bias = bias; g.relu = 1;
    g.head_w = Wh; g.head_b = bh; g.head_out = Yh; g.ldh = ldh; g.head_n = nh;
    if (!lgemm_supported(g)) return false;
    const void* img = limg->get(g, s);
    if (!img) return false;
    if (hipMemsetAsync(Yh, 0, (size_t)M * ldh * sizeof(float), s) != hipSuccess) return false;
    (void)lgemm_run(g, img, cus, s);
    return true;
  }
  // Y[:, :256] = softplus(X W^T + bias), with its backward factors in deriv (or none: deriv NULL)
  int fwd_sp(float* Y, const float* W, int in_ch, const float* bias, const float* X, long ldX, float* deriv) {
    GemmArgs g{};
    g.N = 256;
    g.nseg = 1;
    g.seg[0] = GemmSeg{X, ldX, 1, W, 1, in_ch, in_ch};
    g.C = Y; g.ldc = 256; g.bias = bias;
    g.softplus = 1; g.deriv = deriv; g.ldd = 256;
    return run(g);
  }
  // dX[:, :K] = softplus_bwd((dY W[:, :K]) / div_pre, spd) (pass-through at n >= spd_n)
  int bwd(float* dX, long ldX, int K, const float* dY, long ldY, int Nout, const float* W, int in_ch, const float* spd,
          int spd_n, float div_pre = 0.f) {
    GemmArgs g{};
    g.N = K;
    g.nseg = 1;
    g.seg[0] = GemmSeg{dY, ldY, 1, W, in_ch, 1, Nout};
    g.C = dX; g.ldc = ldX;
    g.spd = spd; g.ldsd = 256; g.spd_n = spd_n; g.spd_h = spd ? spd_h : 0; g.spd_scale = spd_scale;
    g.div_pre = div_pre;
    return run(g);
  }

  // ---- whole layer sequences over the scratch activations Ha / Hb ([M][256] each)
  // The 8-layer-plus-fc skip MLP (sdf_pdf / aligned_aninerf_pdf resd, aligned_aninerf_lbw bw) over X = gamma_10
  // ([M][64], K_in columns) -> Y[:, :nY]. W[l] / B[l]: layer l's weight / bias; layers 0 and 5 (in_ch0 / in_ch5
  // weight columns, layer 5 = [X | h4]) take the folded biases fold0 / fold5 (the latent or pose columns folded
  // in). try_head: layer 7 + fc as one k_lgemm HEAD launch where that runs.
  int skip8(float* Y, long ldY, int nY, const float* const W[8], const float* const B[8], const float* fcW,
            const float* fcB, const float* fold0, const float* fold5, const float* X, int K_in, int in_ch0, int in_ch5,
            float* Ha, float* Hb, bool try_head) {
    ANR_TRY(fwd(Ha, 256, 256, W[0], in_ch0, fold0, X, 64, K_in, 0, true));
    ANR_TRY(fwd(Hb, 256, 256, W[1], 256, B[1], Ha, 256, 256, 0, true));
    ANR_TRY(fwd(Ha, 256, 256, W[2], 256, B[2], Hb, 256, 256, 0, true));
    ANR_TRY(fwd(Hb, 256, 256, W[3], 256, B[3], Ha, 256, 256, 0, true));
    ANR_TRY(fwd(Ha, 256, 256, W[4], 256, B[4], Hb, 256, 256, 0, true));
    ANR_TRY(fwd(Hb, 256, 256, W[5], in_ch5, fold5, X, 64, K_in, 0, true, nullptr, 0.f, false, Ha, 256, 256, in_ch0));
    ANR_TRY(fwd(Ha, 256, 256, W[6], 256, B[6], Hb, 256, 256, 0, true));
    if (try_head && fwd_head(Y, ldY, nY, fcW, fcB, W[7], 256, B[7], Ha, 256, 256))
      return check_launch("k_lgemm (skip MLP, layer 7 + fc)");
    ANR_TRY(fwd(Hb, 256, 256, W[7], 256, B[7], Ha, 256, 256, 0, true));
    return fwd(Y, ldY, nY, fcW, 256, fcB, Hb, 256, 256, 0, false);
  }
  // The density net of aligned_aninerf_lbw / _pdf: weight-normed layers WN[0..8] (biases tp[3 l]) over Xs0
  // ([M][40], gamma_6) -> Y8 ([M][264]: density, feature). Softplus outputs only, no stored factors (nothing
  // differentiates here: the dummy factor pointer selects the softplus epilogue of lin3); lin3 writes X4 (217
  // outputs / sqrt2 beside the gamma columns the caller put there), which lin4 reads.
  int density_sp(const float* const* WN, const float* const* tp, const float* Xs0, float* X4, float* Y8, float* Ha,
                 float* Hb) {
    ANR_TRY(fwd_sp(Ha, WN[0], 39, tp[0], Xs0, 40, nullptr));
    ANR_TRY(fwd_sp(Hb, WN[1], 256, tp[3], Ha, 256, nullptr));
    ANR_TRY(fwd_sp(Ha, WN[2], 256, tp[6], Hb, 256, nullptr));
    ANR_TRY(fwd(X4, 256, 217, WN[3], 256, tp[9], Ha, 256, 256, 0, false, Hb, 1.41421356237309515f, true));
    ANR_TRY(fwd_sp(Ha, WN[4], 256, tp[12], X4, 256, nullptr));
    ANR_TRY(fwd_sp(Hb, WN[5], 256, tp[15], Ha, 256, nullptr));
    ANR_TRY(fwd_sp(Ha, WN[6], 256, tp[18], Hb, 256, nullptr));
    ANR_TRY(fwd_sp(Hb, WN[7], 256, tp[21], Ha, 256, nullptr));
    return fwd(Y8, 264, 257, WN[8], 256, tp[24], Hb, 256, 256, 0, false);
  }
  // The colour net of aligned_aninerf_lbw / _pdf: WN[9..13] (biases tp[cb + 3 l]) over [tpose, gamma_4(tpose_dir)]
  // (30 columns of C0, [M][40]) || feature (Y8 columns 1..256) -> Yc ([M][4]); fold3: lin3's bias with
  // color_latent folded in
  int colour5(const float* const* WN, const float* const* tp, int cb, const float* fold3, const float* C0,
              const float* Y8, float* Yc, float* Ha, float* Hb) {
    ANR_TRY(fwd(Ha, 256, 256, WN[9], 286, tp[cb], C0, 40, 30, 0, true, nullptr, 0.f, false, Y8 + 1, 264, 256, 30));
    ANR_TRY(fwd(Hb, 256, 256, WN[10], 256, tp[cb + 3], Ha, 256, 256, 0, true));
    ANR_TRY(fwd(Ha, 256, 256, WN[11], 256, tp[cb + 6], Hb, 256, 256, 0, true));
    ANR_TRY(fwd(Hb, 256, 256, WN[12], 384, fold3, Ha, 256, 256, 0, true));
    return fwd(Yc, 4, 3, WN[13], 256, tp[cb + 12], Hb, 256, 256, 0, false);
  }
};

}  // namespace anr
