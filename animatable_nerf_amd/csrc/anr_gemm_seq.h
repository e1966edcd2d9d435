// anr_gemm_seq.h — host side of the layer-wise GEMM sequences of the sdf_pdf and aligned_aninerf_lbw renders
// (anr_sdf_capi.hip, anr_lbw_capi.hip): the per-call cache of split-bf16 weight images and the launcher that
// routes one layer to k_lgemm (anr_lgemm.hip) or k_gemm (anr_gemm.hip). Host code only.
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
};

}  // namespace anr
