// anr_testapi.hip — test-only C entries to the training GEMM launchers (tests/libanr_testapi.so).
//
// Each entry takes a plain-C descriptor (mirrored by the ctypes.Structure classes of tests/_gemm_hooks.py,
// sizes checked through anr_test_sizeof), validates the launcher's documented preconditions (anr_train.h,
// lgemm_supported, wgrad_f32_fits, the split-K alignment of the vector loads), fills the internal struct and
// calls the launcher the way the executors do, grids included:
//   gemm()  (anr_train_capi.hip): dim3((N + 63) / 64, (M + 63) / 64, ksplit)
//   launch_rgemm(g, M_host, s), launch_wgrad(g, n_host, s, det), launch_wgrad_group(d, nd, n_host, nz, ...)
// A precondition that does not hold returns its own negative code and launches nothing. The launchers'
// own return values (0 / -1) pass through unchanged. Nothing here is part of the shipped library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../animatable_nerf_amd/csrc/anr_train.h"

using namespace anr;

extern "C" {

enum {
  ANR_T_OK = 0,
  ANR_T_LAUNCHER = -1,   // the launcher's own refusal (passed through)
  ANR_T_NULL = -100,     // a required pointer is NULL
  ANR_T_SHAPE = -101,    // M / N / K / nseg / counts out of range
  ANR_T_LAYOUT = -102,   // operand strides the dispatch does not describe
  ANR_T_SPLITK = -103,   // split-K misuse (segments, non-atomic, kper alignment)
  ANR_T_EPILOGUE = -104, // an epilogue the selected path ignores
  ANR_T_FORMAT = -105,   // an operand format combination the kernels exclude
  ANR_T_ALIGN = -106,    // base / stride alignment the kernel requires
  ANR_T_SLAB = -107,     // workspace too small
  ANR_T_UNSUPPORTED = -108,  // lgemm_supported(g) == false
  ANR_T_HIP = -109,      // a HIP error after the launch
};

// ---------------------------------------------------------------------------------------------------
// generic strided GEMM (launch_gemm / launch_gemm_det) and the LDS-resident layer GEMM (lgemm_*)
// ---------------------------------------------------------------------------------------------------
struct anr_test_gemm_desc {
  int M;              // the host row count: the grid's M, and the M the kernel uses when M_dev is NULL
  int N;
  int nseg;
  int K[2];
  const int* M_dev;
  const int* K_dev;
  const float* A[2];
  long a_rs[2], a_cs[2];
  const float* B[2];
  long b_rs[2], b_cs[2];
  float* C;
  long ldc;
  const float* bias;
  int relu;
  int accumulate;
  const float* mask;
  long ldm;
  int atomic;
  int ksplit;
  int kper;
  int softplus;
  float div_pre;
  float div_post;
  float spd_scale;
  float* deriv;
  long ldd;
  const float* spd;
  long ldsd;
  int spd_n;
  int spd_h;
  int bf16;
  int x3;
  float* rowsum;
  float* rowsum2;
  // launch_gemm_det
  int det;
  int pad0;
  float* scratch;
  unsigned long long scratch_floats;
  // k_lgemm only
  const float* a_softplus_w;
  const float* head_w;
  const float* head_b;
  float* head_out;
  long ldh;
  int head_n;
  int cus;
  void* img;                      // device memory for the weight image
  unsigned long long img_bytes;   // its size
  // out: the dispatch the launcher derives from the descriptor (restated from launch_gemm)
  int out_a_k, out_b_k, out_sw;
  int out_a_vec[2], out_b_vec[2];
  int out_vec_out;
  unsigned long long out_image_bytes;  // lgemm_image_bytes(g)
};

static GemmArgs fill_gemm(const anr_test_gemm_desc* d) {
  GemmArgs g{};
  g.M = d->M;
  g.M_dev = d->M_dev;
  g.K_dev = d->K_dev;
  g.N = d->N;
  g.nseg = d->nseg;
  for (int i = 0; i < 2 && i < d->nseg; ++i)
    g.seg[i] = GemmSeg{d->A[i], d->a_rs[i], d->a_cs[i], d->B[i], d->b_rs[i], d->b_cs[i], d->K[i]};
  g.C = d->C; g.ldc = d->ldc; g.bias = d->bias; g.relu = d->relu; g.mask = d->mask; g.ldm = d->ldm;
  g.accumulate = d->accumulate; g.atomic = d->atomic; g.ksplit = d->ksplit < 1 ? 1 : d->ksplit; g.kper = d->kper;
  g.div_pre = d->div_pre; g.softplus = d->softplus; g.deriv = d->deriv; g.ldd = d->ldd;
  g.spd = d->spd; g.ldsd = d->ldsd; g.spd_n = d->spd_n; g.spd_h = d->spd_h; g.spd_scale = d->spd_scale;
  g.div_post = d->div_post;
  g.bf16 = d->bf16; g.x3 = d->x3;
  g.rowsum = d->rowsum; g.rowsum2 = d->rowsum2;
  return g;
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// launch_gemm's dispatch, restated for the tests to assert which path ran
static void gemm_dispatch(const GemmArgs& g, anr_test_gemm_desc* d) {
  const bool a_k = g.seg[0].a_cs == 1 && !(g.rowsum && g.seg[0].a_rs == 1);
  const bool b_k = g.seg[0].b_rs == 1;
  d->out_a_k = a_k;
  d->out_b_k = b_k;
  for (int i = 0; i < 2; ++i) d->out_a_vec[i] = d->out_b_vec[i] = 0;
  for (int i = 0; i < g.nseg; ++i) {
    const GemmSeg& q = g.seg[i];
    const long a_stride = a_k ? q.a_rs : q.a_cs, b_stride = b_k ? q.b_cs : q.b_rs;
    d->out_a_vec[i] = al16(q.A) && (a_stride % 4 == 0) && (a_k || q.a_rs == 1);
    d->out_b_vec[i] = al16(q.B) && (b_stride % 4 == 0) && (b_k || q.b_cs == 1);
  }
  d->out_sw = !g.atomic;
  d->out_vec_out = !g.atomic && g.N % 4 == 0 && g.ldc % 4 == 0 && al16(g.C) && (!g.bias || al16(g.bias)) &&
                   (!g.mask || (g.ldm % 4 == 0 && al16(g.mask))) && (!g.spd || (g.ldsd % 4 == 0 && al16(g.spd))) &&
                   (!g.softplus || !g.deriv || (g.ldd % 4 == 0 && al16(g.deriv)));
}

// the contract of launch_gemm (anr_train.h GemmArgs, anr_gemm.hip's header and launch_gemm)
static int check_gemm(anr_test_gemm_desc* d) {
  if (!d->C) return ANR_T_NULL;
  if (d->M < 1 || d->N < 1 || d->nseg < 1 || d->nseg > 2) return ANR_T_SHAPE;
  for (int i = 0; i < d->nseg; ++i) {
    if (!d->A[i] || !d->B[i]) return ANR_T_NULL;
    if (d->K[i] < 1) return ANR_T_SHAPE;
    // each operand is contiguous along k or along its row index; the dispatch reads segment 0 only, so
    // segment 1 has the same layout
    if (d->a_rs[i] != 1 && d->a_cs[i] != 1) return ANR_T_LAYOUT;
    if (d->b_rs[i] != 1 && d->b_cs[i] != 1) return ANR_T_LAYOUT;
    if (i && ((d->a_cs[i] == 1) != (d->a_cs[0] == 1) || (d->a_rs[i] == 1) != (d->a_rs[0] == 1))) return ANR_T_LAYOUT;
    if (i && ((d->b_rs[i] == 1) != (d->b_rs[0] == 1) || (d->b_cs[i] == 1) != (d->b_cs[0] == 1))) return ANR_T_LAYOUT;
  }
  const int ksplit = d->ksplit < 1 ? 1 : d->ksplit;
  if (ksplit > 1 && (d->nseg != 1 || !d->atomic)) return ANR_T_SPLITK;  // "split-K only with one segment"
  if (d->kper < 0) return ANR_T_SPLITK;
  if (d->K_dev && d->nseg != 1) return ANR_T_SPLITK;
  if (d->atomic && (d->relu || d->mask || d->accumulate || d->softplus || d->spd || d->div_pre != 0.f ||
                    d->div_post != 0.f))
    return ANR_T_EPILOGUE;  // the atomic epilogue adds the partial (and the bias once), nothing else
  if (d->rowsum2 && !d->rowsum) return ANR_T_EPILOGUE;
  if (d->rowsum && d->a_rs[0] != 1) return ANR_T_EPILOGUE;  // row sums come from the m-contiguous path only
  if (d->spd && (d->spd_n < 0 || d->spd_n > d->N)) return ANR_T_EPILOGUE;
  if (d->x3 && d->a_cs[0] != 1) return ANR_T_FORMAT;         // split-bf16: A k-contiguous
  if (d->x3 && d->rowsum && d->a_rs[0] == 1) return ANR_T_FORMAT;
  // split-K with 16-B operand loads: every split starts on a whole K tile
  GemmArgs g = fill_gemm(d);
  gemm_dispatch(g, d);
  if (ksplit > 1 && d->kper > 0 && (d->out_a_vec[0] || d->out_b_vec[0]) && d->kper % 32 != 0) return ANR_T_SPLITK;
  return ANR_T_OK;
}

int anr_test_gemm(anr_test_gemm_desc* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  const int rc = check_gemm(d);
  if (rc) return rc;
  GemmArgs g = fill_gemm(d);
  if (d->det) {
    const int r = launch_gemm_det(g, d->M, d->scratch, (size_t)d->scratch_floats, s);
    return r;
  }
  launch_gemm(g, dim3((g.N + 63) / 64, (d->M + 63) / 64, g.ksplit), s);
  return hipGetLastError() == hipSuccess ? ANR_T_OK : ANR_T_HIP;
}

unsigned long long anr_test_gemm_det_floats(int M, int N, int ksplit) { return gemm_det_floats(M, N, ksplit); }

// supported-check, image-bytes, pack and run of the LDS-resident layer GEMM; cus from the caller
int anr_test_lgemm(anr_test_gemm_desc* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  const int rc = check_gemm(d);
  if (rc) return rc;
  GemmArgs g = fill_gemm(d);
  g.a_softplus_w = d->a_softplus_w;
  g.head_w = d->head_w; g.head_b = d->head_b; g.head_out = d->head_out; g.ldh = d->ldh; g.head_n = d->head_n;
  if (!lgemm_supported(g)) return ANR_T_UNSUPPORTED;
  d->out_image_bytes = lgemm_image_bytes(g);
  if (!d->img) return ANR_T_NULL;
  if (d->img_bytes < d->out_image_bytes) return ANR_T_SLAB;
  if (d->cus < 1) return ANR_T_SHAPE;
  if (lgemm_pack(g, d->img, s) != 0) return ANR_T_LAUNCHER;
  return lgemm_run(g, d->img, d->cus, s);
}

// lgemm_pack_batch of the images of d[0..n) (n <= 4) into img[0..n), as anr_sdf_train.hip's per-call plan
// does: the descriptors (lgemm_pack_describe) and block starts go to the caller's device memory dev_descs
// (n * lgemm_pack_desc_bytes() bytes) and dev_starts (n + 1 longs)
int anr_test_lgemm_pack_batch(anr_test_gemm_desc* d, int n, void* const* img, void* dev_descs, long* dev_starts,
                              hipStream_t s) {
  if (!d || !img || !dev_descs || !dev_starts) return ANR_T_NULL;
  if (n < 1 || n > 4) return ANR_T_SHAPE;
  const size_t db = lgemm_pack_desc_bytes();
  if (db > 512) return ANR_T_SLAB;
  unsigned char host[4 * 512];
  long starts[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const int rc = check_gemm(&d[i]);
    if (rc) return rc;
    GemmArgs g = fill_gemm(&d[i]);
    if (!lgemm_supported(g)) return ANR_T_UNSUPPORTED;
    if (!img[i]) return ANR_T_NULL;
    starts[i + 1] = starts[i] + lgemm_pack_describe(g, img[i], host + i * db);
  }
  if (hipMemcpyAsync(dev_descs, host, n * db, hipMemcpyHostToDevice, s) != hipSuccess) return ANR_T_HIP;
  if (hipMemcpyAsync(dev_starts, starts, (n + 1) * sizeof(long), hipMemcpyHostToDevice, s) != hipSuccess) return ANR_T_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return ANR_T_HIP;  // the staging arrays live on this stack
  return lgemm_pack_batch(dev_descs, dev_starts, n, starts[n], s);
}

// ---------------------------------------------------------------------------------------------------
// bf16 row GEMM (launch_rgemm)
// ---------------------------------------------------------------------------------------------------
struct anr_test_rgemm_desc {
  int M_host;
  int N;
  int nseg;
  int K[2];
  int bcol[2];
  int rows[2];
  const int* M_dev;
  const void* A[2];   // fp32 rows, or bf16 rows (abf)
  long lda[2];
  const unsigned short* B[2];
  long ldb[2];
  long lo_off[2];
  void* C;            // fp32 rows, or bf16 rows (cbf)
  long ldc;
  const float* bias;
  const void* mask;   // fp32 rows, or bf16 rows (mbf)
  long ldm;
  int relu;
  int accumulate;
  int x3, abf, cbf, mbf;
  // out: launch_rgemm's derived flags and the kernel variant it dispatches (restated)
  int out_vec_out, out_vec16;
  int out_variant;    // 0 fp32 rows, 1 abf, 2 abf + mbf mask, 3 mbf mask, 4 x3
};

static int check_rgemm(const anr_test_rgemm_desc* d) {
  if (!d->C) return ANR_T_NULL;
  if (d->M_host < 1 || d->N < 1 || d->N > 256 || d->nseg < 1 || d->nseg > 2) return ANR_T_SHAPE;  // "N <= 256"
  if (d->x3 && (d->abf || d->cbf || d->mbf)) return ANR_T_FORMAT;  // "Not with x3"
  if (d->cbf && d->accumulate) return ANR_T_FORMAT;                // "C bf16 excludes accumulate"
  const int kc = d->x3 ? 32 : 64;
  for (int i = 0; i < d->nseg; ++i) {
    if (!d->A[i] || !d->B[i]) return ANR_T_NULL;
    if (d->K[i] < 1) return ANR_T_SHAPE;
    // "A_s rows (stride lda elements, 16-B aligned, lda >= K_s rounded up to 64)"
    if (!al16(d->A[i]) || d->lda[i] % (d->abf ? 8 : 4) != 0) return ANR_T_ALIGN;
    if (d->lda[i] < (long)((d->K[i] + 63) / 64 * 64)) return ANR_T_SHAPE;
    // "B_s bf16 image rows (k-contiguous, stride ldb, chunk-aligned column offset bcol, `rows` valid rows)"
    if (!al16(d->B[i]) || d->ldb[i] % 8 != 0 || d->bcol[i] < 0 || d->bcol[i] % kc != 0) return ANR_T_ALIGN;
    if (d->ldb[i] < (long)d->bcol[i] + (d->K[i] + kc - 1) / kc * kc) return ANR_T_SHAPE;
    if (d->rows[i] < d->N) return ANR_T_SHAPE;  // the executor's `rows >= K` (xgrad): every output has an image row
    if (d->x3 && (d->lo_off[i] % 8 != 0 || d->lo_off[i] == 0)) return ANR_T_ALIGN;
  }
  if (((uintptr_t)d->C % (d->cbf ? 2 : 4)) != 0) return ANR_T_ALIGN;
  if (d->mask && ((uintptr_t)d->mask % (d->mbf ? 2 : 4)) != 0) return ANR_T_ALIGN;
  return ANR_T_OK;
}

int anr_test_rgemm(anr_test_rgemm_desc* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  const int rc = check_rgemm(d);
  if (rc) return rc;
  RGemm g{};
  g.M = d->M_host;
  g.M_dev = d->M_dev;
  g.N = d->N;
  g.nseg = d->nseg;
  for (int i = 0; i < d->nseg; ++i)
    g.seg[i] = RGemmSeg{(const float*)d->A[i], d->lda[i], d->K[i], d->B[i], d->ldb[i], d->bcol[i], d->rows[i], d->lo_off[i]};
  g.C = (float*)d->C; g.ldc = d->ldc; g.bias = d->bias; g.relu = d->relu;
  g.mask = (const float*)d->mask; g.ldm = d->ldm; g.accumulate = d->accumulate;
  g.x3 = d->x3; g.abf = d->abf; g.cbf = d->cbf; g.mbf = d->mbf;
  // launch_rgemm's derived flags, restated
  const size_t ce = g.cbf ? 2 : 4, me = g.mbf ? 2 : 4;
  d->out_vec_out = (g.N % 4 == 0) && (g.ldc % 4 == 0) && ((uintptr_t)g.C % (4 * ce) == 0) &&
                   (!g.mask || ((g.ldm % 4 == 0) && ((uintptr_t)g.mask % (4 * me) == 0))) && ((uintptr_t)g.bias % 16 == 0);
  d->out_vec16 = d->out_vec_out && g.cbf && g.ldc % 8 == 0 && (uintptr_t)g.C % 16 == 0;
  const bool mbf = g.mbf && g.mask;
  d->out_variant = g.x3 ? 4 : (g.abf && mbf) ? 2 : g.abf ? 1 : mbf ? 3 : 0;
  launch_rgemm(g, d->M_host, s);
  return hipGetLastError() == hipSuccess ? ANR_T_OK : ANR_T_HIP;
}

// the training GEMM weight images (wimg_pack / wimg_view): t = ANR_NUM_TENSORS (+ novel) tensor pointers
unsigned long long anr_test_wimg_bytes(void) { return wimg_bytes(); }
int anr_test_wimg_pack(const float* const* t, void* dst, hipStream_t s) { return wimg_pack(t, dst, s); }
struct anr_test_wview {
  const unsigned short* B;
  long ldb;
  long lo_off;
  int bcol;
  int rows;
};
int anr_test_wimg_view(const void* base, const float* const* t, const float* W, int c0, int K, int bwd,
                       anr_test_wview* v) {
  WView w{};
  if (!wimg_view(base, t, W, c0, K, bwd != 0, &w)) return 0;
  v->B = w.B; v->ldb = w.ldb; v->lo_off = w.lo_off; v->bcol = w.bcol; v->rows = w.rows;
  return 1;
}

// ---------------------------------------------------------------------------------------------------
// weight gradients (launch_wgrad, launch_wgrad_f32, launch_wgrad_group)
// ---------------------------------------------------------------------------------------------------
struct anr_test_wgrad_desc {
  const void* dY;   // fp32 rows, or bf16 rows (ybf)
  long ldY;
  const void* X;    // fp32 rows, or bf16 rows (xbf)
  long ldX;
  float* dW;        // the first written element (row 0, column c0 of the wider tensor)
  long ldw;
  float* bsum;
  float* bsum2;
  const int* M_dev;
  int nout;
  int K;
  int x3, ybf, xbf;
  int j0;
};

enum { ANR_T_WG_SINGLE = 0, ANR_T_WG_F32 = 1, ANR_T_WG_GROUP = 2 };

struct anr_test_wgrad_call {
  int mode;         // ANR_T_WG_*
  int det;
  int n_host;
  int nd;           // descriptors (1 unless group)
  int nz;           // group: sample ranges per product
  int pad0;
  const anr_test_wgrad_desc* d;
  float* slab;
  unsigned long long slab_floats;
  // out
  int out_f32_fits;   // mode f32: wgrad_f32_fits(d[0])
  int out_format;     // single: 0 x3, 1 bf16 x bf16, 2 bf16 dY, 3 bf16 X, 4 fp32 rows rounded to bf16
};

static int check_wgrad(const anr_test_wgrad_desc& d, int mode, int n_host) {
  if (!d.dY || !d.X || !d.dW) return ANR_T_NULL;
  if (d.nout < 1 || d.nout > 256 || d.K < 1 || d.K > 256) return ANR_T_SHAPE;  // "i < nout <= 256, j < K <= 256"
  if (d.x3 && (d.ybf || d.xbf)) return ANR_T_FORMAT;                          // "not with x3"
  if (mode == ANR_T_WG_F32 && (d.j0 < 0 || d.j0 > 3 || d.j0 >= d.K)) return ANR_T_SHAPE;
  if (mode != ANR_T_WG_F32 && d.j0 != 0) return ANR_T_SHAPE;                  // "k_wgrad_f32: columns j < j0"
  if (mode == ANR_T_WG_F32) return ANR_T_OK;  // the rest is wgrad_f32_fits, the launcher's own refusal
  // "dY, X: fp32 rows, 16-B aligned, ld % 4 == 0"; whole 4-column groups of the used columns lie in a row
  if (!al16(d.dY) || !al16(d.X) || d.ldY % 4 != 0 || d.ldX % 4 != 0) return ANR_T_ALIGN;
  if (d.ldY < (d.nout + 3) / 4 * 4 || d.ldX < (d.K + 3) / 4 * 4 || d.ldw < d.K) return ANR_T_SHAPE;
  (void)n_host;
  return ANR_T_OK;
}

static WGrad fill_wgrad(const anr_test_wgrad_desc& d) {
  WGrad g{};
  g.dY = (const float*)d.dY; g.ldY = d.ldY; g.nout = d.nout;
  g.X = (const float*)d.X; g.ldX = d.ldX; g.K = d.K;
  g.dW = d.dW; g.ldw = d.ldw; g.bsum = d.bsum; g.bsum2 = d.bsum2;
  g.M_dev = d.M_dev;
  g.x3 = d.x3; g.ybf = d.ybf; g.xbf = d.xbf; g.j0 = d.j0;
  return g;
}

unsigned long long anr_test_wgrad_slab_floats(void) { return wgrad_slab_floats(); }

int anr_test_wgrad(anr_test_wgrad_call* c, hipStream_t s) {
  if (!c || !c->d || !c->slab) return ANR_T_NULL;
  if (c->n_host < 1 || c->nd < 1 || (c->mode != ANR_T_WG_GROUP && c->nd != 1)) return ANR_T_SHAPE;
  if (c->mode < ANR_T_WG_SINGLE || c->mode > ANR_T_WG_GROUP) return ANR_T_SHAPE;
  if (c->mode == ANR_T_WG_F32 && c->det) return ANR_T_FORMAT;  // launch_wgrad_f32 has no fixed-order form
  for (int k = 0; k < c->nd; ++k) {
    const int rc = check_wgrad(c->d[k], c->mode, c->n_host);
    if (rc) return rc;
  }
  if (c->mode != ANR_T_WG_GROUP && c->slab_floats < wgrad_slab_floats()) return ANR_T_SLAB;  // "slab: wgrad_slab_floats()"
  if (c->mode == ANR_T_WG_SINGLE) {
    WGrad g = fill_wgrad(c->d[0]);
    g.slab = c->slab;
    c->out_format = g.x3 ? 0 : (g.ybf && g.xbf) ? 1 : g.ybf ? 2 : g.xbf ? 3 : 4;
    return launch_wgrad(g, c->n_host, s, c->det != 0);
  }
  if (c->mode == ANR_T_WG_F32) {
    WGrad g = fill_wgrad(c->d[0]);
    g.slab = c->slab;
    c->out_f32_fits = wgrad_f32_fits(g) ? 1 : 0;
    return launch_wgrad_f32(g, c->n_host, s);
  }
  if (c->nd > 64) return ANR_T_SHAPE;
  WGrad g[64];
  for (int k = 0; k < c->nd; ++k) g[k] = fill_wgrad(c->d[k]);
  return launch_wgrad_group(g, c->nd, c->n_host, c->nz, c->slab, (size_t)c->slab_floats, s, c->det != 0);
}

// sizeof of each descriptor: 0 gemm, 1 rgemm, 2 wgrad descriptor, 3 wgrad call, 4 weight-image view
int anr_test_sizeof(int which) {
  switch (which) {
    case 0: return (int)sizeof(anr_test_gemm_desc);
    case 1: return (int)sizeof(anr_test_rgemm_desc);
    case 2: return (int)sizeof(anr_test_wgrad_desc);
    case 3: return (int)sizeof(anr_test_wgrad_call);
    case 4: return (int)sizeof(anr_test_wview);
    default: return -1;
  }
}

}  // extern "C"
