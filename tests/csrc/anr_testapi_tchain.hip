// anr_testapi_tchain.hip — test-only C entries to the fused chain programs (anr_tchain.hip: tchain_image_bytes,
// tchain_pack, tchain_run), linked into tests/libanr_testapi.so beside anr_testapi.hip.
//
// A file of its own so that the GEMM entries, their ctypes mirrors and the tests that hold them stay as they
// are. The conventions are anr_testapi.hip's: each entry takes a plain-C descriptor (mirrored by the
// ctypes.Structure classes of tests/_tchain_hooks.py, sizes checked through anr_test_tchain_sizeof), validates
// the documented preconditions (TcArgs / TcPackLayer in anr_train.h, the loads and stores of anr_tchain.hip),
// fills the internal struct and calls tchain_pack / tchain_run the way the executor does. A precondition that
// does not hold returns its own negative code and launches nothing; the launchers' own return values pass
// through unchanged. Nothing here is part of the shipped library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../animatable_nerf_amd/csrc/anr_train.h"

using namespace anr;

extern "C" {

// the codes of anr_testapi.hip that the chain entries return
enum {
  ANR_T_OK = 0,
  ANR_T_NULL = -100,   // a required pointer is NULL
  ANR_T_SHAPE = -101,  // prog / counts / widths out of range
  ANR_T_ALIGN = -106,  // base / stride alignment the kernel requires
  ANR_T_SLAB = -107,   // a buffer holds too few rows or bytes
};

static bool al_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }
static bool al16(const void* p) { return al_to(p, 16); }

// the programs' layer tables as the entries need them (restated from kProgBW / NF / BWB / NFB): out-blocks,
// ReLU, output format (0 bf16 rows, 1 fp32 rows, 2 feature bf16 || alpha fp32, 3 bf16 rows + aux, 4 aux only),
// mask, memory k-steps
struct TcRow { int ob, relu, out, mask, kmem; };
static const TcRow kTc[4][12] = {
    {{16, 1, 0, 0, 2}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 2},
     {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {2, 0, 1, 0, 0}},
    {{16, 1, 0, 0, 2}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {16, 1, 0, 0, 2},
     {16, 1, 0, 0, 0}, {16, 1, 0, 0, 0}, {17, 0, 2, 0, 0}, {16, 0, 0, 0, 0}, {8, 1, 1, 0, 1}, {1, 0, 1, 0, 0}},
    {{16, 0, 0, 1, 1}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0}, {20, 0, 3, 1, 0}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0},
     {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0}, {4, 0, 4, 0, 0}},
    {{8, 0, 1, 1, 1}, {16, 0, 0, 0, 0}, {16, 0, 0, 0, 0}, {16, 0, 0, 1, 1}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0},
     {20, 0, 3, 1, 0}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0}, {16, 0, 0, 1, 0}, {4, 0, 4, 0, 0}}};
static int tc_layers(int prog) { return (prog == 0 || prog == 2) ? 9 : 12; }

unsigned long long anr_test_tchain_image_bytes(int prog) {
  return prog < 0 || prog > 3 ? 0ull : (unsigned long long)tchain_image_bytes(prog);
}

// the caller-filled fields of TcPackLayer (start / ob / k-steps are tchain_pack's)
struct anr_test_tcpack_layer {
  const float* W;
  int in_ch, n1;
  const float* W2;
  int in_ch2, n2;
  int cmem, kmem_cols;
  int cprev, kprev_cols;
  int oc0, oa, oc1, nb, ob_b0;
  int pad0;
};

int anr_test_tchain_pack(int prog, const anr_test_tcpack_layer* L, void* img, unsigned long long img_bytes,
                         hipStream_t s) {
  if (prog < 0 || prog > 3) return ANR_T_SHAPE;
  if (!L || !img) return ANR_T_NULL;
  const int nl = tc_layers(prog);
  for (int l = 0; l < nl; ++l) {
    if (!L[l].W) return ANR_T_NULL;
    // the second source: alpha_fc's row of feature || alpha, the memory k-steps of a transposed layer
    if ((prog < 2 ? L[l].n2 > 0 : kTc[prog][l].kmem > 0) && !L[l].W2) return ANR_T_NULL;
  }
  if (img_bytes < tchain_image_bytes(prog)) return ANR_T_SLAB;
  if (!al16(img)) return ANR_T_ALIGN;
  TcPackArgs a{};
  for (int l = 0; l < nl; ++l) {
    TcPackLayer& P = a.L[l];
    P.W = L[l].W; P.in_ch = L[l].in_ch; P.n1 = L[l].n1;
    P.W2 = L[l].W2; P.in_ch2 = L[l].in_ch2; P.n2 = L[l].n2;
    P.cmem = L[l].cmem; P.kmem_cols = L[l].kmem_cols; P.cprev = L[l].cprev; P.kprev_cols = L[l].kprev_cols;
    P.oc0 = L[l].oc0; P.oa = L[l].oa; P.oc1 = L[l].oc1; P.nb = L[l].nb; P.ob_b0 = L[l].ob_b0;
  }
  return tchain_pack(prog, a, img, s);
}

// TcArgs in plain C, the launch shape, the host copy of M and the row capacity of every row buffer
struct anr_test_tcrun {
  int prog, cap, cus, M_host;
  const void* img;
  const float* bias[12];
  const float* bias2;
  int nout[12];
  void* out[12];
  int ldo[12];
  long out_rows[12];
  float* out2;
  long out2_rows;
  const void* mem;
  int ld_mem, kmem_cols;
  long mem_rows;
  const void* mem2;
  int ld_mem2, kmem2_cols;
  long mem2_rows;
  int mem_f32, mem2_f32;
  void* bits[12];
  long bits_rows[12];
  float* aux;
  int ld_aux, aux_cols, aux_acc, pad0;
  long aux_rows;
  const int* M_dev;
};

// rows of 32 B a backward program's mask DMA reads (TcRing::issue: 128 rows from every tile's first row,
// tiles 112 rows apart)
static long tc_bits_rows_read(long M) { return M <= 0 ? 0 : ((M + 111) / 112 - 1) * 112 + 128; }

static int check_tcrun(const anr_test_tcrun* d) {
  if (d->prog < 0 || d->prog > 3) return ANR_T_SHAPE;
  if (d->cus < 1 || d->cap < 0 || d->M_host < 0) return ANR_T_SHAPE;
  const int prog = d->prog, nl = tc_layers(prog);
  const bool bwd = prog >= 2, two = prog == 1 || prog == 3;
  const long M = d->M_host;
  if (!d->img || !d->M_dev || !d->mem) return ANR_T_NULL;
  if (two && !d->mem2) return ANR_T_NULL;
  if (!bwd && !d->bias2) return ANR_T_NULL;
  if (prog == 1 && !d->out2) return ANR_T_NULL;
  for (int l = 0; l < nl; ++l) {
    const TcRow& T = kTc[prog][l];
    if (!bwd && !d->bias[l]) return ANR_T_NULL;
    if (T.out != 4 && !d->out[l]) return ANR_T_NULL;
    if (bwd && T.mask && !d->bits[l]) return ANR_T_NULL;
  }
  // the memory operands: kmem_cols columns of 2 (forward) / 1 (backward) k-steps, one k-step of the second
  const int memk = bwd ? 1 : 2;
  if (d->kmem_cols < 1 || d->kmem_cols > 32 * memk || d->ld_mem < d->kmem_cols) return ANR_T_SHAPE;
  if (two && (d->kmem2_cols < 1 || d->kmem2_cols > 32 || d->ld_mem2 < d->kmem2_cols)) return ANR_T_SHAPE;
  if (!al_to(d->mem, d->mem_f32 ? 4 : 2) || (two && !al_to(d->mem2, d->mem2_f32 ? 4 : 2))) return ANR_T_ALIGN;
  if (!al16(d->img)) return ANR_T_ALIGN;
  for (int l = 0; l < nl; ++l) {
    const TcRow& T = kTc[prog][l];
    if (T.out == 0 || T.out == 2 || T.out == 3) {
      // bf16 rows: every row is eight 16-B stores of 32 neurons (256 columns)
      if (!bwd && (d->nout[l] < 1 || d->nout[l] > 256)) return ANR_T_SHAPE;
      if (d->ldo[l] < 256) return ANR_T_SHAPE;
      if (d->ldo[l] % 8 != 0 || !al16(d->out[l])) return ANR_T_ALIGN;
    } else if (T.out == 1) {
      if (d->nout[l] < 1 || d->nout[l] > 16 * T.ob || d->ldo[l] < d->nout[l]) return ANR_T_SHAPE;
      if (!al_to(d->out[l], 4)) return ANR_T_ALIGN;
      // a whole group of four columns inside nout is one 16-B store
      if (d->nout[l] >= 4 && (d->ldo[l] % 4 != 0 || !al16(d->out[l]))) return ANR_T_ALIGN;
    }
  }
  if (bwd && d->aux) {
    if (d->aux_cols < 1 || d->aux_cols > 64 || d->ld_aux < d->aux_cols) return ANR_T_SHAPE;
    if (!al_to(d->aux, 4)) return ANR_T_ALIGN;
  }
  // mask bits: rows of 32 B, each lane's 8 B one store / one DMA'd dwordx4 quarter
  for (int l = 0; l < nl; ++l) {
    const TcRow& T = kTc[prog][l];
    const bool used = bwd ? T.mask != 0 : (T.relu && d->bits[l]);
    if (!used) continue;
    if (!al_to(d->bits[l], 8)) return ANR_T_ALIGN;
    if (d->bits_rows[l] < (bwd ? tc_bits_rows_read(M) : M)) return ANR_T_SLAB;
  }
  for (int l = 0; l < nl; ++l)
    if (kTc[prog][l].out != 4 && d->out_rows[l] < M) return ANR_T_SLAB;
  if (prog == 1 && d->out2_rows < M) return ANR_T_SLAB;
  if (d->mem_rows < M || (two && d->mem2_rows < M)) return ANR_T_SLAB;
  if (bwd && d->aux && d->aux_rows < M) return ANR_T_SLAB;
  return ANR_T_OK;
}

// the checks alone (host only)
int anr_test_tchain_check(const anr_test_tcrun* d) { return d ? check_tcrun(d) : ANR_T_NULL; }

int anr_test_tchain_run(const anr_test_tcrun* d, hipStream_t s) {
  if (!d) return ANR_T_NULL;
  const int rc = check_tcrun(d);
  if (rc) return rc;
  TcArgs a{};
  a.img = (const unsigned char*)d->img;
  for (int l = 0; l < 12; ++l) {
    a.bias[l] = d->bias[l]; a.nout[l] = d->nout[l]; a.out[l] = d->out[l]; a.ldo[l] = d->ldo[l];
    a.bits[l] = d->bits[l];
  }
  a.bias2 = d->bias2; a.out2 = d->out2;
  a.mem = (const unsigned short*)d->mem; a.ld_mem = d->ld_mem; a.kmem_cols = d->kmem_cols;
  a.mem2 = (const unsigned short*)d->mem2; a.ld_mem2 = d->ld_mem2; a.kmem2_cols = d->kmem2_cols;
  a.mem_f32 = d->mem_f32; a.mem2_f32 = d->mem2_f32;
  a.aux = d->aux; a.ld_aux = d->ld_aux; a.aux_cols = d->aux_cols; a.aux_acc = d->aux_acc;
  a.M_dev = d->M_dev;
  return tchain_run(d->prog, a, d->cap, d->cus, s);
}

// sizeof of the chain descriptors, numbered on from anr_test_sizeof's 0..4: 5 chain pack layer, 6 chain run
int anr_test_tchain_sizeof(int which) {
  switch (which) {
    case 5: return (int)sizeof(anr_test_tcpack_layer);
    case 6: return (int)sizeof(anr_test_tcrun);
    default: return -1;
  }
}

}  // extern "C"
