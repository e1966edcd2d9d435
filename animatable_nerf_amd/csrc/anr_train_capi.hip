// anr_train_capi.hip — C-ABI of the training executor (include/aninerf.h, "training" section).
//
// Layer-wise: the kept samples of a 1,024-ray batch (~24k) are few enough that every layer is a
// GEMM over the whole batch with its activation kept in HBM; the backward runs the same layers in
// reverse (dX = dY W, dW += dY^T X) plus the per-sample kernels of anr_train.hip. The kept-sample
// count stays on the device (M_dev / K_dev in the GEMM arguments, capacity-sized grids), so no call
// syncs with the host (the reference syncs ~6x per chunk).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_kernels.h"
#include "anr_train.h"
#include "anr_ws.h"

using namespace anr;

namespace {

// weight-gradient lanes (side streams below). The box runs GPU_MAX_HW_QUEUES=4 hardware queues per
// process and streams share them round robin: the caller's stream, s2 and two lanes fill four, and
// more lanes would put a weight-gradient lane on s2's queue (measured: the T-pose chain then waits
// behind weight gradients, profiles/r3k trace)
constexpr int kWStreams = 2;
// partial-slab floats per lane: a weight-gradient group of up to 16 products at 16 sample ranges
const size_t kLaneFloats = 4 * wgrad_slab_floats();

// ---- deterministic mode ---------------------------------------------------------------------------
// anr_train_deterministic (process-wide) / ANR_TRAIN_DETERMINISTIC=1|0 (read per call, wins when set).
// With the mode on every float accumulation of a step has a fixed order (DESIGN "Deterministic mode"):
//  - every weight-gradient product, its reduction and the latent-row updates run on ONE stream (lane 0;
//    the caller's under ANR_TRAIN_SERIAL) in issue order, so the adds into one gradient element are
//    ordered by the stream whatever the executor's streams are;
//  - the slab reductions are k_wgrad_reduce_det (all sample ranges in order, one plain add), products of
//    a group that share a target in consecutive launches;
//  - the generic split-K products store per-split partials (launch_gemm_det) instead of atomics;
//  - the latent-row updates of a flush are one launch per post, in post order;
//  - the loss kernels store per-block partials that k_det_sum adds in block order.
std::atomic<int> g_train_det{0};
}  // namespace
namespace anr {
int train_det() {  // anr_train.h: the sdf_pdf step (anr_sdf_train.hip) reads it too
  const char* v = getenv("ANR_TRAIN_DETERMINISTIC");
  if (v && (v[0] == '0' || v[0] == '1') && v[1] == 0) return v[0] == '1';
  return g_train_det.load(std::memory_order_relaxed);
}
}  // namespace anr
namespace {
// scratch of the deterministic split-K products: 512-sample splits of at most 256 x 256 outputs
size_t det_scratch_floats(long N) { return gemm_det_floats(256, 256, (int)((N + 511) / 512)); }
// per-block loss partials (k_tr_loss: 2 sums x 2 rows of blocks; k_an_loss: 1)
size_t loss_part_floats(long N) { return (size_t)((N + 255) / 256) * 4; }

// training workspace = render layout (prefix, incl. raw) + per-sample activations / gradients
struct TLayout {
  Layout L;
  size_t pt, Gp, Ip, Gv, Lp, lbs, Gt, It, Lt, Hp, Ht, Hn, Feat, Alpha, Lat, View, Rgbl;
  size_t draw, dRgb, dAlpha, dA16, dBp, dBt, dLp, dLt, dIt, dGt, dGt2, dHn, dHt, dHp, dFeat, dLat, dView;
  size_t ysum, acc3, d_rgb, d_pbw, d_tbw, wimg, wslab, tcimg, bitsP, bitsT, bitsN, lpart, dscr, dscr_floats, total;
};

// ReLU mask bits of one chain layer (TcArgs::bits): 32 B per sample, 128 rows past the last (a tile's
// mask DMA reads 4 KiB = 128 rows from the tile's first)
// rows of a layer's mask bits: at least TcArgs::bits' (ceil(N / 112) - 1) x 112 + 128 (the last tile's mask
// DMA reads 128 rows from its first row; N rounded up to 128, + 128, covers it for every N)
size_t bits_stride(long N) { return (size_t)((N + 127) / 128 * 128 + 128) * 32; }

// f: the frame, for the voxel counts of its pose / T-pose blend-weight volumes
TLayout tlayout(int n_rays, int chunk, const anr_frame* f) {
  TLayout T{};
  const long np = (long)f->pbw_dims[0] * f->pbw_dims[1] * f->pbw_dims[2];
  const long nt = (long)f->tbw_dims[0] * f->tbw_dims[1] * f->tbw_dims[2];
  T.L = layout(n_rays, chunk, np, nt, true);
  Carve c{T.L.total};
  const size_t N = (size_t)n_rays * 64, R = (size_t)n_rays;
  T.pt = c.floats(N * 8); T.Gp = c.floats(N * 64); T.Ip = c.floats(N * 32); T.Gv = c.floats(N * 32);
  T.Lp = c.floats(N * 32); T.lbs = c.floats(N * 16); T.Gt = c.floats(N * 64); T.It = c.floats(N * 32);
  T.Lt = c.floats(N * 32); T.Hp = c.floats(N * 256 * 8); T.Ht = c.floats(N * 256 * 8); T.Hn = c.floats(N * 256 * 8);
  T.Feat = c.floats(N * 256); T.Alpha = c.floats(N); T.Lat = c.floats(N * 256); T.View = c.floats(N * 128);
  T.Rgbl = c.floats(N * 4); T.draw = c.floats(N * 4); T.dRgb = c.floats(N * 4); T.dAlpha = c.floats(N);
  T.dA16 = c.floats(N * 32); T.dBp = c.floats(N * 24); T.dBt = c.floats(N * 24);
  T.dLp = c.floats(N * 64); T.dLt = c.floats(N * 64); T.dIt = c.floats(N * 32);  // logit gradients in rows of 64
  T.dGt = c.floats(N * 64); T.dGt2 = c.floats(N * 64);
  // every layer's output gradient has its own slot (the weight-gradient products read them on the
  // side stream while the input-gradient chain moves on)
  T.dHn = c.floats(N * 256 * 8); T.dHt = c.floats(N * 256 * 8); T.dHp = c.floats(N * 256 * 8);
  T.dFeat = c.floats(N * 256); T.dLat = c.floats(N * 256); T.dView = c.floats(N * 128);
  T.ysum = c.floats(8 * 256); T.acc3 = c.floats(4); T.d_rgb = c.floats(R * 3); T.d_pbw = c.floats(N * 24);
  T.d_tbw = c.floats(N * 24);
  T.wimg = c.floats((wimg_bytes() + 3) / 4);
  T.wslab = c.floats(kLaneFloats * kWStreams);
  // fused-chain images (anr_tchain.hip): BW / NeRF forward, BW / NeRF input-gradient chains
  T.tcimg = c.floats((tchain_image_bytes(0) + tchain_image_bytes(1) + tchain_image_bytes(2) + tchain_image_bytes(3) + 3) / 4);
  // the forward chains' ReLU mask bits for the input-gradient chains: pose / T-pose BW (8 layers), NeRF
  // (8 layers + view_fc)
  T.bitsP = c.floats(8 * bits_stride((long)N) / 4); T.bitsT = c.floats(8 * bits_stride((long)N) / 4);
  T.bitsN = c.floats(9 * bits_stride((long)N) / 4);
  // deterministic mode: per-block loss partials, per-split partials of the generic weight gradients
  T.lpart = c.floats(loss_part_floats((long)std::max(N, R)));
  T.dscr_floats = det_scratch_floats((long)N);
  T.dscr = c.floats(T.dscr_floats);
  T.total = c.o;
  return T;
}

int check_args(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d, const float* near_,
               const float* far_, int n_rays, const anr_render_opts* o, void* ws) {
  if (!p || !f || !o || !ws || !ray_o || !ray_d || !near_ || !far_) return fail(ANR_E_ARG, "train: NULL argument");
  if (o->n_samples != 64) return fail(ANR_E_ARG, "train: only N_samples == 64 is supported");
  if (o->chunk <= 0 || n_rays <= 0) return fail(ANR_E_ARG, "train: bad chunk / n_rays");
  if (o->novel_pose) return fail(ANR_E_ARG, "train: novel_pose is a render-only option");
  if (o->precision < ANR_FP32 || o->precision > ANR_BF16X3)
    return fail(ANR_E_ARG, "train: bad precision");
  for (int i = 0; i < ANR_NUM_TENSORS; ++i)
    if (!p->t[i]) return fail(ANR_E_ARG, "train: NULL parameter tensor");
  if (!f->A || !f->R || !f->Th || !f->pbw || !f->tbw || !f->pbounds || !f->tbounds || !f->latent_index)
    return fail(ANR_E_ARG, "train: NULL frame tensor");
  return check_views("train", f);
}

// ---- side streams -------------------------------------------------------------------------------
// The backward's critical path is the input-gradient chain (dX = dY W (ReLU mask), layer after
// layer). The weight-gradient products (dW += dY^T X, their slab reductions and the latent-row
// updates) hang off it and run on side streams `sw[]` (round robin, one partial-slab region each;
// the latent-row updates of one table all on sw[0], they share the table row); the T-pose
// blend-weight MLP (forward and
// backward) runs on `s2` beside the canonical NeRF, since both read only gamma(x_T). At ~24k kept
// samples one 128-row GEMM occupies 188 of the 256 CUs for ~20 us, so a single stream leaves the
// chip a quarter idle and serialises ~80 launches that do not depend on each other. The streams
// are per device, created once, ordered with the caller's stream by events (fork / join), so every
// entry point still behaves as one asynchronous call on the caller's stream.
// ANR_TRAIN_SERIAL=1 runs everything on the caller's stream (debugging aid).
// Stream priorities were measured (profiles/r4c): the critical chain on a highest-priority stream of
// the library's own made the bf16 step 3.27 ms instead of 1.96 (one more queue than the hardware
// queues the process gets), the weight-gradient lanes at the lowest priority changed nothing (1.945).
struct SideStreams {
  hipStream_t main = nullptr;  // the library's own main stream (OnMain)
  hipStream_t s2 = nullptr, sw[kWStreams] = {};
  int lanes = kWStreams;  // weight-gradient lanes created (ANR_TRAIN_LANES, 1..kWStreams)
  hipStream_t cap = nullptr;  // origin stream of step-graph captures (created on first use)
  hipEvent_t ev[64] = {};
  unsigned next = 0;
};

SideStreams* side_streams() {
  static SideStreams per_dev[16];
  static std::mutex mu;
  const char* serial = getenv("ANR_TRAIN_SERIAL");
  if (serial && serial[0] == '1') return nullptr;
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 16) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  SideStreams& ss = per_dev[d];
  if (!ss.s2) {
    SideStreams t{};
    if (hipStreamCreateWithFlags(&t.s2, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipStreamCreateWithFlags(&t.main, hipStreamNonBlocking) != hipSuccess) return nullptr;
    const char* lv = getenv("ANR_TRAIN_LANES");
    t.lanes = lv && atoi(lv) >= 1 && atoi(lv) <= kWStreams ? atoi(lv) : kWStreams;
    for (int l = 0; l < kWStreams; ++l) {
      if (l >= t.lanes) {
        t.sw[l] = t.sw[0];  // fewer hardware queues in use: the extra lanes alias lane 0
        continue;
      }
      if (hipStreamCreateWithFlags(&t.sw[l], hipStreamNonBlocking) != hipSuccess) return nullptr;
    }
    for (auto& e : t.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    ss = t;
  }
  return &ss;
}

// work issued to `to` from now on runs after everything already issued to `from`
int order(SideStreams* ss, hipStream_t to, hipStream_t from) {
  if (!ss || to == from) return ANR_OK;
  hipEvent_t ev = ss->ev[ss->next++ & 63];
  if (hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess)
    return fail(ANR_E_HIP, "stream ordering failed");
  return ANR_OK;
}

// two-phase order: mark() records `from`'s position now, after() makes `to` wait for it later (an
// event of the ring: fewer than 64 order / mark calls may come in between)
int mark(SideStreams* ss, hipStream_t from, hipEvent_t* ev) {
  *ev = nullptr;  // no side streams (ANR_TRAIN_SERIAL): one stream, nothing to order
  if (!ss) return ANR_OK;
  *ev = ss->ev[ss->next++ & 63];
  return hipEventRecord(*ev, from) == hipSuccess ? ANR_OK : fail(ANR_E_HIP, "hipEventRecord failed");
}
int after(hipStream_t to, hipEvent_t ev) {
  if (ev && hipStreamWaitEvent(to, ev, 0) != hipSuccess) return fail(ANR_E_HIP, "stream ordering failed");  // NULL: none
  return ANR_OK;
}

// A training entry point runs on the library's own main stream, forked from the caller's stream on
// entry and joined back into it on exit (also on an error return). Round 4 introduced it after the
// grouped weight gradients read unwritten gradient rows (NaN, tools/nan_probe.py) whenever the caller
// was the legacy default stream. The cause (found in round 5) was not the stream kind: Exec::pend_src
// marked "no queued source stream" with nullptr, which is also the legacy default stream's handle, so a
// product queued from stream 0 never recorded its source and flush_w() issued the group on lane 0 with
// no edge after stream 0. pend_src now carries an explicit count (npsrc). Round 6: the caller's stream
// is the main stream by default (the library's side streams are non-blocking, so they order against the
// legacy stream through events like against any other): the fork's two cross-stream edges cost ~20-35 us
// a step (1.035 / 1.055 vs 1.017 ms, profiles/round6/r8d_*). ANR_TRAIN_ON_CALLER=0 (read per call)
// restores the fork onto a library-owned non-blocking stream.
struct OnMain {
  SideStreams* ss;
  hipStream_t caller, s;
  int rc = ANR_OK;
  OnMain(SideStreams* x, hipStream_t c) : ss(x), caller(c), s(c) {
    const char* oc = getenv("ANR_TRAIN_ON_CALLER");
    if (ss && ss->main && oc && oc[0] == '0') {
      rc = order(ss, ss->main, caller);
      s = ss->main;
    }
  }
  ~OnMain() {
    if (s != caller) (void)order(ss, caller, s);
  }
};

// storage flags of a product's operands (training precision 'bf16': hidden activations, their
// gradients and the gamma inputs of the T-pose / canonical MLPs are kept as bf16 — every consumer
// rounds them to bf16 for the MFMA anyway, so the products are unchanged and their bytes halve)
enum : unsigned { BF_A = 1u, BF_C = 2u, BF_M = 4u, BF_X = 8u };  // A (or dY), output, mask, wgrad X

struct Exec {
  hipStream_t s;
  int n;         // kept samples (host copy; unused when n_dev is set)
  int bf16 = 0;       // current GEMMs take bf16 operands
  int pose_fp32 = 0;  // precision ANR_BF16 keeps the pose-space BW MLP in fp32 (ANR_BF16_ALL does not)
  const void* wimg = nullptr;          // bf16 weight images (anr_tgemm.hip), packed for this call
  const float* pt[ANR_NUM_TENSORS + ANR_NUM_NOVEL_TENSORS] = {};  // the tensors they were packed from
  float* wslab = nullptr;              // weight-gradient partial slabs (anr_tgemm.hip k_wgrad)
  int x3 = 0;  // inside the pose scope of ANR_BF16: split-bf16 (fp32-level) row GEMMs instead of fp32
  int hb = 0;  // bf16 storage of the T-pose / canonical activations (precision bf16 / bf16_all, training executor)
  SideStreams* ss = nullptr;  // NULL: every product on s
  int wnext = 0;               // round-robin weight-gradient lane
  size_t lane_floats = 0;      // partial-slab floats per weight-gradient lane
  // grouped weight gradients (ANR_WG_GROUP, default on): wgrad() queues the products of the fast path
  // and flush_w() issues them as one k_wgrad_group + one reduce on lane 0, after everything issued so
  // far to the streams they were queued from, then the latent-row updates that read their column sums.
  // Fewer sample ranges per product (nz, ANR_WG_GROUP_NZ) still fill the chip, because the products of a
  // group run side by side: less partial-slab traffic and ~4x fewer launches than one product at a time.
  int group = 0, group_nz = 16;
  // ANR_WG_FLUSH_EVERY: also flush once this many products are queued (0: at 16 and at the end only);
  // 8 measured 1.400 / 1.538 vs 1.418 / 1.559 ms on two boxes (profiles/r4u_*, r4l1_*)
  int flush_every = 8;
  WGrad pend[WG_GROUP_MAX];
  int npend = 0;
  hipStream_t pend_src[2] = {};  // streams the queued products were issued from (any handle, 0 included)
  int npsrc = 0;
  struct LatentPost {
    const float* ys;
    const float* W;
    int in_ch, c0, ncol;
    const float* tab;
    const int64_t* li;
    int add;
    float *gW, *gtab;
  } post[8];
  int npost = 0;
  int nqueued = 0;  // products queued so far
  // the kept-sample count stays on the device (no host read, so a step can be captured in a graph):
  // every launch is sized for the capacity `cap` and reads the count from n_dev
  const int* n_dev = nullptr;
  int cap = 0;
  // deterministic mode (train_det(), read once per call): one weight-gradient stream, fixed-order reductions
  int det = train_det();
  float* dscr = nullptr;  // per-split partials of the generic weight gradients (det)
  size_t dscr_floats = 0;

  int grid_n() const { return n_dev ? cap : n; }  // rows a per-sample launch covers

  hipStream_t s2() const { return ss ? ss->s2 : s; }
  // a weight-gradient lane (stream + its partial-slab region), ordered after everything issued to s
  // so far; lane < 0: the next one round robin
  int wstream(hipStream_t* w, int* lane, int want = -1) {
    const int l = det ? 0 : want >= 0 ? want : (wnext++ % (ss ? ss->lanes : 1));
    *lane = ss ? l : 0;
    *w = ss ? ss->sw[l] : s;
    return order(ss, *w, s);
  }
  float* slab(int lane) const { return wslab ? wslab + (size_t)lane * lane_floats : nullptr; }
  // issue the queued weight gradients (grouped) and the latent-row updates that follow them
  bool ys_zero = false;  // the latent column-sum scratch was zeroed for this call (one memset, train_backward)
  bool bimg = false;     // the input-gradient chain images are packed for this call (train_forward, on s2)
  int flush_w() {
    if (!npend && !npost) return ANR_OK;
    // ANR_WG_ALT_LANES=1 (read per call): consecutive groups alternate between the weight-gradient lanes
    // (each lane its own slab region; the groups' dW / bias / latent updates are atomic adds), so one
    // group's reduction and small-format launches overlap the next group's products
    const char* al = getenv("ANR_WG_ALT_LANES");
    const int fl = ss && !det && al && al[0] == '1' ? (nflush++ % ss->lanes) : 0;
    hipStream_t w = ss ? ss->sw[fl] : s;
    for (int i = 0; i < npsrc; ++i) ANR_TRY(order(ss, w, pend_src[i]));
    if (npend && launch_wgrad_group(pend, npend, grid_n(), group_nz, slab(fl), lane_floats, w, det != 0) != 0)
      return check_launch("k_wgrad_group");
    if (npost && det) {  // posts can share dW latent columns and table rows: one launch each, in post order
      for (int i = 0; i < npost; ++i) {
        const LatentPost& q = post[i];
        hipLaunchKernelGGL(k_tr_latent_grad, dim3(q.ncol + 128), dim3(128), 0, w, q.ys, q.W, q.in_ch, q.c0, q.ncol, q.tab,
                           q.li, q.add, q.gW, q.gtab);
      }
      ANR_TRY(check_launch("k_tr_latent_grad"));
    } else if (npost) {  // every latent-row update of the flush in one launch
      LatentPosts P{};
      for (int i = 0; i < npost; ++i) {
        const LatentPost& q = post[i];
        P.dysum[i] = q.ys; P.W[i] = q.W; P.in_ch[i] = q.in_ch; P.col0[i] = q.c0; P.nout[i] = q.ncol;
        P.table[i] = q.tab; P.li[i] = q.li; P.add[i] = q.add; P.dW[i] = q.gW; P.dtable[i] = q.gtab;
      }
      hipLaunchKernelGGL(k_tr_latent_grads, dim3(256 + 128, npost), dim3(128), 0, w, P);
      ANR_TRY(check_launch("k_tr_latent_grads"));
    }
    npend = npost = npsrc = 0;
    return ANR_OK;
  }
  // Queued products read their dY / X rows when the group is flushed, not when queued: an output about
  // to be written over rows a queued product still has to read flushes the queue first (the executor's
  // buffers are laid out so that this never triggers today; it keeps a later buffer reuse correct).
  static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    return a && b && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
  }
  int guard_pending(const void* out, long ld, bool obf) {
    if (!npend || !out) return ANR_OK;
    const size_t rows = (size_t)grid_n(), ob = rows * (size_t)ld * (obf ? 2 : 4);
    for (int i = 0; i < npend; ++i) {
      const WGrad& q = pend[i];
      if (overlaps(out, ob, q.dY, rows * (size_t)q.ldY * (q.ybf ? 2 : 4)) ||
          overlaps(out, ob, q.X, rows * (size_t)q.ldX * (q.xbf ? 2 : 4)))
        return flush_w();
    }
    return ANR_OK;
  }
  // zero the column-sum scratch ys (on s, ahead of the products queued after it) and update the latent
  // rows from it once the weight gradient that fills it has run: k_tr_latent_grad after that product
  int latent_rows(float* ys, float* dW, int in_ch, int c0, int Nout, const float* dY, int ldY, const float* X, int ldX,
                  int K, float* bsum, unsigned bf, const LatentPost& q) {
    hipStream_t w = s;
    int lane = 0;
    if (!group) ANR_TRY(wstream(&w, &lane, 0));
    if (!ys_zero && hipMemsetAsync(ys, 0, 256 * 4, w) != hipSuccess) return fail(ANR_E_HIP, "memset");
    if (group && (npend == WG_GROUP_MAX || npost == 8)) ANR_TRY(flush_w());  // product and update in one flush
    const int q0 = nqueued;
    ANR_TRY(wgrad(dW, in_ch, c0, Nout, dY, ldY, X, ldX, K, bsum, ys, 0, bf));
    if (nqueued > q0) {
      post[npost++] = q;
      return ANR_OK;
    }
    if (group) ANR_TRY(wstream(&w, &lane, 0));  // off the fast path: the product ran on lane 0
    hipLaunchKernelGGL(k_tr_latent_grad, dim3(256 + 128), dim3(128), 0, w, q.ys, q.W, q.in_ch, q.c0, q.ncol, q.tab, q.li,
                       q.add, q.gW, q.gtab);
    return check_launch("k_tr_latent_grad");
  }
  // lane 0 waits for the other lanes (every weight gradient issued so far is done when lane 0 is)
  int gather_w() {
    ANR_TRY(flush_w());
    if (!ss) return ANR_OK;
    for (int l = 1; l < ss->lanes; ++l) ANR_TRY(order(ss, ss->sw[0], ss->sw[l]));
    return ANR_OK;
  }
  // s waits for every weight-gradient lane (end of a backward)
  int join_w() {
    ANR_TRY(flush_w());
    if (!ss) return ANR_OK;
    for (int l = 0; l < ss->lanes; ++l) ANR_TRY(order(ss, s, ss->sw[l]));
    return ANR_OK;
  }

  // the bf16 row GEMM when every operand fits it (anr_train.h RGemm); false: use the generic kernel
  bool row_seg(RGemmSeg& q, const float* A, long lda, int K, const float* W, int c0, bool bwd, bool abf = false) {
    if (!A || K <= 0 || lda % (abf ? 8 : 4) != 0 || ((uintptr_t)A & 15) != 0 || lda < (long)((K + 63) / 64 * 64))
      return false;
    WView v;
    if (!wimg_view(wimg, pt, W, c0, K, bwd, &v)) return false;
    q = RGemmSeg{A, lda, K, v.B, v.ldb, v.bcol, v.rows, v.lo_off};
    return true;
  }
  int rgemm(RGemm& g) {
    if (grid_n() <= 0 || g.N <= 0) return ANR_OK;
    g.M = n;
    g.M_dev = n_dev;
    launch_rgemm(g, grid_n(), s);
    return check_launch("k_rgemm");
  }

  int gemm(GemmArgs g, int M, hipStream_t st) {
    if (M <= 0 || g.N <= 0) return ANR_OK;
    if (g.ksplit < 1) g.ksplit = 1;
    dim3 grid((g.N + 63) / 64, (M + 63) / 64, g.ksplit);
    g.M = M;
    g.bf16 = bf16;
    launch_gemm(g, grid, st);
    return check_launch("k_gemm");
  }
  // a GEMM whose rows are the kept samples
  int gemm_rows(GemmArgs g) {
    g.M_dev = n_dev;
    return gemm(g, grid_n(), s);
  }

  // Y[n][Nout] = act( X0[:, :K0] W[:, c0:c0+K0]^T (+ X1 W[:, c1:c1+K1]^T) + bias )
  // bf: BF_A (X0 / X1 bf16), BF_C (Y bf16)
  int fwd(float* Y, int ldY, int Nout, const float* W, int in_ch, const float* bias, bool relu, const float* X0, int ld0,
          int K0, int c0, const float* X1 = nullptr, int ld1 = 0, int K1 = 0, int c1 = 0, unsigned bf = 0) {
    const bool abf = bf & BF_A;
    ANR_TRY(guard_pending(Y, ldY, bf & BF_C));
    if ((bf16 || x3) && wimg && Nout <= 256 && !(x3 && bf)) {
      RGemm r{};
      r.x3 = bf16 ? 0 : 1;
      r.N = Nout;
      r.nseg = X1 ? 2 : 1;
      if (row_seg(r.seg[0], X0, ld0, K0, W, c0, false, abf) && (!X1 || row_seg(r.seg[1], X1, ld1, K1, W, c1, false, abf))) {
        r.C = Y; r.ldc = ldY; r.bias = bias; r.relu = relu ? 1 : 0;
        r.abf = abf; r.cbf = (bf & BF_C) != 0;
        return rgemm(r);
      }
    }
    if (bf) return fail(ANR_E_ARG, "train: bf16-stored operand off the row-GEMM path");
    GemmArgs g{};
    g.N = Nout;
    g.nseg = X1 ? 2 : 1;
    g.seg[0] = GemmSeg{X0, ld0, 1, W + c0, 1, in_ch, K0};
    if (X1) g.seg[1] = GemmSeg{X1, ld1, 1, W + c1, 1, in_ch, K1};
    g.C = Y; g.ldc = ldY; g.bias = bias; g.relu = relu ? 1 : 0; g.ksplit = 1;
    return gemm_rows(g);
  }

  // dW[:, c0:c0+K] += dY^T X (split-K over samples, atomics); the column sums of dY (the bias
  // gradient) are added into bsum (and bsum2) in the same pass when given
  // bf: BF_A (dY bf16), BF_X (X bf16)
  int wgrad(float* dW, int in_ch, int c0, int Nout, const float* dY, int ldY, const float* X, int ldX, int K,
            float* bsum = nullptr, float* bsum2 = nullptr, int want_lane = -1, unsigned bf = 0) {
    if (grid_n() <= 0) return ANR_OK;
    const bool fast = (bf16 || x3) && wslab && Nout <= 256 && K <= 256 && ldY % 4 == 0 && ldX % 4 == 0 &&
                      ((uintptr_t)dY & 15) == 0 && ((uintptr_t)X & 15) == 0 && !(x3 && bf);
    WGrad wg{};
    if (fast) {
      wg.x3 = bf16 ? 0 : 1;
      wg.ybf = (bf & BF_A) != 0;
      wg.xbf = (bf & BF_X) != 0;
      wg.dY = dY; wg.ldY = ldY; wg.nout = Nout; wg.X = X; wg.ldX = ldX; wg.K = K;
      wg.dW = dW + c0; wg.ldw = in_ch; wg.bsum = bsum; wg.bsum2 = bsum2;
      wg.M_dev = n_dev;
    }
    if (fast && group) {
      if (npend == WG_GROUP_MAX || (flush_every > 0 && npend >= flush_every)) ANR_TRY(flush_w());
      if (!(npsrc > 0 && pend_src[0] == s) && !(npsrc > 1 && pend_src[1] == s)) {
        if (npsrc == 2) ANR_TRY(flush_w());
        pend_src[npsrc++] = s;
      }
      pend[npend++] = wg;
      ++nqueued;
      return ANR_OK;
    }
    hipStream_t w;
    int lane;
    ANR_TRY(wstream(&w, &lane, want_lane));
    if (fast) {
      wg.slab = slab(lane);
      if (launch_wgrad(wg, grid_n(), w, det != 0) != 0) return check_launch("k_wgrad");
      return ANR_OK;
    }
    if (bf) return fail(ANR_E_ARG, "train: bf16-stored operand off the weight-gradient path");
    GemmArgs g{};
    g.rowsum = bsum;
    g.rowsum2 = bsum2;
    g.N = K;
    g.nseg = 1;
    g.seg[0] = GemmSeg{dY, 1, ldY, X, ldX, 1, grid_n()};
    g.K_dev = n_dev;
    g.C = dW + c0; g.ldc = in_ch; g.atomic = 1;
    g.ksplit = (grid_n() + 511) / 512;  // 512 samples per split (measured: 1024 / 512 / 256 / 2048)
    g.kper = 512;
    if (det) {  // the splits' partials to scratch, added in split order (no atomics)
      g.bf16 = bf16;
      if (launch_gemm_det(g, Nout, dscr, dscr_floats, w) != 0)
        return fail(ANR_E_WORKSPACE, "train: deterministic weight gradient without scratch");
      return check_launch("k_gemm (deterministic split-K)");
    }
    return gemm(g, Nout, w);
  }

  // dX (+)= dY W[:, c0:c0+K] (masked by mask > 0)
  // bf: BF_A (dY / dY2 bf16), BF_C (dX bf16), BF_M (mask bf16)
  int xgrad(float* dX, int ldX, int K, const float* dY, int ldY, int Nout, const float* W, int in_ch, int c0,
            const float* mask, int ldm, bool accumulate, const float* dY2 = nullptr, int ldY2 = 0, int Nout2 = 0,
            const float* W2 = nullptr, int in_ch2 = 0, unsigned bf = 0) {
    const bool abf = bf & BF_A;
    ANR_TRY(guard_pending(dX, ldX, bf & BF_C));
    if ((bf16 || x3) && wimg && K <= 256 && !(x3 && bf) && !((bf & BF_C) && accumulate)) {
      RGemm r{};
      r.x3 = bf16 ? 0 : 1;
      r.N = K;
      r.nseg = dY2 ? 2 : 1;
      if (row_seg(r.seg[0], dY, ldY, Nout, W, c0, true, abf) &&
          (!dY2 || row_seg(r.seg[1], dY2, ldY2, Nout2, W2, c0, true, abf)) && r.seg[0].rows >= K &&
          (!dY2 || r.seg[1].rows >= K)) {
        r.C = dX; r.ldc = ldX; r.mask = mask; r.ldm = ldm; r.accumulate = accumulate ? 1 : 0;
        r.abf = abf; r.cbf = (bf & BF_C) != 0; r.mbf = (bf & BF_M) != 0;
        return rgemm(r);
      }
    }
    if (bf) return fail(ANR_E_ARG, "train: bf16-stored operand off the row-GEMM path");
    GemmArgs g{};
    g.N = K;
    g.nseg = dY2 ? 2 : 1;
    g.seg[0] = GemmSeg{dY, ldY, 1, W + c0, in_ch, 1, Nout};
    if (dY2) g.seg[1] = GemmSeg{dY2, ldY2, 1, W2 + c0, in_ch2, 1, Nout2};
    g.C = dX; g.ldc = ldX; g.mask = mask; g.ldm = ldm; g.accumulate = accumulate ? 1 : 0; g.ksplit = 1;
    return gemm_rows(g);
  }
  // the fused step's loss sums and latent column-sum scratch, zeroed by the forward's k_tr_point_prep
  // (prezeroed once it is launched) instead of by memsets
  float* pz4 = nullptr;
  float* pz2048 = nullptr;
  bool prezeroed = false;
  int nflush = 0;  // weight-gradient groups flushed so far (ANR_WG_ALT_LANES)
};

// the pose-space BW MLP under precision ANR_BF16 runs exact fp32 (its output moves the canonical
// point that the 2^9-frequency encoding amplifies); restores the executor's mode on scope exit
struct PoseScope {
  Exec& e;
  int keep, keep_hb;
  explicit PoseScope(Exec& x) : e(x), keep(x.bf16), keep_hb(x.hb) {
    // ANR_BF16: fp32-level split products on fp32 rows; ANR_BF16_ALL: bf16 products on bf16 rows (gamma(x)
    // included, TrainBufs.hbp), as the rest of the network
    if (e.pose_fp32) {
      e.hb = 0;
      e.bf16 = 0;
      e.x3 = 1;
    }
  }
  ~PoseScope() {
    e.bf16 = keep;
    e.hb = keep_hb;
    e.x3 = 0;
  }
};

// issue the enclosed products on another stream of the executor (restored on scope exit)
struct OnStream {
  Exec& e;
  hipStream_t keep;
  OnStream(Exec& x, hipStream_t t) : e(x), keep(x.s) { e.s = t; }
  ~OnStream() { e.s = keep; }
};

// bf16 weight images for the row GEMM (bf16 policies only; refreshed on every call, the weights may
// have changed since the last)
int pack_images(Exec& e, const anr_params* p, char* dst, hipStream_t s, float* wslab, size_t lane_floats,
                bool novel = false, bool rows = true) {
  if (!e.bf16) return ANR_OK;
  e.wslab = wslab;
  e.lane_floats = lane_floats;
  const char* gv = getenv("ANR_WG_GROUP");
  e.group = !(gv && gv[0] == '0');
  const char* nz = getenv("ANR_WG_GROUP_NZ");
  if (nz && atoi(nz) > 0) e.group_nz = atoi(nz);
  const char* fe = getenv("ANR_WG_FLUSH_EVERY");
  if (fe) e.flush_every = atoi(fe);
  for (int i = 0; i < ANR_NUM_TENSORS; ++i) e.pt[i] = p->t[i];
  for (int i = 0; i < ANR_NUM_NOVEL_TENSORS; ++i) e.pt[ANR_NUM_TENSORS + i] = novel ? p->novel[i] : nullptr;
  if (!rows) return ANR_OK;  // every product of the call runs in a fused chain or a weight gradient
  if (wimg_pack(e.pt, dst, s) != 0) return check_launch("k_wimg_pack");
  e.wimg = dst;
  return ANR_OK;
}

// the executor of one call: precision policy from the options, scratch from the workspace layout T (a
// TLayout or an ALayout); built in place (Exec holds the queued weight gradients, it is never copied)
template <class LayoutT>
void init_exec(Exec& e, const anr_render_opts& o, hipStream_t s, SideStreams* ss, char* ws, const LayoutT& T) {
  e.s = s;
  e.bf16 = (o.precision == ANR_BF16 || o.precision == ANR_BF16_ALL) ? 1 : 0;
  e.pose_fp32 = o.precision == ANR_BF16 ? 1 : 0;
  e.ss = ss;
  e.hb = e.bf16;
  e.dscr = (float*)(ws + T.dscr);
  e.dscr_floats = T.dscr_floats;
}

// What one call of a training entry point is about, after its argument checks (train_call below): rays
// (x NULL) or free samples (x; Network.forward: R groups of 64 samples as one reference chunk, no
// t_rand, ray pointers NULL), the options in effect, the workspace and its layout.
struct TrainCall {
  const anr_params* p;
  const anr_frame* f;
  const float *ray_o, *ray_d, *near_, *far_;
  const anr_samples* x;
  int R;
  anr_render_opts o;
  char* ws;
  TLayout T;
};

TrainBufs bufs(const TrainCall& c) {
  const anr_frame* f = c.f;
  const TLayout& T = c.T;
  char* ws = c.ws;
  TrainBufs b{};
  if (c.x) {
    b.wpts = c.x->wpts; b.vdir = c.x->viewdir; b.dists = c.x->dists; b.n_pts = c.x->n_pts;
  }
  const Layout& L = T.L;
  b.list = (const int*)(ws + L.list);
  b.n_kept = (const int*)(ws + L.counts);
  b.m_rows = (const int*)(ws + L.counts) + 1;
  b.out_row = (const int*)(ws + L.out_row);
  b.ray_o = c.ray_o; b.ray_d = c.ray_d; b.near_ = c.near_; b.far_ = c.far_; b.t_rand = c.o.t_rand;
  b.R = f->R; b.Th = f->Th; b.A = f->A;
  b.pbw = f->pbw; b.pbounds = f->pbounds; b.tbw = f->tbw; b.tbounds = f->tbounds;
  b.pX = f->pbw_dims[0]; b.pY = f->pbw_dims[1]; b.pZ = f->pbw_dims[2];
  b.tX = f->tbw_dims[0]; b.tY = f->tbw_dims[1]; b.tZ = f->tbw_dims[2];
  b.pt = (float*)(ws + T.pt); b.Gp = (float*)(ws + T.Gp); b.Ip = (float*)(ws + T.Ip); b.Gv = (float*)(ws + T.Gv);
  b.Lp = (float*)(ws + T.Lp); b.Bp = (float*)(ws + L.pbw_rows); b.lbs = (float*)(ws + T.lbs);
  b.Gt = (float*)(ws + T.Gt); b.It = (float*)(ws + T.It); b.Lt = (float*)(ws + T.Lt); b.Bt = (float*)(ws + L.tbw_rows);
  b.Rgbl = (float*)(ws + T.Rgbl); b.Alpha = (float*)(ws + T.Alpha); b.sigma = (float*)(ws + L.sigma);
  b.raw = (float4*)(ws + L.raw);
  b.draw = (float4*)(ws + T.draw); b.dRgb = (float*)(ws + T.dRgb); b.dAlpha = (float*)(ws + T.dAlpha);
  b.dAlpha16 = (unsigned short*)(ws + T.dA16);
  b.dBp = (float*)(ws + T.dBp); b.dBt = (float*)(ws + T.dBt); b.dLp = (float*)(ws + T.dLp);
  b.dLt = (float*)(ws + T.dLt); b.dIt = (float*)(ws + T.dIt); b.dGt = (float*)(ws + T.dGt);
  b.ldl = 64;
  b.n_rays = c.R;
  return b;
}

#define PT(i) (p->t[i])
#define FOLD(k) ((const float*)(ws + T.L.fold) + 256 * (k))

// BW MLP forward over n samples (tpose_nerf_network.py:55-77); H = 8 x [N][256], logits [N][32].
// W = the 19 tensors of one blend-weight field in state_dict order: [bw_latent, bw_linears.{0..7}
// .{weight,bias}, bw_fc.{weight,bias}] (p->t + 27, or p->novel for novel_pose_bw).
int bw_forward(Exec& e, const float* const* W, const float* G, float* H, float* logits, long N, const float* fold0,
               const float* fold5) {
  const long S = N * 256;
  const unsigned h = e.hb ? (BF_A | BF_C) : 0, a = e.hb ? BF_A : 0;  // gamma and H bf16 under e.hb
  ANR_TRY(e.fwd(H, 256, 256, W[1], 191, fold0, true, G, 64, 63, 0, nullptr, 0, 0, 0, h));
  for (int l = 1; l < 8; ++l) {
    const float* Xp = H + (l - 1) * S;
    if (l == 5) {
      ANR_TRY(e.fwd(H + l * S, 256, 256, W[11], 447, fold5, true, G, 64, 63, 0, Xp, 256, 256, 191, h));
    } else {
      ANR_TRY(e.fwd(H + l * S, 256, 256, W[1 + 2 * l], 256, W[2 + 2 * l], true, Xp, 256, 256, 0, nullptr, 0, 0, 0, h));
    }
  }
  return e.fwd(logits, 32, 24, W[17], 256, W[18], false, H + 7 * S, 256, 256, 0, nullptr, 0, 0, 0, a);
}

// BW MLP backward from d logits; accumulates weight/bias grads into g (same table order as W; NULL:
// input gradient only, a frozen field); dG (+)= input-gamma gradient if given (dG_fresh: the first
// contribution overwrites). Layer l's output gradient goes to dY0 + l * dstride (dstride 0: ping-pong
// between dY0 and dY1, only when no weight gradient runs on a side stream). ysum: 2 x 256 scratch for
// the latent-column gradients of layers 0 and 5. Issued one layer per step() on stream st, so that two
// chains on two streams can be issued alternately: the host spends ~4 API calls per layer and would
// otherwise reach the second chain only after the first one's whole issue (profiles/r3l trace).
struct BwBackward {
  Exec& e;
  hipStream_t st;
  const float* const* W;
  float* const* g;
  const float *G, *H, *dlog;
  float *dY0, *dY1;
  long dstride;
  float* dG;
  bool dG_fresh;
  long N;
  float* ysum;
  const int64_t* li;
  int add;
  int ldlog = 32;  // row stride of dlog
  // the input-gradient chain's image (program 2, packed from W), or NULL: one row GEMM per layer. With
  // the chain, the first step issues every layer's output gradient (and dG) in one launch and the steps
  // issue the weight gradients only.
  const unsigned char* cimg = nullptr;
  unsigned char* bits = nullptr;  // the forward chain's mask bits of H_0..7 (bits_stride apart)
  int l = 8;  // 8: the bw_fc head, then layers 7..0; -1: done

  bool chained = false;
  bool done() const { return l < 0; }
  float* dbuf(int k) const { return dstride ? dY0 + k * dstride : ((k & 1) ? dY0 : dY1); }
  // the chain's launch ahead of the steps (which then queue weight gradients only)
  int start() {
    if (!cimg || chained) return ANR_OK;
    OnStream on(e, st);
    ANR_TRY(chain());
    chained = true;
    return ANR_OK;
  }
  int step() {
    OnStream on(e, st);
    const long S = N * 256;
    const unsigned hb = e.hb ? ~0u : 0u;  // flag mask: the hidden rows, their gradients and gamma bf16
    const bool xg = !cimg;
    if (l == 8) {
      if (cimg && !chained) {
        ANR_TRY(chain());
        chained = true;
      }
      if (g) ANR_TRY(e.wgrad(g[17], 256, 0, 24, dlog, ldlog, H + 7 * S, 256, 256, g[18], nullptr, -1, hb & BF_X));
      if (xg)
        ANR_TRY(e.xgrad(dbuf(7), 256, 256, dlog, ldlog, 24, W[17], 256, 0, H + 7 * S, 256, false, nullptr, 0, 0, nullptr, 0,
                        hb & (BF_C | BF_M)));
      --l;
      return ANR_OK;
    }
    const int wi = 1 + 2 * l, bi = wi + 1;
    const int in_ch = l == 0 ? 191 : (l == 5 ? 447 : 256);
    const float* cur = dbuf(l);
    if (l == 0 || l == 5) {
      if (g) {
        float* ys = ysum + (l == 5 ? 256 : 0);
        // bias grad and the latent-row gradient's column sum, in the weight-gradient pass
        ANR_TRY(e.latent_rows(ys, g[wi], in_ch, 0, 256, cur, 256, G, 64, 63, g[bi], hb & (BF_A | BF_X),
                              Exec::LatentPost{ys, W[wi], in_ch, 63, 256, W[0], li, add, g[wi], g[0]}));
      }
      if (dG && xg)
        ANR_TRY(e.xgrad(dG, 64, 63, cur, 256, 256, W[wi], in_ch, 0, nullptr, 0, !(dG_fresh && l == 5), nullptr, 0, 0,
                        nullptr, 0, hb & BF_A));
      if (l == 5) {
        if (g) ANR_TRY(e.wgrad(g[wi], in_ch, 191, 256, cur, 256, H + 4 * S, 256, 256, nullptr, nullptr, -1, hb & (BF_A | BF_X)));
        if (xg)
          ANR_TRY(e.xgrad(dbuf(4), 256, 256, cur, 256, 256, W[wi], in_ch, 191, H + 4 * S, 256, false, nullptr, 0, 0, nullptr,
                          0, hb & (BF_A | BF_C | BF_M)));
      }
    } else {
      if (g)
        ANR_TRY(e.wgrad(g[wi], 256, 0, 256, cur, 256, H + (l - 1) * S, 256, 256, g[bi], nullptr, -1, hb & (BF_A | BF_X)));
      if (xg)
        ANR_TRY(e.xgrad(dbuf(l - 1), 256, 256, cur, 256, 256, W[wi], 256, 0, H + (l - 1) * S, 256, false, nullptr, 0, 0,
                        nullptr, 0, hb & (BF_A | BF_C | BF_M)));
    }
    --l;
    // ping-pong gradient rows are overwritten two layers on: their queued products run now
    if (!dstride) ANR_TRY(e.flush_w());
    return ANR_OK;
  }
  // program 2 over the kept samples: d logits (fp32, ldlog) -> dY0 + l dstride (bf16 rows, masked by H)
  // and dG (fp32, ld 64: layer 5 stores unless accumulating, layer 0 adds)
  int chain() {
    if (!dstride || !e.hb || !bits) return fail(ANR_E_ARG, "train: the BW input-gradient chain needs strided bf16 rows");
    TcArgs a{};
    a.img = cimg;
    for (int i = 0; i < 8; ++i) {  // program layer i = bw layer 8 - i, output d H_{7-i} masked by H_{7-i} > 0
      a.out[i] = dbuf(7 - i);
      a.ldo[i] = 256;
      a.nout[i] = 256;
      a.bits[i] = bits + (7 - i) * bits_stride(N);
    }
    a.mem = (const unsigned short*)dlog; a.ld_mem = ldlog; a.kmem_cols = 24; a.mem_f32 = 1;
    a.aux = dG; a.ld_aux = 64; a.aux_cols = 63; a.aux_acc = dG_fresh ? 0 : 1;
    a.M_dev = e.n_dev;
    ANR_TRY(e.guard_pending(dY0, 16 * dstride / N, true));  // the 8 gradient slots (dstride floats each)
    ANR_TRY(e.guard_pending(dG, 64, false));
    if (tchain_run(2, a, e.grid_n(), num_cus(), st) != 0) return check_launch("k_tchain_bwb");
    return ANR_OK;
  }
};

int bw_backward(Exec& e, const float* const* W, float* const* g, const float* G, const float* H, const float* dlog,
                float* dY0, float* dY1, long dstride, float* dG, bool dG_fresh, long N, float* ysum, const int64_t* li,
                int add, int ldlog = 32, const unsigned char* cimg = nullptr, unsigned char* bits = nullptr) {
  BwBackward b{e, e.s, W, g, G, H, dlog, dY0, dY1, dstride, dG, dG_fresh, N, ysum, li, add, ldlog, cimg, bits};
  while (!b.done()) ANR_TRY(b.step());
  return ANR_OK;
}

// ---- fused forward chains (anr_tchain.hip) for the bf16 storage policies -------------------------
// ANR_TRAIN_FCHAIN (read per call, default 1): each MLP of the training forward as one launch with its
// activations in registers (the pose-space BW MLP too under bf16_all); 0 = one row-GEMM launch per layer
bool fchain_on() {
  const char* v = getenv("ANR_TRAIN_FCHAIN");
  return !(v && v[0] == '0');
}
// ANR_TRAIN_BCHAIN (read per call, default 1): the input gradients of each MLP's backward as one launch
// (programs 2 / 3); the weight gradients stay grouped products (Exec::wgrad). 0 = one row GEMM per layer
bool bchain_on() {
  const char* v = getenv("ANR_TRAIN_BCHAIN");
  return fchain_on() && !(v && v[0] == '0');  // reads the mask bits the forward chains write
}
// Which forward last filled a workspace's ReLU mask bits: only the forward chains write them,
// so the input-gradient chains may run only after a chained forward into the same workspace. The
// split API (anr_train_fwd / anr_train_bwd, anr_network_train_fwd / _bwd) reads the switches per call,
// so a forward with ANR_TRAIN_FCHAIN=0 followed by a default backward would otherwise mask with stale
// bits; such a backward takes the layer-wise input gradients (they read the H rows both forwards write).
struct ChainBits {
  std::mutex mu;
  std::vector<std::pair<const void*, bool>> ws;  // (workspace, written by the forward chains)
};
ChainBits& chain_bits_reg() {
  static ChainBits r;
  return r;
}
void note_chain_bits(const void* ws, bool chained) {
  ChainBits& r = chain_bits_reg();
  std::lock_guard<std::mutex> lk(r.mu);
  for (auto& w : r.ws)
    if (w.first == ws) {
      w.second = chained;
      return;
    }
  if (r.ws.size() >= 64) r.ws.erase(r.ws.begin());  // oldest first
  r.ws.emplace_back(ws, chained);
}
bool chain_bits_valid(const void* ws) {
  ChainBits& r = chain_bits_reg();
  std::lock_guard<std::mutex> lk(r.mu);
  for (const auto& w : r.ws)
    if (w.first == ws) return w.second;
  return false;
}
// every product of a call (forward / backward) runs in a fused chain or a weight gradient: the
// row-GEMM images (k_wimg_pack, 33 us a step) are not needed
bool chains_cover(const Exec& e, bool fwd, bool bwd) {
  return e.hb && !e.pose_fp32 && (!fwd || fchain_on()) && (!bwd || bchain_on());
}
// program k's image in the workspace's chain region
unsigned char* tc_img(unsigned char* base, int prog) {
  for (int k = 0; k < prog; ++k) base += tchain_image_bytes(k);
  return base;
}
// pack the BW (program 0) and NeRF (program 1) images from this call's weights
int chain_pack(const anr_params* p, unsigned char* img, hipStream_t s) {
  const float* const* W = p->t + 27;  // the blend-weight field: [bw_latent, bw_linears.{0..7}.{w,b}, bw_fc.{w,b}]
  TcPackArgs bw{};
  const int bw_in[9] = {191, 256, 256, 256, 256, 447, 256, 256, 256};
  for (int l = 0; l < 9; ++l) {
    TcPackLayer& L = bw.L[l];
    L.W = W[1 + 2 * l];
    L.in_ch = bw_in[l];
    L.n1 = l == 8 ? 24 : 256;
    L.cmem = 0; L.kmem_cols = 63;
    L.cprev = l == 5 ? 191 : 0; L.kprev_cols = 256;
  }
  if (tchain_pack(0, bw, img, s) != 0) return check_launch("k_tc_pack (bw)");
  TcPackArgs nf{};
  const int nf_in[8] = {63, 256, 256, 256, 256, 319, 256, 256};
  for (int l = 0; l < 8; ++l) {
    TcPackLayer& L = nf.L[l];
    L.W = p->t[1 + 2 * l];
    L.in_ch = nf_in[l];
    L.n1 = 256;
    L.cmem = 0; L.kmem_cols = 63;
    L.cprev = l == 5 ? 63 : 0; L.kprev_cols = 256;
  }
  nf.L[8] = TcPackLayer{p->t[19], 256, 256, p->t[17], 256, 1, 0, 0, 0, 256};   // feature_fc || alpha_fc
  nf.L[9] = TcPackLayer{p->t[21], 384, 256, nullptr, 0, 0, 0, 0, 0, 256};      // latent_fc (latent folded)
  nf.L[10] = TcPackLayer{p->t[23], 283, 128, nullptr, 0, 0, 256, 27, 0, 256};  // view_fc [latent, gamma(dir)]
  nf.L[11] = TcPackLayer{p->t[25], 128, 3, nullptr, 0, 0, 0, 0, 0, 128};       // rgb_fc
  if (tchain_pack(1, nf, tc_img(img, 1), s) != 0) return check_launch("k_tc_pack (nerf)");
  return ANR_OK;
}
// pack the input-gradient images (programs 2, 3): transposed layers, output neuron m = a forward input
// column (oc0 + m; at the skip layer 5 the gamma columns follow as out-blocks 16..19)
int chain_pack_bwd(const anr_params* p, unsigned char* img, hipStream_t s) {
  const float* const* W = p->t + 27;
  const int bw_in[9] = {191, 256, 256, 256, 256, 447, 256, 256, 256};
  TcPackArgs bw{};
  bw.L[0].W = W[17]; bw.L[0].in_ch = 256; bw.L[0].W2 = W[17]; bw.L[0].in_ch2 = 256;  // bw_fc^T: d logits (24)
  bw.L[0].kmem_cols = 24; bw.L[0].oa = 256;
  for (int i = 1; i < 9; ++i) {
    const int l = 8 - i;
    TcPackLayer& L = bw.L[i];
    L.W = W[1 + 2 * l]; L.in_ch = bw_in[l]; L.kprev_cols = 256;
    if (l == 5) { L.oc0 = 191; L.oa = 256; L.oc1 = 0; L.nb = 63; L.ob_b0 = 256; }
    else L.oa = l == 0 ? 63 : 256;
  }
  if (tchain_pack(2, bw, tc_img(img, 2), s) != 0) return check_launch("k_tc_pack (bw backward)");
  const int nf_in[8] = {63, 256, 256, 256, 256, 319, 256, 256};
  TcPackArgs nf{};
  nf.L[0].W = PT(25); nf.L[0].in_ch = 128; nf.L[0].W2 = PT(25); nf.L[0].in_ch2 = 128;  // rgb_fc^T: d rgb (3)
  nf.L[0].kmem_cols = 3; nf.L[0].oa = 128;
  nf.L[1].W = PT(23); nf.L[1].in_ch = 283; nf.L[1].kprev_cols = 128; nf.L[1].oa = 256;  // view_fc^T -> d latent
  nf.L[2].W = PT(21); nf.L[2].in_ch = 384; nf.L[2].kprev_cols = 256; nf.L[2].oa = 256;  // latent_fc^T -> d feature
  nf.L[3].W = PT(19); nf.L[3].in_ch = 256; nf.L[3].kprev_cols = 256; nf.L[3].oa = 256;  // feature_fc^T
  nf.L[3].W2 = PT(17); nf.L[3].in_ch2 = 256; nf.L[3].kmem_cols = 1;                     // + alpha_fc^T (d alpha)
  for (int i = 4; i < 12; ++i) {
    const int l = 11 - i;
    TcPackLayer& L = nf.L[i];
    L.W = PT(1 + 2 * l); L.in_ch = nf_in[l]; L.kprev_cols = 256;
    if (l == 5) { L.oc0 = 63; L.oa = 256; L.oc1 = 0; L.nb = 63; L.ob_b0 = 256; }
    else L.oa = l == 0 ? 63 : 256;
  }
  if (tchain_pack(3, nf, tc_img(img, 3), s) != 0) return check_launch("k_tc_pack (nerf backward)");
  return ANR_OK;
}
// the pose-space BW backward's chain image, when the chain runs (bf16 rows, ANR_TRAIN_BCHAIN)
const unsigned char* pose_bchain(const Exec& e, char* ws, const TLayout& T) {
  return e.hb && bchain_on() && chain_bits_valid(ws) ? tc_img((unsigned char*)(ws + T.tcimg), 2) : nullptr;
}
unsigned char* pose_bits(char* ws, const TLayout& T) { return (unsigned char*)(ws + T.bitsP); }
// one BW MLP pass (latent folds f0 / f5) over the kept samples: gamma rows G (bf16, ld 64) -> H (bf16
// rows, layer l at H + l S floats) and the logits (fp32, ld 32)
int chain_bw(const Exec& e, const anr_params* p, const unsigned char* img, const float* G, float* H, float* logits,
             long N, const float* f0, const float* f5, hipStream_t s, unsigned char* bits) {
  const float* const* W = p->t + 27;
  TcArgs a{};
  a.img = img;
  const long S = N * 256;
  for (int l = 0; l < 9; ++l) {
    a.bias[l] = l == 0 ? f0 : l == 5 ? f5 : W[2 + 2 * l];
    a.nout[l] = l == 8 ? 24 : 256;
    a.out[l] = l == 8 ? (void*)logits : (void*)(H + l * S);
    a.ldo[l] = l == 8 ? 32 : 256;
    if (l < 8) a.bits[l] = bits + l * bits_stride(N);
  }
  a.mem = (const unsigned short*)G; a.ld_mem = 64; a.kmem_cols = 63;
  a.M_dev = e.n_dev;
  if (tchain_run(0, a, e.grid_n(), num_cus(), s) != 0) return check_launch("k_tchain_bw");
  return ANR_OK;
}

// ---- the call context of the entry points -------------------------------------------------------
// Every entry point: its argument checks, train_call (layout and workspace check: no HIP call so far),
// then side_streams() / OnMain in the entry point itself (OnMain's destructor joins back into the
// caller's stream on every return path), init_exec, pack_for.
// `who`: the public entry point, for the error message
int train_call(TrainCall& c, const char* who, const anr_params* p, const anr_frame* f, const float* ray_o,
               const float* ray_d, const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
               void* workspace, size_t ws_bytes) {
  c = TrainCall{p, f, ray_o, ray_d, near_, far_, nullptr, n_rays, *o, (char*)workspace, tlayout(n_rays, o->chunk, f)};
  if (ws_bytes < c.T.total) return fail(ANR_E_WORKSPACE, std::string(who) + ": workspace too small");
  return ANR_OK;
}
int train_call(TrainCall& c, const char* who, const anr_params* p, const anr_frame* f, const anr_samples* x,
               const anr_render_opts* o, void* workspace, size_t ws_bytes) {
  const int G = (x->n_pts + 63) / 64;
  anr_render_opts oo = *o;
  oo.chunk = G;
  oo.t_rand = nullptr;
  c = TrainCall{p, f, nullptr, nullptr, nullptr, nullptr, x, G, oo, (char*)workspace, tlayout(G, G, f)};
  if (ws_bytes < c.T.total) return fail(ANR_E_WORKSPACE, std::string(who) + ": workspace too small");
  return ANR_OK;
}

int check_grads(const char* who, float* const* grads, int n = ANR_NUM_TENSORS) {
  if (!grads) return fail(ANR_E_ARG, std::string(who) + ": NULL grads");
  for (int i = 0; i < n; ++i)
    if (!grads[i]) return fail(ANR_E_ARG, std::string(who) + ": NULL grad tensor");
  return ANR_OK;
}

// the bf16 images of this call's forward and / or backward; the row-GEMM images only where a product
// runs outside the chains (a backward alone also needs its forward's mask bits for them)
int pack_for(const TrainCall& c, Exec& e, hipStream_t s, bool fwd, bool bwd) {
  const bool covered = chains_cover(e, fwd, bwd) && (fwd || chain_bits_valid(c.ws));
  return pack_images(e, c.p, c.ws + c.T.wimg, s, (float*)(c.ws + c.T.wslab), kLaneFloats, false, !covered);
}

// pose-space BW MLP backward (latent row latent_index + 1) from the d logits of k_tr_softmax_bwd_p, then
// the caller's stream waits for every weight-gradient lane: the end of a backward
int pose_backward(const TrainCall& c, Exec& e, float* const* grads) {
  const TLayout& T = c.T;
  char* ws = c.ws;
  const long N = (long)c.R * 64;
  PoseScope ps(e);
  ANR_TRY(bw_backward(e, c.p->t + 27, grads + 27, (const float*)(ws + T.Gp), (const float*)(ws + T.Hp),
                      (const float*)(ws + T.dLp), (float*)(ws + T.dHp), nullptr, N * 256, nullptr, false, N,
                      (float*)(ws + T.ysum) + 1024, c.f->latent_index, 1, 64, pose_bchain(e, ws, T), pose_bits(ws, T)));
  return e.join_w();
}

// c.x != NULL: free samples (Network.forward, anr_network_train_fwd): R groups of 64, no compositing
int train_forward(const TrainCall& c, const anr_render_out* out, hipStream_t s, Exec& e,
                  const RaySplit* split = nullptr) {
  const anr_params* p = c.p;
  const TLayout& T = c.T;
  char* ws = c.ws;
  const int R = c.R;
  float4* raw = (float4*)(ws + T.L.raw);
  const bool fchain = e.hb && fchain_on() && R > 0;
  note_chain_bits(ws, fchain);
  unsigned char* tcimg = (unsigned char*)(ws + T.tcimg);
  hipEvent_t fwd_packed = nullptr;
  if (fchain) {
    // the chain images (and the input-gradient ones, for the backward of this step) are packed on s2,
    // beside the front-end: s2 starts after everything issued to s so far (the previous call's chains
    // read the images); s waits for the forward programs' images before its first chain (the
    // input-gradient images follow on s2, ahead of the T-pose chain there and of the forward's join)
    ANR_TRY(order(e.ss, e.s2(), s));
    ANR_TRY(chain_pack(p, tcimg, e.s2()));
    ANR_TRY(mark(e.ss, e.s2(), &fwd_packed));
    if (bchain_on()) {
      ANR_TRY(chain_pack_bwd(p, tcimg, e.s2()));
      e.bimg = true;
    }
  }
  VolCall v{};  // the render stages' view of this call
  v.p = p; v.f = c.f; v.x = c.x;
  v.ray_o = c.ray_o; v.ray_d = c.ray_d; v.near_ = c.near_; v.far_ = c.far_;
  v.R = R; v.o = c.o;
  v.ws = ws; v.L = T.L; v.raw = raw; v.s = s;
  v.split = split;
  ANR_TRY(stage_frontend(v));
  const long N = (long)R * 64;
  e.n_dev = (const int*)(ws + T.L.counts);
  e.cap = (int)N;
  const int n = e.grid_n();
  TrainBufs b = bufs(c);
  b.hb = e.hb;
  b.hbp = e.hb && !e.pose_fp32;
  const int g1 = (n + 255) / 256;
  if (n > 0) {
    b.zero4 = e.pz4;
    b.zero2048 = e.pz2048;
    hipLaunchKernelGGL(k_tr_point_prep, dim3((n + 3) / 4), dim3(256), 0, s, b);
    ANR_TRY(check_launch("k_tr_point_prep"));
    b.zero4 = b.zero2048 = nullptr;
    e.prezeroed = e.pz4 != nullptr;
  }
  // fused forward chains under the bf16 storage policies (every hidden row bf16): the T-pose BW MLP and
  // the NeRF, and the pose-space BW MLP when it is bf16 too (bf16_all)
  if (fchain) ANR_TRY(after(s, fwd_packed));  // the forward programs' images packed on s2
  // pose-space BW MLP (latent_index + 1), softmax + LBS, T-pose BW MLP (latent 0)
  if (fchain && !e.pose_fp32) {
    ANR_TRY(chain_bw(e, p, tcimg, b.Gp, (float*)(ws + T.Hp), b.Lp, N, FOLD(0), FOLD(2), s, (unsigned char*)(ws + T.bitsP)));
  } else {
    PoseScope ps(e);
    ANR_TRY(bw_forward(e, p->t + 27, b.Gp, (float*)(ws + T.Hp), b.Lp, N, FOLD(0), FOLD(2)));
  }
  if (n > 0) {
    hipLaunchKernelGGL(k_tr_softmax_lbs, dim3((g1 * 256 + 3) / 4), dim3(256), 0, s, b);
    ANR_TRY(check_launch("k_tr_softmax_lbs"));
  }
  // T-pose BW MLP on s2, beside the canonical NeRF (both read only gamma(x_T))
  const hipStream_t s2 = e.s2();
  ANR_TRY(order(e.ss, s2, s));
  {
    OnStream on(e, s2);
    if (fchain)
      ANR_TRY(chain_bw(e, p, tcimg, b.Gt, (float*)(ws + T.Ht), b.Lt, N, FOLD(1), FOLD(3), s2, (unsigned char*)(ws + T.bitsT)));
    else ANR_TRY(bw_forward(e, p->t + 27, b.Gt, (float*)(ws + T.Ht), b.Lt, N, FOLD(1), FOLD(3)));
    if (n > 0) {
      hipLaunchKernelGGL(k_tr_softmax_t, dim3(g1), dim3(256), 0, s2, b);
      ANR_TRY(check_launch("k_tr_softmax_t"));
    }
  }
  // canonical NeRF (TPoseHuman.calculate_alpha_rgb)
  float* Hn = (float*)(ws + T.Hn);
  const long S = N * 256;
  float* Feat = (float*)(ws + T.Feat);
  float* Lat = (float*)(ws + T.Lat);
  float* View = (float*)(ws + T.View);
  if (fchain) {
    TcArgs a{};
    a.img = tc_img(tcimg, 1);
    for (int l = 0; l < 8; ++l) {
      a.bias[l] = PT(2 + 2 * l);
      a.nout[l] = 256;
      a.out[l] = Hn + l * S;
      a.ldo[l] = 256;
      a.bits[l] = (unsigned char*)(ws + T.bitsN) + l * bits_stride(N);
    }
    a.bits[10] = (unsigned char*)(ws + T.bitsN) + 8 * bits_stride(N);  // view_fc (View > 0)
    a.bias[8] = PT(20); a.bias2 = PT(18); a.nout[8] = 256; a.out[8] = Feat; a.ldo[8] = 256; a.out2 = b.Alpha;
    a.bias[9] = FOLD(4); a.nout[9] = 256; a.out[9] = Lat; a.ldo[9] = 256;
    a.bias[10] = PT(24); a.nout[10] = 128; a.out[10] = View; a.ldo[10] = 128;
    a.bias[11] = PT(26); a.nout[11] = 3; a.out[11] = b.Rgbl; a.ldo[11] = 4;
    a.mem = (const unsigned short*)b.Gt; a.ld_mem = 64; a.kmem_cols = 63;
    a.mem2 = (const unsigned short*)b.Gv; a.ld_mem2 = 64; a.kmem2_cols = 27;
    a.M_dev = e.n_dev;
    if (tchain_run(1, a, e.grid_n(), num_cus(), s) != 0) return check_launch("k_tchain_nf");
  } else {
    const unsigned h = e.hb ? (BF_A | BF_C) : 0, a = e.hb ? BF_A : 0;  // gamma, H, Feat, Lat bf16 under e.hb
    ANR_TRY(e.fwd(Hn, 256, 256, PT(1), 63, PT(2), true, b.Gt, 64, 63, 0, nullptr, 0, 0, 0, h));
    for (int l = 1; l < 8; ++l) {
      if (l == 5) {
        ANR_TRY(e.fwd(Hn + l * S, 256, 256, PT(11), 319, PT(12), true, b.Gt, 64, 63, 0, Hn + 4 * S, 256, 256, 63, h));
      } else {
        ANR_TRY(e.fwd(Hn + l * S, 256, 256, PT(1 + 2 * l), 256, PT(2 + 2 * l), true, Hn + (l - 1) * S, 256, 256, 0, nullptr,
                      0, 0, 0, h));
      }
  }
  ANR_TRY(e.fwd(b.Alpha, 1, 1, PT(17), 256, PT(18), false, Hn + 7 * S, 256, 256, 0, nullptr, 0, 0, 0, a));
  ANR_TRY(e.fwd(Feat, 256, 256, PT(19), 256, PT(20), false, Hn + 7 * S, 256, 256, 0, nullptr, 0, 0, 0, h));
  ANR_TRY(e.fwd(Lat, 256, 256, PT(21), 384, FOLD(4), false, Feat, 256, 256, 0, nullptr, 0, 0, 0, h));
  const int gvld = e.hb ? 64 : 32;  // bf16 gamma(dir) rows of 64 (row-GEMM K chunk), same bytes
  ANR_TRY(e.fwd(View, 128, 128, PT(23), 283, PT(24), true, Lat, 256, 256, 0, b.Gv, gvld, 27, 256, a));
  ANR_TRY(e.fwd(b.Rgbl, 4, 3, PT(25), 128, PT(26), false, View, 128, 128, 0));
  }
  if (n > 0) {
    hipLaunchKernelGGL(k_tr_raw, dim3(g1), dim3(256), 0, s, b);
    ANR_TRY(check_launch("k_tr_raw"));
  }
  ANR_TRY(stage_alpha_ind(v));
  ANR_TRY(order(e.ss, s, s2));  // join: the tbw rows
  if (c.x) return ANR_OK;
  return stage_composite(v, R, out);
}

// c.x != NULL: free samples; the upstream gradient is d raw (x->n_pts, 4) (NULL: zero) instead of d rgb_map
int train_backward(const TrainCall& c, float* const* g, const float* d_rgb, const float* d_pbw, const float* d_tbw,
                   hipStream_t s, Exec& e, const float* d_raw = nullptr, hipEvent_t nerf_done = nullptr) {
  const anr_params* p = c.p;
  const anr_samples* x = c.x;
  const TLayout& T = c.T;
  char* ws = c.ws;
  const int R = c.R;
  const long N = (long)R * 64;
  e.n_dev = (const int*)(ws + T.L.counts);
  e.cap = (int)N;
  const int n = e.grid_n();
  const long S = N * 256;
  TrainBufs b = bufs(c);
  b.hb = e.hb;
  b.d_rgb_map = d_rgb; b.d_pbw = d_pbw; b.d_tbw = d_tbw;
  const int g1 = (n + 255) / 256;
  if (n <= 0) return ANR_OK;
  float* Ht = (float*)(ws + T.Ht);
  float* Hn = (float*)(ws + T.Hn);
  float* Feat = (float*)(ws + T.Feat);
  float* Lat = (float*)(ws + T.Lat);
  float* View = (float*)(ws + T.View);
  float* dHn = (float*)(ws + T.dHn);
  float* dFeat = (float*)(ws + T.dFeat);
  float* dLat = (float*)(ws + T.dLat);
  float* dView = (float*)(ws + T.dView);
  float* ysum = (float*)(ws + T.ysum);
  // the T-pose BW chain writes its gamma(x_T) gradient into dGt2 (s2), the NeRF's into dGt (s)
  b.dGt2 = (float*)(ws + T.dGt2);
  const bool bchain = e.hb && bchain_on() && chain_bits_valid(ws);
  unsigned char* tcimg = (unsigned char*)(ws + T.tcimg);
  if (bchain && !e.bimg) ANR_TRY(chain_pack_bwd(p, tcimg, s));
  // with the chains every weight gradient is ready at once: groups of up to 16 (no flush at 8) measured
  // 1.201 vs 1.222 ms a step (profiles/r6b_*); ANR_WG_FLUSH_EVERY still overrides
  if (bchain && !getenv("ANR_WG_FLUSH_EVERY")) e.flush_every = 0;
  if (e.group) {
    // the latent column-sum scratch of every latent_rows() of this call, zeroed once (by the fused step's
    // forward when it ran: prezeroed)
    if (!(e.prezeroed && e.pz2048 == ysum) && hipMemsetAsync(ysum, 0, 8 * 256 * 4, s) != hipSuccess)
      return fail(ANR_E_HIP, "memset");
    e.ys_zero = true;
  }
  const hipStream_t s2 = e.s2();
  ANR_TRY(order(e.ss, s2, s));
  // upstream pbw / tbw row gradients, T-pose softmax backward (s2)
  hipLaunchKernelGGL(k_tr_rows_bwd, dim3((g1 * 256 + 7) / 8), dim3(256), 0, s2, b);
  ANR_TRY(check_launch("k_tr_rows_bwd"));
  hipLaunchKernelGGL(k_tr_softmax_bwd_t, dim3((g1 * 256 + 7) / 8), dim3(256), 0, s2, b);
  ANR_TRY(check_launch("k_tr_softmax_bwd_t"));

  // compositing (or the caller's d raw) + raw activations
  if (x) {
    const hipError_t r = d_raw ? hipMemcpyAsync(b.draw, d_raw, (size_t)x->n_pts * 16, hipMemcpyDeviceToDevice, s)
                               : hipMemsetAsync(b.draw, 0, (size_t)x->n_pts * 16, s);
    if (r != hipSuccess) return fail(ANR_E_HIP, "d raw copy failed");
  } else {
    hipLaunchKernelGGL(k_tr_composite_bwd, dim3((R + 3) / 4), dim3(256), 0, s, b);
    ANR_TRY(check_launch("k_tr_composite_bwd"));
  }
  hipLaunchKernelGGL(k_tr_raw_bwd, dim3(g1), dim3(256), 0, s, b);
  ANR_TRY(check_launch("k_tr_raw_bwd"));
  // the T-pose BW backward (latent row 0) on s2, issued a layer at a time between the NeRF's layers
  BwBackward tb{e, s2, p->t + 27, g + 27, b.Gt, Ht, b.dLt, (float*)(ws + T.dHt), nullptr, S, b.dGt2, true, N, ysum,
                nullptr, 0, 64, bchain ? tc_img(tcimg, 2) : nullptr, (unsigned char*)(ws + T.bitsT)};
  // issued a layer at a time between the NeRF's layers; with the chains the first tick launches the
  // T-pose chain and the ticks queue its weight gradients between the NeRF's (groups of both MLPs:
  // flushing each MLP's products separately, on two lanes, measured 1.353 vs 1.324 ms, profiles/r5y_*)
  // ANR_WG_NERF_FIRST (read per call, chains only, default 1): the T-pose chain launches first, but its
  // weight gradients are queued after all of the NeRF's, and the NeRF's group is flushed once its chain
  // is issued, so that group waits for program 3 alone (not for the longer T-pose chain) and starts on
  // the weight-gradient lane while the T-pose chain still runs: 1.017 / 1.018 vs 1.009 / 1.006 ms a step
  // (alternating runs, one box, profiles/round6/r8r_*)
  const char* nf_env = getenv("ANR_WG_NERF_FIRST");
  const bool nerf_first = bchain && !(nf_env && nf_env[0] == '0');
  auto tick = [&]() { return nerf_first || tb.done() ? ANR_OK : tb.step(); };
  if (nerf_first) ANR_TRY(tb.start());
  ANR_TRY(tick());
  // d alpha: fp32 (ld 1), or under e.hb bf16 rows of 64 (k_tr_raw_bwd) so both products stay on the fast paths
  const float* dAl = e.hb ? (const float*)b.dAlpha16 : b.dAlpha;
  const int ldAl = e.hb ? 64 : 1;
  if (bchain) {
    // program 3: every input gradient of the canonical NeRF in one launch (d view fp32, d latent,
    // d feature, d H_7..0 bf16, d gamma(x_T) fp32); the weight gradients below read its rows
    TcArgs a{};
    a.img = tc_img(tcimg, 3);
    unsigned char* bn = (unsigned char*)(ws + T.bitsN);
    a.out[0] = dView; a.ldo[0] = 128; a.nout[0] = 128; a.bits[0] = bn + 8 * bits_stride(N);
    a.out[1] = dLat; a.ldo[1] = 256; a.nout[1] = 256;
    a.out[2] = dFeat; a.ldo[2] = 256; a.nout[2] = 256;
    for (int i = 3; i < 11; ++i) {  // feature_fc || alpha_fc, then pts_linears 7..1: d H_{10-i}
      a.out[i] = dHn + (10 - i) * S; a.ldo[i] = 256; a.nout[i] = 256;
      a.bits[i] = bn + (10 - i) * bits_stride(N);
    }
    a.mem = (const unsigned short*)b.dRgb; a.ld_mem = 4; a.kmem_cols = 3; a.mem_f32 = 1;
    a.mem2 = (const unsigned short*)dAl; a.ld_mem2 = 64; a.kmem2_cols = 1;
    a.aux = b.dGt; a.ld_aux = 64; a.aux_cols = 63;
    a.M_dev = e.n_dev;
    ANR_TRY(e.guard_pending(dHn, 16 * S / N, true));
    ANR_TRY(e.guard_pending(b.dGt, 64, false));
    if (tchain_run(3, a, e.grid_n(), num_cus(), s) != 0) return check_launch("k_tchain_nfb");
  }
  // rgb_fc, view_fc (ReLU), latent_fc (latent folded), feature_fc || alpha_fc
  ANR_TRY(e.wgrad(g[25], 128, 0, 3, b.dRgb, 4, View, 128, 128, g[26]));
  if (!bchain) ANR_TRY(e.xgrad(dView, 128, 128, b.dRgb, 4, 3, PT(25), 128, 0, View, 128, false));
  ANR_TRY(tick());
  const unsigned hb = e.hb ? ~0u : 0u;  // flag mask: gamma, H, Feat, Lat and their gradients bf16
  ANR_TRY(e.wgrad(g[23], 283, 0, 128, dView, 128, Lat, 256, 256, g[24], nullptr, -1, hb & BF_X));
  ANR_TRY(e.wgrad(g[23], 283, 256, 128, dView, 128, b.Gv, e.hb ? 64 : 32, 27, nullptr, nullptr, -1, hb & BF_X));
  if (!bchain)
    ANR_TRY(e.xgrad(dLat, 256, 256, dView, 128, 128, PT(23), 283, 0, nullptr, 0, false, nullptr, 0, 0, nullptr, 0,
                    hb & BF_C));
  {
    float* ys = ysum + 512;
    ANR_TRY(e.latent_rows(ys, g[21], 384, 0, 256, dLat, 256, Feat, 256, 256, g[22], hb & (BF_A | BF_X),
                          Exec::LatentPost{ys, PT(21), 384, 256, 256, PT(0), c.f->latent_index, 0, g[21], g[0]}));
  }
  if (!bchain)
    ANR_TRY(e.xgrad(dFeat, 256, 256, dLat, 256, 256, PT(21), 384, 0, nullptr, 0, false, nullptr, 0, 0, nullptr, 0,
                    hb & (BF_A | BF_C)));
  ANR_TRY(tick());
  ANR_TRY(e.wgrad(g[19], 256, 0, 256, dFeat, 256, Hn + 7 * S, 256, 256, g[20], nullptr, -1, hb & (BF_A | BF_X)));
  ANR_TRY(e.wgrad(g[17], 256, 0, 1, dAl, ldAl, Hn + 7 * S, 256, 256, g[18], nullptr, -1, hb & (BF_A | BF_X)));
  if (!bchain)
    ANR_TRY(e.xgrad(dHn + 7 * S, 256, 256, dFeat, 256, 256, PT(19), 256, 0, Hn + 7 * S, 256, false, dAl, ldAl, 1,
                    PT(17), 256, hb & (BF_A | BF_C | BF_M)));
  // NeRF pts_linears 7..0 (skip at 5: [gamma(x_T), net]); layer l's output gradient at dHn + l S
  for (int l = 7; l >= 0; --l) {
    const int wi = 1 + 2 * l, bi = wi + 1;
    const float* cur = dHn + l * S;
    const unsigned ax = hb & (BF_A | BF_X), acm = hb & (BF_A | BF_C | BF_M);
    if (l == 0) {
      ANR_TRY(e.wgrad(g[wi], 63, 0, 256, cur, 256, b.Gt, 64, 63, g[bi], nullptr, -1, ax));
      if (!bchain)
        ANR_TRY(e.xgrad(b.dGt, 64, 63, cur, 256, 256, PT(wi), 63, 0, nullptr, 0, true, nullptr, 0, 0, nullptr, 0, hb & BF_A));
    } else if (l == 5) {
      ANR_TRY(e.wgrad(g[wi], 319, 0, 256, cur, 256, b.Gt, 64, 63, g[bi], nullptr, -1, ax));
      ANR_TRY(e.wgrad(g[wi], 319, 63, 256, cur, 256, Hn + 4 * S, 256, 256, nullptr, nullptr, -1, ax));
      if (!bchain) {
        ANR_TRY(e.xgrad(b.dGt, 64, 63, cur, 256, 256, PT(wi), 319, 0, nullptr, 0, false, nullptr, 0, 0, nullptr, 0,
                        hb & BF_A));  // first contribution
        ANR_TRY(e.xgrad(dHn + 4 * S, 256, 256, cur, 256, 256, PT(wi), 319, 63, Hn + 4 * S, 256, false, nullptr, 0, 0,
                        nullptr, 0, acm));
      }
    } else {
      ANR_TRY(e.wgrad(g[wi], 256, 0, 256, cur, 256, Hn + (l - 1) * S, 256, 256, g[bi], nullptr, -1, ax));
      if (!bchain)
        ANR_TRY(e.xgrad(dHn + (l - 1) * S, 256, 256, cur, 256, 256, PT(wi), 256, 0, Hn + (l - 1) * S, 256, false, nullptr,
                        0, 0, nullptr, 0, acm));
    }
    ANR_TRY(tick());
  }
  if (nerf_first) ANR_TRY(e.flush_w());
  // the canonical NeRF's gradients (tensors 0..26) are final once the weight-gradient stream has
  // run what is issued so far: a caller may start reducing them while the blend-weight backward
  // below runs (bucketed all-reduce, anr_train_hooks)
  if (nerf_done) {
    hipStream_t w;
    int lane;
    ANR_TRY(e.gather_w());
    ANR_TRY(e.wstream(&w, &lane, 0));
    if (hipEventRecord(nerf_done, w) != hipSuccess) return fail(ANR_E_HIP, "hipEventRecord failed");
  }
  while (!tb.done()) ANR_TRY(tb.step());
  ANR_TRY(order(e.ss, s, s2));  // join: dGt2, dBp rows
  // x_T gradient (gamma + init_tbw lookup) -> LBS -> d pbw; pose BW backward (latent row li + 1)
  hipLaunchKernelGGL(k_tr_tpose_bwd, dim3((g1 * 256 + 3) / 4), dim3(256), 0, s, b);
  ANR_TRY(check_launch("k_tr_tpose_bwd"));
  hipLaunchKernelGGL(k_tr_softmax_bwd_p, dim3((g1 * 256 + 7) / 8), dim3(256), 0, s, b);
  ANR_TRY(check_launch("k_tr_softmax_bwd_p"));
  return ANR_OK;
}

// ---- (f) animation stage: aninerf_animation_trainer.NetworkWrapper.forward + backward ----------
struct ALayout {
  size_t counts, amax, acc, pt, Gp, Ip, Lp, Bp, lbs, Gt, It, Lt, Bt, Hp, Ht, Hn, Alpha, sel;
  size_t dBp, dBt, dLp, dLt, dIt, dGt, dA, dB, ysum, fold, wimg, wslab, lpart, dscr, dscr_floats, total;
};

ALayout alayout(long N) {
  ALayout T{};
  Carve c;
  const size_t n = (size_t)N;
  T.counts = c.bytes(16); T.amax = c.bytes(8); T.acc = c.bytes(16); T.pt = c.bytes(n * 32); T.Gp = c.bytes(n * 256);
  T.Ip = c.bytes(n * 128); T.Lp = c.bytes(n * 128); T.Bp = c.bytes(n * 96); T.lbs = c.bytes(n * 64);
  T.Gt = c.bytes(n * 256); T.It = c.bytes(n * 128); T.Lt = c.bytes(n * 128); T.Bt = c.bytes(n * 96);
  T.Hp = c.bytes(n * 256 * 8 * 4); T.Ht = c.bytes(n * 256 * 8 * 4); T.Hn = c.bytes(n * 256 * 2 * 4);
  T.Alpha = c.bytes(n * 4); T.sel = c.bytes(n * 4); T.dBp = c.bytes(n * 96); T.dBt = c.bytes(n * 96);
  T.dLp = c.bytes(n * 128); T.dLt = c.bytes(n * 128); T.dIt = c.bytes(n * 128); T.dGt = c.bytes(n * 256);
  T.dA = c.bytes(n * 1024); T.dB = c.bytes(n * 1024); T.ysum = c.bytes(8 * 256 * 4); T.fold = c.bytes(1280 * 4);
  T.wimg = c.bytes(wimg_bytes()); T.wslab = c.bytes(wgrad_slab_floats() * 4);
  T.lpart = c.bytes(loss_part_floats(N) * 4);
  T.dscr_floats = det_scratch_floats(N);
  T.dscr = c.bytes(T.dscr_floats * 4);
  T.total = c.o;
  return T;
}

TrainBufs abufs(const ALayout& T, char* ws, const anr_frame* f) {
  TrainBufs b{};
  b.n_kept = (const int*)(ws + T.counts);
  b.R = f->R; b.Th = f->Th; b.A = f->A;
  b.pbw = f->pbw; b.pbounds = f->pbounds; b.tbw = f->tbw; b.tbounds = f->tbounds;
  b.pX = f->pbw_dims[0]; b.pY = f->pbw_dims[1]; b.pZ = f->pbw_dims[2];
  b.tX = f->tbw_dims[0]; b.tY = f->tbw_dims[1]; b.tZ = f->tbw_dims[2];
  b.pt = (float*)(ws + T.pt); b.Gp = (float*)(ws + T.Gp); b.Ip = (float*)(ws + T.Ip); b.Lp = (float*)(ws + T.Lp);
  b.Bp = (float*)(ws + T.Bp); b.lbs = (float*)(ws + T.lbs); b.Gt = (float*)(ws + T.Gt); b.It = (float*)(ws + T.It);
  b.Lt = (float*)(ws + T.Lt); b.Bt = (float*)(ws + T.Bt); b.Alpha = (float*)(ws + T.Alpha);
  b.sigma = (float*)(ws + T.sel);
  b.dBp = (float*)(ws + T.dBp); b.dBt = (float*)(ws + T.dBt); b.dLp = (float*)(ws + T.dLp);
  b.dLt = (float*)(ws + T.dLt); b.dIt = (float*)(ws + T.dIt); b.dGt = (float*)(ws + T.dGt);
  return b;
}

#define AFOLD(k) ((const float*)(ws + T.fold) + 256 * (k))

// TPoseHuman.calculate_alpha (tpose_nerf_network.py:241-250) over the n points of Gt -> b.Alpha
int nerf_alpha_fwd(Exec& e, const anr_params* p, const TrainBufs& b, float* Hn, long N) {
  const long S = N * 256;
  float* cur = Hn;
  float* prv = Hn + S;
  ANR_TRY(e.fwd(cur, 256, 256, PT(1), 63, PT(2), true, b.Gt, 64, 63, 0));
  for (int l = 1; l < 8; ++l) {
    float* t = prv;
    prv = cur;
    cur = t;
    if (l == 5) ANR_TRY(e.fwd(cur, 256, 256, PT(11), 319, PT(12), true, b.Gt, 64, 63, 0, prv, 256, 256, 63));
    else ANR_TRY(e.fwd(cur, 256, 256, PT(1 + 2 * l), 256, PT(2 + 2 * l), true, prv, 256, 256, 0));
  }
  return e.fwd(b.Alpha, 1, 1, PT(17), 256, PT(18), false, cur, 256, 256, 0);
}

int anim_path(const anr_params* p, float* const* grads, const anr_frame* f, const float* pts, int n, bool obs,
              const anr_render_opts* o, char* ws, const ALayout& T, hipStream_t s, Exec& e) {
  e.n = n;
  TrainBufs b = abufs(T, ws, f);
  int* counts = (int*)(ws + T.counts);
  unsigned long long* amax = (unsigned long long*)(ws + T.amax);
  float* acc = (float*)(ws + T.acc);
  const int g1 = (n + 255) / 256, g4 = (n + 3) / 4;
  const long N = n;
  float* Hp = (float*)(ws + T.Hp);
  float* Ht = (float*)(ws + T.Ht);
  float* dA = (float*)(ws + T.dA);
  float* dB = (float*)(ws + T.dB);
  float* ysum = (float*)(ws + T.ysum);
  hipLaunchKernelGGL(k_an_set, dim3(1), dim3(1), 0, s, counts, n);
  if (hipMemsetAsync(amax, 0, 8, s) != hipSuccess) return fail(ANR_E_HIP, "memset");
  if (obs) {
    // ppts_to_tpose (aninerf_animation_trainer.py:63-99)
    hipLaunchKernelGGL(k_an_prep_obs, dim3(g4), dim3(256), 0, s, b, pts);
    {
      PoseScope ps(e);
      ANR_TRY(bw_forward(e, p->novel, b.Gp, Hp, b.Lp, N, AFOLD(0), AFOLD(2)));
    }
    hipLaunchKernelGGL(k_tr_softmax_lbs, dim3((g1 * 256 + 3) / 4), dim3(256), 0, s, b);
    ANR_TRY(bw_forward(e, p->t + 27, b.Gt, Ht, b.Lt, N, AFOLD(1), AFOLD(3)));
    hipLaunchKernelGGL(k_tr_softmax_t, dim3(g1), dim3(256), 0, s, b);
    ANR_TRY(nerf_alpha_fwd(e, p, b, (float*)(ws + T.Hn), N));
  } else {
    // tpose_to_ppts (:102-131)
    hipLaunchKernelGGL(k_an_prep_can, dim3(g4), dim3(256), 0, s, b, pts);
    ANR_TRY(bw_forward(e, p->t + 27, b.Gt, Ht, b.Lt, N, AFOLD(1), AFOLD(3)));
    hipLaunchKernelGGL(k_tr_softmax_t, dim3(g1), dim3(256), 0, s, b);
    ANR_TRY(nerf_alpha_fwd(e, p, b, (float*)(ws + T.Hn), N));
    hipLaunchKernelGGL(k_an_lbs_fwd, dim3(g1), dim3(256), 0, s, b);
    {
      PoseScope ps(e);
      ANR_TRY(bw_forward(e, p->novel, b.Gp, Hp, b.Lp, N, AFOLD(0), AFOLD(2)));
    }
    hipLaunchKernelGGL(k_an_softmax_p, dim3(g1), dim3(256), 0, s, b);
  }
  const int k = obs ? 0 : 1;
  hipLaunchKernelGGL(k_an_select, dim3(g1), dim3(256), 0, s, b, obs ? 1 : 0, o->norm_th, amax);
  if (e.det) b.loss_part = (float*)(ws + T.lpart);  // per-block partials instead of the atomic sum
  hipLaunchKernelGGL(k_an_loss, dim3(g1), dim3(256), 0, s, b, o->train_th, (const unsigned long long*)amax, acc + k,
                     counts + 1 + k);
  if (e.det) {
    DetSum d{};
    d.src[0] = b.loss_part; d.n[0] = g1; d.stride[0] = 1; d.dst[0] = acc + k;
    hipLaunchKernelGGL(k_det_sum, dim3(1), dim3(256), 0, s, d);
    b.loss_part = nullptr;
  }
  hipLaunchKernelGGL(k_an_loss_grads, dim3(g1), dim3(256), 0, s, b, (const int*)(counts + 1 + k), obs ? 1 : 0);
  ANR_TRY(check_launch("anim forward"));
  if (obs) {
    // tbw0 depends on novel_pose_bw through x_T: frozen T-pose BW MLP (input gradient only),
    // gamma + init_tbw lookup, LBS inverse -> d pbw (k_tr_tpose_bwd)
    hipLaunchKernelGGL(k_tr_softmax_bwd_t, dim3((g1 * 256 + 7) / 8), dim3(256), 0, s, b);
    if (hipMemsetAsync(b.dGt, 0, (size_t)n * 64 * 4, s) != hipSuccess) return fail(ANR_E_HIP, "memset");
    ANR_TRY(bw_backward(e, p->t + 27, nullptr, b.Gt, Ht, b.dLt, dA, dB, 0, b.dGt, false, N, ysum, nullptr, 0));
    hipLaunchKernelGGL(k_tr_tpose_bwd, dim3((g1 * 256 + 3) / 4), dim3(256), 0, s, b);
  }
  hipLaunchKernelGGL(k_tr_softmax_bwd_p, dim3((g1 * 256 + 7) / 8), dim3(256), 0, s, b);
  ANR_TRY(check_launch("anim backward"));
  PoseScope ps(e);
  return bw_backward(e, p->novel, grads, b.Gp, Hp, b.dLp, dA, dB, 0, nullptr, false, N, ysum + 512, f->bw_latent_index, 0);
}

}  // namespace

extern "C" {

int anr_train_deterministic(int on) {
  if (on == -1) return g_train_det.load(std::memory_order_relaxed);
  if (on != 0 && on != 1) return -fail(ANR_E_ARG, "anr_train_deterministic: on must be 0, 1 or -1");
  return g_train_det.exchange(on, std::memory_order_relaxed);
}

size_t anr_train_workspace_bytes(int n_rays, const anr_render_opts* o, const anr_frame* f) {
  if (!o || !f || n_rays <= 0) return 0;
  return tlayout(n_rays, o->chunk, f).total;
}

int anr_train_fwd(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d, const float* near_,
                  const float* far_, int n_rays, const anr_render_opts* o, const anr_render_out* out, void* workspace,
                  size_t ws_bytes, void* stream) {
  ANR_TRY(check_args(p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace));
  if (!out || !out->rgb_map || !out->acc_map || !out->depth_map) return fail(ANR_E_ARG, "anr_train_fwd: NULL output");
  TrainCall c;
  ANR_TRY(train_call(c, "anr_train_fwd", p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace, ws_bytes));
  OnMain om(side_streams(), (hipStream_t)stream);
  ANR_TRY(om.rc);
  Exec e{};
  init_exec(e, c.o, om.s, om.ss, c.ws, c.T);
  ANR_TRY(pack_for(c, e, om.s, true, false));
  ANR_TRY(train_forward(c, out, om.s, e));
  if (out->raw && hipMemcpyAsync(out->raw, c.ws + c.T.L.raw, (size_t)n_rays * 64 * 16, hipMemcpyDeviceToDevice,
                                 om.s) != hipSuccess)
    return fail(ANR_E_HIP, "raw copy failed");
  return ANR_OK;
}

int anr_train_bwd(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o, const float* ray_d,
                  const float* near_, const float* far_, int n_rays, const anr_render_opts* o, const float* d_rgb_map,
                  const float* d_pbw, const float* d_tbw, void* workspace, size_t ws_bytes, void* stream) {
  ANR_TRY(check_args(p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace));
  ANR_TRY(check_grads("anr_train_bwd", grads));
  TrainCall c;
  ANR_TRY(train_call(c, "anr_train_bwd", p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace, ws_bytes));
  OnMain om(side_streams(), (hipStream_t)stream);
  ANR_TRY(om.rc);
  Exec e{};
  init_exec(e, c.o, om.s, om.ss, c.ws, c.T);
  ANR_TRY(pack_for(c, e, om.s, false, true));
  ANR_TRY(train_backward(c, grads, d_rgb_map, d_pbw, d_tbw, om.s, e));
  return pose_backward(c, e, grads);
}

int anr_train_step(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o,
                   const float* ray_d, const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                   const float* rgb_gt, const uint8_t* mask_at_box, const anr_render_out* out, float* loss3,
                   void* workspace, size_t ws_bytes, void* stream) {
  return anr_train_step_hooked(p, grads, f, ray_o, ray_d, near_, far_, n_rays, o, rgb_gt, mask_at_box, out, loss3,
                               nullptr, workspace, ws_bytes, stream);
}

}  // extern "C"

namespace {

// one training step, issued to s (eagerly, or into a graph capture whose origin is s)
int train_step_body(const TrainCall& c, float* const* grads, const float* rgb_gt, const uint8_t* mask_at_box,
                    const anr_render_out* out, float* loss3, hipEvent_t nerf_done, hipStream_t s, SideStreams* ss,
                    const RaySplit* split = nullptr) {
  const TLayout& T = c.T;
  char* ws = c.ws;
  const int n_rays = c.R;
  Exec e{};
  init_exec(e, c.o, s, ss, ws, T);
  ANR_TRY(pack_for(c, e, s, true, true));
  float* acc3 = (float*)(ws + T.acc3);
  e.pz4 = acc3;
  e.pz2048 = (float*)(ws + T.ysum);
  ANR_TRY(train_forward(c, out, s, e, split));
  // fused losses (tpose_trainer.py:50-63) and their upstream gradients
  TrainBufs b = bufs(c);
  b.rgb_map = out->rgb_map;
  if (!e.prezeroed && hipMemsetAsync(acc3, 0, 16, s) != hipSuccess) return fail(ANR_E_HIP, "memset");
  const long N = (long)n_rays * 64;
  const int gx = (int)((std::max<long>(n_rays, N) + 255) / 256);
  if (e.det) b.loss_part = (float*)(ws + T.lpart);  // per-block partials instead of the atomic sums
  hipLaunchKernelGGL(k_tr_loss, dim3(gx, 2), dim3(256), 0, s, b, rgb_gt, mask_at_box, acc3);
  ANR_TRY(check_launch("k_tr_loss"));
  if (e.det) {  // the partials in block order into the (zeroed) sums: squared error, mask rays, smooth-L1
    DetSum d{};
    for (int q = 0; q < 3; ++q) {
      d.src[q] = b.loss_part + (q == 2 ? 2 * (long)gx : q);
      d.n[q] = gx;
      d.stride[q] = 2;
      d.dst[q] = acc3 + q;
    }
    hipLaunchKernelGGL(k_det_sum, dim3(3), dim3(256), 0, s, d);
    ANR_TRY(check_launch("k_det_sum"));
    b.loss_part = nullptr;
  }
  if (split) ANR_TRY(split->run(acc3, 4, ANR_REDUCE_SUM_F32, s));  // the batch's loss sums and row count
  b.loss3_out = loss3;  // the loss values (loss_final) from k_tr_loss_grads' first thread
  float* d_rgb = (float*)(ws + T.d_rgb);
  float* d_pbw = (float*)(ws + T.d_pbw);
  float* d_tbw = (float*)(ws + T.d_tbw);
  hipLaunchKernelGGL(k_tr_loss_grads, dim3(gx, 2), dim3(256), 0, s, b, rgb_gt, mask_at_box, (const float*)acc3, d_rgb,
                     d_pbw, d_tbw);
  ANR_TRY(check_launch("k_tr_loss_grads"));
  ANR_TRY(train_backward(c, grads, d_rgb, d_pbw, d_tbw, s, e, nullptr, nerf_done));
  return pose_backward(c, e, grads);
}

// ---- step graphs ----------------------------------------------------------------------------------
// A step issues ~175 launches and ~60 cross-stream event waits. Issued one by one, the host falls
// behind the GPU: the T-pose chain and the weight-gradient lanes start hundreds of microseconds
// after their inputs are ready (profiles/r3i trace). Nothing in a step reads device data on the
// host (the kept-sample count stays on the device), so a step whose arguments — every pointer,
// shape and option — equal an earlier call's is that call's work exactly: the second time a key is
// seen the step is captured into a graph (origin: the library's capture stream, since the caller's
// may be the null stream), and from then on one graph launch replays it. Callers keep the inputs
// in fixed buffers (trainer.FusedStep does). Opt-in (ANR_TRAIN_GRAPH=1): on ROCm 7.2 the replay
// measured slower than eager issue (2.86 vs 2.52 ms per bf16 step, profiles/r3j_*): the graph
// executor ran the nodes one after another across its queues with ~10 us between them, losing the
// overlap of the two chains and the weight-gradient lanes. Eager issue keeps up now that nothing in
// the step waits on the host.
struct StepGraphs {
  std::mutex mu;
  std::vector<std::pair<std::string, hipGraphExec_t>> cache;  // least recently used first
  std::vector<std::string> seen;                              // keys issued once eagerly
};

StepGraphs& step_graphs() {
  static StepGraphs g;
  return g;
}

template <typename T>
void key_add(std::string& k, const T& v) {
  k.append((const char*)&v, sizeof(T));
}

}  // namespace

extern "C" {

int anr_train_step_hooked(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o,
                          const float* ray_d, const float* near_, const float* far_, int n_rays,
                          const anr_render_opts* o, const float* rgb_gt, const uint8_t* mask_at_box,
                          const anr_render_out* out, float* loss3, const anr_train_hooks* hooks, void* workspace,
                          size_t ws_bytes, void* stream) {
  ANR_TRY(check_args(p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace));
  if (!grads || !rgb_gt || !loss3 || !out || !out->rgb_map || !out->acc_map || !out->depth_map)
    return fail(ANR_E_ARG, "anr_train_step: NULL argument");
  ANR_TRY(check_grads("anr_train_step", grads));
  TrainCall c;
  ANR_TRY(train_call(c, "anr_train_step", p, f, ray_o, ray_d, near_, far_, n_rays, o, workspace, ws_bytes));
  hipStream_t s = (hipStream_t)stream;
  SideStreams* ss = side_streams();
  if (hooks && hooks->struct_size != sizeof(anr_train_hooks))
    return fail(ANR_E_ARG, "anr_train_step_hooked: hooks->struct_size != sizeof(anr_train_hooks) (header version mismatch)");
  hipEvent_t nerf_done = hooks ? (hipEvent_t)hooks->nerf_grads_ready : nullptr;
  RaySplit split{};
  const bool splitting = hooks && hooks->reduce;
  if (splitting) {
    split.ray_offset = hooks->ray_offset;
    split.reduce = hooks->reduce;
    split.user = hooks->reduce_user;
    if (split.ray_offset < 0 || split.ray_offset + n_rays > o->chunk)
      return fail(ANR_E_ARG, "anr_train_step: a ray split needs ray_offset >= 0 and ray_offset + n_rays <= chunk");
  }
  const char* gv = getenv("ANR_TRAIN_GRAPH");
  // an external event (bucketed all-reduce) must be signalled by a plain record, and a ray split calls
  // its host hook mid-step: eager only
  const bool graphs = ss && !nerf_done && !splitting && gv && gv[0] == '1';
  if (!graphs) {
    // (a ray split's reduce hook is handed the main stream and issues its collectives there)
    OnMain om(ss, s);
    ANR_TRY(om.rc);
    return train_step_body(c, grads, rgb_gt, mask_at_box, out, loss3, nerf_done, om.s, ss, splitting ? &split : nullptr);
  }
  std::string key;
  int dev = 0;
  (void)hipGetDevice(&dev);
  key_add(key, dev);
  key_add(key, *p);
  for (int i = 0; i < ANR_NUM_TENSORS; ++i) key_add(key, grads[i]);
  key_add(key, *f);
  key_add(key, ray_o); key_add(key, ray_d); key_add(key, near_); key_add(key, far_); key_add(key, n_rays);
  key_add(key, *o);
  key_add(key, rgb_gt); key_add(key, mask_at_box); key_add(key, *out); key_add(key, loss3);
  key_add(key, workspace); key_add(key, ws_bytes);
  key_add(key, train_det());  // a graph captured in one mode is never replayed in the other
  StepGraphs& G = step_graphs();
  std::lock_guard<std::mutex> lock(G.mu);
  for (size_t i = 0; i < G.cache.size(); ++i)
    if (G.cache[i].first == key) {
      auto hit = G.cache[i];
      G.cache.erase(G.cache.begin() + i);
      G.cache.push_back(hit);
      if (hipGraphLaunch(hit.second, s) != hipSuccess) return fail(ANR_E_HIP, "anr_train_step: graph launch failed");
      return ANR_OK;
    }
  const auto seen = std::find(G.seen.begin(), G.seen.end(), key);
  if (seen == G.seen.end()) {
    G.seen.push_back(key);
    if (G.seen.size() > 64) G.seen.erase(G.seen.begin());
    OnMain om(ss, s);
    ANR_TRY(om.rc);
    return train_step_body(c, grads, rgb_gt, mask_at_box, out, loss3, nullptr, om.s, ss);
  }
  G.seen.erase(seen);
  // second sighting: capture, instantiate, launch
  if (!ss->cap && hipStreamCreateWithFlags(&ss->cap, hipStreamNonBlocking) != hipSuccess)
    return fail(ANR_E_HIP, "anr_train_step: capture stream");
  if (hipStreamBeginCapture(ss->cap, hipStreamCaptureModeRelaxed) != hipSuccess)
    return fail(ANR_E_HIP, "anr_train_step: hipStreamBeginCapture failed");
  const int rc = train_step_body(c, grads, rgb_gt, mask_at_box, out, loss3, nullptr, ss->cap, ss);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(ss->cap, &graph);
  if (rc != ANR_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ec != hipSuccess || !graph) return fail(ANR_E_HIP, "anr_train_step: hipStreamEndCapture failed");
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) return fail(ANR_E_HIP, "anr_train_step: hipGraphInstantiate failed");
  if (G.cache.size() >= 32) {
    (void)hipGraphExecDestroy(G.cache.front().second);
    G.cache.erase(G.cache.begin());
  }
  G.cache.emplace_back(key, exec);
  if (hipGraphLaunch(exec, s) != hipSuccess) return fail(ANR_E_HIP, "anr_train_step: graph launch failed");
  return ANR_OK;
}

size_t anr_anim_workspace_bytes(int n_points) {
  if (n_points <= 0) return 0;
  return alayout(n_points).total;
}

int anr_anim_step(const anr_params* p, float* const* grads, const anr_frame* f, const float* wpts, int n_obs,
                  const float* tpts, int n_can, const anr_render_opts* o, float* loss3, void* workspace,
                  size_t ws_bytes, void* stream) {
  if (!p || !grads || !f || !wpts || !tpts || !o || !loss3 || !workspace) return fail(ANR_E_ARG, "anr_anim_step: NULL argument");
  if (n_obs <= 0 || n_can <= 0) return fail(ANR_E_ARG, "anr_anim_step: empty point set");
  for (int i = 0; i < ANR_NUM_TENSORS; ++i)
    if (!p->t[i]) return fail(ANR_E_ARG, "anr_anim_step: NULL parameter tensor");
  for (int i = 0; i < ANR_NUM_NOVEL_TENSORS; ++i)
    if (!p->novel[i]) return fail(ANR_E_ARG, "anr_anim_step: the novel_pose_bw tensors are required");
  ANR_TRY(check_grads("anr_anim_step", grads, ANR_NUM_NOVEL_TENSORS));
  if (!f->A || !f->R || !f->Th || !f->pbw || !f->tbw || !f->pbounds || !f->tbounds || !f->bw_latent_index)
    return fail(ANR_E_ARG, "anr_anim_step: NULL frame tensor");
  for (int i = 0; i < 3; ++i)
    if (f->pbw_dims[i] <= 0 || f->tbw_dims[i] <= 0) return fail(ANR_E_ARG, "anr_anim_step: bad volume dims");
  if (o->precision < ANR_FP32 || o->precision > ANR_BF16X3) return fail(ANR_E_ARG, "anr_anim_step: bad precision");
  const int N = n_obs > n_can ? n_obs : n_can;
  const ALayout T = alayout(N);
  if (ws_bytes < T.total) return fail(ANR_E_WORKSPACE, "anr_anim_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if (hipMemsetAsync(ws + T.counts, 0, 16, s) != hipSuccess || hipMemsetAsync(ws + T.acc, 0, 16, s) != hipSuccess)
    return fail(ANR_E_HIP, "memset");
  // folded biases: pose pass from novel_pose_bw (bw_latent_index), T-pose pass from bw_latent row 0
  PrepArgs pa{};
  pa.np = 0; pa.nt = 0;
  pa.w_bw0 = p->t[28]; pa.b_bw0 = p->t[29]; pa.w_bw5 = p->t[38]; pa.b_bw5 = p->t[39];
  pa.bw_latent = p->t[27]; pa.w_lat = p->t[21]; pa.b_lat = p->t[22]; pa.nf_latent = p->t[0];
  pa.latent_index = f->latent_index ? f->latent_index : f->bw_latent_index;  // only the unused nf fold reads it
  pa.fold = (float*)(ws + T.fold);
  pa.novel = 1;
  pa.n_latent = p->novel[0];
  pa.nw_bw0 = p->novel[1]; pa.nb_bw0 = p->novel[2];
  pa.nw_bw5 = p->novel[11]; pa.nb_bw5 = p->novel[12];
  pa.bw_latent_index = f->bw_latent_index;
  hipLaunchKernelGGL(k_prep, dim3(prep_blocks(0, 0)), dim3(256), 0, s, pa);
  ANR_TRY(check_launch("k_prep(anim)"));
  Exec e{};
  init_exec(e, *o, s, nullptr, ws, T);  // one stream, one weight-gradient lane
  e.hb = 0;                             // fp32 rows under every policy
  ANR_TRY(pack_images(e, p, ws + T.wimg, s, (float*)(ws + T.wslab), wgrad_slab_floats(), true));
  ANR_TRY(anim_path(p, grads, f, wpts, n_obs, true, o, ws, T, s, e));
  ANR_TRY(anim_path(p, grads, f, tpts, n_can, false, o, ws, T, s, e));
  ANR_TRY(e.flush_w());
  hipLaunchKernelGGL(k_an_loss_final, dim3(1), dim3(1), 0, s, (const float*)(ws + T.acc),
                     (const int*)(ws + T.counts) + 1, loss3);
  return check_launch("k_an_loss_final");
}

// ---- Network.forward under autograd (free samples) -------------------------------------------
static int check_network_train(const anr_params* p, const anr_frame* f, const anr_samples* x, const anr_render_opts* o,
                               void* ws) {
  if (!x || !x->wpts || !x->viewdir || !x->dists || x->n_pts <= 0 || (long)x->n_pts > 0x7fffffffL / 24 - 64)
    return fail(ANR_E_ARG, "network train: bad samples");
  if (f && f->n_views) return fail(ANR_E_ARG, "network train: the visibility filter is a renderer option");
  // check_args wants ray pointers: the samples stand in for them
  return check_args(p, f, x->wpts, x->viewdir, x->dists, x->dists, (x->n_pts + 63) / 64, o, ws);
}

size_t anr_network_train_workspace_bytes(int n_pts, const anr_render_opts* o, const anr_frame* f) {
  if (!o || !f || n_pts <= 0) return 0;
  const int G = (n_pts + 63) / 64;
  return tlayout(G, G, f).total;
}

int anr_network_train_fwd(const anr_params* p, const anr_frame* f, const anr_samples* x, const anr_render_opts* o,
                          float* raw, void* workspace, size_t ws_bytes, void* stream) {
  ANR_TRY(check_network_train(p, f, x, o, workspace));
  if (!raw) return fail(ANR_E_ARG, "anr_network_train_fwd: NULL raw");
  TrainCall c;
  ANR_TRY(train_call(c, "anr_network_train_fwd", p, f, x, o, workspace, ws_bytes));
  OnMain om(side_streams(), (hipStream_t)stream);
  ANR_TRY(om.rc);
  Exec e{};
  init_exec(e, c.o, om.s, om.ss, c.ws, c.T);
  ANR_TRY(pack_for(c, e, om.s, true, false));
  ANR_TRY(train_forward(c, nullptr, om.s, e));
  if (hipMemcpyAsync(raw, c.ws + c.T.L.raw, (size_t)x->n_pts * 16, hipMemcpyDeviceToDevice, om.s) != hipSuccess)
    return fail(ANR_E_HIP, "anr_network_train_fwd: raw copy failed");
  return ANR_OK;
}

int anr_network_train_bwd(const anr_params* p, float* const* grads, const anr_frame* f, const anr_samples* x,
                          const anr_render_opts* o, const float* d_raw, const float* d_pbw, const float* d_tbw,
                          void* workspace, size_t ws_bytes, void* stream) {
  ANR_TRY(check_network_train(p, f, x, o, workspace));
  ANR_TRY(check_grads("anr_network_train_bwd", grads));
  TrainCall c;
  ANR_TRY(train_call(c, "anr_network_train_bwd", p, f, x, o, workspace, ws_bytes));
  OnMain om(side_streams(), (hipStream_t)stream);
  ANR_TRY(om.rc);
  Exec e{};
  init_exec(e, c.o, om.s, om.ss, c.ws, c.T);
  ANR_TRY(pack_for(c, e, om.s, false, true));
  ANR_TRY(train_backward(c, grads, nullptr, d_pbw, d_tbw, om.s, e, d_raw));
  return pose_backward(c, e, grads);
}

// ---- free-point helpers: calculate_neural_blend_weights / novel_pose_bw, TPoseHuman.calculate_alpha --
// gamma rows G, initial SMPL-weight rows I, logits Lg, the hidden rows H of one MLP, the two folded biases
struct PLayout {
  size_t G, I, Lg, H, fold, total;
};
static PLayout playout(int n) {
  const size_t N = (size_t)n;
  Carve c;
  PLayout P{};
  P.G = c.floats(N * 64); P.I = c.floats(N * 32); P.Lg = c.floats(N * 32); P.H = c.floats(N * 256 * 8);
  P.fold = c.floats(512);
  P.total = c.o;
  return P;
}

size_t anr_points_workspace_bytes(int n) { return n <= 0 ? 0 : playout(n).total; }

int anr_blend_weights(const anr_params* p, int field, const float* pts, const float* smpl_bw, int n,
                      const int64_t* latent_row, int row_add, float* bw, void* workspace, size_t ws_bytes, void* stream) {
  if (!p || !pts || !smpl_bw || !latent_row || !bw || !workspace || n <= 0 || (field != 0 && field != 1))
    return fail(ANR_E_ARG, "anr_blend_weights: bad arguments");
  const float* const* W = field ? p->novel : p->t + 27;
  for (int i = 0; i < 19; ++i)
    if (!W[i]) return fail(ANR_E_ARG, "anr_blend_weights: NULL blend-weight field tensor");
  const PLayout P = playout(n);
  if (ws_bytes < P.total) return fail(ANR_E_WORKSPACE, "anr_blend_weights: workspace too small");
  char* ws = (char*)workspace;
  float *G = (float*)(ws + P.G), *I = (float*)(ws + P.I), *Lg = (float*)(ws + P.Lg), *H = (float*)(ws + P.H);
  float* fold = (float*)(ws + P.fold);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pt_prep, dim3((n + 3) / 4), dim3(256), 0, s, pts, smpl_bw, n, G, I);
  FoldArgs fa{W[1], W[2], W[11], W[12], W[0], latent_row, row_add, fold};
  hipLaunchKernelGGL(k_fold_latent, dim3(1), dim3(256), 0, s, fa);
  ANR_TRY(check_launch("anr_blend_weights prep"));
  Exec e{s, n, 0, 0};
  ANR_TRY(bw_forward(e, W, G, H, Lg, n, fold, fold + 256));
  hipLaunchKernelGGL(k_pt_softmax_out, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)Lg, (const float*)I, n, bw);
  return check_launch("k_pt_softmax_out");
}

int anr_canonical_alpha(const anr_params* p, const float* pts, int n, float* alpha, void* workspace, size_t ws_bytes,
                        void* stream) {
  if (!p || !pts || !alpha || !workspace || n <= 0) return fail(ANR_E_ARG, "anr_canonical_alpha: bad arguments");
  for (int i = 1; i <= 18; ++i)
    if (!p->t[i]) return fail(ANR_E_ARG, "anr_canonical_alpha: NULL parameter tensor");
  const PLayout P = playout(n);
  if (ws_bytes < P.total) return fail(ANR_E_WORKSPACE, "anr_canonical_alpha: workspace too small");
  char* ws = (char*)workspace;
  float *G = (float*)(ws + P.G), *H = (float*)(ws + P.H);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pt_prep, dim3((n + 3) / 4), dim3(256), 0, s, pts, (const float*)nullptr, n, G, (float*)nullptr);
  ANR_TRY(check_launch("k_pt_prep"));
  Exec e{s, n, 0, 0};
  TrainBufs b{};
  b.Gt = G;
  b.Alpha = alpha;
  return nerf_alpha_fwd(e, p, b, H, n);
}

int anr_adam(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
             float eps, float weight_decay, int step, float clip_value, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return fail(ANR_E_ARG, "anr_adam: bad arguments");
  if (n == 0) return ANR_OK;
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, clip_value);
  return check_launch("k_adam");
}

}  // extern "C"
