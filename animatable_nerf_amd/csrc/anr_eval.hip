// anr_eval.hip — the frame evaluator (A18, lib/evaluators/if_nerf.py:15-74) on the device: PSNR and the
// windowed SSIM of one rendered frame, from the in-box rays and the frame's mask_at_box.
//
// Launch sequence of anr_eval_frame (all on the caller's stream, no kernel waits on another workgroup):
//   k_eval_count  per 1024-pixel block: popcount of the mask and the block's column / row extents
//   k_eval_scan   one block: exclusive scan of the block counts, the bounding rectangle, the header
//   k_eval_apply  pixel -> ray row (exclusive scan of the mask, -1 outside); the optional scattered images
//   k_eval_sse    per-block partial sums of (pred - gt)^2 and of gt, in float64
//   k_eval_ssim   a 32x32 tile of SSIM values per (tile, channel): one partial sum each
//   k_eval_final  one block: adds every partial in index order and writes the 12-double record
// Every reduction has a fixed order (per-thread strides, a fixed shuffle tree, partials added in index
// order) and there is no floating-point atomic: the same inputs give the same bits.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/aninerf.h"
#include "anr_common.h"
#include "anr_ws.h"

using namespace anr;

namespace {

constexpr int EV_PIX = 1024;      // mask pixels per block of the count / apply launches
constexpr int EV_SSE_ELEMS = 2048;  // elements per block and grid-stride step of k_eval_sse
constexpr int EV_SSE_BLOCKS = 256;  // its largest grid (the partials' workspace is sized from H, W alone)
constexpr int EV_TILE = 32, EV_WIN = 7, EV_PAD = EV_WIN / 2, EV_HALO = EV_TILE + EV_WIN - 1;
constexpr long EV_MAX_PIX = 1L << 28;

// header ints: [0] popcount(mask) [1] x [2] y [3] w [4] h
struct EvalBlock { int cnt, minx, maxx, miny, maxy, base; };

struct EvalLayout {
  size_t hdr, blk, rowmap, sse, ssim, total;
  int nb, tiles_x, tiles_y;
};

EvalLayout eval_layout(int H, int W) {
  EvalLayout L{};
  const size_t hw = (size_t)H * (size_t)W;
  L.nb = (int)((hw + EV_PIX - 1) / EV_PIX);
  L.tiles_x = (W + EV_TILE - 1) / EV_TILE;
  L.tiles_y = (H + EV_TILE - 1) / EV_TILE;
  Carve c;
  L.hdr = c.bytes(8 * sizeof(int));
  L.blk = c.bytes((size_t)L.nb * sizeof(EvalBlock));
  L.rowmap = c.bytes(hw * sizeof(int));
  L.sse = c.bytes((size_t)2 * EV_SSE_BLOCKS * sizeof(double));
  L.ssim = c.bytes((size_t)3 * L.tiles_x * L.tiles_y * sizeof(double));
  L.total = c.o;
  return L;
}

// sum over a 256-thread block in a fixed order: xor butterfly inside each wave, then the 4 wave sums
// left to right (sh: 4 doubles of LDS); every thread returns the total
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return t;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

__global__ __launch_bounds__(256) void k_eval_count(const uint8_t* __restrict__ mask, int H, int W,
                                                    EvalBlock* __restrict__ blk) {
  __shared__ int sh[4], shx[4][4];
  const int hw = H * W;
  int cnt = 0, minx = W, maxx = -1, miny = H, maxy = -1;
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * EV_PIX + k * 256 + threadIdx.x;
    if (i < hw && mask[i] != 0) {
      const int y = i / W, x = i - y * W;
      ++cnt;
      minx = min(minx, x); maxx = max(maxx, x);
      miny = min(miny, y); maxy = max(maxy, y);
    }
  }
  minx = wave_min(minx); miny = wave_min(miny);
  maxx = wave_max(maxx); maxy = wave_max(maxy);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    shx[w][0] = minx; shx[w][1] = maxx; shx[w][2] = miny; shx[w][3] = maxy;
  }
  int total;
  block_excl_scan_256(cnt, sh, total);  // its barriers also publish shx
  if (threadIdx.x == 0) {
    EvalBlock b;
    b.cnt = total;
    b.minx = min(min(shx[0][0], shx[1][0]), min(shx[2][0], shx[3][0]));
    b.maxx = max(max(shx[0][1], shx[1][1]), max(shx[2][1], shx[3][1]));
    b.miny = min(min(shx[0][2], shx[1][2]), min(shx[2][2], shx[3][2]));
    b.maxy = max(max(shx[0][3], shx[1][3]), max(shx[2][3], shx[3][3]));
    b.base = 0;
    blk[blockIdx.x] = b;
  }
}

// one block: block bases (exclusive scan of the counts, 256 blocks per pass) and the rectangle
__global__ __launch_bounds__(256) void k_eval_scan(EvalBlock* __restrict__ blk, int nb, int H, int W,
                                                   int* __restrict__ hdr) {
  __shared__ int sh[4], shx[4][4];
  int run = 0, minx = W, maxx = -1, miny = H, maxy = -1;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    int c = 0;
    if (b < nb) {
      const EvalBlock e = blk[b];
      c = e.cnt;
      minx = min(minx, e.minx); maxx = max(maxx, e.maxx);
      miny = min(miny, e.miny); maxy = max(maxy, e.maxy);
    }
    int total;
    const int ex = block_excl_scan_256(c, sh, total);
    if (b < nb) blk[b].base = run + ex;
    run += total;
  }
  minx = wave_min(minx); miny = wave_min(miny);
  maxx = wave_max(maxx); maxy = wave_max(maxy);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    shx[w][0] = minx; shx[w][1] = maxx; shx[w][2] = miny; shx[w][3] = maxy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int x0 = min(min(shx[0][0], shx[1][0]), min(shx[2][0], shx[3][0]));
    const int x1 = max(max(shx[0][1], shx[1][1]), max(shx[2][1], shx[3][1]));
    const int y0 = min(min(shx[0][2], shx[1][2]), min(shx[2][2], shx[3][2]));
    const int y1 = max(max(shx[0][3], shx[1][3]), max(shx[2][3], shx[3][3]));
    const bool any = run > 0;  // cv2.boundingRect of an empty mask: (0, 0, 0, 0)
    hdr[0] = run;
    hdr[1] = any ? x0 : 0;
    hdr[2] = any ? y0 : 0;
    hdr[3] = any ? x1 - x0 + 1 : 0;
    hdr[4] = any ? y1 - y0 + 1 : 0;
  }
}

// rgb -> the reference's PNG sample before cv2.imwrite's cast: rint(clip(255 v, 0, 255)), half to even
__device__ __forceinline__ uint8_t to_u8(float v) {
  return (uint8_t)(int)rint(fmin(fmax(255.0 * (double)v, 0.0), 255.0));
}

__global__ __launch_bounds__(256) void k_eval_apply(const uint8_t* __restrict__ mask, int H, int W, int n_rays,
                                                    const EvalBlock* __restrict__ blk, int* __restrict__ rowmap,
                                                    const float* __restrict__ rgb_pred, const float* __restrict__ rgb_gt,
                                                    float* __restrict__ img_pred, float* __restrict__ img_gt,
                                                    uint8_t* __restrict__ img8_pred, uint8_t* __restrict__ img8_gt) {
  __shared__ int sh[4];
  const int hw = H * W;
  int base = blk[blockIdx.x].base;
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * EV_PIX + k * 256 + threadIdx.x;
    const int f = (i < hw && mask[i] != 0) ? 1 : 0;
    int total;
    const int ex = block_excl_scan_256(f, sh, total);
    if (i < hw) {
      int r = f ? base + ex : -1;
      if (r >= n_rays) r = -1;  // more set pixels than rays (status 3): read nothing, count as zero
      rowmap[i] = r;
      float p[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
      if (r >= 0 && (img_pred || img8_pred))
        for (int c = 0; c < 3; ++c) p[c] = rgb_pred[(size_t)r * 3 + c];
      if (r >= 0 && (img_gt || img8_gt))
        for (int c = 0; c < 3; ++c) g[c] = rgb_gt[(size_t)r * 3 + c];
      const size_t o = (size_t)i * 3;
      for (int c = 0; c < 3; ++c) {
        if (img_pred) img_pred[o + c] = p[c];
        if (img_gt) img_gt[o + c] = g[c];
        if (img8_pred) img8_pred[o + c] = to_u8(p[c]);
        if (img8_gt) img8_gt[o + c] = to_u8(g[c]);
      }
    }
    base += total;
  }
}

// partial[2 b] = sum (double(pred) - double(gt))^2, partial[2 b + 1] = sum gt over block b's elements
__global__ __launch_bounds__(256) void k_eval_sse(const float* __restrict__ pred, const float* __restrict__ gt,
                                                  long n3, double* __restrict__ partial) {
  __shared__ double sh[4];
  double se = 0.0, sg = 0.0;
  for (long b0 = (long)blockIdx.x * EV_SSE_ELEMS; b0 < n3; b0 += (long)gridDim.x * EV_SSE_ELEMS) {
#pragma unroll
    for (int j = 0; j < EV_SSE_ELEMS / 256; ++j) {
      const long i = b0 + j * 256 + threadIdx.x;
      if (i < n3) {
        const double g = (double)gt[i], d = (double)pred[i] - g;
        se += d * d;
        sg += g;
      }
    }
  }
  se = block_sum_256(se, sh);
  sg = block_sum_256(sg, sh);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = se;
    partial[2 * blockIdx.x + 1] = sg;
  }
}

// structural_similarity (scikit-image 0.16-0.18, multichannel, uniform 7x7 window, sample covariance) of
// one channel over one 32x32 tile of pixels: the 38x38 halo of both images is gathered through the row
// map into LDS as fp32, the five moments are separable 7-tap sums in fp64 (rows into LDS, then columns),
// and the tile's S values whose window lies wholly inside the crop (the crop minus its 3-pixel border)
// are added into partial[(channel * tiles_y + tile_y) * tiles_x + tile_x].
__global__ __launch_bounds__(256) void k_eval_ssim(const float* __restrict__ rgb_pred, const float* __restrict__ rgb_gt,
                                                   const int* __restrict__ rowmap, const int* __restrict__ hdr,
                                                   int H, int W, double c1, double c2, double* __restrict__ partial) {
  __shared__ float s_x[EV_HALO * EV_HALO], s_y[EV_HALO * EV_HALO];
  __shared__ double s_h[5][EV_HALO * EV_TILE];
  __shared__ double sh[4];
  const int c = blockIdx.z;
  const int ty0 = blockIdx.y * EV_TILE, tx0 = blockIdx.x * EV_TILE;
  double* out = partial + ((size_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int rx = hdr[1], ry = hdr[2], rw = hdr[3], rh = hdr[4];
  // pixels that carry an S value: [oy0, oy1) x [ox0, ox1)
  const int ox0 = rx + EV_PAD, ox1 = rx + rw - EV_PAD, oy0 = ry + EV_PAD, oy1 = ry + rh - EV_PAD;
  if (max(ox0, tx0) >= min(ox1, tx0 + EV_TILE) || max(oy0, ty0) >= min(oy1, ty0 + EV_TILE)) {  // block-uniform
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  for (int k = threadIdx.x; k < EV_HALO * EV_HALO; k += 256) {
    const int hy = k / EV_HALO, hx = k - hy * EV_HALO;
    const int py = ty0 - EV_PAD + hy, px = tx0 - EV_PAD + hx;
    float vx = 0.f, vy = 0.f;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const int r = rowmap[py * W + px];
      if (r >= 0) {
        vx = rgb_pred[(size_t)r * 3 + c];
        vy = rgb_gt[(size_t)r * 3 + c];
      }
    }
    s_x[k] = vx;
    s_y[k] = vy;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < EV_HALO * EV_TILE; k += 256) {
    const int hy = k / EV_TILE, ox = k - hy * EV_TILE;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int d = 0; d < EV_WIN; ++d) {
      const double x = (double)s_x[hy * EV_HALO + ox + d], y = (double)s_y[hy * EV_HALO + ox + d];
      sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
    }
    s_h[0][k] = sx; s_h[1][k] = sy; s_h[2][k] = sxx; s_h[3][k] = syy; s_h[4][k] = sxy;
  }
  __syncthreads();
  constexpr double inv_n = 1.0 / (EV_WIN * EV_WIN), cov_norm = (double)(EV_WIN * EV_WIN) / (EV_WIN * EV_WIN - 1);
  double acc = 0.0;
  for (int k = threadIdx.x; k < EV_TILE * EV_TILE; k += 256) {
    const int oy = k / EV_TILE, ox = k - oy * EV_TILE;
    const int py = ty0 + oy, px = tx0 + ox;
    if (py < oy0 || py >= oy1 || px < ox0 || px >= ox1) continue;
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < EV_WIN; ++d) s += s_h[q][(oy + d) * EV_TILE + ox];
      m[q] = s * inv_n;
    }
    const double ux = m[0], uy = m[1];
    const double vx = cov_norm * (m[2] - ux * ux), vy = cov_norm * (m[3] - uy * uy), vxy = cov_norm * (m[4] - ux * uy);
    const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
    const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
    acc += (a1 * a2) / (b1 * b2);
  }
  acc = block_sum_256(acc, sh);
  if (threadIdx.x == 0) *out = acc;
}

// sum of p[0], p[stride], ... (n terms) by one block in a fixed order: thread t adds its contiguous run
// of terms left to right, thread 0 adds the 256 run sums left to right (sh: 256 doubles)
__device__ double ordered_sum(const double* __restrict__ p, int n, int stride, double* sh) {
  const int per = (n + 255) / 256;
  double s = 0.0;
  for (int j = 0; j < per; ++j) {
    const int i = threadIdx.x * per + j;
    if (i < n) s += p[(size_t)i * stride];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < 256; ++k) t += sh[k];
  __syncthreads();
  return t;  // valid in thread 0
}

__global__ __launch_bounds__(256) void k_eval_final(const int* __restrict__ hdr, const double* __restrict__ sse_part,
                                                    int n_sse, const double* __restrict__ ssim_part, int n_tiles,
                                                    int n_rays, double* __restrict__ out) {
  __shared__ double sh[256];
  const double sse = ordered_sum(sse_part, n_sse, 2, sh);
  const double sum_gt = ordered_sum(sse_part + 1, n_sse, 2, sh);
  double ch[3];
  for (int c = 0; c < 3; ++c) ch[c] = ordered_sum(ssim_part + (size_t)c * n_tiles, n_tiles, 1, sh);
  if (threadIdx.x != 0) return;
  const int pop = hdr[0], x = hdr[1], y = hdr[2], w = hdr[3], h = hdr[4];
  const double n3 = 3.0 * (double)n_rays;
  const double nan = __builtin_nan("");
  double mse = sse / n3, psnr = -10.0 * log10(mse), ssim = nan;
  int status = 0;
  if (pop == 0) status = 1;
  else if (pop != n_rays) status = 3;
  else if (sum_gt == 0.0) status = 1;
  else if (w < EV_WIN || h < EV_WIN) status = 2;
  if (status == 0) {
    const double cnt = (double)(w - 2 * EV_PAD) * (double)(h - 2 * EV_PAD);
    ssim = ((ch[0] / cnt + ch[1] / cnt) + ch[2] / cnt) / 3.0;
  }
  if (status == 3) mse = psnr = nan;
  out[0] = sse; out[1] = n3; out[2] = mse; out[3] = psnr; out[4] = ssim;
  out[5] = x; out[6] = y; out[7] = w; out[8] = h;
  out[9] = sum_gt; out[10] = status; out[11] = 0.0;
}

}  // namespace

extern "C" {

size_t anr_eval_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (long)H * (long)W > EV_MAX_PIX) return 0;
  return eval_layout(H, W).total;
}

int anr_eval_frame(const float* rgb_pred, const float* rgb_gt, int n_rays, const uint8_t* mask_at_box, int H, int W,
                   const anr_eval_opts* o, double* out, float* img_pred, float* img_gt, uint8_t* img8_pred,
                   uint8_t* img8_gt, void* workspace, size_t ws_bytes, void* stream) {
  if (!rgb_pred || !rgb_gt || !mask_at_box || !out || !workspace)
    return fail(ANR_E_ARG, "anr_eval_frame: NULL argument");
  if (n_rays <= 0 || H <= 0 || W <= 0) return fail(ANR_E_ARG, "anr_eval_frame: n_rays, H and W must be positive");
  if ((long)H * (long)W > EV_MAX_PIX) return fail(ANR_E_ARG, "anr_eval_frame: H * W above 2^28");
  double range = 2.0;
  if (o) {
    if (o->struct_size != sizeof(anr_eval_opts))
      return fail(ANR_E_ARG, "anr_eval_frame: opts.struct_size is not sizeof(anr_eval_opts)");
    if (o->win != EV_WIN) return fail(ANR_E_ARG, "anr_eval_frame: only win = 7 is supported");
    if (!(o->data_range > 0.0) || !std::isfinite(o->data_range))
      return fail(ANR_E_ARG, "anr_eval_frame: data_range must be positive and finite");
    range = o->data_range;
  }
  const EvalLayout L = eval_layout(H, W);
  if (ws_bytes < L.total) return fail(ANR_E_WORKSPACE, "anr_eval_frame: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* hdr = (int*)(ws + L.hdr);
  EvalBlock* blk = (EvalBlock*)(ws + L.blk);
  int* rowmap = (int*)(ws + L.rowmap);
  double* sse = (double*)(ws + L.sse);
  double* ssim = (double*)(ws + L.ssim);
  hipLaunchKernelGGL(k_eval_count, dim3(L.nb), dim3(256), 0, s, mask_at_box, H, W, blk);
  ANR_TRY(check_launch("k_eval_count"));
  hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(256), 0, s, blk, L.nb, H, W, hdr);
  ANR_TRY(check_launch("k_eval_scan"));
  hipLaunchKernelGGL(k_eval_apply, dim3(L.nb), dim3(256), 0, s, mask_at_box, H, W, n_rays, (const EvalBlock*)blk, rowmap,
                     rgb_pred, rgb_gt, img_pred, img_gt, img8_pred, img8_gt);
  ANR_TRY(check_launch("k_eval_apply"));
  const long n3 = 3L * n_rays;
  const int n_sse = (int)std::min<long>((n3 + EV_SSE_ELEMS - 1) / EV_SSE_ELEMS, EV_SSE_BLOCKS);
  hipLaunchKernelGGL(k_eval_sse, dim3(n_sse), dim3(256), 0, s, rgb_pred, rgb_gt, n3, sse);
  ANR_TRY(check_launch("k_eval_sse"));
  const double c1 = (0.01 * range) * (0.01 * range), c2 = (0.03 * range) * (0.03 * range);
  hipLaunchKernelGGL(k_eval_ssim, dim3(L.tiles_x, L.tiles_y, 3), dim3(256), 0, s, rgb_pred, rgb_gt, (const int*)rowmap,
                     (const int*)hdr, H, W, c1, c2, ssim);
  ANR_TRY(check_launch("k_eval_ssim"));
  hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(256), 0, s, (const int*)hdr, (const double*)sse, n_sse,
                     (const double*)ssim, L.tiles_x * L.tiles_y, n_rays, out);
  return check_launch("k_eval_final");
}

}  // extern "C"
