/*
 * aninerf.h — C-ABI of the MI355X-native Animatable-NeRF volume-rendering hot path.
 *
 * Plain C: device pointers + sizes + a hipStream_t passed as void*; no torch types. Every entry
 * point is asynchronous on the given stream and returns 0 or an ANR_E* code (a hipError_t is
 * returned as ANR_E_HIP, its text via anr_last_error()).
 *
 * Reference interfaces each entry point replaces (paths relative to the reference tree):
 *   anr_near_far            lib/utils/if_nerf/if_nerf_data_utils.py:156-196   get_near_far (A14)
 *   anr_camera_rays         if_nerf_data_utils.py:64-89, 310-339  get_rays + get_rays_within_bounds
 *   anr_params_pack         lib/networks/bw_deform/tpose_nerf_network.py:11-38, 218-239
 *                           (state_dict -> the kernel's weight image; called when weights change)
 *   anr_render_fwd          lib/networks/renderer/tpose_renderer.py:159-186   Renderer.render (A1)
 *                             -> get_wsampling_points :14-39, get_density_color :41-69,
 *                                Network.forward tpose_nerf_network.py:139-215,
 *                                raw2outputs nerf_net_utils.py:6-36
 *   anr_render_counts       the host syncs the reference makes at pind/alpha_ind (:153-157, :192-196)
 *   anr_render_bw_rows      tpose_nerf_network.py:195-196 (pbw/tbw rows selected by alpha_ind)
 *   anr_sdf_render_fwd      the same Renderer.render over the sdf_pdf network (config 5):
 *                             lib/networks/bw_deform/anisdf_pdf_network.py:156-223 Network.forward,
 *                             sample_utils.py:309-348 (KNN blend), TPoseHuman :288-338,
 *                             tpose_renderer.py:134-152 (msk_sdf / msk_label)
 *   anr_sdf_train_step      lib/train/trainers/tpose_trainer.py:21-73 over the sdf_pdf network
 *                             (configs/sdf_pdf/anisdf_pdf_s9p.yaml:13-14), forward + loss.backward()
 *   anr_sdf_render_counts / anr_sdf_render_rows   the compact outputs 'resd', 'gradients',
 *                             'msk_sdf', 'msk_label' (sizes known only after the keep mask)
 *   anr_network_fwd         lib/networks/bw_deform/tpose_nerf_network.py:139-215 Network.forward
 *                             (wpts, viewdir, dists, batch), the per-chunk call of tpose_renderer.py:95
 *   anr_network_train_fwd/bwd  the same call under autograd (forward + loss.backward() through it)
 *   anr_blend_weights       tpose_nerf_network.py:55-77 calculate_neural_blend_weights and
 *                             :304-315 BackwardBlendWeight.forward (novel_pose_bw)
 *   anr_canonical_alpha     tpose_nerf_network.py:241-250 TPoseHuman.calculate_alpha
 *   anr_alpha_points        lib/networks/bw_deform/tpose_nerf_network.py:105-137 Network.get_alpha
 *                             over the batchify chunks of aninerf_mesh_renderer.py:14-23, 34-36
 *   anr_anim_step           lib/train/trainers/aninerf_animation_trainer.py:33-140 (forward + backward)
 *   anr_mc_count/anr_mc_emit  mcubes.marching_cubes(np.pad(cube, 10), cfg.mesh_th)
 *                             (aninerf_mesh_renderer.py:38-45; PyMCubes, third-party, not installed)
 *   anr_eval_frame          lib/evaluators/if_nerf.py:15-74 Evaluator.evaluate (mse, psnr, ssim; A18)
 *   anr_mesh_cc_count/anr_mesh_cc_emit  max(trimesh.Trimesh(v, t).split(), key=lambda m: len(m.vertices))
 *                             (sdf_mesh_renderer.py:77-78; trimesh, third-party, not installed)
 *   anr_bw_volume           tools/custom_dataset/prepare_blend_weights.py:156-211, 229-283 (the per-frame
 *                             bweights/{i}.npy and the tbw.npy / bigpose_bw.npy volumes)
 *   anr_mesh_sample         trimesh.sample.sample_surface (lib/evaluators/mesh_evaluator.py:103-107, 126-127;
 *                             trimesh, third-party, not installed)
 *   anr_mesh_point_dist     trimesh.proximity.closest_point (mesh_evaluator.py:109-112, 129-130)
 *   anr_mesh_metrics        MeshEvaluator.get_chamfer_dist + get_surface_dist of one frame (:100-136)
 *   anr_mesh_order          the linear-time Morton ordering of the faces that the search is built on
 *   anr_mesh_dist_workspace_bytes  the workspace of the four above
 *
 * All float tensors are fp32, contiguous, row-major, with the reference's shapes (batch dim 1).
 */
#ifndef ANINERF_H
#define ANINERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  ANR_OK = 0,
  ANR_E_HIP = 1,        /* a HIP runtime call failed; see anr_last_error() */
  ANR_E_ARG = 2,        /* bad shape / NULL pointer / unsupported option */
  ANR_E_WORKSPACE = 3   /* workspace too small */
};

/* Number of tensors of the aninerf Network state_dict (tpose_nerf_network.py:11-38, 218-239),
 * in this order (weights are Conv1d (out, in, 1), embeddings (rows, 128)):
 *   0 tpose_human.nf_latent.weight (F,128)
 *   1..16  tpose_human.pts_linears.{0..7}.{weight,bias}   in: 63,256,256,256,256,319,256,256
 *   17,18 tpose_human.alpha_fc.{weight,bias} (1,256,1)
 *   19,20 tpose_human.feature_fc.{weight,bias} (256,256,1)
 *   21,22 tpose_human.latent_fc.{weight,bias} (256,384,1)
 *   23,24 tpose_human.view_fc.{weight,bias} (128,283,1)
 *   25,26 tpose_human.rgb_fc.{weight,bias} (3,128,1)
 *   27 bw_latent.weight (F+1,128)
 *   28..43 bw_linears.{0..7}.{weight,bias}   in: 191,256,256,256,256,447,256,256
 *   44,45 bw_fc.{weight,bias} (24,256,1)                                                     */
#define ANR_NUM_TENSORS 46
/* novel_pose_bw (BackwardBlendWeight, tpose_nerf_network.py:278-315; present when
 * cfg.aninerf_animation): bw_latent.weight (E,128), bw_linears.{0..7}.{weight,bias},
 * bw_fc.{weight,bias} — 19 tensors, state_dict order. */
#define ANR_NUM_NOVEL_TENSORS 19

typedef struct anr_params {
  const float* t[ANR_NUM_TENSORS];  /* device pointers, state_dict order above */
  int num_train_frame;              /* F: rows of nf_latent (bw_latent has F+1) */
  const void* packed;               /* device weight image written by anr_params_pack */
  const float* novel[ANR_NUM_NOVEL_TENSORS];  /* novel_pose_bw tensors or all NULL */
} anr_params;

typedef struct anr_frame {
  const float* A;          /* (24,4,4) device */
  const float* R;          /* (3,3) device (smpl->world rotation, Rodrigues(Rh)) */
  const float* Th;         /* (3) device */
  const float* pbw;        /* (X,Y,Z,25) device: posed blend-weight volume, ch 24 = distance */
  int pbw_dims[3];
  const float* pbounds;    /* (2,3) device */
  const float* tbw;        /* (X',Y',Z',25) device: T-pose blend-weight volume */
  int tbw_dims[3];
  const float* tbounds;    /* (2,3) device */
  const int64_t* latent_index;  /* (1) device: batch['latent_index'] */
  const int64_t* bw_latent_index;  /* (1) device: batch['bw_latent_index'] (novel pose only) */
  /* novel-view visibility filter (tpose_renderer_mmsk.py:14-57); n_views = 0 disables it:
   * a sample is kept only if it projects inside every training view's mask. */
  int n_views;
  const float* Ks;         /* (V,3,3) device */
  const float* RT;         /* (V,3,4) device, world -> camera */
  const uint8_t* msks;     /* (V,img_h,img_w) device */
  int img_h, img_w;
} anr_frame;

typedef struct anr_render_opts {
  int n_samples;     /* cfg.N_samples; 64 (anr_render_ns_fwd: 64, 128, 192 or 256) */
  int chunk;         /* rays per reference chunk (2048, tpose_renderer.py:170); semantics depend on it */
  float norm_th;     /* cfg.norm_th (0.05) */
  float train_th;    /* cfg.train_th (0) */
  const float* t_rand;  /* (R, n_samples) device stratification draws, or NULL (eval / perturb 0) */
  int novel_pose;    /* cfg.test_novel_pose: pose-space blend weights from novel_pose_bw
                        with bw_latent_index (tpose_nerf_network.py:93-94); render only */
  int precision;     /* training GEMM operands: ANR_FP32 (exact fp32 MFMA); ANR_BF16 (config 3:
                        operands rounded to bf16, fp32 accumulation, fp32 master weights and Adam,
                        the pose-space blend-weight MLP kept fp32); ANR_BF16_ALL (every GEMM bf16).
                        anr_render_fwd / anr_alpha_points: ANR_FP32 (exact fp32 MFMA everywhere) or
                        ANR_BF16X3 (every MLP layer as hi/lo-split bf16 MFMA, lo*bh + hi*bl + hi*bh
                        with fp32 accumulation: ~2^-16 relative per product, outputs within the
                        1e-4 fp32 tolerance); anr_render_fwd / anr_network_fwd / anr_alpha_points
                        also ANR_BF16X6
                        (hi/mid/lo-split bf16, six products per multiply-add, fp32 accumulation:
                        fp32-level products, <= ~2^-23 relative, on the bf16 MFMA pipe).
                        anr_sdf_render_fwd: ANR_BF16X3 splits its layer GEMMs the same way (the
                        residual MLP as one fused launch). Other entry points treat ANR_BF16X3 /
                        ANR_BF16X6 as ANR_FP32. */
} anr_render_opts;

enum { ANR_FP32 = 0, ANR_BF16 = 1, ANR_BF16_ALL = 2, ANR_BF16X3 = 3, ANR_BF16X6 = 4 };

/* Outputs (device). raw may be NULL (then kept in the workspace). */
typedef struct anr_render_out {
  float* rgb_map;    /* (R,3) */
  float* acc_map;    /* (R)   */
  float* depth_map;  /* (R)   */
  float* raw;        /* (R*n_samples, 4) or NULL */
} anr_render_out;

/* ---- A14: ray / box intersection in float64 (bit-exact with numpy) ---------------------
 * rays (n,3) f32, bounds (2,3) f32 -> mask (n) u8, near/far (n) f32 at EVERY ray
 * (garbage where mask==0). */
int anr_near_far(const float* ray_o, const float* ray_d, int n, const float* bounds,
                 uint8_t* mask, float* near_, float* far_, void* stream);

/* ---- (f) eval-split ray pipeline: get_rays_within_bounds (if_nerf_data_utils.py:310-339) ------
 * get_rays (:64-89) for every pixel of an H x W camera, the A14 box test, and the ordered list of
 * the hit pixels (row-major, like np.argwhere). Kinv = np.linalg.inv(K) and origin = -R^T T are
 * passed in as the reference computes them on the host (LAPACK / BLAS results); fp64 selects the
 * float64 arithmetic of float64 camera annotations, else float32 (float32 cameras). Outputs
 * (device, capacity H*W): ray_o/ray_d (n,3), near/far (n), coord (n,2) (row, col), mask (H*W);
 * count (device int32) = n. */
size_t anr_camera_rays_workspace_bytes(int H, int W);
int anr_camera_rays(int H, int W, const double* Kinv, const double* R, const double* T, const double* origin, int fp64,
                    const float* bounds, float* ray_o, float* ray_d, float* near_, float* far_, int32_t* coord,
                    uint8_t* mask, int32_t* count, void* workspace, size_t ws_bytes, void* stream);

/* ---- (f) train-split ray sampler: sample_ray_h36m(split='train') (if_nerf_data_utils.py:198-283) ----
 * Replaces the float64 numpy sampler the reference runs in its DataLoader workers
 * (tpose_dataset.py:228). Two calls, both asynchronous on `stream`:
 *  anr_train_ray_lists: the pixel lists np.argwhere(msk == 1), (msk == 13), (bound_mask == 1) of
 *    :238-249 (row-major), after msk = msk * bound_mask and bound_mask[msk == 100] = 0 (:230-231).
 *    msk / bound_mask (H*W) u8 device; lists (3 * H*W) int32 device; counts (3) int32 device.
 *  anr_train_ray_gather: one round of the sampling loop (:236-271). draws (n_body + n_face + n_rand)
 *    int32 device = the np.random.randint draws into lists 0, 1, 2 in that order (the caller makes
 *    them with numpy, so the random stream is the reference's); per draw get_rays (:64-89) at the
 *    pixel, get_near_far (:156-196) on get_rays' arrays (float64 for a float64 camera), rgb = img
 *    (H*W,3) f32, zero outside bound_mask when mask_bkgd (:228). Hits are appended in draw order
 *    at index *n_out (device int32, updated), at most cap; outputs ray_o/ray_d/rgb (cap,3),
 *    near/far (cap), coord (cap,2) (row, col). Camera arguments as anr_camera_rays. */
size_t anr_train_ray_workspace_bytes(int H, int W);
int anr_train_ray_lists(int H, int W, const uint8_t* msk, const uint8_t* bound_mask, int32_t* lists, int32_t* counts,
                        void* workspace, size_t ws_bytes, void* stream);
int anr_train_ray_gather(int H, int W, const double* Kinv, const double* R, const double* T, const double* origin,
                         int fp64, const float* bounds, const float* img, const uint8_t* bound_mask, int mask_bkgd,
                         const int32_t* lists, const int32_t* draws, int n_body, int n_face, int n_rand, int cap,
                         float* ray_o, float* ray_d, float* rgb, float* near_, float* far_, int32_t* coord,
                         int32_t* n_out, void* stream);

/* ---- (f) train-split ray sampler, whole loop on the device -------------------------------------
 * anr_train_ray_sample replaces the loop `while nsampled < nrays` of sample_ray_h36m(split='train')
 * (if_nerf_data_utils.py:236-271) and the occupancy lookup of tpose_dataset.py:233 with ONE launch
 * of one 1024-thread workgroup: no host sync, no host RNG, no H2D copy between training steps.
 *  Inputs (device unless said): camera arguments as anr_camera_rays; img (H*W,3) f32; bound_mask
 *    (H*W) u8, the one anr_train_ray_lists saw; occ_mask (H*W) u8 or NULL; list_body / list_face /
 *    list_bound = the used prefixes of anr_train_ray_lists' three lists, their lengths n_body_px /
 *    n_face_px / n_bound_px by value (an empty list may be NULL).
 *  Per round, with rem = nrays - (rays so far): n_body = (int)((double)rem * body_ratio), n_face =
 *    (int)((double)rem * face_ratio), n_rand = rem - n_body - n_face. An empty face list
 *    gets no slots but n_rand keeps the subtraction above (the reference then concatenates body and
 *    random draws only). Slots i = 0.. run over [body, face, rand]; slot i of round r draws
 *        x = word (i & 3) of Philox4x32-10(counter = (i >> 2, r, step_lo, step_hi), key = (seed_lo, seed_hi))
 *        index = ((uint64)x * n_list) >> 32
 *    which is uniform over the slot's list up to a relative bias of at most n_list / 2^32. Per slot
 *    the work is anr_train_ray_gather's (get_rays, box test in the camera's precision, rgb with the
 *    mask_bkgd zeroing), hits appended in slot order.
 *  Ends when nrays rays are in, or after max_rounds rounds (1..1024; the reference's loop is
 *    unbounded). *n_out (device int32) = rays sampled. Rows >= n_out are filled as rays the training
 *    losses skip: mask_at_box 0, ray_o = origin, ray_d = (0,0,1), near = far = 0, rgb = 0, coord = 0,
 *    occupancy = 0; *shortfall (device int32, accumulating: zero it once) += nrays - n_out.
 *  Outputs: ray_o/ray_d/rgb (nrays,3) f32, near/far (nrays) f32, coord (nrays,2) int32 (row, col),
 *    mask_at_box (nrays) u8, occupancy (nrays) u8 (NULL exactly when occ_mask is).
 *  ANR_E_ARG before any HIP call for: a NULL pointer, nrays outside 1..65536, max_rounds outside
 *    1..1024, a ratio outside [0,1] or body_ratio + face_ratio > 1, n_bound_px <= 0, n_body_px <= 0
 *    with body_ratio > 0. Multi-process training: fold the rank into seed. */
int anr_train_ray_sample(int H, int W, const double* Kinv, const double* R, const double* T, const double* origin,
                         int fp64, const float* bounds, const float* img, const uint8_t* bound_mask,
                         const uint8_t* occ_mask, const int32_t* list_body, const int32_t* list_face,
                         const int32_t* list_bound, int n_body_px, int n_face_px, int n_bound_px, int mask_bkgd,
                         double body_ratio, double face_ratio, int nrays, int max_rounds, uint64_t seed, uint64_t step,
                         float* ray_o, float* ray_d, float* rgb, float* near_, float* far_, int32_t* coord,
                         uint8_t* mask_at_box, uint8_t* occupancy, int32_t* n_out, int32_t* shortfall, void* stream);

/* ---- weights --------------------------------------------------------------------------- */
size_t anr_params_packed_bytes(void);
int anr_params_pack(const anr_params* p, void* packed, void* stream);

/* ---- render ---------------------------------------------------------------------------- */
size_t anr_render_workspace_bytes(int n_rays, const anr_render_opts* o, const anr_frame* f);
int anr_render_fwd(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d,
                   const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                   const anr_render_out* out, void* workspace, size_t ws_bytes, void* stream);
/* device int32[2] inside the workspace: {kept points n', alpha_ind rows m}. */
const int32_t* anr_render_counts(const void* workspace, int n_rays);
/* Gather the m alpha_ind rows of pbw / tbw (each (m,24)) after the counts were read. */
int anr_render_bw_rows(const void* workspace, int n_rays, float* pbw, float* tbw, void* stream);
/* The sample id (ray * N_samples + sample, frame order) of each of the m alpha_ind rows, ids (m) int32:
 * which samples tpose_nerf_network.py:192-196 selected (rows compared by sample in tests). */
int anr_render_row_ids(const void* workspace, int n_rays, int32_t* ids, void* stream);

/* ---- image-only render --------------------------------------------------------------------
 * anr_render_fwd for callers that want images and no training rows (evaluation, novel views,
 * visualisation): the same rgb_map / acc_map / depth_map / raw, bit for bit, from the image render
 * program, which leaves out the T-pose blend-weight MLP (tpose_nerf_network.py:170-174; it only fills
 * the tbw rows of the loss) and the alpha_ind stage. The visibility filter (f->n_views), novel_pose,
 * t_rand and the three render precisions work as in anr_render_fwd.
 *  f->tbw and f->tbw_dims are not read (NULL / zeros are fine); f->tbounds is (the T-pose bbox mask).
 *  The workspace has a smaller layout of its own (no pbw / tbw rows, no row bookkeeping, no tbw copy).
 *    anr_render_counts works on it: entry 0 is the kept count, entry 1 is 0. anr_render_bw_rows and
 *    anr_render_row_ids are invalid on an image workspace (there are no rows).
 *  anr_render_image_workspace_bytes returns 0 for NULL o / f, n_rays <= 0, o->chunk <= 0 or a
 *    non-positive pbw dim.
 *  ANR_E_ARG / ANR_E_WORKSPACE before any HIP call, for what anr_render_fwd rejects minus tbw. */
size_t anr_render_image_workspace_bytes(int n_rays, const anr_render_opts* o, const anr_frame* f);
int anr_render_image_fwd(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d,
                         const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                         const anr_render_out* out, void* workspace, size_t ws_bytes, void* stream);

/* ---- render with 64, 128, 192 or 256 samples per ray ------------------------------------------
 * anr_render_fwd (image_only = 0) and anr_render_image_fwd (image_only != 0) for o->n_samples = 64 k,
 * k = 1..4 (cfg.N_samples, tpose_renderer.py:26): the same programs, outputs and argument rules, with
 * raw (R * n_samples, 4), o->t_rand (R, n_samples), sample ids ray * n_samples + sample and the
 * reference's per-chunk forced argmin / argmax over chunk * n_samples samples. At n_samples = 64 every
 * output equals the 64-sample entries' bit for bit, and so do the workspace sizes. The visibility
 * filter, novel_pose, t_rand and the three render precisions work as there.
 *  Any other n_samples: ANR_E_ARG ("N_samples must be 64, 128, 192 or 256"); the size query returns 0.
 *  One call takes 24 * n_rays * n_samples < 2^31 (a 512 x 512 frame at 256 samples fits).
 *  The workspace scales with n_rays * n_samples wherever anr_render_fwd's scales with n_rays * 64; the
 *    pbw / tbw rows (192 B per sample) dominate the full program's, which the image-only one does not
 *    have. anr_render_counts works on it (pass any n_rays).
 *  anr_render_ns_bw_rows / anr_render_ns_row_ids: anr_render_bw_rows / anr_render_row_ids on a full
 *    (image_only = 0) workspace of this entry; ids are ray * n_samples + sample.
 *  ANR_E_ARG / ANR_E_WORKSPACE before any HIP call. Training, the animation stage and the sdf_pdf
 *  programs take 64 samples only. */
size_t anr_render_ns_workspace_bytes(int n_rays, const anr_render_opts* o, const anr_frame* f, int image_only);
int anr_render_ns_fwd(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d,
                      const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                      const anr_render_out* out, int image_only, void* workspace, size_t ws_bytes, void* stream);
int anr_render_ns_bw_rows(const void* workspace, int n_rays, int n_samples, float* pbw, float* tbw, void* stream);
int anr_render_ns_row_ids(const void* workspace, int n_rays, int n_samples, int32_t* ids, void* stream);

/* ---- Network.forward over free samples (tpose_nerf_network.py:139-215) ----------------------
 * The call a reference renderer makes per chunk, self.net(wpts, viewdir, dists, batch)
 * (tpose_renderer.py:95): n_pts samples given by world points wpts (n,3), view directions viewdir
 * (n,3) and interval lengths dists (n). The prefilter's forced argmin and the alpha_ind argmax run
 * over the whole call, as the reference's pnorm.argmin(dim=1) / argmax(alpha, dim=1) do (one call =
 * one reference chunk); o->chunk and o->t_rand are ignored. raw (n,4) is zero at dropped samples
 * (raw_full). anr_network_counts: device int32 {kept n', alpha_ind rows m} in the workspace;
 * anr_network_bw_rows: the m rows of pbw / tbw (each (m,24)) after the counts were read; both work on
 * either workspace below.
 *  anr_network_fwd: the fused network kernel (o->precision ANR_FP32 or ANR_BF16X3), no host sync.
 *  anr_network_train_fwd / _bwd: the layer-wise training executor (o->precision as for training),
 *    activations kept in the workspace until the backward; n' stays on the device (no host sync). _bwd
 *    ACCUMULATES the parameter gradients (anr_params order) from the upstream d raw (n,4) and d pbw /
 *    d tbw rows (m,24); any of the three may be NULL (zero). */
typedef struct anr_samples {
  const float* wpts;     /* (n,3) device, world frame */
  const float* viewdir;  /* (n,3) device */
  const float* dists;    /* (n) device */
  int n_pts;
} anr_samples;
size_t anr_network_workspace_bytes(int n_pts, const anr_render_opts* o, const anr_frame* f);
int anr_network_fwd(const anr_params* p, const anr_frame* f, const anr_samples* x, const anr_render_opts* o, float* raw,
                    void* workspace, size_t ws_bytes, void* stream);
const int32_t* anr_network_counts(const void* workspace, int n_pts);
int anr_network_bw_rows(const void* workspace, int n_pts, float* pbw, float* tbw, void* stream);
size_t anr_network_train_workspace_bytes(int n_pts, const anr_render_opts* o, const anr_frame* f);
int anr_network_train_fwd(const anr_params* p, const anr_frame* f, const anr_samples* x, const anr_render_opts* o,
                          float* raw, void* workspace, size_t ws_bytes, void* stream);
int anr_network_train_bwd(const anr_params* p, float* const* grads, const anr_frame* f, const anr_samples* x,
                          const anr_render_opts* o, const float* d_raw, const float* d_pbw, const float* d_tbw,
                          void* workspace, size_t ws_bytes, void* stream);

/* ---- network helpers the reference's other trainers / renderers call --------------------------
 * anr_blend_weights: field 0 = calculate_neural_blend_weights(pts, smpl_bw, latent_index)
 *   (tpose_nerf_network.py:55-77; bw_latent, bw_linears, bw_fc), field 1 = novel_pose_bw(pts, smpl_bw,
 *   latent_index) (BackwardBlendWeight.forward :304-315): pts (n,3), smpl_bw (24,n) (the reference's
 *   (1,24,n)) -> bw (24,n) = softmax(log(smpl_bw + 1e-9) + MLP([gamma(pts), latent row])), latent row =
 *   latent_row[0] + row_add (latent_row: device int64, the caller's index tensor).
 * anr_canonical_alpha: TPoseHuman.calculate_alpha(nf_pts) (:241-250): raw alpha (n) of canonical points.
 * Forward only, exact fp32 MFMA layer GEMMs, no host sync. */
size_t anr_points_workspace_bytes(int n);
int anr_blend_weights(const anr_params* p, int field, const float* pts, const float* smpl_bw, int n,
                      const int64_t* latent_row, int row_add, float* bw, void* workspace, size_t ws_bytes, void* stream);
int anr_canonical_alpha(const anr_params* p, const float* pts, int n, float* alpha, void* workspace, size_t ws_bytes,
                        void* stream);

/* ---- training (A16/A17; lib/train/trainers/tpose_trainer.py:21-73, trainer.py:50-68) ------
 * anr_train_fwd: the render forward of the training step (perturb via o->t_rand), keeping every
 *   activation in the workspace; same outputs as anr_render_fwd (+ anr_render_counts /
 *   anr_render_bw_rows on this workspace). Reads the kept-sample count once (host sync).
 * anr_train_bwd: given upstream gradients d rgb_map (R,3) and d pbw / d tbw rows (m,24) (any may
 *   be NULL = zero), ACCUMULATES parameter gradients into grads[ANR_NUM_TENSORS] (state_dict
 *   order, same shapes as anr_params.t) — what loss.backward() does in the reference.
 * anr_train_step: forward + the reference losses (img MSE over mask_at_box rays + smooth-L1 of
 *   the pbw/tbw rows; loss3 = {loss, img_loss, bw_loss} on device) + backward, one call.
 * anr_adam: clip_grad_value_(clip) then torch.optim.Adam on a flat parameter blob (trainer.py:64-68). */
size_t anr_train_workspace_bytes(int n_rays, const anr_render_opts* o, const anr_frame* f);
int anr_train_fwd(const anr_params* p, const anr_frame* f, const float* ray_o, const float* ray_d,
                  const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                  const anr_render_out* out, void* workspace, size_t ws_bytes, void* stream);
int anr_train_bwd(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o,
                  const float* ray_d, const float* near_, const float* far_, int n_rays,
                  const anr_render_opts* o, const float* d_rgb_map, const float* d_pbw, const float* d_tbw,
                  void* workspace, size_t ws_bytes, void* stream);
int anr_train_step(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o,
                   const float* ray_d, const float* near_, const float* far_, int n_rays,
                   const anr_render_opts* o, const float* rgb_gt, const uint8_t* mask_at_box,
                   const anr_render_out* out, float* loss3, void* workspace, size_t ws_bytes, void* stream);
/* anr_train_step_hooked: anr_train_step plus events for overlapping the gradient all-reduce with
 * the backward (DDP's reverse-order buckets): nerf_grads_ready (a hipEvent_t or
 * NULL) is recorded on the stream once the gradients of tensors 0..26 (tpose_human.*, the canonical
 * NeRF) are final; the blend-weight backward (tensors 27..45) follows on the stream. */
typedef int (*anr_reduce_fn)(void* user, void* device_buf, int count, int op, void* stream);
#define ANR_REDUCE_MIN_U64 0 /* unsigned 64-bit keys, min over ranks (all-ones = empty) */
#define ANR_REDUCE_MAX_U64 1 /* unsigned 64-bit keys, max over ranks */
#define ANR_REDUCE_SUM_F32 2 /* float sums over ranks */
/* struct_size must be sizeof(anr_train_hooks) (ANR_TRAIN_HOOKS_VERSION 2, anr_version() >= 2): the struct
 * grew from version 1's single nerf_grads_ready field, and a caller built against another layout is
 * rejected with ANR_E_ARG instead of having its memory read as the newer fields. */
#define ANR_TRAIN_HOOKS_VERSION 2
typedef struct anr_train_hooks {
  size_t struct_size;
  void* nerf_grads_ready;
  /* Ray split of ONE reference chunk over ranks (north_star "rays-per-iteration shard"; strong scaling of
   * a 1,024-ray step): this call's rays are rays [ray_offset, ray_offset + n_rays) of a
   * batch that is a single reference chunk (ray_offset + n_rays <= o->chunk). The chunk-wide decisions are
   * exchanged through reduce (NULL: no split), which the library calls on the host, in issue order, with
   * a device buffer of the workspace; it must make `stream` wait for the reduction over all ranks (e.g. an
   * RCCL all-reduce on that stream): the per-chunk argmin key of the prefilter (tpose_nerf_network.py:154,
   * MIN_U64) before compaction, the per-chunk argmax key of sigma' (:193-194, MAX_U64) before the
   * alpha_ind rows are flagged, and the loss sums {squared error, mask rays, smooth-L1 sum, alpha_ind
   * rows} (SUM_F32) before the loss and its gradients. Losses are then the batch's on every rank and
   * the gradients are this rank's share of the batch gradient (sum them over ranks). */
  int ray_offset;
  anr_reduce_fn reduce;
  void* reduce_user;
} anr_train_hooks;
int anr_train_step_hooked(const anr_params* p, float* const* grads, const anr_frame* f, const float* ray_o,
                          const float* ray_d, const float* near_, const float* far_, int n_rays,
                          const anr_render_opts* o, const float* rgb_gt, const uint8_t* mask_at_box,
                          const anr_render_out* out, float* loss3, const anr_train_hooks* hooks, void* workspace,
                          size_t ws_bytes, void* stream);
/* anr_train_deterministic: the process-wide deterministic training mode (default 0). on = 1 / 0 sets it,
 * on = -1 only queries; the return value is the mode in force BEFORE the call (0 or 1). Any other
 * argument changes nothing and returns -ANR_E_ARG (negative, so it cannot be mistaken for a mode; the text
 * via anr_last_error()). It makes no HIP call. The environment variable ANR_TRAIN_DETERMINISTIC=1|0, read
 * at every training call, wins over the setter when it is set (precedence: environment, then this setter,
 * then a binding's own default such as the Python cfg key train_deterministic).
 * With the mode on, anr_train_step(_hooked), anr_train_bwd, anr_network_train_bwd and anr_anim_step
 * produce gradients, loss3 and (through anr_adam) weights that are a function of the parameters, the batch,
 * t_rand, the precision, the shapes and the gradient buffers' contents on entry only: bit-identical from
 * run to run and whatever streams the executor uses (ANR_TRAIN_SERIAL, ANR_TRAIN_ON_CALLER, ANR_TRAIN_GRAPH).
 * The sdf_pdf trainer honours the mode in the same way: anr_sdf_train_step(_hooked) and
 * anr_sdf_network_train_bwd read it once per call, and their 63 gradients and the loss vector (both
 * precisions, ANR_FP32 and ANR_BF16X3) then depend on those inputs and iter_step only. They run on the
 * caller's stream alone; ANR_SDF_WG32=0 and ANR_SDF_LG32=0 select other kernels with another summation
 * tree, each reproducible against itself.
 * Every weight-gradient product and its reduction then run on one stream in issue order and every float
 * sum has a fixed order (no floating-point atomics); switches that change the summation tree itself
 * (ANR_WG_GROUP, ANR_WG_DMA, ANR_WG_GROUP_NZ, ANR_WG_FILL, ANR_WG_FLUSH_EVERY, the chain switches) give
 * another, equally reproducible, result. With the mode off nothing changes.
 * Not covered: under a ray split (anr_train_hooks.reduce), and with several ranks all-reducing the sdf_pdf
 * gradient blob, the result is deterministic only if the caller's all-reduce is. */
int anr_train_deterministic(int on);
int anr_adam(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
             float beta2, float eps, float weight_decay, int step, float clip_value, void* stream);

/* ---- (f) animation stage (lib/train/trainers/aninerf_animation_trainer.py:33-140) -------------
 * anr_anim_step: NetworkWrapper.forward + loss.backward of the second training stage, which fits
 *   novel_pose_bw with every other parameter frozen. wpts (n_obs,3): points drawn in wbounds
 *   (observation space, world frame; get_sampling_points :143-160); tpts (n_can,3): points drawn in
 *   tbounds (canonical). Path 1 (ppts_to_tpose :63-99): pbw0 = novel_pose_bw at the posed point,
 *   tbw0 = the frozen blend-weight MLP at its LBS-inverse T-pose point (differentiable through x_T),
 *   rows where alpha (zeroed outside tbounds or pnorm >= o->norm_th) > o->train_th plus the argmax.
 *   Path 2 (tpose_to_ppts :102-131): tbw1 frozen at the canonical point, pbw1 = novel_pose_bw at its
 *   forward-LBS posed point, rows alpha > train_th plus the argmax. loss3 = {bw_loss0 + bw_loss1,
 *   bw_loss0, bw_loss1} (smooth_l1 means, device). ACCUMULATES the gradients of the 19
 *   novel_pose_bw tensors into grads (anr_params.novel order). Reads frame A, R, Th, pbw, pbounds,
 *   tbw, tbounds, bw_latent_index; o->precision as for training (ANR_BF16 keeps the pose-space
 *   novel_pose_bw MLP fp32). No host sync. */
size_t anr_anim_workspace_bytes(int n_points);
int anr_anim_step(const anr_params* p, float* const* grads, const anr_frame* f, const float* wpts, int n_obs,
                  const float* tpts, int n_can, const anr_render_opts* o, float* loss3, void* workspace,
                  size_t ws_bytes, void* stream);

/* ---- sdf_pdf variant (config 5, anisdf_pdf_network.py) ------------------------------------
 * Parameters: the 63 tensors of anisdf_pdf_network.Network's state_dict, in order:
 *   0..26  tpose_human.sdf_network.lin{0..8}.{bias, weight_g (o,1), weight_v (o,i)}
 *          i/o: 39/256, 256/256, 256/256, 256/217, 256/256 x4, 256/257
 *   27     tpose_human.beta_network.beta ()
 *   28     tpose_human.color_network.color_latent.weight (L,128)
 *   29..43 tpose_human.color_network.lin{0..4}.{bias, weight_g, weight_v}  i: 289,256,256,384,256
 *   44     resd_latent.weight (L,128)            (not read by the render)
 *   45..60 resd_linears.{0..7}.{weight,bias}     Conv1d, in: 135,256,256,256,256,391,256,256
 *   61,62  resd_fc.{weight,bias} (3,256,1)                                                   */
#define ANR_SDF_NUM_TENSORS 63

typedef struct anr_sdf_params {
  const float* t[ANR_SDF_NUM_TENSORS];  /* device pointers, state_dict order above */
} anr_sdf_params;

typedef struct anr_sdf_frame {
  const float* A;          /* (24,4,4) device */
  const float* big_A;      /* (24,4,4) device: big pose (tpose_pdf_dataset.py:91-100) */
  const float* R;          /* (3,3) */
  const float* Th;         /* (3) */
  const float* poses;      /* (72) batch['poses'] */
  const float* pvertices;  /* (V,3) posed SMPL vertices in the pose frame, V <= 6912 */
  const float* weights;    /* (V,24) skin weights */
  int n_verts;
  const float* tbounds;    /* (2,3) batch['tbounds'] as passed in */
  const int64_t* latent_index;  /* (1) colour latent row */
  const uint8_t* occupancy;     /* (R) batch['occupancy'] */
  /* novel-view visibility filter of tpose_renderer_mmsk (:14-57, the config-5 novel_view_cfg /
   * pose_sequence_cfg renderer over this network), anr_sdf_render_fwd only; n_views = 0 disables it. A
   * sample reaches the network only if it projects inside every training view's mask: the KNN keep and
   * the per-chunk forced argmin range over the visible samples (one Network.forward call per chunk on
   * them), and tbounds widens only at chunks with a visible sample (a chunk without one makes no call). */
  int n_views;
  const float* Ks;         /* (V,3,3) device */
  const float* RT;         /* (V,3,4) device, world -> camera */
  const uint8_t* msks;     /* (V,img_h,img_w) device */
  int img_h, img_w;
} anr_sdf_frame;

typedef struct anr_sdf_render_out {
  float* rgb_map;      /* (R,3) */
  float* acc_map;      /* (R) */
  float* depth_map;    /* (R) */
  float* raw;          /* (R*64,4) */
  float* sdf;          /* (R*64) (10 at samples the KNN filter drops) */
  float* tbounds_out;  /* (2,3) or NULL: batch['tbounds'] after the reference's in-place widening
                          by 0.05 per chunk (anisdf_pdf_network.py:203-205) */
} anr_sdf_render_out;

/* o->norm_th is the KNN distance threshold (0.1 in the reference, :172). Reads the kept-sample
 * count once (host sync) to size the layer GEMMs. Eval path: the training-only
 * 'observed_gradients' (:187-193) are not produced. */
size_t anr_sdf_render_workspace_bytes(int n_rays, const anr_render_opts* o);
int anr_sdf_render_fwd(const anr_sdf_params* p, const anr_sdf_frame* f, const float* ray_o, const float* ray_d,
                       const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                       const anr_sdf_render_out* out, void* workspace, size_t ws_bytes, void* stream);
/* device int32[2] inside the workspace: {kept samples n', msk_sdf length}. */
const int32_t* anr_sdf_render_counts(const void* workspace, int n_rays, const anr_render_opts* o);
/* device uint32 (R*64, 8) inside the workspace: the front-end's per-sample KNN records (w0..w4 float
 * bits, i0 | i1 << 16, i2 | i3 << 16, i4) of the last anr_sdf_render_fwd -- a debugging / test view of
 * the pytorch3d knn_points boundary (sample_utils.py:309-348). */
const uint32_t* anr_sdf_render_knn(const void* workspace, int n_rays, const anr_render_opts* o);
/* copy resd (n',3), gradients (n',3), msk_sdf / msk_label (len) out of the workspace */
int anr_sdf_render_rows(const void* workspace, int n_rays, const anr_render_opts* o, float* resd, float* gradients,
                        float* msk_sdf, float* msk_label, void* stream);

/* ---- sdf_pdf Network.forward over free samples (anisdf_pdf_network.py:156-224) -----------------
 * The call tpose_renderer makes per chunk over the sdf_pdf network, self.net(wpts, viewdir, dists,
 * batch) (tpose_renderer.py:95; configs/sdf_pdf/anisdf_pdf_s9p.yaml:9-12): x->n_pts samples (world
 * points, world view directions; dists is not read: the Laplace density uses the constant 0.005,
 * :330). One call = one reference chunk: the KNN prefilter keeps pnorm < o->norm_th (0.1) plus the
 * argmin of pnorm over the call, and batch['tbounds'] is widened ONCE (tbounds_out, or NULL).
 * world -> pose follows torch's matmul rule for an (n_pts, 3) product (n_pts < 45: its small path).
 *  anr_sdf_network_fwd: evaluation (no observed_gradients), o->precision ANR_FP32 or ANR_BF16X3 as the
 *    sdf render; raw (n,4) zero at dropped samples and outside the widened tbounds, sdf (n) = 10 at
 *    dropped samples. Reads the kept count once (host sync).
 *  anr_sdf_network_counts: device int32 {kept n', 0}; anr_sdf_network_rows: resd (n',3) and gradients
 *    (n',3) of the kept samples, in sample order. */
size_t anr_sdf_network_workspace_bytes(int n_pts, const anr_render_opts* o);
int anr_sdf_network_fwd(const anr_sdf_params* p, const anr_sdf_frame* f, const anr_samples* x, const anr_render_opts* o,
                        float* raw, float* sdf, float* tbounds_out, void* workspace, size_t ws_bytes, void* stream);
const int32_t* anr_sdf_network_counts(const void* workspace, int n_pts);
int anr_sdf_network_rows(const void* workspace, int n_pts, float* resd, float* gradients, void* stream);
/* Under autograd (the reference's training forward, :187-199): the layer-wise exact-fp32 executor of
 * anr_sdf_train_step over the call's samples.
 *  anr_sdf_network_train_fwd: as anr_sdf_network_fwd plus 'observed_gradients' = d sdf(x + resd(x)) / d x
 *    at the kept samples with |sdf| < 0.02 (x = init_bigpose, :140-154). Two host reads (counts).
 *  anr_sdf_network_train_counts: device int32 {kept n', 0, observed rows n_o, 0}.
 *  anr_sdf_network_train_rows: resd (n',3), gradients (n',3), observed_gradients (n_o,3) (any NULL: skipped).
 *  anr_sdf_network_train_bwd: loss.backward() through the call: ACCUMULATES into grads (anr_sdf_params
 *    order; resd_latent may be NULL) the parameter gradients of the upstream adjoints d raw (n,4),
 *    d sdf (n), d resd (n',3), d gradients (n',3), d observed_gradients (n_o,3) (any NULL = 0), with the
 *    second-order terms the reference's create_graph=True input gradients carry. It re-runs the forward
 *    on the same workspace first, so f->tbounds must hold the bounds the forward call was given (before
 *    its widening). With the deterministic training mode on (anr_train_deterministic) every sum of the
 *    backward has a fixed order.
 *  anr_sdf_network_train_workspace_bytes: the same size in both training modes; it includes the
 *    deterministic mode's scratch (per-split and per-block partials), since ANR_TRAIN_DETERMINISTIC can
 *    switch the mode at any call. It makes no HIP call. */
size_t anr_sdf_network_train_workspace_bytes(int n_pts);
int anr_sdf_network_train_fwd(const anr_sdf_params* p, const anr_sdf_frame* f, const anr_samples* x,
                              const anr_render_opts* o, float* raw, float* sdf, float* tbounds_out, void* workspace,
                              size_t ws_bytes, void* stream);
const int32_t* anr_sdf_network_train_counts(const void* workspace, int n_pts);
int anr_sdf_network_train_rows(const void* workspace, int n_pts, float* resd, float* gradients,
                               float* observed_gradients, void* stream);
int anr_sdf_network_train_bwd(const anr_sdf_params* p, float* const* grads, const anr_sdf_frame* f, const anr_samples* x,
                              const anr_render_opts* o, const float* d_raw, const float* d_sdf, const float* d_resd,
                              const float* d_gradients, const float* d_observed_gradients, void* workspace,
                              size_t ws_bytes, void* stream);

/* ---- sdf_pdf point helpers (the sdf mesh path, lib/networks/renderer/sdf_mesh_renderer.py:16-110) ----
 * anr_sdf_points over n free points x (n,3) in the big-pose (canonical) space, exact fp32 products on the
 * sdf training executor's layers (weight norm formed per call; f needs poses and latent_index only):
 *   ANR_SDFP_NETWORK            tpose_human.sdf_network(x, batch) (anisdf_pdf_network.py:421-437):
 *                               out (n,257) = [sdf || feature vector] (scale 1)
 *   ANR_SDFP_GRADIENT           SDFNetwork.gradient(x) (:441-451): out (n,3) d sdf / d x, out2 (n) sdf (or NULL)
 *   ANR_SDFP_DEFORMED_GRADIENT  Network.gradient_of_deformed_sdf(x, batch) (:140-154): out (n,3) the gradient
 *                               of sdf(x + resd(x)) w.r.t. x (residual MLP included), out2 (n) that sdf (or NULL)
 * The host reads nothing; the call is asynchronous on the stream. */
#define ANR_SDFP_NETWORK 0
#define ANR_SDFP_GRADIENT 1
#define ANR_SDFP_DEFORMED_GRADIENT 2
size_t anr_sdf_points_workspace_bytes(int n);
int anr_sdf_points(const anr_sdf_params* p, const anr_sdf_frame* f, const float* x, int n, int mode, float* out,
                   float* out2, void* workspace, size_t ws_bytes, void* stream);
/* sample_blend_closest_points (lib/utils/sample_utils.py:323-348) of n free points against nv vertices
 * (nv, 3) with their weights (nv, 24): the render front-end's exact 5-NN (lexicographic (d^2, index) ties)
 * and inverse-distance blend. bw (n, 24) the blended weights and / or inside (n) = weighted distance
 * < norm_th (no forced argmin: the sdf mesh path's filter, sdf_mesh_renderer.py:58-60). */
size_t anr_knn_blend_workspace_bytes(int n);
int anr_knn_blend(const float* verts, const float* weights, int nv, const float* pts, int n, float norm_th, float* bw,
                  uint8_t* inside, void* workspace, size_t ws_bytes, void* stream);
/* The sdf mesh path's posed vertices (sdf_mesh_renderer.py:96-101): pose_points_to_tpose_points(pts, bw,
 * big_A), tpose_points_to_pose_points(., bw, A), pose_points_to_world_points(., R, Th) -> out (n, 3). */
int anr_sdf_mesh_pose(const float* pts, const float* bw, int n, const float* big_A, const float* A, const float* R,
                      const float* Th, float* out, void* stream);
/* pts_sample_blend_weights (lib/utils/blend_utils.py:119-149; Network.calculate_bigpose_smpl_bw,
 * anisdf_pdf_network.py:109-112): trilinear grid_sample (align_corners, border padding) of the volume vol
 * (X,Y,Z,C) over bounds (2,3) at pts (n,3) -> out (C, n), the reference's (1, 25, n) without the batch axis,
 * bit-exact in the reference's CPU accumulation order. */
int anr_sample_volume(const float* vol, int X, int Y, int Z, int C, const float* bounds, const float* pts, int n,
                      float* out, void* stream);

/* ---- sdf_pdf training (config 5; lib/train/trainers/tpose_trainer.py:21-73, crit.py:5-19) ---------
 * anr_sdf_train_step: NetworkWrapper.forward + loss.backward() of one batch through the sdf_pdf
 *   network and tpose_renderer (anisdf_pdf_network.py:156-224 in training mode: gradients with
 *   create_graph, observed_gradients at the kept samples with |sdf| < 0.02), then the losses
 *   offset 0.01 mean|resd|, eikonal 0.01 mean(|g|-1)^2 (gradients and observed_gradients), msk_sdf
 *   BCE (alpha 50 doubled past iteration 10k, 20k, ... as crit.sdf_mask_crit) and the image MSE over
 *   mask_at_box (NULL: every ray). ACCUMULATES the gradients of every tensor of anr_sdf_params into
 *   grads (state_dict order; resd_latent, never read, may be NULL). loss (device float[10]) = {loss,
 *   offset_loss, grad_loss, ograd_loss, mask_loss, img_loss, observed rows, msk_sdf entries, kept
 *   samples, 0}.
 *   out: rgb_map / acc_map / depth_map (R), tbounds_out (widened) or NULL; raw / sdf unused.
 *   Perturbation through o->t_rand; o->norm_th = 0.1. Two host reads (kept and observed counts).
 *   With the deterministic training mode on (anr_train_deterministic) the gradients and the loss vector
 *   are bit-identical from run to run.
 * anr_sdf_train_workspace_bytes: the same size in both training modes; it includes the deterministic
 *   mode's scratch (about 1 % of the total), since ANR_TRAIN_DETERMINISTIC can switch the mode at any
 *   call. It makes no HIP call. */
size_t anr_sdf_train_workspace_bytes(int n_rays, const anr_render_opts* o);
int anr_sdf_train_step(const anr_sdf_params* p, float* const* grads, const anr_sdf_frame* f, const float* ray_o,
                       const float* ray_d, const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                       const float* rgb_gt, const uint8_t* mask_at_box, int iter_step, const anr_sdf_render_out* out,
                       float* loss, void* workspace, size_t ws_bytes, void* stream);
/* anr_sdf_train_step_hooked: anr_sdf_train_step plus a hook for overlapping the gradient all-reduce
 * with the rest of the backward (DDP's buckets, trainer.py:13-18). Once the gradients of tensors 28..43
 * (color_network.*, colour latent included) are final, colour_grads_ready (a hipEvent_t, or NULL) is
 * recorded on the stream and then colour_ready (or NULL) is called on the host with that event and the
 * stream, while the SDF's stacked reverse, the residual backward and the observed-gradient passes
 * (tensors 0..27, 45..62) are still to be issued: the caller issues the colour bucket's collective there
 * (ordered after the event) and it runs beside them. A non-zero return from colour_ready fails the call.
 * struct_size must be sizeof(anr_sdf_train_hooks). hooks == NULL: anr_sdf_train_step. */
typedef int (*anr_ready_fn)(void* user, void* event, void* stream);
typedef struct anr_sdf_train_hooks {
  size_t struct_size;
  void* colour_grads_ready;
  anr_ready_fn colour_ready;
  void* user;
} anr_sdf_train_hooks;
int anr_sdf_train_step_hooked(const anr_sdf_params* p, float* const* grads, const anr_sdf_frame* f,
                              const float* ray_o, const float* ray_d, const float* near_, const float* far_,
                              int n_rays, const anr_render_opts* o, const float* rgb_gt, const uint8_t* mask_at_box,
                              int iter_step, const anr_sdf_render_out* out, float* loss,
                              const anr_sdf_train_hooks* hooks, void* workspace, size_t ws_bytes, void* stream);

/* ---- (f) mesh path (lib/networks/renderer/aninerf_mesh_renderer.py) ----------------------
 * anr_alpha_points: raw alpha (no activation, no bbox mask) of n free world points, zero where the
 *   pbw prefilter drops the point: pnorm < o->norm_th (0.1 in get_alpha) plus the argmin of pnorm
 *   over each chunk of o->chunk_pts points (2048 * 64 in the reference; a multiple of 64). Uses
 *   the pose-space BW MLP (or novel_pose_bw with o->novel_pose), the LBS inverse, the NeRF trunk
 *   and alpha_fc; o->precision ANR_FP32 (exact fp32 MFMA) or ANR_BF16X3. Frame fields read: A, R,
 *   Th, pbw(+dims), pbounds, latent_index (bw_latent_index for novel_pose). No host sync.
 *   anr_alpha_counts: device int32 {kept points} inside the workspace. */
typedef struct anr_alpha_opts {
  int chunk_pts;   /* points per reference chunk (2048 * 64) */
  float norm_th;   /* 0.1 (tpose_nerf_network.py:113) */
  int novel_pose;  /* cfg.test_novel_pose */
  int precision;   /* ANR_FP32 or ANR_BF16X3 */
} anr_alpha_opts;
size_t anr_alpha_workspace_bytes(long n_pts, const anr_alpha_opts* o, const anr_frame* f);
int anr_alpha_points(const anr_params* p, const anr_frame* f, const float* wpts, long n_pts, const anr_alpha_opts* o,
                     float* alpha, void* workspace, size_t ws_bytes, void* stream);
const int32_t* anr_alpha_counts(const void* workspace);
/* Marching cubes over vol (X,Y,Z) f32 padded by `pad` zero voxels on every side (virtually):
 * anr_mc_count writes device int32 {V, T} to counts; anr_mc_emit (same vol / workspace, after the
 * caller sized the outputs) writes vertices (V,3) f64 in padded index coordinates and triangles
 * (T,3) int64. A corner is outside iff value <= iso. One vertex per crossing grid edge, numbered in
 * grid order (C order of the padded grid, then axis x, y, z); triangles per cube in grid order from
 * the case table of tools/gen_mc_table.py, wound with the normal towards the outside. */
size_t anr_mc_workspace_bytes(int X, int Y, int Z, int pad);
int anr_mc_count(const float* vol, int X, int Y, int Z, int pad, double iso, int32_t* counts, void* workspace,
                 size_t ws_bytes, void* stream);
int anr_mc_emit(const float* vol, int X, int Y, int Z, int pad, double iso, double* vertices, int64_t* triangles,
                void* workspace, size_t ws_bytes, void* stream);
/* The largest watertight component of a triangle mesh (vertices (nv,3) f64, triangles (nt,3) int64, both on
 * the device), with the semantics of the host renderer_sdf_mesh.largest_component for every input whose
 * indices lie in [0, nv): faces are joined through shared undirected edges only; an edge's multiplicity is
 * the number of face sides carrying its vertex pair (all three sides of every face count, duplicate and
 * degenerate faces included); a component's label is its lowest face index; a component is watertight when
 * every one of its edges has multiplicity 2; the watertight component with the most distinct vertices is
 * kept, the lowest label on a tie. Output faces keep their input order, output vertices are the sorted
 * distinct vertex ids of the kept faces, and the faces are renumbered to those positions.
 * anr_mesh_cc_count writes device int32 counts {V', T', n_components, n_watertight, kept_label, status} and,
 * when labels != NULL, each face's component label. status 0: ok. status 1: no watertight component (or
 * nt == 0): kept_label -1, V' = nv, T' = nt and anr_mesh_cc_emit copies the inputs. status 2: an index was
 * outside [0, nv): V' = T' = 0, no index is dereferenced, labels are -1 and anr_mesh_cc_emit writes nothing.
 * anr_mesh_cc_emit (same triangles / workspace, after the caller sized the outputs) writes out_vertices (V',3)
 * and out_triangles (T',3). No allocation, no host synchronisation, integer reductions only (two calls on one
 * input write the same bits). 3 nt >= 2^31, nv + 1 >= 2^31, negative counts, NULL pointers (triangles may be
 * NULL when nt == 0, vertices when nv == 0) and a short workspace are rejected before any HIP call;
 * anr_mesh_cc_workspace_bytes returns 0 for such counts. */
#define ANR_MESHCC_NCOUNT 6
size_t anr_mesh_cc_workspace_bytes(long nv, long nt);
int anr_mesh_cc_count(const int64_t* triangles, long nt, long nv, int32_t* counts, int32_t* labels, void* workspace,
                      size_t ws_bytes, void* stream);
int anr_mesh_cc_emit(const double* vertices, const int64_t* triangles, long nt, long nv, double* out_vertices,
                     int64_t* out_triangles, void* workspace, size_t ws_bytes, void* stream);

/* ---- frame evaluator (lib/evaluators/if_nerf.py:15-74 Evaluator.evaluate: mse, psnr, ssim) -------------
 * One frame on the device: rgb_pred / rgb_gt (n_rays,3) are the in-box rays in raster order of
 * mask_at_box (H*W bytes, non-zero = set), as `img[mask_at_box] = rgb` assumes (if_nerf.py:26-29).
 * ssim is skimage.metrics.structural_similarity(img_pred, img_gt, multichannel=True) on the float64 crop
 * [y:y+h, x:x+w] (cv2.boundingRect of the mask) of the zero-filled (H,W,3) images: 7x7 uniform window,
 * K1 0.01, K2 0.03, sample covariance, mean of S over the crop minus its 3-pixel border, then over the
 * channels; all moments in float64. data_range defaults to 2.0: the reference passes none, and the
 * scikit-image releases that accept its call (0.16-0.18) give a float64 image the dtype range (-1, 1).
 * mse = sse / (3 n_rays) in float64, psnr = -10 log10(mse). Every reduction has a fixed order, so two
 * calls on the same inputs write the same bits. A set pixel whose scanned index is >= n_rays reads
 * nothing and counts as zero (status 3).
 * out (ANR_EVAL_NOUT device doubles):
 *   [0] sse  [1] 3*n_rays  [2] mse  [3] psnr  [4] ssim  [5] x [6] y [7] w [8] h (bounding rect)
 *   [9] sum of rgb_gt
 *   [10] status: 0 ok; 1 skipped (sum of rgb_gt == 0 or empty mask: the reference skips the frame);
 *        2 crop narrower than the 7-pixel window (ssim = NaN, mse/psnr valid);
 *        3 popcount(mask) != n_rays (nothing valid)
 *   [11] 0
 * Optional outputs (NULL: not written): img_pred / img_gt (H,W,3) f32, the zero-filled scatter;
 * img8_pred / img8_gt (H,W,3) u8 RGB = rint(clip(255 v, 0, 255)), half to even.
 * o == NULL means the defaults {data_range 2.0, win 7}; otherwise struct_size must be the size of the
 * struct. Allocates nothing, does not synchronise, everything is enqueued on `stream`. */
#define ANR_EVAL_NOUT 12
typedef struct anr_eval_opts {
  size_t struct_size;
  double data_range; /* R of C1 = (0.01 R)^2, C2 = (0.03 R)^2 */
  int win;           /* 7; others rejected */
} anr_eval_opts;
size_t anr_eval_workspace_bytes(int H, int W);
int anr_eval_frame(const float* rgb_pred, const float* rgb_gt, int n_rays, const uint8_t* mask_at_box, int H, int W,
                   const anr_eval_opts* o, double* out, float* img_pred, float* img_gt, uint8_t* img8_pred,
                   uint8_t* img8_gt, void* workspace, size_t ws_bytes, void* stream);

/* ---- blend-weight volumes (tools/custom_dataset/prepare_blend_weights.py:156-211, 229-283) --------------
 * volume (X,Y,Z,nb+1) f32 over the 'ij' grid whose voxel (x, y, z) sits at origin + (x, y, z) * vsize
 * (float64; origin is a HOST array of 3 doubles, the dims come from numpy's own arange on the host).
 * mode 0 (vertex, bweights/{i}.npy): channels 0..nb-1 = skin (nv,nb) row of the closest vertex, bit for bit;
 * channel nb = distance to it. mode 1 (surface, tbw.npy / bigpose_bw.npy): the closest point of the
 * triangle mesh faces (nf,3) — its projection onto the triangle when that lies inside, else the closest
 * of the three edge segments — channels 0..nb-1 = barycentric interpolation of the three vertices' rows
 * there, channel nb = distance to it. The search runs in float32 ((dx*dx + dy*dy) + dz*dz fused, over
 * the float32-rounded voxel position); among candidates with equal float32 squared distance the lowest
 * vertex / face index wins, whatever the launch geometry. The winner's weights and distance are then
 * recomputed in float64 and cast to float32 once. A zero-area triangle counts as its edges; no input
 * geometry produces a NaN. index (X*Y*Z int32, optional) receives the winning vertex / face id.
 * exhaustive: 0 = the library's default search, 1 = visit every primitive, 2 = skip cells of 64
 * primitives by their bounding boxes; all three write the same bits.
 * Face indices must lie in [0, nv): that is the caller's contract (the kernels clamp them, so a bad
 * index reads a wrong vertex, never outside the array). o == NULL means {mode 0, exhaustive 0}.
 * Allocates nothing, does not synchronise, everything is enqueued on `stream`; every element of volume
 * (and index) is written. */
typedef struct anr_bwv_opts {
  uint32_t struct_size;
  int mode;       /* 0 vertex, 1 surface */
  int exhaustive; /* 0 default, 1 exhaustive, 2 pruned */
} anr_bwv_opts;
size_t anr_bw_volume_workspace_bytes(int nv, int nf, int X, int Y, int Z);
int anr_bw_volume(const float* verts, int nv, const int32_t* faces, int nf, const float* skin, int nb,
                  const double* origin, double vsize, int X, int Y, int Z, const anr_bwv_opts* o,
                  float* volume, int32_t* index, void* workspace, size_t ws_bytes, void* stream);

/* ---- mesh evaluator (lib/evaluators/mesh_evaluator.py:19-136: Chamfer and point-to-surface) -------------
 * Meshes are vertices (nv,3) f32 and faces (nf,3) int32 on the device, as for anr_bw_volume; a face index
 * outside [0, nv) is clamped before any read. Limits: nf <= 2^26, points per call <= 2^24.
 * anr_mesh_sample restates trimesh.sample.sample_surface(mesh, n) (trimesh is third-party and not installed:
 *   parity unpinned). area = 0.5 |e0 x e1| in float64 (e0 = b - a, e1 = c - a), cum = its inclusive float64
 *   prefix sum; sample i takes u[i] = (u0, u1, u2) in [0, 1) (u (n,3) f64, device): face k =
 *   searchsorted(cum, u0 cum[-1], side='left'); if u1 + u2 > 1 both become |u - 1|; point = a_k + (e0 u1 +
 *   e1 u2) in float64 without contraction. points (n,3) f64, face (n) int32. status (one device int32): 0, or
 *   1 when nf <= 0 or the total area is zero or not finite; then nothing is drawn (points 0, face -1).
 * anr_mesh_point_dist: for each of n points (n,3) f64 the closest face and the distance to it (dist (n) f64,
 *   face (n) int32 or NULL). The search is anr_bw_volume's surface search over a point list: float32 records
 *   and queries taken about the centre of the mesh's box (subtracted in float64, so a mesh metres from the
 *   origin loses nothing), faces and queries in 30-bit Morton order (a linear-time radix sort), cells of 64
 *   faces pruned by their boxes, groups of 64 cells by a box of their own; the winner is the lowest (float32
 *   d^2, face index), then its distance is recomputed in float64 from the original vertices. exhaustive: 0 = the
 *   library's default search, 1 = visit every face, 2 = both levels of boxes, 3 = the cell boxes alone; all
 *   write the same bits, and the result of a point does not depend on the other points. mean (one device double, or NULL)
 *   receives the mean distance with a NaN counted as 0 (mesh_evaluator.py:114-115), summed in a fixed order.
 * anr_mesh_metrics: one frame. u ((2 n_chamfer + n_p2s),3) f64 in the reference's draw order: source Chamfer,
 *   target Chamfer, source P2S. out (ANR_MESHM_NOUT device doubles):
 *   [0] chamfer = (src_tgt + tgt_src) / 2   [1] p2s = mean distance of the n_p2s source samples to the target
 *   [2] src_tgt, [3] tgt_src: the means over the n_chamfer samples   [4] status: bit 0 the source, bit 1 the
 *   target has no face or no finite positive area (then [0..3] are NaN)   [5..7] 0
 * o == NULL means {exhaustive 0, n_chamfer 1000, n_p2s 10000}; a zero n_chamfer / n_p2s selects that default.
 * One workspace serves all three: anr_mesh_dist_workspace_bytes(nf, n_pts) with nf the larger face count and
 * n_pts the points of the call (2 n_chamfer + n_p2s for anr_mesh_metrics); it returns 0 for sizes outside the
 * limits. NULL pointers, bad sizes and a short workspace are rejected before any HIP call. Allocates nothing,
 * does not synchronise, everything is enqueued on `stream`. */
#define ANR_MESHM_NOUT 8
typedef struct anr_meshdist_opts {
  uint32_t struct_size;
  int exhaustive; /* 0 default, 1 exhaustive, 2 pruned by two levels of boxes, 3 pruned by the cell boxes alone */
  int n_chamfer;  /* 0: 1000 */
  int n_p2s;      /* 0: 10000 */
} anr_meshdist_opts;
size_t anr_mesh_dist_workspace_bytes(int nf, int n_pts);
int anr_mesh_sample(const float* verts, int nv, const int32_t* faces, int nf, const double* u, int n, double* points,
                    int32_t* face, int32_t* status, void* workspace, size_t ws_bytes, void* stream);
int anr_mesh_point_dist(const float* verts, int nv, const int32_t* faces, int nf, const double* points, int n,
                        const anr_meshdist_opts* o, double* dist, int32_t* face, double* mean, void* workspace,
                        size_t ws_bytes, void* stream);
/* The ordering alone (tools/mesh_eval_ab.py times it; the search does not depend on it): perm (nf) int32 = the
 * faces sorted by (30-bit Morton code of the centroid over the mesh's box, face index). Workspace:
 * anr_mesh_dist_workspace_bytes(nf, 1). */
int anr_mesh_order(const float* verts, int nv, const int32_t* faces, int nf, int32_t* perm, void* workspace,
                   size_t ws_bytes, void* stream);
int anr_mesh_metrics(const float* src_verts, int src_nv, const int32_t* src_faces, int src_nf, const float* tgt_verts,
                     int tgt_nv, const int32_t* tgt_faces, int tgt_nf, const double* u, const anr_meshdist_opts* o,
                     double* out, void* workspace, size_t ws_bytes, void* stream);

/* ---- aligned_aninerf_lbw variant (aligned_aninerf_lbw_network.py; the configs/aligned_nerf_lbw yamls) ---
 * The KNN-skinned NeRF of the extended paper, eval (no-grad) whole-frame render under tpose_renderer.render
 * (:159-186, Network.forward :90-147 per 2048-ray chunk): 5-NN blend over pvertices with the keep mask
 * pnorm < o->norm_th (cfg.norm_th, 0.05) + the chunk's argmin, the pose-space blend-weight MLP with
 * bw_latent[latent_index + 1], LBS pose -> T -> big pose for points and view directions (tpose_viewdir), a
 * second 5-NN blend of the warped points over tvertices and the same MLP with bw_latent[0] (tbw), the
 * weight-normed softplus(beta 100) density net, alpha = 1 - exp(-relu(y0) dist), the IDR colour net without a
 * normal (286 inputs), raw zeroed outside tbounds widened in place by 0.05 per chunk, the alpha_ind rows
 * (alpha > o->train_th + the chunk's argmax) of pbw / tbw, raw2outputs.
 * Parameters: the 62 tensors of aligned_aninerf_lbw_network.Network's state_dict, in order (a checkpoint's
 * novel_pose_bw.* tensors, present under cfg.aninerf_animation, follow them and are not read):
 *   0..26  tpose_human.nerf_network.lin{0..8}.{bias, weight_g (o,1), weight_v (o,i)}
 *          i/o: 39/256, 256/256, 256/256, 256/217, 256/256 x4, 256/257
 *   27     tpose_human.color_network.color_latent.weight (L,128)
 *   28..42 tpose_human.color_network.lin{0..4}.{bias, weight_g, weight_v}  i: 286,256,256,384,256
 *   43     bw_latent.weight (num_train_frame + 1, 128)
 *   44..59 bw_linears.{0..7}.{weight,bias}      Conv1d, in: 191,256,256,256,256,447,256,256
 *   60,61  bw_fc.{weight,bias} (24,256,1)
 * Precisions: ANR_FP32 (exact fp32 MFMA layer products as layer GEMMs, the parity anchor; the environment switch
 * ANR_SDF_LG32=0 of the sdf_pdf render moves them from k_lgemm to k_gemm here too), ANR_BF16X3 and ANR_BF16X6 (the
 * blend-weight MLP with its log-softmax epilogue, the density net and the colour net as one fused launch per batch
 * each, split bf16 with 3 products or, fp32-level, 6).
 * Not covered (ANR_E_ARG where an option would ask for it): training / autograd, cfg.test_novel_pose
 * (o->novel_pose), get_alpha / mesh extraction, the mmsk visibility filter, Network.forward over free
 * samples, N_samples != 64, cfg.tpose_viewdir False, color_with_viewdir False.
 * The KNN boundary is unpinned as for sdf_pdf: pytorch3d knn_points is restated, not run (k_sdf_front). */
#define ANR_LBW_NUM_TENSORS 62

typedef struct anr_lbw_params {
  const float* t[ANR_LBW_NUM_TENSORS];  /* device pointers, state_dict order above */
} anr_lbw_params;

typedef struct anr_lbw_frame {
  const float* A;          /* (24,4,4) device */
  const float* big_A;      /* (24,4,4) device: big pose */
  const float* R;          /* (3,3) */
  const float* Th;         /* (3) */
  const float* pvertices;  /* (V,3) posed SMPL vertices in the pose frame, V <= 6912 */
  const float* tvertices;  /* (V,3) big-pose SMPL vertices (NULL allowed for an image-only call) */
  const float* weights;    /* (V,24) skin weights */
  int n_verts;
  const float* tbounds;    /* (2,3) batch['tbounds'] as passed in */
  const int64_t* latent_index;  /* (1): colour latent row; bw_latent row latent_index + 1 */
} anr_lbw_frame;

typedef struct anr_lbw_render_out {
  float* rgb_map;      /* (R,3) */
  float* acc_map;      /* (R) */
  float* depth_map;    /* (R) */
  float* raw;          /* (R*64,4) */
  float* tbounds_out;  /* (2,3) or NULL: batch['tbounds'] after the in-place widening by 0.05 per chunk (:124-126) */
} anr_lbw_render_out;

/* Asynchronous on the caller's stream except for one host read of the kept-sample count (it sizes the layer
 * GEMMs); allocates nothing. image_only != 0 (cfg.render_image_only): no second search, no T-pose blend-weight
 * MLP, no alpha_ind rows -- no rendered map depends on them, and raw and the maps equal the full call's bit for
 * bit; anr_lbw_render_rows then has nothing to return and counts[1] is 0.
 * ANR_E_ARG / ANR_E_WORKSPACE before any HIP call for: a NULL pointer, n_verts outside 1..6912,
 * o->n_samples != 64, o->novel_pose, a precision other than ANR_FP32 / ANR_BF16X3 / ANR_BF16X6, a workspace smaller than
 * anr_lbw_render_workspace_bytes(n_rays, o, image_only) (which makes no HIP call; 0 for bad arguments).
 * Kept samples run in batches of at most 2^18 rows (the environment variable ANR_LBW_BATCH, a multiple of
 * 256, overrides the batch size for tests; it must hold the same value for the size query and the call). */
size_t anr_lbw_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only);
int anr_lbw_render_fwd(const anr_lbw_params* p, const anr_lbw_frame* f, const float* ray_o, const float* ray_d,
                       const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                       const anr_lbw_render_out* out, int image_only, void* workspace, size_t ws_bytes, void* stream);
/* device int32[2] inside the workspace: {kept samples n', alpha_ind rows m}. */
const int32_t* anr_lbw_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
/* copy the alpha_ind rows pbw (m,24), tbw (m,24) and / or their sample ids (m; ray * 64 + sample) out of the
 * workspace of a full (not image-only) call; NULL outputs are skipped */
int anr_lbw_render_rows(const void* workspace, int n_rays, const anr_render_opts* o, float* pbw, float* tbw,
                        int32_t* ids, void* stream);
/* device uint32 (R*64, 8) inside the workspace: the first search's per-sample KNN records, as
 * anr_sdf_render_knn -- a debugging / test view of the knn_points boundary. */
const uint32_t* anr_lbw_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
/* two more test views into the workspace of the last call (unstable: they follow the workspace layout, not a
 * contract; for tests and debugging only): the kept sample ids (n' int32, ray * 64 + sample, in
 * order), and the colour-net input rows of the last batch of kept samples ((rows, 40) floats: the warped point
 * in columns 0..2, the warped view direction in 3..5). */
const int32_t* anr_lbw_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
const float* anr_lbw_render_points(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);

/* ---- aligned_aninerf_pdf variant (aligned_aninerf_pdf_network.py; the configs/aligned_nerf_pdf yamls) ---
 * The extended paper's NeRF with a pose-dependent displacement field, eval (no-grad) whole-frame render under
 * tpose_renderer.render (Network.forward :97-138 per 2048-ray chunk): 5-NN blend over pvertices with the keep mask
 * pnorm < 0.1 (hard-coded in the network: o->norm_th is NOT read) + the chunk's argmin, LBS pose -> T -> big pose
 * for points and view directions, the displacement MLP over [gamma_10(init_bigpose), poses] with
 * resd = 0.05 tanh(.), tpose = init_bigpose + resd, the weight-normed softplus(beta 100) density net,
 * alpha = 1 - exp(-relu(y0) dist), the IDR colour net without a normal (286 inputs), raw zeroed outside tbounds
 * widened in place by 0.05 per chunk (strict test on tpose), raw2outputs.
 * Parameters: the 62 tensors of aligned_aninerf_pdf_network.Network's state_dict, in order:
 *   0..26  tpose_human.nerf_network.lin{0..8}.{bias, weight_g (o,1), weight_v (o,i)}
 *          i/o: 39/256, 256/256, 256/256, 256/217, 256/256 x4, 256/257
 *   27     tpose_human.color_network.color_latent.weight (L,128)
 *   28..42 tpose_human.color_network.lin{0..4}.{bias, weight_g, weight_v}  i: 286,256,256,384,256
 *   43     resd_latent.weight (L,128)            (not read by the forward; NULL allowed)
 *   44..59 resd_linears.{0..7}.{weight,bias}     Conv1d, in: 135,256,256,256,256,391,256,256
 *   60,61  resd_fc.{weight,bias} (3,256,1)
 * Precisions: ANR_FP32 (exact fp32 MFMA layer products as layer GEMMs, the parity anchor), ANR_BF16X3 and
 * ANR_BF16X6 (the displacement MLP with its tanh / tpose epilogue, the density net and the colour net as one
 * fused launch per batch each, split bf16 with 3 products or, fp32-level, 6).
 * n_views > 0 applies the novel-view visibility filter of tpose_renderer_mmsk as anr_sdf_frame does: chunks with
 * no visible sample make no network call and do not widen tbounds.
 * Not covered (ANR_E_ARG where an option would ask for it): training / autograd, cfg.test_novel_pose,
 * Network.forward over free samples, N_samples != 64, cfg.tpose_viewdir False, color_with_viewdir False.
 * The KNN boundary is unpinned as for sdf_pdf: pytorch3d knn_points is restated, not run (k_sdf_front). */
#define ANR_PDF_NUM_TENSORS 62

typedef struct anr_pdf_params {
  const float* t[ANR_PDF_NUM_TENSORS];  /* device pointers, state_dict order above */
} anr_pdf_params;

typedef struct anr_pdf_frame {
  const float* A;          /* (24,4,4) device */
  const float* big_A;      /* (24,4,4) device: big pose */
  const float* R;          /* (3,3) */
  const float* Th;         /* (3) */
  const float* pvertices;  /* (V,3) posed SMPL vertices in the pose frame, V <= 6912 */
  const float* weights;    /* (V,24) skin weights */
  const float* poses;      /* (72) batch['poses'] */
  const float* tbounds;    /* (2,3) batch['tbounds'] as passed in */
  const int64_t* latent_index;  /* (1): colour latent row */
  int n_verts;
  /* the visibility filter's views, as anr_sdf_frame's (n_views == 0: off) */
  int n_views;
  const float* Ks;         /* (n_views,3,3) */
  const float* RT;         /* (n_views,3,4) */
  const uint8_t* msks;     /* (n_views,img_h,img_w) */
  int img_h, img_w;
} anr_pdf_frame;

typedef struct anr_pdf_render_out {
  float* rgb_map;      /* (R,3) */
  float* acc_map;      /* (R) */
  float* depth_map;    /* (R) */
  float* raw;          /* (R*64,4) */
  float* tbounds_out;  /* (2,3) or NULL: batch['tbounds'] after the in-place widening by 0.05 per chunk (:125-127) */
} anr_pdf_render_out;

/* Asynchronous on the caller's stream except for one host read of the kept-sample count (it sizes the batches);
 * allocates nothing. image_only != 0 (cfg.render_image_only): the compact resd rows are not kept; raw and the maps
 * equal the full call's bit for bit, and anr_pdf_render_rows then has nothing to return.
 * ANR_E_ARG / ANR_E_WORKSPACE before any HIP call for: a NULL pointer, n_verts outside 1..6912,
 * o->n_samples != 64, o->novel_pose, a precision other than ANR_FP32 / ANR_BF16X3 / ANR_BF16X6, bad view fields,
 * a workspace smaller than anr_pdf_render_workspace_bytes(n_rays, o, image_only) (which makes no HIP call; 0 for
 * bad arguments). Kept samples run in batches of at most 2^18 rows (the environment variable ANR_PDF_BATCH, a
 * multiple of 256, overrides the batch size for tests; it is read per call and must hold the same value for the
 * size query and the call). */
size_t anr_pdf_render_workspace_bytes(int n_rays, const anr_render_opts* o, int image_only);
int anr_pdf_render_fwd(const anr_pdf_params* p, const anr_pdf_frame* f, const float* ray_o, const float* ray_d,
                       const float* near_, const float* far_, int n_rays, const anr_render_opts* o,
                       const anr_pdf_render_out* out, int image_only, void* workspace, size_t ws_bytes, void* stream);
/* device int32[2] inside the workspace: {kept samples n', 0}. */
const int32_t* anr_pdf_render_counts(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
/* copy the resd rows (n',3), in kept order, and / or their sample ids (n'; ray * 64 + sample) out of the workspace
 * of a full (not image-only) call; NULL outputs are skipped. Reads n' on the host. */
int anr_pdf_render_rows(const void* workspace, int n_rays, const anr_render_opts* o, float* resd, int32_t* ids,
                        void* stream);
/* test views into the workspace of the last call (unstable: they follow the workspace layout, not a contract; for
 * tests and debugging only): the per-sample KNN records (R*64, 8) as anr_sdf_render_knn, the kept sample ids (n'
 * int32, in order), the colour-net input rows of the last batch ((rows, 40) floats: tpose in columns 0..2, the
 * warped view direction in 3..5) and its point rows ((rows, 8): init_bigpose in 0..2, the direction in 3..5,
 * dist in 6). */
const uint32_t* anr_pdf_render_knn(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
const int32_t* anr_pdf_render_kept(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
const float* anr_pdf_render_points(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);
const float* anr_pdf_render_bigpose(const void* workspace, int n_rays, const anr_render_opts* o, int image_only);

/* Network.get_alpha (:140-174) over n_pts free world points, as aninerf_mesh_renderer's batchify calls it: one
 * network call per chunk of o->chunk_pts points (a positive multiple of 64; the last chunk partial), each with the
 * keep mask pnorm < 0.1 (hard-coded; o->norm_th is not read) + the chunk's forced argmin, the displacement MLP and
 * the density net. alpha (n_pts): the density net's RAW output 0 at kept points (no relu, no 1 - exp, no box test:
 * get_alpha has none), 0 where a point is dropped. Frame fields read: A, big_A, R, Th, pvertices, weights, poses,
 * n_verts; n_views must be 0. One host read of the kept count per chunk. ANR_E_ARG before any HIP call for a NULL
 * pointer, n_pts outside [1, 2^24], a bad chunk_pts, o->novel_pose, another precision, n_verts outside 1..6912;
 * anr_pdf_alpha_workspace_bytes makes no HIP call and returns 0 for bad arguments. */
size_t anr_pdf_alpha_workspace_bytes(long n_pts, const anr_alpha_opts* o);
int anr_pdf_alpha_points(const anr_pdf_params* p, const anr_pdf_frame* f, const float* wpts, long n_pts,
                         const anr_alpha_opts* o, float* alpha, void* workspace, size_t ws_bytes, void* stream);

/* ---- measurement ----------------------------------------------------------------------
 * When enabled, anr_render_fwd records a hipEvent pair around the fused network kernel (k_mlp)
 * on the caller's stream, and anr_sdf_render_fwd one around each fused sdf_pdf network launch. anr_profile_read waits for the recorded events, returns the summed
 * kernel time (ms) and launch count since the last read, and resets. */
int anr_profile_enable(int on);
int anr_profile_read(double* mlp_ms, int* launches);
/* anr_profile_read plus the median in-kernel shader clock (MHz) over every stamped workgroup of the
 * profiled fused launches (thread 0 stamps s_memtime / s_memrealtime at entry and exit; 0 if none ran
 * long enough): tells a DVFS-throttled box from a slower kernel. */
int anr_profile_read_clock(double* mlp_ms, int* launches, double* clk_mhz);

const char* anr_last_error(void);
int anr_version(void);

#ifdef __cplusplus
}
#endif
#endif
