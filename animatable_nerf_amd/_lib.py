"""ctypes binding of the C-ABI library ``libaninerf_hip.so`` (include/aninerf.h).

The library is built in-tree by ``make`` (``__graft_entry__.build()``). Loading it is mandatory:
there is no CPU or PyTorch fallback for the render path, a missing or stale library raises.
``torch`` is imported first so the HIP runtime torch ships (same SONAME ``libamdhip64.so.7``)
is the one the library binds to — one runtime, one set of streams.
"""
import ctypes
import os

import torch  # noqa: F401  (must be loaded before the library, see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libaninerf_hip.so')
# kernel experiments (tools/): an alternative build of the same C-ABI, e.g. with other -D options
if os.environ.get('ANR_LIB_PATH'):
    LIB_PATH = os.environ['ANR_LIB_PATH']
NUM_TENSORS = 46
NUM_NOVEL_TENSORS = 19
NUM_SDF_TENSORS = 63
NUM_LBW_TENSORS = 62
NUM_PDF_TENSORS = 62

EXPORTS = ('anr_near_far', 'anr_params_packed_bytes', 'anr_params_pack', 'anr_render_workspace_bytes',
           'anr_render_fwd', 'anr_render_counts', 'anr_render_bw_rows', 'anr_render_row_ids', 'anr_profile_enable', 'anr_profile_read', 'anr_profile_read_clock',
           'anr_train_workspace_bytes', 'anr_train_fwd', 'anr_train_bwd', 'anr_train_step', 'anr_adam',
           'anr_camera_rays_workspace_bytes', 'anr_camera_rays', 'anr_sdf_render_workspace_bytes', 'anr_sdf_render_fwd', 'anr_sdf_render_counts', 'anr_sdf_render_rows',
           'anr_alpha_workspace_bytes', 'anr_alpha_points', 'anr_alpha_counts', 'anr_mc_workspace_bytes',
           'anr_mc_count', 'anr_mc_emit', 'anr_anim_workspace_bytes', 'anr_anim_step',
           'anr_train_ray_workspace_bytes', 'anr_train_ray_lists', 'anr_train_ray_gather',
           'anr_train_ray_sample',
           'anr_network_workspace_bytes', 'anr_network_fwd', 'anr_network_counts', 'anr_network_bw_rows',
           'anr_network_train_workspace_bytes', 'anr_network_train_fwd', 'anr_network_train_bwd',
           'anr_points_workspace_bytes', 'anr_blend_weights', 'anr_canonical_alpha', 'anr_train_step_hooked',
           'anr_sdf_train_workspace_bytes', 'anr_sdf_train_step', 'anr_sdf_train_step_hooked', 'anr_sdf_render_knn',
           'anr_sdf_network_workspace_bytes', 'anr_sdf_network_fwd', 'anr_sdf_network_counts', 'anr_sdf_network_rows',
           'anr_sdf_network_train_workspace_bytes', 'anr_sdf_network_train_fwd', 'anr_sdf_network_train_counts',
           'anr_sdf_network_train_rows', 'anr_sdf_network_train_bwd', 'anr_sdf_points_workspace_bytes', 'anr_sdf_points',
           'anr_sample_volume', 'anr_knn_blend_workspace_bytes', 'anr_knn_blend', 'anr_sdf_mesh_pose',
           'anr_train_deterministic', 'anr_eval_workspace_bytes', 'anr_eval_frame', 'anr_bw_volume_workspace_bytes',
           'anr_bw_volume', 'anr_mesh_cc_workspace_bytes', 'anr_mesh_cc_count', 'anr_mesh_cc_emit',
           'anr_mesh_dist_workspace_bytes', 'anr_mesh_sample', 'anr_mesh_point_dist', 'anr_mesh_metrics', 'anr_mesh_order',
           'anr_render_image_workspace_bytes', 'anr_render_image_fwd',
           'anr_render_ns_workspace_bytes', 'anr_render_ns_fwd', 'anr_render_ns_bw_rows', 'anr_render_ns_row_ids',
           'anr_lbw_render_workspace_bytes', 'anr_lbw_render_fwd', 'anr_lbw_render_counts', 'anr_lbw_render_rows',
           'anr_lbw_render_knn', 'anr_lbw_render_kept', 'anr_lbw_render_points',
           'anr_pdf_render_workspace_bytes', 'anr_pdf_render_fwd', 'anr_pdf_render_counts', 'anr_pdf_render_rows',
           'anr_pdf_render_knn', 'anr_pdf_render_kept', 'anr_pdf_render_points', 'anr_pdf_render_bigpose',
           'anr_pdf_alpha_workspace_bytes', 'anr_pdf_alpha_points',
           'anr_last_error', 'anr_version')

c_float_p = ctypes.c_void_p


class Params(ctypes.Structure):
    _fields_ = [('t', ctypes.c_void_p * NUM_TENSORS), ('num_train_frame', ctypes.c_int),
                ('packed', ctypes.c_void_p), ('novel', ctypes.c_void_p * NUM_NOVEL_TENSORS)]


class Frame(ctypes.Structure):
    _fields_ = [('A', ctypes.c_void_p), ('R', ctypes.c_void_p), ('Th', ctypes.c_void_p),
                ('pbw', ctypes.c_void_p), ('pbw_dims', ctypes.c_int * 3), ('pbounds', ctypes.c_void_p),
                ('tbw', ctypes.c_void_p), ('tbw_dims', ctypes.c_int * 3), ('tbounds', ctypes.c_void_p),
                ('latent_index', ctypes.c_void_p), ('bw_latent_index', ctypes.c_void_p),
                ('n_views', ctypes.c_int), ('Ks', ctypes.c_void_p), ('RT', ctypes.c_void_p), ('msks', ctypes.c_void_p),
                ('img_h', ctypes.c_int), ('img_w', ctypes.c_int)]


class RenderOpts(ctypes.Structure):
    _fields_ = [('n_samples', ctypes.c_int), ('chunk', ctypes.c_int), ('norm_th', ctypes.c_float),
                ('train_th', ctypes.c_float), ('t_rand', ctypes.c_void_p), ('novel_pose', ctypes.c_int),
                ('precision', ctypes.c_int)]


FP32, BF16, BF16_ALL, BF16X3, BF16X6 = 0, 1, 2, 3, 4  # anr_render_opts.precision


class RenderOut(ctypes.Structure):
    _fields_ = [('rgb_map', ctypes.c_void_p), ('acc_map', ctypes.c_void_p), ('depth_map', ctypes.c_void_p),
                ('raw', ctypes.c_void_p)]


class Samples(ctypes.Structure):
    _fields_ = [('wpts', ctypes.c_void_p), ('viewdir', ctypes.c_void_p), ('dists', ctypes.c_void_p),
                ('n_pts', ctypes.c_int)]


REDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)
SDFP_NETWORK, SDFP_GRADIENT, SDFP_DEFORMED_GRADIENT = 0, 1, 2  # anr_sdf_points modes
REDUCE_MIN_U64, REDUCE_MAX_U64, REDUCE_SUM_F32 = 0, 1, 2  # anr_train_hooks.reduce ops


class TrainHooks(ctypes.Structure):
    """anr_train_hooks (ANR_TRAIN_HOOKS_VERSION 2): struct_size is filled in by the constructor."""
    _fields_ = [('struct_size', ctypes.c_size_t), ('nerf_grads_ready', ctypes.c_void_p), ('ray_offset', ctypes.c_int),
                ('reduce', REDUCE_FN), ('reduce_user', ctypes.c_void_p)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(TrainHooks), *args, **kw)


READY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


class SdfTrainHooks(ctypes.Structure):
    """anr_sdf_train_hooks: struct_size is filled in by the constructor."""
    _fields_ = [('struct_size', ctypes.c_size_t), ('colour_grads_ready', ctypes.c_void_p), ('colour_ready', READY_FN),
                ('user', ctypes.c_void_p)]

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(SdfTrainHooks), *args, **kw)


class AlphaOpts(ctypes.Structure):
    _fields_ = [('chunk_pts', ctypes.c_int), ('norm_th', ctypes.c_float), ('novel_pose', ctypes.c_int),
                ('precision', ctypes.c_int)]


class SdfParams(ctypes.Structure):
    _fields_ = [('t', ctypes.c_void_p * NUM_SDF_TENSORS)]


class SdfFrame(ctypes.Structure):
    _fields_ = [('A', ctypes.c_void_p), ('big_A', ctypes.c_void_p), ('R', ctypes.c_void_p), ('Th', ctypes.c_void_p),
                ('poses', ctypes.c_void_p), ('pvertices', ctypes.c_void_p), ('weights', ctypes.c_void_p),
                ('n_verts', ctypes.c_int), ('tbounds', ctypes.c_void_p), ('latent_index', ctypes.c_void_p),
                ('occupancy', ctypes.c_void_p), ('n_views', ctypes.c_int), ('Ks', ctypes.c_void_p),
                ('RT', ctypes.c_void_p), ('msks', ctypes.c_void_p), ('img_h', ctypes.c_int), ('img_w', ctypes.c_int)]


class SdfRenderOut(ctypes.Structure):
    _fields_ = [('rgb_map', ctypes.c_void_p), ('acc_map', ctypes.c_void_p), ('depth_map', ctypes.c_void_p),
                ('raw', ctypes.c_void_p), ('sdf', ctypes.c_void_p), ('tbounds_out', ctypes.c_void_p)]


class LbwParams(ctypes.Structure):
    _fields_ = [('t', ctypes.c_void_p * NUM_LBW_TENSORS)]


class LbwFrame(ctypes.Structure):
    _fields_ = [('A', ctypes.c_void_p), ('big_A', ctypes.c_void_p), ('R', ctypes.c_void_p), ('Th', ctypes.c_void_p),
                ('pvertices', ctypes.c_void_p), ('tvertices', ctypes.c_void_p), ('weights', ctypes.c_void_p),
                ('n_verts', ctypes.c_int), ('tbounds', ctypes.c_void_p), ('latent_index', ctypes.c_void_p)]


class LbwRenderOut(ctypes.Structure):
    _fields_ = [('rgb_map', ctypes.c_void_p), ('acc_map', ctypes.c_void_p), ('depth_map', ctypes.c_void_p),
                ('raw', ctypes.c_void_p), ('tbounds_out', ctypes.c_void_p)]


class PdfParams(ctypes.Structure):
    _fields_ = [('t', ctypes.c_void_p * NUM_PDF_TENSORS)]


class PdfFrame(ctypes.Structure):
    _fields_ = [('A', ctypes.c_void_p), ('big_A', ctypes.c_void_p), ('R', ctypes.c_void_p), ('Th', ctypes.c_void_p),
                ('pvertices', ctypes.c_void_p), ('weights', ctypes.c_void_p), ('poses', ctypes.c_void_p),
                ('tbounds', ctypes.c_void_p), ('latent_index', ctypes.c_void_p), ('n_verts', ctypes.c_int),
                ('n_views', ctypes.c_int), ('Ks', ctypes.c_void_p), ('RT', ctypes.c_void_p), ('msks', ctypes.c_void_p),
                ('img_h', ctypes.c_int), ('img_w', ctypes.c_int)]


class PdfRenderOut(ctypes.Structure):
    _fields_ = [('rgb_map', ctypes.c_void_p), ('acc_map', ctypes.c_void_p), ('depth_map', ctypes.c_void_p),
                ('raw', ctypes.c_void_p), ('tbounds_out', ctypes.c_void_p)]


EVAL_NOUT = 12  # ANR_EVAL_NOUT: doubles of one anr_eval_frame record
# indices into the record
EVAL_SSE, EVAL_COUNT, EVAL_MSE, EVAL_PSNR, EVAL_SSIM, EVAL_X, EVAL_Y, EVAL_W, EVAL_H, EVAL_SUM_GT, EVAL_STATUS = range(11)
EVAL_OK, EVAL_SKIPPED, EVAL_NARROW, EVAL_MISMATCH = 0, 1, 2, 3  # record[EVAL_STATUS]


class EvalOpts(ctypes.Structure):
    """anr_eval_opts: struct_size is filled in by the constructor; the defaults are the library's."""
    _fields_ = [('struct_size', ctypes.c_size_t), ('data_range', ctypes.c_double), ('win', ctypes.c_int)]

    def __init__(self, data_range=2.0, win=7):
        super().__init__(ctypes.sizeof(EvalOpts), data_range, win)


MESHCC_NCOUNT = 6  # ANR_MESHCC_NCOUNT: int32 counts of anr_mesh_cc_count
# indices into the counts, and the status values
MESHCC_V, MESHCC_T, MESHCC_NCOMP, MESHCC_NWATERTIGHT, MESHCC_KEPT, MESHCC_STATUS = range(6)
MESHCC_OK, MESHCC_NONE_WATERTIGHT, MESHCC_BAD_INDEX = 0, 1, 2

BWV_VERTEX, BWV_SURFACE = 0, 1  # anr_bwv_opts.mode
BWV_DEFAULT, BWV_EXHAUSTIVE, BWV_PRUNED = 0, 1, 2  # anr_bwv_opts.exhaustive


class BwvOpts(ctypes.Structure):
    """anr_bwv_opts: struct_size is filled in by the constructor."""
    _fields_ = [('struct_size', ctypes.c_uint32), ('mode', ctypes.c_int), ('exhaustive', ctypes.c_int)]

    def __init__(self, mode=BWV_VERTEX, exhaustive=BWV_DEFAULT):
        super().__init__(ctypes.sizeof(BwvOpts), mode, exhaustive)


MESHM_NOUT = 8  # ANR_MESHM_NOUT: doubles of one anr_mesh_metrics row
MESHM_CHAMFER, MESHM_P2S, MESHM_SRC_TGT, MESHM_TGT_SRC, MESHM_STATUS = range(5)
MESHM_BAD_SOURCE, MESHM_BAD_TARGET = 1, 2  # bits of row[MESHM_STATUS]
MESH_MAX_FACES, MESH_MAX_POINTS = 1 << 26, 1 << 24
# anr_meshdist_opts.exhaustive: BWV_DEFAULT, BWV_EXHAUSTIVE, BWV_PRUNED (two levels of boxes) and
MESHDIST_PRUNED_CELLS = 3  # pruned by the cell boxes alone


class MeshDistOpts(ctypes.Structure):
    """anr_meshdist_opts: struct_size is filled in by the constructor; 0 samples mean the reference's counts."""
    _fields_ = [('struct_size', ctypes.c_uint32), ('exhaustive', ctypes.c_int), ('n_chamfer', ctypes.c_int),
                ('n_p2s', ctypes.c_int)]

    def __init__(self, exhaustive=BWV_DEFAULT, n_chamfer=0, n_p2s=0):
        super().__init__(ctypes.sizeof(MeshDistOpts), exhaustive, n_chamfer, n_p2s)


_lib = None


def load():
    """Load (once) and return the library; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} not built: run `make` (or __graft_entry__.build()) first; '
                           'the HIP path has no fallback')
    lib = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    lib.anr_near_far.argtypes = [P, P, ctypes.c_int, P, P, P, P, P]
    lib.anr_params_packed_bytes.restype = ctypes.c_size_t
    lib.anr_params_pack.argtypes = [ctypes.POINTER(Params), P, P]
    lib.anr_render_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_render_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(RenderOpts), ctypes.POINTER(Frame)]
    lib.anr_render_fwd.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(Frame), P, P, P, P, ctypes.c_int,
                                   ctypes.POINTER(RenderOpts), ctypes.POINTER(RenderOut), P, ctypes.c_size_t, P]
    lib.anr_render_image_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_render_image_workspace_bytes.argtypes = lib.anr_render_workspace_bytes.argtypes
    lib.anr_render_image_fwd.argtypes = lib.anr_render_fwd.argtypes
    lib.anr_render_ns_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_render_ns_workspace_bytes.argtypes = lib.anr_render_workspace_bytes.argtypes + [ctypes.c_int]
    lib.anr_render_ns_fwd.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(Frame), P, P, P, P, ctypes.c_int,
                                      ctypes.POINTER(RenderOpts), ctypes.POINTER(RenderOut), ctypes.c_int, P,
                                      ctypes.c_size_t, P]
    lib.anr_render_ns_bw_rows.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P, P]
    lib.anr_render_ns_row_ids.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P]
    lib.anr_render_counts.restype = P
    lib.anr_render_counts.argtypes = [P, ctypes.c_int]
    lib.anr_render_bw_rows.argtypes = [P, ctypes.c_int, P, P, P]
    lib.anr_render_row_ids.argtypes = [P, ctypes.c_int, P, P]
    lib.anr_train_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_train_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(RenderOpts), ctypes.POINTER(Frame)]
    lib.anr_train_fwd.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(Frame), P, P, P, P, ctypes.c_int,
                                  ctypes.POINTER(RenderOpts), ctypes.POINTER(RenderOut), P, ctypes.c_size_t, P]
    lib.anr_train_bwd.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p * NUM_TENSORS, ctypes.POINTER(Frame), P, P, P, P,
                                  ctypes.c_int, ctypes.POINTER(RenderOpts), P, P, P, P, ctypes.c_size_t, P]
    lib.anr_train_step.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p * NUM_TENSORS, ctypes.POINTER(Frame), P, P, P,
                                   P, ctypes.c_int, ctypes.POINTER(RenderOpts), P, P, ctypes.POINTER(RenderOut), P, P,
                                   ctypes.c_size_t, P]
    lib.anr_train_step_hooked.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p * NUM_TENSORS, ctypes.POINTER(Frame), P,
                                          P, P, P, ctypes.c_int, ctypes.POINTER(RenderOpts), P, P,
                                          ctypes.POINTER(RenderOut), P, ctypes.POINTER(TrainHooks), P, ctypes.c_size_t, P]
    lib.anr_adam.argtypes = [P, P, P, P, ctypes.c_long, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                             ctypes.c_float, ctypes.c_int, ctypes.c_float, P]
    lib.anr_sdf_render_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_sdf_render_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(RenderOpts)]
    lib.anr_sdf_render_fwd.argtypes = [ctypes.POINTER(SdfParams), ctypes.POINTER(SdfFrame), P, P, P, P, ctypes.c_int,
                                       ctypes.POINTER(RenderOpts), ctypes.POINTER(SdfRenderOut), P, ctypes.c_size_t, P]
    lib.anr_sdf_render_counts.restype = P
    lib.anr_sdf_render_counts.argtypes = [P, ctypes.c_int, ctypes.POINTER(RenderOpts)]
    lib.anr_sdf_render_knn.restype = P
    lib.anr_sdf_render_knn.argtypes = [P, ctypes.c_int, ctypes.POINTER(RenderOpts)]
    lib.anr_sdf_render_rows.argtypes = [P, ctypes.c_int, ctypes.POINTER(RenderOpts), P, P, P, P, P]
    lib.anr_sdf_train_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_sdf_train_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(RenderOpts)]
    lib.anr_sdf_train_step.argtypes = [ctypes.POINTER(SdfParams), ctypes.c_void_p * NUM_SDF_TENSORS,
                                       ctypes.POINTER(SdfFrame), P, P, P, P, ctypes.c_int, ctypes.POINTER(RenderOpts),
                                       P, P, ctypes.c_int, ctypes.POINTER(SdfRenderOut), P, P, ctypes.c_size_t, P]
    lib.anr_sdf_train_step_hooked.argtypes = [ctypes.POINTER(SdfParams), ctypes.c_void_p * NUM_SDF_TENSORS,
                                              ctypes.POINTER(SdfFrame), P, P, P, P, ctypes.c_int,
                                              ctypes.POINTER(RenderOpts), P, P, ctypes.c_int,
                                              ctypes.POINTER(SdfRenderOut), P, ctypes.POINTER(SdfTrainHooks), P,
                                              ctypes.c_size_t, P]
    SP, SF, SS = ctypes.POINTER(SdfParams), ctypes.POINTER(SdfFrame), ctypes.POINTER(Samples)
    lib.anr_sdf_network_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_sdf_network_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(RenderOpts)]
    lib.anr_sdf_network_fwd.argtypes = [SP, SF, SS, ctypes.POINTER(RenderOpts), P, P, P, P, ctypes.c_size_t, P]
    lib.anr_sdf_network_counts.restype = P
    lib.anr_sdf_network_counts.argtypes = [P, ctypes.c_int]
    lib.anr_sdf_network_rows.argtypes = [P, ctypes.c_int, P, P, P]
    lib.anr_sdf_network_train_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_sdf_network_train_workspace_bytes.argtypes = [ctypes.c_int]
    lib.anr_sdf_network_train_fwd.argtypes = [SP, SF, SS, ctypes.POINTER(RenderOpts), P, P, P, P, ctypes.c_size_t, P]
    lib.anr_sdf_network_train_counts.restype = P
    lib.anr_sdf_network_train_counts.argtypes = [P, ctypes.c_int]
    lib.anr_sdf_network_train_rows.argtypes = [P, ctypes.c_int, P, P, P, P]
    lib.anr_sdf_network_train_bwd.argtypes = [SP, ctypes.c_void_p * NUM_SDF_TENSORS, SF, SS, ctypes.POINTER(RenderOpts),
                                              P, P, P, P, P, P, ctypes.c_size_t, P]
    lib.anr_sdf_points_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_sdf_points_workspace_bytes.argtypes = [ctypes.c_int]
    lib.anr_sdf_points.argtypes = [SP, SF, P, ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_size_t, P]
    lib.anr_sample_volume.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, ctypes.c_int, P, P]
    lib.anr_knn_blend_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_knn_blend_workspace_bytes.argtypes = [ctypes.c_int]
    lib.anr_knn_blend.argtypes = [P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_float, P, P, P, ctypes.c_size_t, P]
    lib.anr_sdf_mesh_pose.argtypes = [P, P, ctypes.c_int, P, P, P, P, P, P]
    lib.anr_camera_rays_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_camera_rays_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    D = ctypes.POINTER(ctypes.c_double)
    lib.anr_camera_rays.argtypes = [ctypes.c_int, ctypes.c_int, D, D, D, D, ctypes.c_int, P, P, P, P, P, P, P, P, P,
                                    ctypes.c_size_t, P]
    lib.anr_train_ray_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_train_ray_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.anr_train_ray_lists.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, ctypes.c_size_t, P]
    lib.anr_train_ray_gather.argtypes = [ctypes.c_int, ctypes.c_int, D, D, D, D, ctypes.c_int, P, P, P, ctypes.c_int,
                                         P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         P, P, P, P, P, P, P, P]
    lib.anr_train_ray_sample.argtypes = [ctypes.c_int, ctypes.c_int, D, D, D, D, ctypes.c_int, P, P, P, P, P, P, P,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_uint64, ctypes.c_uint64, P, P, P, P, P, P, P, P, P, P, P]
    lib.anr_alpha_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_alpha_workspace_bytes.argtypes = [ctypes.c_long, ctypes.POINTER(AlphaOpts), ctypes.POINTER(Frame)]
    lib.anr_alpha_points.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(Frame), P, ctypes.c_long,
                                     ctypes.POINTER(AlphaOpts), P, P, ctypes.c_size_t, P]
    lib.anr_alpha_counts.restype = P
    lib.anr_alpha_counts.argtypes = [P]
    lib.anr_mc_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_mc_workspace_bytes.argtypes = [ctypes.c_int] * 4
    lib.anr_mc_count.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, P, P,
                                 ctypes.c_size_t, P]
    lib.anr_mc_emit.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, P, P, P,
                                ctypes.c_size_t, P]
    lib.anr_anim_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_anim_workspace_bytes.argtypes = [ctypes.c_int]
    lib.anr_anim_step.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p * NUM_NOVEL_TENSORS, ctypes.POINTER(Frame), P,
                                  ctypes.c_int, P, ctypes.c_int, ctypes.POINTER(RenderOpts), P, P, ctypes.c_size_t, P]
    S, PP, PF, PO = ctypes.POINTER(Samples), ctypes.POINTER(Params), ctypes.POINTER(Frame), ctypes.POINTER(RenderOpts)
    for name in ('anr_network_workspace_bytes', 'anr_network_train_workspace_bytes'):
        getattr(lib, name).restype = ctypes.c_size_t
        getattr(lib, name).argtypes = [ctypes.c_int, PO, PF]
    lib.anr_network_fwd.argtypes = [PP, PF, S, PO, P, P, ctypes.c_size_t, P]
    lib.anr_network_train_fwd.argtypes = [PP, PF, S, PO, P, P, ctypes.c_size_t, P]
    lib.anr_network_train_bwd.argtypes = [PP, ctypes.c_void_p * NUM_TENSORS, PF, S, PO, P, P, P, P, ctypes.c_size_t, P]
    lib.anr_network_counts.restype = P
    lib.anr_network_counts.argtypes = [P, ctypes.c_int]
    lib.anr_network_bw_rows.argtypes = [P, ctypes.c_int, P, P, P]
    lib.anr_points_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_points_workspace_bytes.argtypes = [ctypes.c_int]
    lib.anr_blend_weights.argtypes = [PP, ctypes.c_int, P, P, ctypes.c_int, P, ctypes.c_int, P, P, ctypes.c_size_t, P]
    lib.anr_canonical_alpha.argtypes = [PP, P, ctypes.c_int, P, P, ctypes.c_size_t, P]
    lib.anr_profile_enable.argtypes = [ctypes.c_int]
    lib.anr_profile_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    lib.anr_profile_read_clock.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_double)]
    lib.anr_train_deterministic.argtypes = [ctypes.c_int]
    lib.anr_eval_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_eval_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.anr_eval_frame.argtypes = [P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(EvalOpts), P,
                                   P, P, P, P, P, ctypes.c_size_t, P]
    lib.anr_bw_volume_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_bw_volume_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.anr_bw_volume.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_int, D, ctypes.c_double, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, ctypes.POINTER(BwvOpts), P, P, P, ctypes.c_size_t, P]
    lib.anr_mesh_cc_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_mesh_cc_workspace_bytes.argtypes = [ctypes.c_long, ctypes.c_long]
    lib.anr_mesh_cc_count.argtypes = [P, ctypes.c_long, ctypes.c_long, P, P, P, ctypes.c_size_t, P]
    lib.anr_mesh_cc_emit.argtypes = [P, P, ctypes.c_long, ctypes.c_long, P, P, P, ctypes.c_size_t, P]
    lib.anr_mesh_dist_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_mesh_dist_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    MO = ctypes.POINTER(MeshDistOpts)
    lib.anr_mesh_sample.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_int, P, P, P, P, ctypes.c_size_t, P]
    lib.anr_mesh_point_dist.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_int, MO, P, P, P, P,
                                        ctypes.c_size_t, P]
    lib.anr_mesh_order.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, P, ctypes.c_size_t, P]
    lib.anr_mesh_metrics.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_int, P, ctypes.c_int, P, MO, P, P,
                                     ctypes.c_size_t, P]
    LO = ctypes.POINTER(RenderOpts)
    lib.anr_lbw_render_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_lbw_render_workspace_bytes.argtypes = [ctypes.c_int, LO, ctypes.c_int]
    lib.anr_lbw_render_fwd.argtypes = [ctypes.POINTER(LbwParams), ctypes.POINTER(LbwFrame), P, P, P, P, ctypes.c_int, LO,
                                       ctypes.POINTER(LbwRenderOut), ctypes.c_int, P, ctypes.c_size_t, P]
    lib.anr_lbw_render_counts.restype = P
    lib.anr_lbw_render_counts.argtypes = [P, ctypes.c_int, LO, ctypes.c_int]
    lib.anr_lbw_render_knn.restype = P
    lib.anr_lbw_render_knn.argtypes = [P, ctypes.c_int, LO, ctypes.c_int]
    for name in ('anr_lbw_render_kept', 'anr_lbw_render_points'):
        getattr(lib, name).restype = P
        getattr(lib, name).argtypes = [P, ctypes.c_int, LO, ctypes.c_int]
    lib.anr_lbw_render_rows.argtypes = [P, ctypes.c_int, LO, P, P, P, P]
    lib.anr_pdf_render_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_pdf_render_workspace_bytes.argtypes = [ctypes.c_int, LO, ctypes.c_int]
    lib.anr_pdf_render_fwd.argtypes = [ctypes.POINTER(PdfParams), ctypes.POINTER(PdfFrame), P, P, P, P, ctypes.c_int, LO,
                                       ctypes.POINTER(PdfRenderOut), ctypes.c_int, P, ctypes.c_size_t, P]
    for name in ('anr_pdf_render_counts', 'anr_pdf_render_knn', 'anr_pdf_render_kept', 'anr_pdf_render_points',
                 'anr_pdf_render_bigpose'):
        getattr(lib, name).restype = P
        getattr(lib, name).argtypes = [P, ctypes.c_int, LO, ctypes.c_int]
    lib.anr_pdf_render_rows.argtypes = [P, ctypes.c_int, LO, P, P, P]
    lib.anr_pdf_alpha_workspace_bytes.restype = ctypes.c_size_t
    lib.anr_pdf_alpha_workspace_bytes.argtypes = [ctypes.c_long, ctypes.POINTER(AlphaOpts)]
    lib.anr_pdf_alpha_points.argtypes = [ctypes.POINTER(PdfParams), ctypes.POINTER(PdfFrame), P, ctypes.c_long,
                                         ctypes.POINTER(AlphaOpts), P, P, ctypes.c_size_t, P]
    lib.anr_last_error.restype = ctypes.c_char_p
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = _lib.anr_last_error().decode() if _lib is not None else ''
        raise RuntimeError(f'{what} failed (code {rc}): {msg}')


class deterministic:
    """Scope of the library's deterministic training mode (``anr_train_deterministic``): sets the
    process-wide mode on entry and restores the value that was in force on exit, so callers in
    different modes can coexist in one process. ``on=None`` leaves the mode alone."""

    def __init__(self, on):
        self.on = on
        self.prev = None

    def __enter__(self):
        if self.on is not None:
            self.prev = load().anr_train_deterministic(1 if self.on else 0)
            if self.prev < 0:
                raise RuntimeError(f'anr_train_deterministic failed (code {-self.prev})')
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            load().anr_train_deterministic(self.prev)
        return False


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
