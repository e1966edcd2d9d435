"""ctypes mirrors of the helper probes and small-kernel entries of the test-only entry library
(tests/csrc/anr_testapi_small.hip, linked into tests/libanr_testapi.so). The library handle and the return
codes are tests/_gemm_hooks.py's. Loaded by the helper and small-kernel tests only; not a test file."""
import ctypes as C
import functools

from . import _gemm_hooks as G
from ._gemm_hooks import OK, E_NULL, E_SHAPE, E_SLAB, E_HIP, stream_ptr, vp, i32, i64, f32  # noqa: F401

# anr_test_probe1's selectors
SINCOS, SP_FAC, SP, EXP, LOG1P, SPF_H, DIV = range(7)
# anr_test_probe_embed's selectors
EMBED_FEATURE, EMBED, EMBED_B = range(3)
# path selectors of the compaction and alpha_ind entries
PATH_AUTO, PATH_GENERAL, PATH_ONE = range(3)


class Compact(C.Structure):
    _fields_ = [
        ('n_rays', i32), ('chunk', i32), ('ray_offset', i32), ('path', i32),
        ('mask', vp), ('chunk_min', vp), ('ray_off', vp), ('block_sum', vp), ('list', vp), ('total', vp),
        ('list_cap', i64),
    ]


class Alpha(C.Structure):
    _fields_ = [
        ('n_rays', i32), ('chunk', i32), ('ray_offset', i32), ('path', i32),
        ('train_th', f32), ('pad0', i32),
        ('ray_off', vp), ('n_kept', vp), ('sigma', vp), ('chunk_max', vp), ('flags', vp), ('block_sum', vp),
        ('out_row', vp), ('list', vp), ('mask', vp), ('total', vp),
    ]


class Composite(C.Structure):
    _fields_ = [
        ('n_rays', i32), ('pad0', i32),
        ('raw', vp), ('near_', vp), ('far_', vp), ('t_rand', vp),
        ('rgb', vp), ('acc', vp), ('depth', vp), ('weights', vp),
    ]


# anr_test_small_sizeof's indices, numbered on from _tchain_hooks.SIZEOF
SIZEOF = {7: Compact, 8: Alpha, 9: Composite}


@functools.lru_cache(maxsize=1)
def lib():
    """The test entry library with the small entries' signatures set."""
    L = G.lib()
    L.anr_test_small_sizeof.argtypes = [i32]
    L.anr_test_small_sizeof.restype = i32
    L.anr_test_probe1.argtypes = [i32, vp, vp, vp, i64, f32, f32, vp]
    L.anr_test_probe_inv33.argtypes = [vp, vp, i64, vp]
    L.anr_test_probe_embed.argtypes = [i32, vp, i32, vp, i64, vp]
    L.anr_test_embed_tan.argtypes = [vp, i64, vp, i64, i32, i32, vp, i64, i32, f32, vp]
    L.anr_test_embed_rev6.argtypes = [vp, i64, vp, i64, vp, vp, i32, vp, vp, vp]
    L.anr_test_embed_bwd10.argtypes = [vp, i64, vp, i64, i32, vp, i64, vp]
    L.anr_test_scan_blocks.argtypes = [vp, i32, vp, vp]
    L.anr_test_compact_run.argtypes = [C.POINTER(Compact), vp]
    L.anr_test_alpha_run.argtypes = [C.POINTER(Alpha), vp]
    L.anr_test_composite_run.argtypes = [C.POINTER(Composite), vp]
    for nm in ('anr_test_probe1', 'anr_test_probe_inv33', 'anr_test_probe_embed', 'anr_test_embed_tan',
               'anr_test_embed_rev6', 'anr_test_embed_bwd10', 'anr_test_scan_blocks', 'anr_test_compact_run',
               'anr_test_alpha_run', 'anr_test_composite_run'):
        getattr(L, nm).restype = i32
    return L
