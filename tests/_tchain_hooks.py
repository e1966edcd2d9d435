"""ctypes mirrors of the chain entries of the test-only entry library (tests/csrc/anr_testapi_tchain.hip, linked
into tests/libanr_testapi.so). The library handle, the return codes and the device side of the guarded
buffers are tests/_gemm_hooks.py's, passed on here so that the chain tests import one module. Loaded by the
chain kernel tests only; not a test file."""
import ctypes as C
import functools

from . import _gemm_hooks as G
from ._gemm_hooks import (OK, LAUNCHER, E_NULL, E_SHAPE, E_ALIGN, E_SLAB,  # noqa: F401
                          DevBufs, dev_int, stream_ptr, vp, i32, i64, u64)


class TcPackLayer(C.Structure):
    """The caller-filled fields of TcPackLayer (anr_train.h)."""
    _fields_ = [
        ('W', vp), ('in_ch', i32), ('n1', i32), ('W2', vp), ('in_ch2', i32), ('n2', i32),
        ('cmem', i32), ('kmem_cols', i32), ('cprev', i32), ('kprev_cols', i32),
        ('oc0', i32), ('oa', i32), ('oc1', i32), ('nb', i32), ('ob_b0', i32), ('pad0', i32),
    ]


class TcRun(C.Structure):
    """TcArgs (anr_train.h), the launch shape, the host copy of M and every row buffer's capacity in rows."""
    _fields_ = [
        ('prog', i32), ('cap', i32), ('cus', i32), ('M_host', i32),
        ('img', vp), ('bias', vp * 12), ('bias2', vp), ('nout', i32 * 12),
        ('out', vp * 12), ('ldo', i32 * 12), ('out_rows', i64 * 12), ('out2', vp), ('out2_rows', i64),
        ('mem', vp), ('ld_mem', i32), ('kmem_cols', i32), ('mem_rows', i64),
        ('mem2', vp), ('ld_mem2', i32), ('kmem2_cols', i32), ('mem2_rows', i64),
        ('mem_f32', i32), ('mem2_f32', i32),
        ('bits', vp * 12), ('bits_rows', i64 * 12),
        ('aux', vp), ('ld_aux', i32), ('aux_cols', i32), ('aux_acc', i32), ('pad0', i32), ('aux_rows', i64),
        ('M_dev', vp),
    ]


# anr_test_tchain_sizeof's indices, numbered on from _gemm_hooks.SIZEOF
SIZEOF = {5: TcPackLayer, 6: TcRun}


@functools.lru_cache(maxsize=1)
def lib():
    """The test entry library with the chain entries' signatures set."""
    L = G.lib()
    L.anr_test_tchain_sizeof.argtypes = [i32]
    L.anr_test_tchain_sizeof.restype = i32
    L.anr_test_tchain_image_bytes.argtypes = [i32]
    L.anr_test_tchain_image_bytes.restype = u64
    L.anr_test_tchain_pack.argtypes = [i32, C.POINTER(TcPackLayer), vp, u64, vp]
    L.anr_test_tchain_pack.restype = i32
    L.anr_test_tchain_run.argtypes = [C.POINTER(TcRun), vp]
    L.anr_test_tchain_run.restype = i32
    L.anr_test_tchain_check.argtypes = [C.POINTER(TcRun)]
    L.anr_test_tchain_check.restype = i32
    return L
