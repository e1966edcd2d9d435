"""ctypes mirrors of the test-only entry library (tests/csrc/anr_testapi.hip -> tests/libanr_testapi.so) and
the device side of the guarded buffers of tests/gemm_ref.py. Loaded by the GEMM kernel tests only; not a
test file."""
import ctypes as C
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libanr_testapi.so')

OK, LAUNCHER = 0, -1
E_NULL, E_SHAPE, E_LAYOUT, E_SPLITK, E_EPILOGUE, E_FORMAT, E_ALIGN, E_SLAB, E_UNSUPPORTED, E_HIP = range(-100, -110, -1)

WG_SINGLE, WG_F32, WG_GROUP = 0, 1, 2

vp, i32, i64, u64, f32 = C.c_void_p, C.c_int, C.c_long, C.c_ulonglong, C.c_float


class GemmDesc(C.Structure):
    _fields_ = [
        ('M', i32), ('N', i32), ('nseg', i32), ('K', i32 * 2),
        ('M_dev', vp), ('K_dev', vp),
        ('A', vp * 2), ('a_rs', i64 * 2), ('a_cs', i64 * 2),
        ('B', vp * 2), ('b_rs', i64 * 2), ('b_cs', i64 * 2),
        ('C', vp), ('ldc', i64), ('bias', vp), ('relu', i32), ('accumulate', i32),
        ('mask', vp), ('ldm', i64),
        ('atomic', i32), ('ksplit', i32), ('kper', i32), ('softplus', i32),
        ('div_pre', f32), ('div_post', f32), ('spd_scale', f32),
        ('deriv', vp), ('ldd', i64), ('spd', vp), ('ldsd', i64),
        ('spd_n', i32), ('spd_h', i32), ('bf16', i32), ('x3', i32),
        ('rowsum', vp), ('rowsum2', vp),
        ('det', i32), ('pad0', i32), ('scratch', vp), ('scratch_floats', u64),
        ('a_softplus_w', vp), ('head_w', vp), ('head_b', vp), ('head_out', vp), ('ldh', i64),
        ('head_n', i32), ('cus', i32), ('img', vp), ('img_bytes', u64),
        ('out_a_k', i32), ('out_b_k', i32), ('out_sw', i32),
        ('out_a_vec', i32 * 2), ('out_b_vec', i32 * 2), ('out_vec_out', i32),
        ('out_image_bytes', u64),
    ]


class RGemmDesc(C.Structure):
    _fields_ = [
        ('M_host', i32), ('N', i32), ('nseg', i32), ('K', i32 * 2), ('bcol', i32 * 2), ('rows', i32 * 2),
        ('M_dev', vp), ('A', vp * 2), ('lda', i64 * 2), ('B', vp * 2), ('ldb', i64 * 2), ('lo_off', i64 * 2),
        ('C', vp), ('ldc', i64), ('bias', vp), ('mask', vp), ('ldm', i64),
        ('relu', i32), ('accumulate', i32), ('x3', i32), ('abf', i32), ('cbf', i32), ('mbf', i32),
        ('out_vec_out', i32), ('out_vec16', i32), ('out_variant', i32),
    ]


class WView(C.Structure):
    _fields_ = [('B', vp), ('ldb', i64), ('lo_off', i64), ('bcol', i32), ('rows', i32)]


class WGradDesc(C.Structure):
    _fields_ = [
        ('dY', vp), ('ldY', i64), ('X', vp), ('ldX', i64), ('dW', vp), ('ldw', i64), ('bsum', vp), ('bsum2', vp),
        ('M_dev', vp), ('nout', i32), ('K', i32), ('x3', i32), ('ybf', i32), ('xbf', i32), ('j0', i32),
    ]


class WGradCall(C.Structure):
    _fields_ = [
        ('mode', i32), ('det', i32), ('n_host', i32), ('nd', i32), ('nz', i32), ('pad0', i32),
        ('d', C.POINTER(WGradDesc)), ('slab', vp), ('slab_floats', u64),
        ('out_f32_fits', i32), ('out_format', i32),
    ]


SIZEOF = {0: GemmDesc, 1: RGemmDesc, 2: WGradDesc, 3: WGradCall, 4: WView}


@functools.lru_cache(maxsize=1)
def lib():
    """The test entry library; a missing library is an error (the build makes it)."""
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} is missing: run the build (make) first')
    L = C.CDLL(LIB_PATH)
    L.anr_test_sizeof.argtypes = [i32]
    L.anr_test_sizeof.restype = i32
    for nm, T in (('anr_test_gemm', GemmDesc), ('anr_test_lgemm', GemmDesc), ('anr_test_rgemm', RGemmDesc),
                  ('anr_test_wgrad', WGradCall)):
        f = getattr(L, nm)
        f.argtypes = [C.POINTER(T), vp]
        f.restype = i32
    L.anr_test_lgemm_pack_batch.argtypes = [C.POINTER(GemmDesc), i32, C.POINTER(vp), vp, vp, vp]
    L.anr_test_lgemm_pack_batch.restype = i32
    L.anr_test_gemm_det_floats.argtypes = [i32, i32, i32]
    L.anr_test_gemm_det_floats.restype = u64
    L.anr_test_wgrad_slab_floats.argtypes = []
    L.anr_test_wgrad_slab_floats.restype = u64
    L.anr_test_wimg_bytes.argtypes = []
    L.anr_test_wimg_bytes.restype = u64
    L.anr_test_wimg_pack.argtypes = [C.POINTER(vp), vp, vp]
    L.anr_test_wimg_pack.restype = i32
    L.anr_test_wimg_view.argtypes = [vp, C.POINTER(vp), vp, i32, i32, i32, C.POINTER(WView)]
    L.anr_test_wimg_view.restype = i32
    return L


# ---- device side of gemm_ref.Buf ------------------------------------------------------------------------
class DevBufs:
    """The allocations of a case on the device: upload, pointers, download."""

    def __init__(self, bufs, dev):
        import torch
        self.bufs = bufs
        self.t = {}
        for k, b in bufs.items():
            a = b.flat
            if a.dtype == np.uint16:  # torch has no uint16 arithmetic; the bits travel as int16
                a = a.view(np.int16)
            self.t[k] = torch.from_numpy(a.copy()).to(dev)
            assert self.t[k].data_ptr() % 256 == 0  # the allocator's alignment the `aligned` flag builds on

    def ptr(self, k):
        if k not in self.bufs:
            return None
        b = self.bufs[k]
        return self.t[k].data_ptr() + b.off * b.flat.dtype.itemsize

    def get(self, k):
        a = self.t[k].cpu().numpy()
        return a.view(np.uint16) if self.bufs[k].flat.dtype == np.uint16 else a

    def reset(self, k):
        """Back to the uploaded content (a second run on the same buffers)."""
        import torch
        a = self.bufs[k].flat
        self.t[k].copy_(torch.from_numpy((a.view(np.int16) if a.dtype == np.uint16 else a).copy()))

    def check_outputs(self):
        from . import gemm_ref as R
        rep = {}
        for k, b in self.bufs.items():
            if b.out:
                rep[k] = R.check_out(k, b, self.get(k))
        return rep


def dev_int(v, dev):
    import torch
    return torch.tensor([int(v)], dtype=torch.int32, device=dev)


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gemm_desc(d, bufs, st, db, extra):
    """The descriptor of a gemm_ref.GemmCase on the device buffers db; extra: M_dev / K_dev int tensors."""
    c = d.case
    g = GemmDesc()
    g.M, g.N, g.nseg = c.M, c.N, len(c.K)
    for s, K in enumerate(c.K):
        g.K[s] = K
        g.A[s], g.B[s] = db.ptr(f'A{s}'), db.ptr(f'B{s}')
        g.a_rs[s], g.a_cs[s] = st[f'a{s}']
        g.b_rs[s], g.b_cs[s] = st[f'b{s}']
    g.M_dev = extra['M_dev'].data_ptr() if 'M_dev' in extra else None
    g.K_dev = extra['K_dev'].data_ptr() if 'K_dev' in extra else None
    g.C, g.ldc = db.ptr('C'), st['ldc']
    g.bias = db.ptr('bias')
    g.relu, g.accumulate, g.atomic = int(c.relu), int(c.accumulate), int(c.atomic)
    g.mask, g.ldm = db.ptr('mask'), st.get('ldm', 0)
    g.ksplit, g.kper = c.ksplit, c.kper
    g.softplus = int(c.softplus)
    g.div_pre, g.div_post, g.spd_scale = c.div_pre, c.div_post, c.spd_scale
    g.deriv, g.ldd = db.ptr('deriv'), st.get('ldd', 0)
    g.spd, g.ldsd, g.spd_n, g.spd_h = db.ptr('spd'), st.get('ldsd', 0), c.spd_n, int(c.spd == 'h')
    g.bf16, g.x3 = int(c.prec == 'bf16'), int(c.prec == 'x3')
    g.rowsum, g.rowsum2 = db.ptr('rowsum'), db.ptr('rowsum2')
    g.det = int(c.det)
    g.a_softplus_w = db.ptr('atr')
    g.head_w, g.head_b, g.head_out = db.ptr('head_w'), db.ptr('head_b'), db.ptr('head_out')
    g.ldh, g.head_n = st.get('ldh', 0), c.head_n
    return g


def rgemm_desc(rc, st, db, M_dev_t):
    """The descriptor of a gemm_ref.RCase on the device buffers db."""
    g = RGemmDesc()
    g.M_host, g.N, g.nseg = rc.M, rc.N, len(rc.K)
    for s, K in enumerate(rc.K):
        g.K[s], g.bcol[s], g.rows[s] = K, rc.bcol[s], rc.rows[s]
        g.A[s], g.lda[s] = db.ptr(f'A{s}'), st[f'lda{s}']
        g.B[s], g.ldb[s], g.lo_off[s] = db.ptr(f'B{s}'), st[f'ldb{s}'], st[f'lo_off{s}']
    g.M_dev = M_dev_t.data_ptr() if M_dev_t is not None else None
    g.C, g.ldc, g.bias = db.ptr('C'), st['ldc'], db.ptr('bias')
    g.mask, g.ldm = db.ptr('mask'), st.get('ldm', 0)
    g.relu, g.accumulate = int(rc.relu), int(rc.accumulate)
    g.x3, g.abf, g.cbf, g.mbf = int(rc.x3), int(rc.abf), int(rc.cbf), int(rc.mbf)
    return g


def wgrad_desc(wc, st, db, M_dev_t):
    """The WGradDesc of a gemm_ref.WCase on the device buffers db (dW: the window's first element)."""
    g = WGradDesc()
    g.dY, g.ldY, g.X, g.ldX = db.ptr('dY'), st['ldY'], db.ptr('X'), st['ldX']
    g.dW, g.ldw = db.ptr('dW') + 4 * st['c0'], st['ldw']
    g.bsum, g.bsum2 = db.ptr('bsum'), db.ptr('bsum2')
    g.M_dev = M_dev_t.data_ptr() if M_dev_t is not None else None
    g.nout, g.K = wc.nout, wc.K
    g.x3, g.ybf, g.xbf, g.j0 = int(wc.fmt == 'x3'), int(wc.ybf), int(wc.xbf), wc.j0
    return g
