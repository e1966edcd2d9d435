"""CPU: anr_bw_volume rejects bad arguments before any HIP call (no GPU needed), and the workspace
size behaves."""
import ctypes
import os

import pytest

from animatable_nerf_amd import _lib

ARG, WORKSPACE = 2, 3


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def call(lib, verts=1, nv=10, faces=1, nf=4, skin=1, nb=24, origin=True, vsize=0.025, dims=(4, 5, 6), opts='surface',
         volume=1, index=None, ws=1, ws_bytes=1 << 30):
    """anr_bw_volume with dummy non-NULL device pointers (never dereferenced when the call is rejected)."""
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0) if origin else None
    if opts == 'surface':
        opts = _lib.BwvOpts(_lib.BWV_SURFACE)
    elif opts == 'vertex':
        opts = _lib.BwvOpts(_lib.BWV_VERTEX)
    o = ctypes.byref(opts) if opts is not None else None
    return lib.anr_bw_volume(p(verts), nv, p(faces), nf, p(skin), nb, org, vsize, dims[0], dims[1], dims[2], o,
                             p(volume), p(index), p(ws), ws_bytes, None)


def test_opts_struct():
    o = _lib.BwvOpts(_lib.BWV_SURFACE, _lib.BWV_EXHAUSTIVE)
    assert ctypes.sizeof(_lib.BwvOpts) == 12 and o.struct_size == 12
    assert (o.mode, o.exhaustive) == (1, 1)


@pytest.mark.parametrize('kw', [dict(verts=0), dict(skin=0), dict(origin=False), dict(volume=0), dict(ws=0)])
def test_null_pointers(lib, kw):
    assert call(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('kw,word', [
    (dict(nb=0), b'nb'), (dict(nb=65), b'nb'), (dict(nv=0), b'nv'), (dict(nv=-3), b'nv'),
    (dict(nf=0), b'faces'), (dict(nf=-1), b'faces'), (dict(faces=0), b'faces'),
    (dict(opts='vertex', nf=-1), b'nf'),
    (dict(dims=(0, 5, 6)), b'X, Y, Z'), (dict(dims=(4, 5, -1)), b'X, Y, Z'), (dict(dims=(1 << 12, 1 << 12, 1 << 12)), b'2^28'),
    (dict(vsize=0.0), b'vsize'), (dict(vsize=float('nan')), b'vsize'),
])
def test_bad_values(lib, kw, word):
    assert call(lib, **kw) == ARG
    assert word in lib.anr_last_error()


def test_bad_opts(lib):
    o = _lib.BwvOpts(_lib.BWV_SURFACE)
    o.struct_size = 8
    assert call(lib, opts=o) == ARG and b'struct_size' in lib.anr_last_error()
    assert call(lib, opts=_lib.BwvOpts(2)) == ARG and b'mode' in lib.anr_last_error()
    assert call(lib, opts=_lib.BwvOpts(_lib.BWV_SURFACE, 3)) == ARG and b'exhaustive' in lib.anr_last_error()
    assert call(lib, opts=_lib.BwvOpts(_lib.BWV_SURFACE, -1)) == ARG


def test_vertex_mode_needs_no_faces_but_a_workspace(lib):
    # valid vertex-mode arguments without faces get as far as the workspace check, which rejects them
    assert call(lib, opts='vertex', faces=0, nf=0, ws_bytes=0) == WORKSPACE
    assert call(lib, opts=None, faces=0, nf=0, ws_bytes=0) == WORKSPACE  # NULL opts: vertex mode
    need = lib.anr_bw_volume_workspace_bytes(10, 4, 4, 5, 6)
    assert call(lib, ws_bytes=need - 1) == WORKSPACE
    assert b'workspace' in lib.anr_last_error()


def test_workspace_bytes(lib):
    a = lib.anr_bw_volume_workspace_bytes(6890, 13776, 63, 75, 38)
    assert 0 < a < 64 << 20
    assert lib.anr_bw_volume_workspace_bytes(6890, 0, 63, 75, 38) <= a
    assert lib.anr_bw_volume_workspace_bytes(6890, 13776, 126, 75, 38) > a
    assert a % 256 == 0
    for bad in ((0, 4, 4, 5, 6), (10, -1, 4, 5, 6), (10, 4, 0, 5, 6), (10, 4, 1 << 12, 1 << 12, 1 << 12)):
        assert lib.anr_bw_volume_workspace_bytes(*bad) == 0
