"""CPU: anr_mesh_sample, anr_mesh_point_dist and anr_mesh_metrics reject bad arguments before any HIP call
(no GPU needed; the dummy pointers are never dereferenced), and the workspace size refuses the caps."""
import ctypes
import os

import pytest

from animatable_nerf_amd import _lib

ARG, WORKSPACE = 2, 3
BIG = 1 << 40


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def p(v):
    return ctypes.c_void_p(v) if v else None


def opts_ref(opts):
    if opts == 'default':
        opts = _lib.MeshDistOpts()
    return ctypes.byref(opts) if opts is not None else None


def sample(lib, verts=1, nv=10, faces=1, nf=4, u=1, n=100, points=1, face=1, status=1, ws=1, ws_bytes=BIG):
    return lib.anr_mesh_sample(p(verts), nv, p(faces), nf, p(u), n, p(points), p(face), p(status), p(ws), ws_bytes, None)


def dist(lib, verts=1, nv=10, faces=1, nf=4, points=1, n=100, opts='default', out=1, face=None, mean=None, ws=1,
         ws_bytes=BIG):
    return lib.anr_mesh_point_dist(p(verts), nv, p(faces), nf, p(points), n, opts_ref(opts), p(out), p(face), p(mean),
                                   p(ws), ws_bytes, None)


def metrics(lib, sv=1, snv=10, sf=1, snf=4, tv=1, tnv=10, tf=1, tnf=4, u=1, opts='default', out=1, ws=1, ws_bytes=BIG):
    return lib.anr_mesh_metrics(p(sv), snv, p(sf), snf, p(tv), tnv, p(tf), tnf, p(u), opts_ref(opts), p(out), p(ws),
                                ws_bytes, None)


def test_opts_struct():
    o = _lib.MeshDistOpts(_lib.BWV_EXHAUSTIVE, 10, 20)
    assert ctypes.sizeof(_lib.MeshDistOpts) == 16 and o.struct_size == 16
    assert (o.exhaustive, o.n_chamfer, o.n_p2s) == (1, 10, 20)
    assert _lib.MESHM_NOUT == 8


@pytest.mark.parametrize('kw', [dict(verts=0), dict(faces=0), dict(u=0), dict(points=0), dict(face=0), dict(status=0),
                                dict(ws=0)])
def test_sample_null_pointers(lib, kw):
    assert sample(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('kw,word', [(dict(nv=0), b'nv'), (dict(nv=-2), b'nv'), (dict(nf=(1 << 26) + 1), b'2^26'),
                                     (dict(n=0), b'n must'), (dict(n=-1), b'n must'), (dict(n=(1 << 24) + 1), b'2^24')])
def test_sample_bad_values(lib, kw, word):
    assert sample(lib, **kw) == ARG
    assert word in lib.anr_last_error()


def test_sample_workspace(lib):
    need = lib.anr_mesh_dist_workspace_bytes(4, 100)
    assert sample(lib, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    # a mesh without faces is a status on the device, not a rejected call: it gets as far as the workspace check
    assert sample(lib, verts=0, faces=0, nv=0, nf=0, ws_bytes=0) == WORKSPACE


@pytest.mark.parametrize('kw', [dict(verts=0), dict(faces=0), dict(points=0), dict(out=0), dict(ws=0)])
def test_point_dist_null_pointers(lib, kw):
    assert dist(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('kw,word', [(dict(nv=0), b'nv'), (dict(nf=0), b'nf'), (dict(nf=-1), b'nf'),
                                     (dict(nf=(1 << 26) + 1), b'2^26'), (dict(n=0), b'n must'),
                                     (dict(n=(1 << 24) + 1), b'2^24')])
def test_point_dist_bad_values(lib, kw, word):
    assert dist(lib, **kw) == ARG
    assert word in lib.anr_last_error()


def test_bad_opts(lib):
    o = _lib.MeshDistOpts()
    o.struct_size = 12
    assert dist(lib, opts=o) == ARG and b'struct_size' in lib.anr_last_error()
    assert metrics(lib, opts=o) == ARG and b'struct_size' in lib.anr_last_error()
    assert dist(lib, opts=_lib.MeshDistOpts(4)) == ARG and b'exhaustive' in lib.anr_last_error()
    assert dist(lib, opts=_lib.MeshDistOpts(_lib.MESHDIST_PRUNED_CELLS), ws_bytes=0) == WORKSPACE  # 3 is a search
    assert dist(lib, opts=_lib.MeshDistOpts(-1)) == ARG
    assert metrics(lib, opts=_lib.MeshDistOpts(0, -1, 0)) == ARG and b'n_chamfer' in lib.anr_last_error()
    assert metrics(lib, opts=_lib.MeshDistOpts(0, 1 << 23, 1)) == ARG and b'2^24' in lib.anr_last_error()


def test_point_dist_workspace(lib):
    need = lib.anr_mesh_dist_workspace_bytes(4, 100)
    assert dist(lib, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    assert dist(lib, opts=None, ws_bytes=0) == WORKSPACE  # NULL opts: the defaults


@pytest.mark.parametrize('kw', [dict(sv=0), dict(sf=0), dict(tv=0), dict(tf=0), dict(u=0), dict(out=0), dict(ws=0)])
def test_metrics_null_pointers(lib, kw):
    assert metrics(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('kw,word', [(dict(snv=0), b'nv'), (dict(tnv=-1), b'nv'), (dict(snf=(1 << 26) + 1), b'2^26'),
                                     (dict(tnf=(1 << 26) + 1), b'2^26')])
def test_metrics_bad_values(lib, kw, word):
    assert metrics(lib, **kw) == ARG
    assert word in lib.anr_last_error()


def test_metrics_workspace(lib):
    need = lib.anr_mesh_dist_workspace_bytes(4, 12000)
    assert metrics(lib, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    assert metrics(lib, opts=None, ws_bytes=need - 1) == WORKSPACE
    # the larger face count sizes it
    assert metrics(lib, tnf=4000, ws_bytes=need) == WORKSPACE


def test_workspace_bytes(lib):
    a = lib.anr_mesh_dist_workspace_bytes(19712, 12000)
    assert 0 < a < 16 << 20 and a % 256 == 0
    big = lib.anr_mesh_dist_workspace_bytes(3_100_000, 12000)
    assert a < big < 1 << 30
    assert big < 200 * a  # linear in the face count (157x the faces)
    assert lib.anr_mesh_dist_workspace_bytes(19712, 24000) > a
    assert lib.anr_mesh_dist_workspace_bytes(1 << 26, 1 << 24) > 0  # the caps themselves are accepted
    for bad in ((0, 100), (-1, 100), (4, 0), (4, -5), ((1 << 26) + 1, 100), (4, (1 << 24) + 1)):
        assert lib.anr_mesh_dist_workspace_bytes(*bad) == 0


def order(lib, verts=1, nv=10, faces=1, nf=4, perm=1, ws=1, ws_bytes=BIG):
    return lib.anr_mesh_order(p(verts), nv, p(faces), nf, p(perm), p(ws), ws_bytes, None)


def test_order_rejects_bad_arguments(lib):
    for kw in (dict(verts=0), dict(faces=0), dict(perm=0), dict(ws=0)):
        assert order(lib, **kw) == ARG and b'NULL' in lib.anr_last_error()
    for kw in (dict(nv=0), dict(nf=0), dict(nf=(1 << 26) + 1)):
        assert order(lib, **kw) == ARG
    assert order(lib, ws_bytes=lib.anr_mesh_dist_workspace_bytes(4, 1) - 1) == WORKSPACE
