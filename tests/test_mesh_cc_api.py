"""CPU: anr_mesh_cc_count / anr_mesh_cc_emit reject bad arguments before any HIP call (no GPU needed), the
workspace size behaves, and the meshes of tests/meshcc_cases.py have, under the host pass alone, the
properties the GPU tests (tests/test_gpu_mesh_cc.py) rely on, so that none of those can pass vacuously."""
import ctypes
import os

import numpy as np
import pytest

from animatable_nerf_amd import _lib
from animatable_nerf_amd.renderer_sdf_mesh import largest_component

from . import meshcc_cases as mc

ARG, WORKSPACE = 2, 3
BIG = 1 << 40


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libaninerf_hip.so is not built (run `make` / __graft_entry__.build())')
    return _lib.load()


def p(v):
    return ctypes.c_void_p(v) if v else None


def count(lib, tris=1, nt=12, nv=8, counts=1, labels=0, ws=1, ws_bytes=BIG):
    """anr_mesh_cc_count with dummy non-NULL device pointers (never dereferenced when the call is rejected)"""
    return lib.anr_mesh_cc_count(p(tris), nt, nv, p(counts), p(labels), p(ws), ws_bytes, None)


def emit(lib, verts=1, tris=1, nt=12, nv=8, out_v=1, out_t=1, ws=1, ws_bytes=BIG):
    return lib.anr_mesh_cc_emit(p(verts), p(tris), nt, nv, p(out_v), p(out_t), p(ws), ws_bytes, None)


def test_workspace_bytes(lib):
    w = lib.anr_mesh_cc_workspace_bytes
    assert w(0, 0) > 0 and w(0, 0) % 256 == 0
    sizes = [w(1000, nt) for nt in (0, 1, 255, 256, 257, 2000, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert w(2000, 2000) > w(1000, 2000)
    # the reference's 5 mm grid (DESIGN: 3.1 M triangles) fits comfortably
    assert w(1_600_000, 3_100_000) < 1 << 30
    last = ((1 << 31) - 1) // 3  # the largest nt with 3 nt < 2^31
    assert w(10, last) > 0 and w(10, last + 1) == 0
    assert w((1 << 31) - 2, 10) > 0 and w((1 << 31) - 1, 10) == 0
    for bad in ((-1, 10), (10, -1), (10, 1 << 40), (1 << 40, 10)):
        assert w(*bad) == 0


@pytest.mark.parametrize('call,kw', [(count, dict(tris=0)), (count, dict(counts=0)), (count, dict(ws=0)),
                                     (emit, dict(verts=0)), (emit, dict(tris=0)), (emit, dict(out_v=0)),
                                     (emit, dict(out_t=0)), (emit, dict(ws=0))])
def test_null_pointers(lib, call, kw):
    assert call(lib, **kw) == ARG
    assert b'NULL' in lib.anr_last_error()


@pytest.mark.parametrize('call', [count, emit])
def test_sizes_and_workspace(lib, call):
    last = ((1 << 31) - 1) // 3
    assert call(lib, nt=last + 1) == ARG and b'2^31' in lib.anr_last_error()
    assert call(lib, nv=(1 << 31) - 1) == ARG and b'2^31' in lib.anr_last_error()
    assert call(lib, nt=-1) == ARG and b'negative' in lib.anr_last_error()
    assert call(lib, nv=-1) == ARG and b'negative' in lib.anr_last_error()
    need = lib.anr_mesh_cc_workspace_bytes(8, 12)
    assert call(lib, ws_bytes=need - 1) == WORKSPACE and b'workspace' in lib.anr_last_error()
    assert call(lib, ws_bytes=0) == WORKSPACE


def test_counts_layout():
    assert _lib.MESHCC_NCOUNT == 6
    assert (_lib.MESHCC_V, _lib.MESHCC_T, _lib.MESHCC_NCOMP, _lib.MESHCC_NWATERTIGHT, _lib.MESHCC_KEPT,
            _lib.MESHCC_STATUS) == tuple(range(6))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'aninerf.h')).read()
    assert '#define ANR_MESHCC_NCOUNT 6' in src


def test_device_function_refuses_host_arrays():
    from animatable_nerf_amd.renderer_sdf_mesh import largest_component_device
    import torch
    v, t = mc.case('boxes3')
    with pytest.raises(ValueError):
        largest_component_device(torch.from_numpy(v.copy()), torch.from_numpy(t.copy()))
    with pytest.raises(TypeError):
        largest_component_device(torch.from_numpy(v.copy()).float(), torch.from_numpy(t.copy()))


# ---- the cases ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', mc.CASES)
def test_host_labels_agree_with_the_host_pass(name):
    """the restated union-find gives the components the host pass keeps one of"""
    v, t = mc.case(name)
    kv, kt = mc.host(name)
    comps = mc.components(t)
    wt = {r: n for r, (ok, n) in comps.items() if ok}
    if not wt:
        assert kv.shape == v.shape and np.array_equal(kt, t)
        return
    best = min(r for r, n in wt.items() if n == max(wt.values()))
    sel = mc.labels(name) == best
    uv, inv = np.unique(t[sel], return_inverse=True)
    assert np.array_equal(kv, v[uv]) and np.array_equal(kt, inv.reshape(-1, 3))
    assert 0 < len(kt) < len(t) or len(comps) == 1


def test_boxes_cases():
    kv, kt = mc.host('boxes3')
    assert len(kv) == 8 and len(kt) == 12
    comps = mc.components(mc.case('boxes3')[1])
    assert sorted(comps.values()) == [(False, 8), (True, 8), (True, 8)]
    kv, kt = mc.host('glued')
    assert len(kv) == 8 and np.array_equal(kv, mc.box(0.0)[0])
    assert sorted(mc.components(mc.case('glued')[1]).values()) == [(False, 9), (True, 8), (True, 8)]
    v, t = mc.case('open')
    assert not any(ok for ok, _ in mc.components(t).values())
    assert mc.host('open')[0].shape == v.shape and np.array_equal(mc.host('open')[1], t)
    assert len(mc.case('empty')[1]) == 0 and len(mc.case('empty')[0]) == 4


@pytest.mark.parametrize('n', mc.TET_COUNTS)
def test_tet_cases_really_tie(n):
    for name, extra in ((f'tets{n}', 0), (f'tets{n}o', 1)):
        v, t = mc.case(name)
        assert len(t) == 4 * n + extra
        comps = mc.components(t)
        assert len(comps) == n + extra
        assert sum(ok for ok, _ in comps.values()) == n
        assert {nv for ok, nv in comps.values() if ok} == {4}  # every watertight piece ties
        kv, kt = mc.host(name)
        assert len(kv) == 4 and len(kt) == 4
        # the winner is the piece of face 0 (the lowest label), unless face 0 is the open triangle
        lab = mc.labels(name)
        win = min(r for r, (ok, _) in comps.items() if ok)
        assert np.array_equal(kv, v[np.unique(t[lab == win])])
        assert not np.array_equal(np.sort(t[:, 0]), t[:, 0])  # shuffled
    # nt straddles one 256-element scan block at n = 64
    assert [4 * m for m in mc.TET_COUNTS[:3]] == [252, 256, 260]


def test_tube_cases():
    v, t = mc.case('tube')
    assert 5000 < len(t) < 20000
    comps = mc.components(t)
    assert list(comps.values()) == [(True, len(v))]  # one closed piece using every vertex
    for name in ('tube_reversed', 'tube_random'):
        assert sorted(map(tuple, mc.case(name)[1].tolist())) == sorted(map(tuple, t.tolist()))
        assert not np.array_equal(mc.case(name)[1], t)


def test_bipyramid_shared_vertex_and_degenerate_cases():
    v, t = mc.case('bipyramid')
    assert mc.components(t) == {0: (True, 302)}
    assert np.bincount(t.ravel()).max() == 300  # valence above a wave (64) and a block (256)
    v, t = mc.case('shared_vertex')
    comps = mc.components(t)
    assert sorted(comps.values()) == [(True, 4), (True, 4)] and len(v) == 7  # 4 + 4 vertices of 7: one in both
    assert np.array_equal(mc.host('shared_vertex')[0], v[:4])
    v, t = mc.case('dup_degenerate')
    _, cnt, _ = mc.edge_multiplicities(t)
    assert set(cnt.tolist()) == {1, 2, 4}
    assert any(a == b for a, b, c in t.tolist())
    assert sorted(mc.components(t).values()) == [(False, 4), (False, 4), (True, 3), (True, 8)]
    assert len(mc.host('dup_degenerate')[0]) == 8


def test_vertex_order_cases():
    v, t = mc.case('unreferenced')
    assert len(np.unique(t)) == 8 and len(v) == 40
    assert len(mc.host('unreferenced')[0]) == 8
    v, t = mc.case('interleaved')
    kv, kt = mc.host('interleaved')
    kept = np.nonzero(np.isin(np.arange(len(v)), [1, 3, 5, 7, 8, 9, 10, 11]))[0]
    assert np.array_equal(kv, v[kept]) and np.any(np.diff(kept) > 1)
    v, t = mc.case('many_vertices')
    assert (len(v) + 1 + 255) // 256 > 1024
    kv, kt = mc.host('many_vertices')
    assert len(kv) == 8 and np.array_equal(kv, v[262_140 + 2 * np.arange(8)])


def test_pieces_case():
    v, t = mc.case('pieces')
    comps = mc.components(t)
    assert len(comps) >= 3 and sum(ok for ok, _ in comps.values()) >= 2
    wt = sorted(n for ok, n in comps.values() if ok)
    assert len(set(wt)) == len(wt)  # no tie: the largest sphere wins on vertices alone
    assert max(n for ok, n in comps.values() if not ok) > wt[-1]  # the open piece is the largest of all
    kv, kt = mc.host('pieces')
    assert len(kv) == wt[-1] and 5000 < len(t) < 40000


def test_host_pass_untouched_by_the_helper():
    v, t = mc.box(0.0)
    kv, kt = largest_component(v, t)
    assert np.array_equal(kv, v) and np.array_equal(kt, t)
