"""The curvature probe on the device (csrc/sdf_curvature.hip, `engine.Mesh.vertex_curvature`, sdf_amd/curvature.py, `save(...,
curvature=...)`): the four curvatures' bits and the status identical to the definition (tests/curvature_ref.py) run over the same
interpreter (`Engine.eval_points`); ragged vertex counts through adopted soups; every status in one launch and the device's counts;
the refusals; the feature end to end.  Every comparison with the definition is bitwise.  Every refusal is decided on the host before a
launch; no test repeats a device call that failed."""
import ctypes

import numpy as np
import pytest

import curvature_ref as ref
import fixtures
import thickness_ref
from sdf_amd import core, engine, tape
from test_register_slots import is_trig
from test_thickness_gpu import Soup

pytestmark = pytest.mark.gpu

EPS = 1e-3


def same(got, want, what=''):
    """(curv, status, counts) of the device against (curv, status) of the definition: types, shapes, bits, and the histogram"""
    assert got[0].dtype == np.float64 and got[0].shape == want[0].shape and got[1].dtype == np.uint8 and got[1].shape == want[1].shape, what
    bad = (ref.bits(got[0]) != ref.bits(want[0])).any(axis=1) | (got[1] != want[1])
    assert not bad.any(), '%s: %d of %d vertices differ, first at %d: %r %r / %r %r' % (
        what, bad.sum(), bad.size, np.flatnonzero(bad)[0], got[0][np.flatnonzero(bad)[0]], got[1][np.flatnonzero(bad)[0]],
        want[0][np.flatnonzero(bad)[0]], want[1][np.flatnonzero(bad)[0]])
    assert got[2].dtype == np.int64 and got[2].tolist() == ref.counts(want[1]).tolist(), what


def soup_of(n_vertices, seed=17):
    """a soup whose weld has exactly n_vertices: ceil(n / 3) random triangles, the last one repeating its first corner"""
    n_tris = (n_vertices + 2) // 3
    tris = np.random.RandomState(seed + n_vertices).uniform(-1.1, 1.1, size=(n_tris, 3, 3))
    for k in range(3 * n_tris - n_vertices):
        tris[-1, 2 - k] = tris[-1, 0]
    return tris.reshape(n_tris, 9)


@pytest.mark.parametrize('name', ('ex_example', 'twist'))
@pytest.mark.parametrize('n', (1, 63, 64, 65, 255, 256, 257, 999))
def test_ragged_vertex_counts_through_adopted_soups(n, name, ns, eng):
    """a lone lane, partial waves, waves wholly beyond n inside a launched workgroup, several workgroups; the plain and the
    trigonometric instantiation"""
    f = fixtures.build(name, ns)
    assert is_trig(tape.lower(f)) == (name == 'twist')
    s = Soup(eng, soup_of(n))
    try:
        pts = s.welded()
        assert len(pts) == n
        for eps in (EPS, 0.03):
            with np.errstate(all='ignore'):
                want = ref.curvature(lambda P: eng.eval_points(f, P), pts, eps)
            same(s.mesh.vertex_curvature(f, eps), want, '%s %d %g' % (name, n, eps))
        assert (want[1] == ref.CURVED).any()
    finally:
        s.close()


def test_every_status_in_one_launch(ns, eng):
    """sphere(1): its centre is FLAT, a point at 1e200 is NAN through infinite values, everything else is CURVED"""
    f = ns['sphere'](1)
    tris = soup_of(300).reshape(-1, 3, 3)
    tris[5, 0] = 0.0
    tris[40, 1] = (1e200, 0.0, 0.0)
    tris[77, 2] = (0.0, -1e200, 1e200)
    s = Soup(eng, tris)
    try:
        pts = s.welded()
        with np.errstate(all='ignore'):
            want = ref.curvature(lambda P: eng.eval_points(f, P), pts, EPS)
        assert len(pts) == 300 and ref.counts(want[1]).tolist() == [297, 1, 2]
        got = s.mesh.vertex_curvature(f, EPS)
        same(got, want)
        assert got[2].tolist() == [297, 1, 2] and (got[0].view(np.uint64)[got[1] != ref.CURVED] == ref.NAN_BITS).all()
        assert eng.lib.sdf_mesh_curvature_last_kernel_ms() > 0
    finally:
        s.close()


def test_empty_mesh(ns, eng):
    s = Soup(eng, np.zeros((0, 9)))
    try:
        curv, status, counts = s.mesh.vertex_curvature(ns['sphere'](1), EPS)
        assert curv.shape == (0, 4) and status.shape == (0,) and counts.tolist() == [0, 0, 0]
    finally:
        s.close()


def test_refusals(ns, eng):
    f = ns['sphere'](1)
    lib = eng.lib
    s = Soup(eng, soup_of(12))
    other = engine.Engine(0)                                    # a second context on the same device
    odt = other.tape_for(f)
    try:
        dt = eng.tape_for(f)
        curv, status, counts = np.zeros((12, 4)), np.zeros(12, np.uint8), np.zeros(3, np.int64)
        f64p, u8p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)

        def call(mesh, tp, eps):
            return lib.sdf_mesh_vertex_curvature(mesh, tp, eps, curv.ctypes.data_as(f64p), status.ctypes.data_as(u8p), counts.ctypes.data_as(i64p))
        assert call(s.mesh.handle, dt.handle, EPS) == 2 and b'sdf_mesh_weld first' in lib.sdf_last_error()      # before the weld
        assert s.mesh._welded() == 12
        lib.sdf_test_fail_alloc(1)                              # the library's test hook: its next allocation fails
        try:
            for bad in (0.0, -1.0, float('nan'), float('inf')):
                assert call(s.mesh.handle, dt.handle, bad) == 2 and b'eps' in lib.sdf_last_error(), (bad, lib.sdf_last_error())
                assert b'sdf_mesh_vertex_curvature' in lib.sdf_last_error()
            # the hook is still armed, so the refusals allocated nothing: the call that is in order is the one that meets it
            assert call(s.mesh.handle, dt.handle, EPS) == 1 and b'emory' in lib.sdf_last_error(), lib.sdf_last_error()
        finally:
            lib.sdf_test_fail_alloc(0)
        assert call(s.mesh.handle, None, EPS) == 2 and call(None, dt.handle, EPS) == 2
        assert lib.sdf_mesh_vertex_curvature(s.mesh.handle, dt.handle, EPS, None, status.ctypes.data_as(u8p), counts.ctypes.data_as(i64p)) == 2
        assert call(s.mesh.handle, odt.handle, EPS) == 2 and b'different contexts' in lib.sdf_last_error()
        assert not curv.any() and not status.any() and not counts.any()
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError):
                s.mesh.vertex_curvature(f, bad)
        eng.precision = engine.PRECISION_F32
        try:
            with pytest.raises(ValueError, match='float32'):
                s.mesh.vertex_curvature(f, EPS)
        finally:
            eng.precision = engine.PRECISION_F64
        with pytest.raises(ValueError):
            f.curvature(eps=0.0, samples=2 ** 13, verbose=False)
        # ... and the mesh serves the call that is in order
        same(s.mesh.vertex_curvature(f, EPS), ref.curvature(lambda P: eng.eval_points(f, P), s.welded(), EPS))
    finally:
        s.close()
        odt._fin()
        other._fin()


def test_sphere_end_to_end(ns, eng):
    """marching-cubes vertices lie at most about step^2 / 8R = 1.25e-3 inside the sphere, and the level set through such a point p
    has curvature 1 / |p|: within 1 % of 1"""
    f = ns['sphere'](1)
    c = f.curvature(step=0.1, eps=EPS, verbose=False)
    assert c.params == {'eps': EPS} and c.k1.shape == (len(c.points),) and c.cells.shape[1] == 3 and len(c.points) > 256
    assert c.measured.all() and c.counts == {'CURVED': len(c.points), 'FLAT': 0, 'NAN': 0}
    print('sphere: %d vertices, k1 %.6f .. %.6f, k2 %.6f .. %.6f; %r' % (len(c.points), c.k1.min(), c.k1.max(), c.k2.min(), c.k2.max(), c))
    assert np.abs(c.k1 - 1).max() <= 0.01 and np.abs(c.k2 - 1).max() <= 0.01
    assert abs(c.min_convex_radius - 1) <= 0.01 and c.min_concave_radius == np.inf
    want = ref.curvature(lambda P: eng.eval_points(f, P), c.points, EPS)
    assert np.array_equal(ref.bits(np.stack([c.mean, c.gauss, c.k1, c.k2], axis=1)), ref.bits(want[0])) and np.array_equal(c.status, want[1])
    d = f.curvature(step=0.1, verbose=False)                    # the default: the smallest grid step
    assert d.params == {'eps': 0.1} and np.array_equal(d.points, c.points)


def test_box_creases(ns, eng):
    """at the default eps = step a vertex bends tighter than r = 0.2 = 4 steps only where the stencil reaches over an edge: within
    2 steps of it (the stencil's corners lie eps = 1 step away along two axes)"""
    f = ns['box'](1)
    step = 0.05
    c = f.curvature(step=step, verbose=False)
    assert c.params == {'eps': step} and c.measured.all()
    tight = c.tighter_than(0.2)
    # the distance of a surface point to the nearest edge: the second smallest of 0.5 - |coordinate|
    to_edge = np.sort(0.5 - np.abs(c.points), axis=1)[:, 1]
    print('box: %d vertices, %d tighter than 0.2, the farthest of them %.4f from an edge; sharpest %r' % (
        len(c.points), tight.sum(), to_edge[tight].max(), c.sharpest_point))
    assert tight.any() and (to_edge[tight] <= 2 * step).all()
    assert (np.abs(c.k1[to_edge > 2 * step]) <= 1e-9).all() and (np.abs(c.k2[to_edge > 2 * step]) <= 1e-9).all()     # the faces are flat


def test_save_writes_the_quality_column(tmp_path, ns, eng):
    f = ns['sphere'](1) - ns['sphere'](0.5).translate((0.0, 0.0, 0.9))
    c = f.curvature(step=0.1, verbose=False)
    f.save(str(tmp_path / 'm.ply'), curvature='mean', step=0.1, verbose=False)
    p, n, q, cells, head = thickness_ref.parse_ply(str(tmp_path / 'm.ply'))
    assert n is None and head == thickness_ref.ply_header(len(c.points), len(c.cells), False, True) and np.array_equal(cells, c.cells)
    assert np.array_equal(p.view(np.int32), c.points.astype(np.float32).view(np.int32))
    assert np.array_equal(q.view(np.int32), c.mean.astype(np.float32).view(np.int32))
    c.save(str(tmp_path / 'c.ply'))
    assert (tmp_path / 'c.ply').read_bytes() == (tmp_path / 'm.ply').read_bytes()
    f.save(str(tmp_path / 'x.ply'), curvature={'quality': 'max', 'eps': 0.01}, normals=True, step=0.1, verbose=False)
    p, n, q, cells, head = thickness_ref.parse_ply(str(tmp_path / 'x.ply'))
    fine = f.curvature(step=0.1, eps=0.01, verbose=False)
    assert n is not None and np.array_equal(q.view(np.int32), fine.quality('max').astype(np.float32).view(np.int32))
    assert (fine.k2 < 0).any() and fine.min_concave_radius < 1.0                  # the dimple is concave
    with pytest.raises(ValueError):
        f.save(str(tmp_path / 'b.ply'), curvature='mean', thickness=True, step=0.1, verbose=False)


def test_a_file_is_measured_in_the_field(tmp_path, ns, eng):
    from sdf_amd.mesh import Mesh
    f = ns['sphere'](1)
    f.save(str(tmp_path / 's.stl'), step=0.1, verbose=False)
    file_mesh = Mesh.from_stl(str(tmp_path / 's.stl'))
    c = file_mesh.curvature(f, eps=EPS)
    assert np.array_equal(c.points, file_mesh.points) and c.params == {'eps': EPS}
    want = ref.curvature(lambda P: eng.eval_points(f, P), file_mesh.points, EPS)
    assert np.array_equal(ref.bits(np.stack([c.mean, c.gauss, c.k1, c.k2], axis=1)), ref.bits(want[0])) and np.array_equal(c.status, want[1])
    assert file_mesh.curvature(f, step=(0.1, 0.2, 0.3)).params == {'eps': 0.1}
    with pytest.raises(ValueError, match='step'):
        file_mesh.curvature(f)


def test_a_model_with_closures_takes_the_definition_on_the_host(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    X, Y, Z, step = core.grid_axes(((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), samples=2 ** 13)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        pts = m.weld()[0]
        dt = eng.tape_for(f)
        curv, status, counts = np.zeros((len(pts), 4)), np.zeros(len(pts), np.uint8), np.zeros(3, np.int64)
        rc = eng.lib.sdf_mesh_vertex_curvature(m.handle, dt.handle, EPS, curv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        assert rc == 2 and b'closures' in eng.lib.sdf_last_error() and b'sdf_mesh_vertex_curvature' in eng.lib.sdf_last_error()
        got = m.vertex_curvature(f, EPS)
        same(got, ref.curvature(lambda P: eng.eval_points(f, P), pts, EPS))
        assert (got[1] == ref.CURVED).any() and got[2].sum() == len(pts)
    finally:
        m.close()
