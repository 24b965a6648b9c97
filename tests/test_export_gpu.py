"""The indexed export on the device (csrc/sdf_normals.hip, k_ply_* of csrc/sdf_plain.hip, `Mesh.vertex_normals`, `Mesh.ply_records`,
`generate_mesh`, the native writers of `save`): the normals bit-identical to the definition (tests/normals_ref.py) run over the same
interpreter (`Engine.eval_points`) and, for the models without libm calls, over the CPU checker; every byte of the PLY records; the
files; the refusals.  Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
import ctypes
import sys

import numpy as np
import pytest

import fixtures
import normals_ref as ref
from sdf_amd import core, engine

pytestmark = pytest.mark.gpu

# plain family, trig family (twice), smooth unions, the largest register files
# (opcode coverage lives in the sweep, tests/test_probe_sweep_gpu.py: every tape of the suite goes through this kernel there; these few
# models walk the kernel's own states)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'slots_plain_8_8_p8d8')
LIBM_FREE = ('ex_example', 'ex_blobby', 'torus')
SAMPLES = 2 ** 13
_meshes = {}
BOX = ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def meshed(name, ns, eng):
    """(model, bounds, eps, welded points, cells) at 2^13 samples, the preview's eps: meshed and welded once per model"""
    if name not in _meshes:
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
        eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
        X, Y, Z, _ = core.grid_axes(bounds, samples=SAMPLES)
        m = eng.generate(f, X, Y, Z, 32, True)
        try:
            pts, cells = m.weld()
            pts, cells = pts.copy(), cells.copy()
        finally:
            m.close()
        pts.setflags(write=False); cells.setflags(write=False)
        _meshes[name] = (f, bounds, eps, pts, cells)
    return _meshes[name]


def device_mesh(name, ns, eng):
    f, bounds, eps, pts, cells = meshed(name, ns, eng)
    X, Y, Z, _ = core.grid_axes(bounds, samples=SAMPLES)
    return eng.generate(f, X, Y, Z, 32, True)


def same_normals(got, want):
    (gn, gf), (wn, wf) = got, want
    assert gn.dtype == np.float64 and gn.shape == wn.shape, (gn.dtype, gn.shape, wn.shape)
    bad = bits(gn) != bits(wn)
    assert not bad.any(), '%d of %d values differ, first at %s: %r != %r' % (bad.sum(), bad.size, np.argwhere(bad)[0], gn[bad][0], wn[bad][0])
    assert gf == wf, (gf, wf)


class Soup:
    """a float64 soup in device memory (torch owns it) and the Mesh that adopts it"""

    def __init__(self, eng, tris):
        import torch
        self.host = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 9)
        self.buf = torch.from_numpy(self.host.reshape(-1).copy()).to('cuda:0') if len(self.host) else None
        torch.cuda.synchronize()
        self.mesh = eng.adopt_soup(self.buf.data_ptr() if len(self.host) else 0, len(self.host))

    def welded(self):
        pts, inv = np.unique(self.host.reshape(-1, 3), axis=0, return_inverse=True)
        return pts, np.asarray(inv).reshape(-1, 3)

    def close(self):
        self.mesh.close()


def random_soup(n_tris, seed=7):
    rng = np.random.RandomState(seed + n_tris)
    return rng.uniform(-1.1, 1.1, size=(n_tris, 9))


@pytest.mark.parametrize('name', MODELS)
def test_normals_are_bit_identical_to_the_definition(name, ns, eng):
    f, bounds, eps, pts, cells = meshed(name, ns, eng)
    assert len(pts) > 256
    m = device_mesh(name, ns, eng)
    try:
        got = m.vertex_normals(f, eps)
        again = m.vertex_normals(f, eps)                       # served from the mesh's cache
    finally:
        m.close()
    want = ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, eps)
    same_normals(got, want)
    same_normals(again, want)
    ln = np.sqrt((got[0] ** 2).sum(axis=1))
    keep = ln != 0
    assert (np.abs(ln[keep] - 1) <= 4 * np.spacing(1.0)).all() and (~keep).sum() == got[1]


@pytest.mark.parametrize('name', LIBM_FREE)
def test_normals_are_bit_identical_to_the_definition_over_the_checker(name, ns, eng, oracle_lib):
    f, bounds, eps, pts, cells = meshed(name, ns, eng)
    m = device_mesh(name, ns, eng)
    try:
        got = m.vertex_normals(f, eps)
    finally:
        m.close()
    same_normals(got, ref.vertex_normals(lambda P: oracle_lib.evaluate(f, P), pts, eps))


def test_another_model_or_eps_is_not_served_from_the_cache(ns, eng):
    f, bounds, eps, pts, cells = meshed('ex_example', ns, eng)
    g = ns['sphere'](0.7)
    m = device_mesh('ex_example', ns, eng)
    try:
        a = m.vertex_normals(f, eps)
        b = m.vertex_normals(f, 3 * eps)
        c = m.vertex_normals(g, eps)
        d = m.vertex_normals(f, eps)
        d = (d[0].copy(), d[1])
        vb, fb = m.ply_records(normals=True)                  # ... and the records carry the last ones
    finally:
        m.close()
    same_normals(b, ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 3 * eps))
    same_normals(c, ref.vertex_normals(lambda P: eng.eval_points(g, P), pts, eps))
    same_normals(d, a)
    assert (bits(b[0]) != bits(a[0])).any() and (bits(c[0]) != bits(a[0])).any()
    wv, wf = ref.ply_records(pts, cells, d[0])
    assert np.array_equal(vb, wv) and np.array_equal(fb, wf)


@pytest.mark.parametrize('n_tris', (1, 64, 85, 86))
def test_ragged_vertex_counts_through_adopted_soups(n_tris, ns, eng):
    """U = 3, 192, 255, 258: one partial wave, whole waves, one below and two above a workgroup"""
    f = ns['sphere'](1)
    s = Soup(eng, random_soup(n_tris))
    try:
        pts, cells = s.welded()
        assert len(pts) == 3 * n_tris
        got = s.mesh.vertex_normals(f, 1e-3)
        same_normals(got, ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3))
        for with_normals in (False, True):
            vb, fb = s.mesh.ply_records(normals=with_normals)
            wv, wf = ref.ply_records(pts, cells, got[0] if with_normals else None)
            assert vb.dtype == np.uint8 and fb.dtype == np.uint8
            assert np.array_equal(vb, wv) and np.array_equal(fb, wf), (n_tris, with_normals)
    finally:
        s.close()


def test_empty_mesh(ns, eng):
    s = Soup(eng, np.zeros((0, 9)))
    try:
        n, n_flat = s.mesh.vertex_normals(ns['sphere'](1), 1e-3)
        assert n.shape == (0, 3) and n_flat == 0
        for with_normals in (False, True):
            vb, fb = s.mesh.ply_records(normals=with_normals)
            assert vb.shape == (0,) and fb.shape == (0,)
    finally:
        s.close()


def test_a_vertex_at_the_centre_of_a_sphere_is_flat(ns, eng):
    f = ns['sphere'](1)
    tris = random_soup(5)
    tris[2, 3:6] = 0.0                                          # one vertex at the centre
    s = Soup(eng, tris)
    try:
        pts, cells = s.welded()
        n, n_flat = s.mesh.vertex_normals(f, 1e-3)
        same_normals((n, n_flat), ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3))
        at = np.flatnonzero(~pts.any(axis=1))
        assert n_flat == 1 and len(at) == 1 and not n[at[0]].any()
        others = np.delete(np.arange(len(pts)), at[0])
        r = np.sqrt((pts[others] ** 2).sum(axis=1))
        # the neighbours are unaffected: radial, to the central difference's truncation -- the third derivatives of |p| are of
        # order 1 / r^2, so the term is of order (eps / r)^2 (random vertices come close to the centre) -- plus rounding
        err = np.abs(n[others] - pts[others] / r[:, None]).max(axis=1)
        assert (err <= (1e-3 / r) ** 2 + 1e-9).all(), (err / ((1e-3 / r) ** 2 + 1e-9)).max()
    finally:
        s.close()


@pytest.mark.parametrize('name', ('ex_example', 'twist'))
def test_ply_records_of_a_generated_mesh(name, ns, eng):
    f, bounds, eps, pts, cells = meshed(name, ns, eng)
    m = device_mesh(name, ns, eng)
    try:
        plain = m.ply_records()
        n, _ = m.vertex_normals(f, eps)
        n = n.copy()
        full = m.ply_records(normals=True)
    finally:
        m.close()
    wv, wf = ref.ply_records(pts, cells)
    assert len(cells) > 256 and np.array_equal(plain[0], wv) and np.array_equal(plain[1], wf)
    wv, wf = ref.ply_records(pts, cells, n)
    assert np.array_equal(full[0], wv) and np.array_equal(full[1], wf)


def test_save_and_generate_mesh_end_to_end(tmp_path, ns, eng):
    f = fixtures.build('ex_example', ns)
    pts, cells, n = f.generate_mesh(normals=True, samples=SAMPLES, verbose=False)
    assert n.shape == pts.shape and cells.shape[1] == 3 and cells.dtype == np.int64 and core.generate_mesh.last_flat == 0
    p0, c0, n0 = core.generate_mesh(f, samples=SAMPLES, verbose=False)
    f_, bounds, eps, wp, wc = meshed('ex_example', ns, eng)      # (Engine.generate(...).weld() on the grid of the same bounds and samples)
    assert n0 is None and np.array_equal(p0, wp) and np.array_equal(c0, wc) and np.array_equal(pts, wp) and np.array_equal(cells, wc)
    # the default eps is the preview's: 1e-4 x the half-diagonal of the bounds
    same_normals((n, 0), ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, eps))
    f.save(tmp_path / 'a.ply', normals=True, samples=SAMPLES, writer='native', verbose=False)
    p, nn, c, head = ref.parse_ply(str(tmp_path / 'a.ply'))
    assert head == ref.ply_header(len(pts), len(cells), True)
    assert np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    assert np.array_equal(nn.view(np.int32), n.astype(np.float32).view(np.int32))
    f.save(str(tmp_path / 'a.obj'), normals=True, samples=SAMPLES, writer='native', verbose=False)
    p, nn, c = ref.parse_obj(str(tmp_path / 'a.obj'))
    assert np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    assert np.array_equal(nn.view(np.int32), n.astype(np.float32).view(np.int32))
    f.save(str(tmp_path / 'e.ply'), normals=True, normal_eps=3 * eps, samples=SAMPLES, verbose=False)
    same = ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 3 * eps)[0]
    assert np.array_equal(ref.parse_ply(str(tmp_path / 'e.ply'))[1].view(np.int32), same.astype(np.float32).view(np.int32))


def test_save_without_meshio_writes_the_native_file(tmp_path, monkeypatch, ns, eng):
    monkeypatch.setitem(sys.modules, 'meshio', None)
    f, bounds, eps, pts, cells = meshed('ex_example', ns, eng)
    core.save(str(tmp_path / 'b.ply'), f, samples=SAMPLES, verbose=False)
    p, nn, c, head = ref.parse_ply(str(tmp_path / 'b.ply'))
    assert nn is None and head == ref.ply_header(len(pts), len(cells), False)
    assert np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    core.save(str(tmp_path / 'b.obj'), f, samples=SAMPLES, verbose=False)
    p, nn, c = ref.parse_obj(str(tmp_path / 'b.obj'))
    assert nn is None and np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    with pytest.raises(ImportError):
        core.save(str(tmp_path / 'b.off'), f, samples=SAMPLES, verbose=False)
    with pytest.raises(ValueError, match='STL has no vertex normals'):
        core.save(str(tmp_path / 'b.stl'), f, samples=SAMPLES, verbose=False, normals=True)


def test_a_model_with_closures_takes_the_definition_on_the_host(tmp_path, ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    lib = eng.lib
    X, Y, Z, _ = core.grid_axes(BOX, samples=SAMPLES)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        pts, cells = m.weld()
        dt = eng.tape_for(f)
        flat = ctypes.c_int64(0)
        assert lib.sdf_mesh_vertex_normals(m.handle, dt.handle, 1e-3, None, ctypes.byref(flat)) == 2      # the C entry refuses
        assert b'closures' in lib.sdf_last_error()
        got = m.vertex_normals(f, 1e-3)
        same_normals(got, ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3))
        with pytest.raises(ValueError, match='sdf_mesh_vertex_normals first'):
            m.ply_records(normals=True)                         # nothing was kept on the device
    finally:
        m.close()
    f.save(str(tmp_path / 'c.ply'), normals=True, normal_eps=1e-3, bounds=BOX, samples=SAMPLES, verbose=False)
    p, nn, c, head = ref.parse_ply(str(tmp_path / 'c.ply'))
    assert np.array_equal(c, cells) and np.array_equal(nn.view(np.int32), got[0].astype(np.float32).view(np.int32))


def test_refusals(ns, eng):
    f = ns['sphere'](1)
    lib = eng.lib
    s = Soup(eng, random_soup(4))
    try:
        dt = eng.tape_for(f)
        flat = ctypes.c_int64(0)
        out = np.zeros((12, 3))
        p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        # normals before the weld; PLY records before the weld
        assert lib.sdf_mesh_vertex_normals(s.mesh.handle, dt.handle, 1e-3, p, ctypes.byref(flat)) == 2
        assert b'sdf_mesh_weld first' in lib.sdf_last_error()
        assert lib.sdf_mesh_emit_ply_host(s.mesh.handle, 0, p, p) == 2 and b'sdf_mesh_weld first' in lib.sdf_last_error()
        assert s.mesh._welded() == 12
        for bad in (0.0, -1e-3, float('nan'), float('inf'), -float('inf')):
            assert lib.sdf_mesh_vertex_normals(s.mesh.handle, dt.handle, bad, p, ctypes.byref(flat)) == 2, bad
            assert b'eps' in lib.sdf_last_error()
            with pytest.raises(ValueError, match='eps'):
                s.mesh.vertex_normals(f, bad)
        assert lib.sdf_mesh_vertex_normals(s.mesh.handle, None, 1e-3, p, ctypes.byref(flat)) == 2
        assert lib.sdf_mesh_vertex_normals(s.mesh.handle, dt.handle, 1e-3, p, None) == 2
        assert not out.any()
        with pytest.raises(ValueError, match='sdf_mesh_vertex_normals first'):
            s.mesh.ply_records(normals=True)                    # with_normals before the normals
        eng.precision = engine.PRECISION_F32
        try:
            with pytest.raises(ValueError, match='float32'):
                s.mesh.vertex_normals(f, 1e-3)
        finally:
            eng.precision = engine.PRECISION_F64
        # ... and the mesh serves the calls that are in order
        pts, cells = s.welded()
        same_normals(s.mesh.vertex_normals(f, 1e-3), ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3))
    finally:
        s.close()


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing_and_close_frees_the_normals(ns, eng):
    """sdf_test_fail_alloc walked through sdf_mesh_vertex_normals and sdf_mesh_emit_ply_host: each fails with the allocator's
    message, the free device memory is what it was, and the next call succeeds; the mesh's destructor gives the cached normals
    back.  400,000 random triangles: 1.2 M vertices, 28.8 MB of normals -- large enough to show in hipMemGetInfo."""
    f = ns['sphere'](1)
    lib = eng.lib
    warm = Soup(eng, random_soup(3))                            # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.vertex_normals(f, 1e-3)
        warm.mesh.ply_records(normals=True)
    finally:
        warm.close()
    n_tris = 400000
    s = Soup(eng, random_soup(n_tris))
    closed = False
    try:
        pts, cells = s.welded()
        want = ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3)       # (sizes the context's scratch: before f0)
        eng.synchronize()
        f0 = _free(lib)
        nu = s.mesh._welded()
        assert nu == 3 * n_tris
        dt = eng.tape_for(f)
        flat = ctypes.c_int64(0)
        f1 = _free(lib)
        failures = 0
        for n in range(1, 6):                                   # ---- sdf_mesh_vertex_normals ----
            lib.sdf_test_fail_alloc(n)
            rc = lib.sdf_mesh_vertex_normals(s.mesh.handle, dt.handle, 1e-3, None, ctypes.byref(flat))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error(), lib.sdf_last_error()
            assert _free(lib) == f1
            with pytest.raises(ValueError):
                s.mesh.ply_records(normals=True)                # a failed call leaves no normals behind
        assert failures >= 1 and rc == 0 and flat.value == 0
        f2 = _free(lib)
        assert f1 - f2 >= 24 * nu, (f1, f2)
        failures = 0
        for n in range(1, 6):                                   # ---- sdf_mesh_emit_ply_host ----
            lib.sdf_test_fail_alloc(n)
            try:
                vb, fb = s.mesh.ply_records(normals=True)
                lib.sdf_test_fail_alloc(0)
                break
            except engine.SdfHipError as e:
                lib.sdf_test_fail_alloc(0)
                failures += 1
                assert 'emory' in str(e), e
                assert _free(lib) == f2
        assert failures >= 1
        assert _free(lib) == f2                                 # the records' device block is freed before the call returns
        wv, wf = ref.ply_records(pts[:1000], cells[:0], want[0][:1000])
        assert np.array_equal(vb[:24000], wv)
        assert np.array_equal(fb.reshape(-1, 13)[:, 0], np.full(n_tris, 3, np.uint8))
        assert np.array_equal(np.ascontiguousarray(fb.reshape(-1, 13)[:, 1:]).view('<i4'), cells)
        s.close()
        closed = True
        f3 = _free(lib)
        assert f3 >= f0 and f3 - f2 >= 24 * nu, (f0, f2, f3)
    finally:
        lib.sdf_test_fail_alloc(0)
        if not closed:
            s.close()
