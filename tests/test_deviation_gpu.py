"""A mesh held to the field on the device (csrc/sdf_deviation.hip, `engine.Mesh.triangle_deviation`, `engine.Mesh.snap`,
sdf_amd/deviation.py, `snap=` of the mesh pipeline): bits identical to the definition (tests/deviation_ref.py) run over the same
interpreter (`Engine.eval_points`) and, for the models without libm calls, over the CPU checker; ragged counts through adopted soups;
every status; NaN; the files; closures; the refusals.  "Identical" is bit for bit, except that a NaN equals a NaN (`ref.same_bits`:
IEEE 754 does not fix a NaN's sign and payload).  Every refusal is decided on the host before a launch; no test repeats a device call
that failed."""
import ctypes

import numpy as np
import pytest

import fixtures
import normals_ref
import deviation_ref as ref
from sdf_amd import core, engine
from sdf_amd.deviation import snap_params
from sdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu

# plain family, trig family (twice), smooth unions, the largest register files
# (opcode coverage lives in the sweep, tests/test_probe_sweep_gpu.py: every tape of the suite goes through this kernel there; these few
# models walk the kernel's own states)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'slots_plain_8_8_p8d8')
LIBM_FREE = ('ex_example', 'ex_blobby', 'torus')
SAMPLES = 2 ** 13
ORDERS = (1, 2, 4, 8)
_meshes = {}
F64P, U8P, I32P = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)


def meshed(name, ns, eng):
    """(model, soup (T, 3, 3), grid axes, grid steps, bounds) at 2^13 samples: meshed once per model"""
    if name not in _meshes:
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=SAMPLES)
        m = eng.generate(f, X, Y, Z, 32, True)
        try:
            soup = np.array(m.points()).reshape(-1, 3, 3)
        finally:
            m.close()
        soup.setflags(write=False)
        _meshes[name] = (f, soup, (X, Y, Z), step, bounds)
    return _meshes[name]


def default_snap(bounds, step, cluster=None, **over):
    return snap_params(over, bounds, step, cluster)


def same(got, want, what=''):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        ok = ref.same_bits(g, w)
        ok = ok.all(axis=1) if ok.ndim == 2 else ok
        assert ok.all(), '%s: %d of %d differ, first at %d: %r / %r' % (what, (~ok).sum(), ok.size, np.flatnonzero(~ok)[0], g[np.flatnonzero(~ok)[0]],
                                                                          w[np.flatnonzero(~ok)[0]])


def counts(status):
    return dict(zip(ref.NAMES, np.bincount(status, minlength=5).tolist()))


def snapped(mesh, f, par):
    """(the moved Mesh, (points, status, residual, evals))"""
    moved = mesh.snap(f, **par)
    return moved, moved.snap_result + (moved.snap_evals,)


class Soup:
    """a float64 soup in device memory (torch owns it) and the Mesh that adopts it"""

    def __init__(self, eng, tris):
        import torch
        self.host = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 9)
        self.buf = torch.from_numpy(self.host.reshape(-1).copy()).to('cuda:0') if len(self.host) else None
        torch.cuda.synchronize()
        self.mesh = eng.adopt_soup(self.buf.data_ptr() if len(self.host) else 0, len(self.host))

    def welded(self):
        return np.unique(self.host.reshape(-1, 3), axis=0, return_inverse=True)

    def close(self):
        self.mesh.close()


def random_soup(n_tris, seed=7):
    return np.random.RandomState(seed + n_tris).uniform(-1.1, 1.1, size=(n_tris, 9))


@pytest.mark.parametrize('name', MODELS)
def test_deviation_is_bit_identical_to_the_definition(name, ns, eng):
    f, soup, (X, Y, Z), step, bounds = meshed(name, ns, eng)
    T = len(soup)
    assert T > 256 and T % 64 != 0
    ev = lambda P: eng.eval_points(f, P)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        for order in ORDERS:
            got = m.triangle_deviation(f, order)
            want = ref.deviation(ev, soup, order)
            print(name, T, 'order', order, 'max |dev| %.4g' % np.abs(want[0]).max(), 'at', np.bincount(want[1], minlength=ref.n_samples(order)).tolist())
            same(got, want, '%s order %d' % (name, order))
    finally:
        m.close()


@pytest.mark.parametrize('name', LIBM_FREE)
def test_deviation_is_bit_identical_to_the_definition_over_the_checker(name, ns, eng, oracle_lib):
    f, soup, (X, Y, Z), step, bounds = meshed(name, ns, eng)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        for order in (1, 4):
            same(m.triangle_deviation(f, order), ref.deviation(lambda P: oracle_lib.evaluate(f, P), soup, order), '%s order %d' % (name, order))
    finally:
        m.close()


_seen = set()
RUNS = ({}, {'iters': 1}, {'max_move': None}, {'tol': 0.0})      # (max_move None: a hundredth of the grid step)


@pytest.mark.parametrize('n_tris', (1, 21, 22, 86, 333))
def test_ragged_counts_through_adopted_soups(n_tris, ns, eng):
    """T = 1, 21, 22, 86, 333 and U = 3, 63, 66, 258, 999: a partial wave, a wave less one lane, a wave plus two lanes, a workgroup plus
    two lanes, many workgroups -- for both kernels.  Snap with the defaults, one pass, a max_move of a hundredth of the step, tol = 0.
    One vertex of the largest soup is the model's centre (FLAT)."""
    f, _, _, step, bounds = meshed('ex_example', ns, eng)
    tris = random_soup(n_tris)
    if n_tris == 333:
        tris[100, 3:6] = 0.0
    s = Soup(eng, tris)
    try:
        pts, inv = s.welded()
        assert len(pts) == 3 * n_tris
        ev = lambda P: eng.eval_points(f, P)
        for order in ORDERS:
            same(s.mesh.triangle_deviation(f, order), ref.deviation(ev, tris.reshape(-1, 3, 3), order), '%d order %d' % (n_tris, order))
        assert s.mesh._welded() == len(pts)
        for over in RUNS:
            over = {'max_move': min(step) / 100} if 'max_move' in over else over
            par = default_snap(bounds, step, **over)
            want = ref.snap(ev, pts, **par)
            moved, got = snapped(s.mesh, f, par)
            try:
                same(got, want, '%d %r' % (n_tris, over))
                assert moved.n_triangles == n_tris
                same([np.array(moved.points()).reshape(-1, 3, 3)], [want[0][np.asarray(inv).reshape(-1, 3)]], 'soup %d %r' % (n_tris, over))
                assert {k: moved.snap_stats[k] for k in ('left', 'snapped', 'held', 'flat', 'nan')} == \
                    {k.lower(): v for k, v in counts(want[1]).items()} and moved.snap_stats['vertices'] == len(pts)
            finally:
                moved.close()
            _seen.update(want[1].tolist())
            if n_tris == 333:
                print(over, counts(want[1]), 'lockstep share %.2f' % ref.lockstep_share(want[3], par['iters']))
    finally:
        s.close()
    if n_tris == 333:
        assert {ref.SNAPPED, ref.LEFT, ref.HELD, ref.FLAT} <= _seen, _seen


def test_nan(ns, eng, oracle_lib):
    """`ellipsoid` divides 0 by 0 at its centre and nowhere else: a triangle with a corner there has dev NaN with `at` that corner's
    sample index, a vertex there is NAN and stays; the same over the checker"""
    f = ns['ellipsoid']((1, 1, 1))
    assert np.isnan(oracle_lib.evaluate(f, np.zeros((1, 3)))[0]) and np.isnan(eng.eval_points(f, np.zeros((1, 3)))[0])
    tris = random_soup(30)
    tris[:, :] = np.where(np.abs(tris) < 0.05, 0.05, tris)
    tris[7, 0:3] = 0.0           # corner A: sample 0
    tris[8, 6:9] = 0.0           # corner C: sample n
    tris[9, 3:6] = 0.0           # corner B: the last sample
    s = Soup(eng, tris)
    try:
        pts, inv = s.welded()
        for order in (1, 3):
            want = ref.deviation(lambda P: eng.eval_points(f, P), tris.reshape(-1, 3, 3), order)
            assert np.isnan(want[0][[7, 8, 9]]).all() and np.isnan(want[0]).sum() == 3
            assert want[1][[7, 8, 9]].tolist() == [0, order, ref.n_samples(order) - 1]
            same(s.mesh.triangle_deviation(f, order), want, 'order %d' % order)
            same(want, ref.deviation(lambda P: oracle_lib.evaluate(f, P), tris.reshape(-1, 3, 3), order), 'checker order %d' % order)
        par = dict(eps=1e-4, tol=1e-5, max_move=0.5, iters=4)
        want = ref.snap(lambda P: eng.eval_points(f, P), pts, **par)
        origin = np.flatnonzero((pts == 0).all(axis=1))
        assert len(origin) == 1 and want[1][origin[0]] == ref.NAN and (want[1] == ref.NAN).sum() == 1 and np.isnan(want[2][origin[0]])
        assert np.array_equal(want[0][origin[0]], [0.0, 0.0, 0.0])
        s.mesh._welded()
        moved, got = snapped(s.mesh, f, par)
        moved.close()
        same(got, want, 'snap')
        same(want, ref.snap(lambda P: oracle_lib.evaluate(f, P), pts, **par), 'snap over the checker')
    finally:
        s.close()


@pytest.mark.parametrize('name', MODELS)
def test_snap_of_simplified_meshes(name, ns, eng):
    f, soup, (X, Y, Z), step, bounds = meshed(name, ns, eng)
    ev = lambda P: eng.eval_points(f, P)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        small = m.simplify(np.array([X[0], Y[0], Z[0]]), 2 * np.asarray(step, dtype=np.float64))
        try:
            pts, cells = small.weld()
            pts, cells = pts.copy(), cells.copy()
            before = (small.moments()['sums'], small.vertex_normals(f, 1e-4)[0].copy(), small.triangle_deviation(f, 2))
            par = default_snap(bounds, step, 2)
            want = ref.snap(ev, pts, **par)
            moved, got = snapped(small, f, par)
            try:
                print(name, len(pts), counts(want[1]), 'evals <= %d' % want[3].max(), 'lockstep share %.2f' % ref.lockstep_share(want[3], par['iters']),
                      'max |dev| %.4g -> %.4g' % (np.abs(before[2][0]).max(), np.abs(moved.triangle_deviation(f, 2)[0]).max()))
                same(got, want, name)
                new_soup = want[0][cells]
                same([np.array(moved.points()).reshape(-1, 3, 3)], [new_soup], name + ' soup')
                # the new mesh serves the readers
                wp, wc = np.unique(new_soup.reshape(-1, 3), axis=0, return_inverse=True)
                mp, mc = moved.weld()
                assert np.array_equal(mp, wp) and np.array_equal(mc, np.asarray(wc).reshape(-1, 3))
                assert moved.moments()['triangles'] == len(cells)
                same([moved.vertex_normals(f, 1e-4)[0]], [normals_ref.vertex_normals(ev, wp, 1e-4)[0]], name + ' normals')
                same(moved.triangle_deviation(f, 2), ref.deviation(ev, new_soup, 2), name + ' deviation')
                mended = moved.mend()
                assert mended.n_triangles <= moved.n_triangles and mended.mend_stats['triangles_in'] == len(cells)
                mended.close()
            finally:
                moved.close()
            # the source still serves its readers, unchanged
            assert np.array_equal(small.moments()['sums'], before[0])
            same([small.vertex_normals(f, 1e-4)[0]], [before[1]])
            same(small.triangle_deviation(f, 2), before[2])
            sp, sc = small.weld()
            assert np.array_equal(sp, pts) and np.array_equal(sc, cells)
        finally:
            small.close()
    finally:
        m.close()


def test_sphere_end_to_end(ns, eng):
    f = ns['sphere'](1)
    plain = f.deviation(simplify=4, step=0.1, verbose=False)
    snap = f.deviation(simplify=4, snap=True, order=1, step=0.1, verbose=False)
    tol = 1e-3 * 0.1
    print('sphere simplify=4: max |dev| %.4g (rms %.4g), snapped at the vertices %.4g (tol %.4g), %r' % (plain.max, plain.rms, snap.max, tol, snap.snap_stats))
    assert plain.snap_stats is None and snap.snap_stats['vertices'] == len(snap.points)
    assert plain.max > snap.max
    assert snap.snap_stats['snapped'] == snap.snap_stats['vertices'], snap.snap_stats        # (as the NumPy trial found for a sphere)
    assert snap.max <= tol
    assert plain.argmax is not None and plain.worst_point.shape == (3,) and plain.counts['nan'] == 0
    # order 1 samples the corners: the deviation there is the snap's residual
    assert abs(eng.eval_points(f, snap.worst_point[None])[0]) == snap.max
    pts, cells, nrm = core.generate_mesh(f, simplify=4, snap=True, normals=True, step=0.1, verbose=False)
    assert core.generate_mesh.last_snap['snapped'] == len(pts) and np.array_equal(pts, snap.points) and np.array_equal(cells, snap.cells)
    bounds = eng.estimate_bounds(f)
    eps = default_snap(bounds, (0.1, 0.1, 0.1))['eps']
    same([nrm], [normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, eps)[0]], 'normals at the snapped vertices')
    assert np.abs(eng.eval_points(f, pts)).max() <= tol
    # measure and thickness pass snap= through
    from sdf_amd.measure import measure
    a, b = measure(f, simplify=4, step=0.1, verbose=False), measure(f, simplify=4, snap=True, step=0.1, verbose=False)
    assert a.volume != b.volume and a.triangles == b.triangles
    t = f.thickness(simplify=4, snap=True, step=0.1, verbose=False)
    assert np.array_equal(t.points, pts)


def test_files_and_pipeline_are_unchanged_without_snap(tmp_path, ns, eng):
    f, soup, (X, Y, Z), step, bounds = meshed('ex_example', ns, eng)
    f.save(str(tmp_path / 'a.ply'), simplify=4, samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 's.ply'), simplify=4, snap=True, writer='native', samples=SAMPLES, verbose=False)
    f.deviation(simplify=4, snap={'iters': 2}, samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 'b.ply'), simplify=4, samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 'c.ply'), simplify=4, snap=False, samples=SAMPLES, verbose=False)
    a = (tmp_path / 'a.ply').read_bytes()
    assert a == (tmp_path / 'b.ply').read_bytes() == (tmp_path / 'c.ply').read_bytes()
    s = (tmp_path / 's.ply').read_bytes()
    assert s != a and len(s) > 200
    # the file holds the snapped mesh
    pts, cells, _ = core.generate_mesh(f, simplify=4, snap=True, samples=SAMPLES, verbose=False)
    p, n, c, head = normals_ref.parse_ply(str(tmp_path / 's.ply'))
    assert np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    # a file measured and snapped in the field
    f.save(str(tmp_path / 'a.stl'), simplify=4, samples=SAMPLES, verbose=False)
    file_mesh = Mesh.from_stl(str(tmp_path / 'a.stl'))
    d = file_mesh.deviation(f, order=2)
    tri = np.asarray(file_mesh.points)[np.asarray(file_mesh.triangles)]
    same((d.dev, d.at, d.sumsq), ref.deviation(lambda P: eng.eval_points(f, P), tri, 2), 'file')
    moved = file_mesh.snap(f, step=step)
    want = ref.snap(lambda P: eng.eval_points(f, P), file_mesh.points, **default_snap((file_mesh.points.min(axis=0), file_mesh.points.max(axis=0)), step))
    same((moved.points, moved.snap_status, moved.snap_residual), want[:3], 'file snap')
    assert np.array_equal(moved.triangles, file_mesh.triangles)
    with pytest.raises(ValueError, match='step'):
        file_mesh.snap(f)


def test_a_model_with_closures_takes_the_definition_on_the_host(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    bounds = ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))
    X, Y, Z, step = core.grid_axes(bounds, samples=SAMPLES)
    par = default_snap(bounds, step)
    ev = lambda P: eng.eval_points(f, P)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        pts, cells = m.weld()
        soup = np.array(m.points()).reshape(-1, 3, 3)
        dt = eng.tape_for(f)
        T, U = len(soup), len(pts)
        dev, at, sumsq = np.zeros(T), np.zeros(T, np.int32), np.zeros(T)
        rc = eng.lib.sdf_mesh_triangle_deviation(m.handle, dt.handle, 2, dev.ctypes.data_as(F64P), at.ctypes.data_as(I32P), sumsq.ctypes.data_as(F64P))
        assert rc == 2 and b'closures' in eng.lib.sdf_last_error() and b'sdf_mesh_triangle_deviation' in eng.lib.sdf_last_error()
        p4 = np.array([par['eps'], par['tol'], par['max_move'], 0.0])
        h, st = ctypes.c_void_p(), engine.SdfSnapStats()
        rc = eng.lib.sdf_mesh_snap(m.handle, dt.handle, p4.ctypes.data_as(F64P), 4, ctypes.byref(h), None, None, None, None, ctypes.byref(st))
        assert rc == 2 and b'closures' in eng.lib.sdf_last_error() and b'sdf_mesh_snap' in eng.lib.sdf_last_error() and not h.value
        assert not dev.any() and not at.any() and not sumsq.any()
        same(m.triangle_deviation(f, 2), ref.deviation(ev, soup, 2))
        want = ref.snap(ev, pts, **par)
        moved, got = snapped(m, f, par)
        try:
            same(got, want)
            same([np.array(moved.points()).reshape(-1, 3, 3)], [want[0][cells]])
            assert moved.snap_stats['snapped'] == (want[1] == ref.SNAPPED).sum() and moved.snap_stats['vertices'] == U
            assert len(moved.weld()[1]) == T
        finally:
            moved.close()
    finally:
        m.close()


def test_refusals(ns, eng):
    f = ns['sphere'](1)
    lib = eng.lib
    tris = random_soup(4)
    s = Soup(eng, tris)
    other = engine.Engine(0)                                    # a second context on the same device
    odt = other.tape_for(f)
    try:
        dt = eng.tape_for(f)
        dev, at, sumsq = np.zeros(4), np.zeros(4, np.int32), np.zeros(4)
        q, status, residual, evals = np.zeros((12, 3)), np.zeros(12, np.uint8), np.zeros(12), np.zeros(12, np.int32)
        h, st = ctypes.c_void_p(), engine.SdfSnapStats()

        def deviation(mesh, tape, order, a=dev, b=at, c=sumsq):
            return lib.sdf_mesh_triangle_deviation(mesh, tape, order, a.ctypes.data_as(F64P) if a is not None else None,
                                                   b.ctypes.data_as(I32P) if b is not None else None, c.ctypes.data_as(F64P) if c is not None else None)

        def snap(mesh, tape, p4, iters=4, out=ctypes.byref(h), stats=ctypes.byref(st)):
            p4 = np.array(p4, np.float64) if p4 is not None else None
            return lib.sdf_mesh_snap(mesh, tape, p4.ctypes.data_as(F64P) if p4 is not None else None, iters, out, q.ctypes.data_as(F64P),
                                     status.ctypes.data_as(U8P), residual.ctypes.data_as(F64P), evals.ctypes.data_as(I32P), stats)
        name = b'sdf_mesh_triangle_deviation'
        for order in (0, 9, -1):
            assert deviation(s.mesh.handle, dt.handle, order) == 2 and b'order' in lib.sdf_last_error() and name in lib.sdf_last_error()
        assert deviation(None, dt.handle, 2) == 2 and deviation(s.mesh.handle, None, 2) == 2 and name in lib.sdf_last_error()
        assert deviation(s.mesh.handle, dt.handle, 2, a=None) == 2 and deviation(s.mesh.handle, dt.handle, 2, b=None) == 2
        assert deviation(s.mesh.handle, dt.handle, 2, c=None) == 2 and b'NULL' in lib.sdf_last_error()
        assert deviation(s.mesh.handle, odt.handle, 2) == 2 and b'different contexts' in lib.sdf_last_error()
        name = b'sdf_mesh_snap'
        good = [1e-4, 1e-5, 0.1, 0.0]
        assert snap(s.mesh.handle, dt.handle, good) == 2 and b'sdf_mesh_weld first' in lib.sdf_last_error()      # before the weld
        assert s.mesh._welded() == 12
        for bad, word in (([0.0, 1e-5, 0.1, 0.0], b'eps'), ([-1e-4, 1e-5, 0.1, 0.0], b'eps'), ([1e-4, -1e-5, 0.1, 0.0], b'tol'),
                          ([1e-4, 1e-5, -0.1, 0.0], b'max_move'), ([float('nan'), 1e-5, 0.1, 0.0], b'finite'), ([1e-4, float('inf'), 0.1, 0.0], b'finite'),
                          ([1e-4, 1e-5, float('inf'), 0.0], b'finite'), ([1e-4, 1e-5, 0.1, float('nan')], b'finite')):
            assert snap(s.mesh.handle, dt.handle, bad) == 2 and word in lib.sdf_last_error() and name in lib.sdf_last_error(), (bad, lib.sdf_last_error())
        assert snap(s.mesh.handle, dt.handle, good, iters=0) == 2 and b'iters' in lib.sdf_last_error()
        assert snap(None, dt.handle, good) == 2 and snap(s.mesh.handle, None, good) == 2 and snap(s.mesh.handle, dt.handle, None) == 2
        assert snap(s.mesh.handle, dt.handle, good, out=None) == 2 and snap(s.mesh.handle, dt.handle, good, stats=None) == 2 and b'NULL' in lib.sdf_last_error()
        assert snap(s.mesh.handle, odt.handle, good) == 2 and b'different contexts' in lib.sdf_last_error()
        assert not dev.any() and not at.any() and not sumsq.any() and not q.any() and not status.any() and not residual.any() and not evals.any()
        assert not h.value and st.vertices == 0
        for bad in (0, 9, 2.5):
            with pytest.raises(ValueError):
                s.mesh.triangle_deviation(f, bad)
        for bad in ({'eps': 0.0}, {'tol': -1.0}, {'max_move': -1.0}, {'iters': 0}, {'eps': float('nan')}, {'max_move': float('inf')}):
            with pytest.raises(ValueError):
                s.mesh.snap(f, **dict(dict(eps=1e-4, tol=1e-5, max_move=0.1, iters=4), **bad))
        with pytest.raises(ValueError):
            s.mesh.triangle_deviation(odt, 2)
        with pytest.raises(ValueError):
            s.mesh.snap(odt, 1e-4, 1e-5, 0.1)
        eng.precision = engine.PRECISION_F32
        try:
            with pytest.raises(ValueError, match='float32'):
                s.mesh.triangle_deviation(f, 2)
            with pytest.raises(ValueError, match='float32'):
                s.mesh.snap(f, 1e-4, 1e-5, 0.1)
        finally:
            eng.precision = engine.PRECISION_F64
        with pytest.raises(ValueError):
            f.deviation(order=0, samples=SAMPLES, verbose=False)
        with pytest.raises(ValueError):
            f.deviation(snap={'iters': 0}, samples=SAMPLES, verbose=False)
        # an empty mesh: empty arrays, no launch
        e = Soup(eng, np.zeros((0, 9)))
        try:
            assert [x.shape for x in e.mesh.triangle_deviation(f, 2)] == [(0,)] * 3
            e.mesh._welded()
            moved = e.mesh.snap(f, 1e-4, 1e-5, 0.1)
            assert moved.n_triangles == 0 and moved.snap_result[0].shape == (0, 3) and moved.snap_stats['vertices'] == 0
            moved.close()
        finally:
            e.close()
        # ... and the mesh serves the calls that are in order
        ev = lambda P: eng.eval_points(f, P)
        same(s.mesh.triangle_deviation(f, 2), ref.deviation(ev, tris.reshape(-1, 3, 3), 2))
        assert lib.sdf_mesh_deviation_last_kernel_ms() > 0
        moved, got = snapped(s.mesh, f, dict(eps=1e-4, tol=1e-5, max_move=4.0, iters=4))
        moved.close()
        same(got, ref.snap(ev, s.welded()[0], 1e-4, 1e-5, 4.0, 4))
        assert moved.snap_stats['kernel_ms'] > 0
    finally:
        s.close()
        odt._fin()
        other._fin()
