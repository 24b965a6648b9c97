"""A mesh simplified to a tolerance on the device (csrc/sdf_simplify.hip, `engine.Mesh.simplify_adaptive`, `simplify_tolerance=`):
every soup compared EXACTLY, as int64 bit patterns, with the definition (tests/adaptive_ref.py) applied to the mesh's own weld, and
every statistic but kernel_ms as integers; then through the public API.  Every refusal is decided on the host or before any output
exists; no test repeats a device call that failed."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as aref
import measure_ref
import mend_ref
import normals_ref
import simplify_ref as ref
import test_adaptive_host as ahost
import test_simplify_host as host
from sdf_amd import core, engine, simplify

pytestmark = pytest.mark.gpu

BOUNDS = ((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85))
SAMPLES = 2 ** 15
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(small, want, tolerance):
    """a device mesh simplified to a tolerance against the definition's Adaptive: the soup bit for bit, the statistics as integers"""
    got = small.points()
    assert small.n_triangles == len(want.soup) and got.shape == (3 * len(want.soup), 3) and got.dtype == np.float64
    bad = bits(got) != bits(want.soup.reshape(-1, 3))
    assert not bad.any(), '%d of %d doubles differ, first at %s' % (bad.sum(), bad.size, np.argwhere(bad)[0])
    st = small.simplify_stats
    assert {k: st[k] for k in aref.STAT_KEYS} == want.stats, (st, want.stats)
    assert all(isinstance(st[k], int) for k in aref.STAT_KEYS if k not in ('clusters_used', 'vertices'))
    assert all(isinstance(n, int) for k in ('clusters_used', 'vertices') for n in st[k])
    assert st['kernel_ms'] >= 0.0 and st['tolerance'] == float(tolerance)


def check(mesh, origin, cell, tolerance, levels, reg=1e-3):
    """mesh.simplify_adaptive against the definition on the mesh's OWN weld; returns the definition's Adaptive"""
    pts, cells = mesh.weld()
    want = aref.simplify_adaptive(pts.copy(), cells.copy(), origin, cell, tolerance, levels, reg)
    small = mesh.simplify_adaptive(origin, cell, tolerance, levels, reg)
    try:
        same(small, want, tolerance)
    finally:
        small.close()
    print('tolerance %g, levels %d: triangles %d -> %d, vertices per level %s, clusters used %s, mean_fallback %d, flat %d'
          % (tolerance, levels, len(cells), len(want.soup), want.stats['vertices'], want.stats['clusters_used'], want.stats['mean_fallback'],
             want.stats['flat']))
    return want


def check_soup(tris, origin, cell, tolerance, levels, reg=1e-3):
    with core.adopted(np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 3, 3)) as mesh:
        return check(mesh, origin, cell, tolerance, levels, reg)


# ---- constructed cases ----
def test_a_triangle_inside_one_cluster_leaves_nothing(eng):
    soup, origin, cell = host.case('one_cluster')
    for tol, levels in ((0.0, 0), (0.1, 2), (np.inf, 2)):
        want = check_soup(soup, origin, cell, tol, levels)
        assert want.soup.shape == (0, 3, 3) and want.stats['collapsed'] == 1 and sum(want.stats['clusters_used']) == 1


@pytest.mark.parametrize('levels', (0, 1, 10))
@pytest.mark.parametrize('tol', (0.0, 0.2, np.inf))
def test_a_tetrahedron_over_four_cells(tol, levels, eng):
    soup, origin, cell = host.case('tetrahedron')
    want = check_soup(soup, origin, cell, tol, levels)
    assert sum(want.stats['vertices']) == 4 and len(want.stats['vertices']) == levels + 1
    if levels == 0 or tol == 0.0:
        assert want.stats['triangles_out'] == 4                   # one vertex per cluster, three planes through it: err is rounding noise at best
    if np.isinf(tol) and levels == 10:
        assert want.stats['vertices'][10] == 4 and want.stats['triangles_out'] == 0      # the level-10 grid is a single cluster


@pytest.mark.parametrize('which', ('well_below', 'well_above', 'zero', 'inf'))
def test_a_sheet_with_a_tent(which, eng):
    pts, cells, origin, cell = ahost.tent()
    lo, hi = ahost.tent_thresholds()
    tol = {'well_below': lo, 'well_above': hi, 'zero': 0.0, 'inf': np.inf}[which]
    want = check_soup(pts[cells], origin, cell, tol, 2)
    if which == 'well_below':
        assert want.stats['vertices'] == [64, 192, 0] and want.stats['clusters_used'] == [4, 3, 0] and want.stats['triangles_out'] > 0
    if which in ('well_above', 'inf'):
        assert want.stats['vertices'] == [0, 0, 256] and want.stats['clusters_used'] == [0, 0, 1] and want.stats['triangles_out'] == 0


@pytest.mark.parametrize('name', ('cell_faces', 'straddles_the_origin', 'zero_area_across_cells', 'two_planes_across_cells'))
def test_constructed_numeric_cases(name, eng):
    """negative zero and cell faces, negative coordinates, flat clusters and fallen-back ones, on three levels"""
    soup, origin, cell = host.case(name)
    for tol in (0.0, 0.02, np.inf):
        want = check_soup(soup, origin, cell / 2.0, tol, 2)
    if name == 'zero_area_across_cells':
        assert want.stats['flat'] > 0
    want = check_soup(soup, origin, cell, 0.01, 0)
    if name == 'two_planes_across_cells':
        assert want.stats['mean_fallback'] > 0


def strip(u):
    """a soup with exactly u welded vertices: the first u vertices of a sheet of two rows, 0.25 apart, with the triangles among
    them, a lifted vertex, and a degenerate triangle for every vertex that no other triangle uses"""
    pts, cells, origin, cell = ahost.tent(h=0.0, n=130, rows=2)
    pts = pts[:u].copy()
    if u > 12:
        pts[11, 2] = 0.05
    cells = cells[(cells < u).all(axis=1)]
    unused = np.setdiff1d(np.arange(u), cells.reshape(-1))
    cells = np.concatenate([cells, np.repeat(unused, 3).reshape(-1, 3)])
    return pts[cells], origin, cell


@pytest.mark.parametrize('u', (1, 63, 64, 65, 255, 256, 257))
def test_vertex_counts_at_the_edges_of_a_wave_and_a_workgroup(u, eng):
    soup, origin, cell = strip(u)
    assert len(ref.weld(soup)[0]) == u
    want = check_soup(soup, origin, cell / 4.0, 0.004, 4)         # level 0: one vertex per cluster along x
    assert sum(want.stats['vertices']) == u
    if u > 12:
        assert want.stats['vertices'][0] > 0 and sum(want.stats['vertices'][1:]) > 0      # the tent stays fine, the rest does not
    want = check_soup(soup, origin, cell / 8.0, 0.004, 1)         # level 0: every vertex is a cluster of its own, u of them
    assert len(want.accepted[0]) == u


def test_no_triangles_no_launch(eng):
    with core.adopted(np.zeros((0, 3, 3))) as mesh:
        small = mesh.simplify_adaptive(np.zeros(3), np.ones(3), 0.1, 3)
        try:
            assert small.n_triangles == 0 and small.points().shape == (0, 3)
            st = small.simplify_stats
            assert st['clusters_used'] == [0] * 4 and st['vertices'] == [0] * 4 and st['levels'] == 3 and st['triangles_in'] == 0
        finally:
            small.close()


# ---- meshed models ----
def grid():
    if 'grid' not in _cache:
        _cache['grid'] = core.grid_axes(BOUNDS, samples=SAMPLES)
    return _cache['grid']


def model(ns, name):
    return host.example(ns) if name == 'example' else ns['sphere'](1).shell(0.06)


@pytest.mark.parametrize('name', ('example', 'shell'))
def test_meshed_models(name, ns, eng):
    """the shell's two sheets fall into the same coarse clusters: its output is not closed and has duplicates"""
    X, Y, Z, step = grid() if name == 'example' else core.grid_axes(((-1.1,) * 3, (1.1,) * 3), samples=SAMPLES)
    origin, cell = simplify.resolve_cell(1, X, Y, Z, step)
    mesh = eng.generate(model(ns, name), X, Y, Z, 32, True)
    try:
        for tol in (0.05, 0.1):
            want = check(mesh, origin, cell, tol * step[0], 5)
            assert 0 < want.stats['triangles_out'] < want.stats['triangles_in']
        if name == 'shell':
            pts, cells = ref.weld(want.soup)
            c = measure_ref.edge_census(cells, len(pts))
            assert mend_ref.mend(cells).stats['triangles_out'] < len(cells) or not c['closed'], c
        # levels = 0 is Mesh.simplify on the same grid, on the device too
        a, b = mesh.simplify_adaptive(origin, cell * 2.0, 0.3, 0), mesh.simplify(origin, cell * 2.0)
        try:
            assert a.n_triangles == b.n_triangles > 0 and np.array_equal(bits(a.points()), bits(b.points()))
            sa, sb = a.simplify_stats, b.simplify_stats
            assert sa['clusters_used'] == [sb['clusters']] and (sa['mean_fallback'], sa['flat'], sa['collapsed']) == (sb['mean_fallback'], sb['flat'], sb['collapsed'])
        finally:
            a.close()
            b.close()
        # tolerance = inf is Mesh.simplify on the coarsest grid
        a, b = mesh.simplify_adaptive(origin, cell, np.inf, 2), mesh.simplify(origin, cell * 4.0)
        try:
            assert a.n_triangles == b.n_triangles > 0 and np.array_equal(bits(a.points()), bits(b.points()))
        finally:
            a.close()
            b.close()
    finally:
        mesh.close()


# ---- through the public API ----
def wanted(ns):
    """the example's full weld, downloaded once, and the definition on it at 0.1 step"""
    if 'want' not in _cache:
        X, Y, Z, step = grid()
        pts, cells, _ = host.example(ns).generate_mesh(bounds=BOUNDS, samples=SAMPLES, verbose=False)
        pts, cells = np.array(pts), np.array(cells)
        tol = 0.1 * step[0]
        want = aref.simplify_adaptive(pts, cells, *simplify.resolve_cell(1, X, Y, Z, step), tol, 5)
        _cache['want'] = (tol, want) + ref.weld(want.soup)
    return _cache['want']


def test_generate_mesh_measure_and_save_with_a_tolerance(tmp_path, ns, eng):
    f = host.example(ns)
    tol, want, wp, wc = wanted(ns)
    kw = dict(bounds=BOUNDS, samples=SAMPLES, verbose=False)
    pts, cells, n = f.generate_mesh(simplify_tolerance=tol, **kw)
    assert n is None and np.array_equal(bits(pts), bits(wp)) and np.array_equal(cells, wc) and 0 < len(cells) < want.stats['triangles_in']
    st = core.generate_mesh.last_simplify
    assert {k: st[k] for k in aref.STAT_KEYS} == want.stats and st['tolerance'] == tol
    # simplify= is the finest cluster, simplify_levels= the levels above it
    X, Y, Z, step = grid()
    pts0, cells0, _ = f.generate_mesh(**kw)
    two = aref.simplify_adaptive(np.array(pts0), np.array(cells0), *simplify.resolve_cell(2, X, Y, Z, step), tol, 3)
    pts, cells, _ = f.generate_mesh(simplify=2, simplify_tolerance=tol, simplify_levels=3, **kw)
    assert np.array_equal(bits(pts), bits(ref.weld(two.soup)[0])) and core.generate_mesh.last_simplify['vertices'] == two.stats['vertices']
    # measure, mended: keep -> simplify -> mend
    m = f.measure(simplify_tolerance=tol, mend=True, **kw)
    mended = mend_ref.mend(wc, want.soup)
    v = measure_ref.derive(measure_ref.moments(mended.soup))['volume']
    assert m.triangles == mended.stats['triangles_out'] and abs(m.volume - v) <= 1e-12 * abs(v)
    # a PLY file with normals, parsed back
    f.save(str(tmp_path / 'x.ply'), simplify_tolerance=tol, normals=True, **kw)
    p, nn, c, head = normals_ref.parse_ply(str(tmp_path / 'x.ply'))
    assert head == normals_ref.ply_header(len(wp), len(wc), True) and np.array_equal(c, wc)
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32))
    lo, hi = np.asarray(BOUNDS[0]), np.asarray(BOUNDS[1])
    eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    want_n = normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), wp, eps)[0]
    assert np.array_equal(nn.view(np.int32), want_n.astype(np.float32).view(np.int32))
    # an STL file read back, simplified to a tolerance and mended: Mesh.from_stl(p).simplify_adaptive(...).mend()
    f.save(str(tmp_path / 'x.stl'), **kw)
    mesh = ns['Mesh'].from_stl(str(tmp_path / 'x.stl'))
    small = mesh.simplify_adaptive(step[0], tol, levels=3)
    soup = np.asarray(mesh.points, dtype=np.float64)[np.asarray(mesh.triangles)]
    fp, fc = ref.weld(soup)
    fwant = aref.simplify_adaptive(fp, fc, fp.min(axis=0), np.full(3, step[0]), tol, 3)
    assert isinstance(small, ns['Mesh']) and np.array_equal(small.points, ref.weld(fwant.soup)[0]) and np.array_equal(small.triangles, ref.weld(fwant.soup)[1])
    again = small.mend()
    assert isinstance(again, ns['Mesh']) and len(again.triangles) == mend_ref.mend(ref.weld(fwant.soup)[1]).stats['triangles_out']


def test_without_a_tolerance_nothing_changes(monkeypatch, ns, eng):
    f = host.example(ns)
    kw = dict(bounds=BOUNDS, samples=SAMPLES, verbose=False)
    called = []
    real = engine.Mesh.simplify_adaptive
    monkeypatch.setattr(engine.Mesh, 'simplify_adaptive', lambda self, *a, **k: called.append(1) or real(self, *a, **k))
    a, b = f.generate_mesh(simplify=2, **kw), f.generate_mesh(simplify=2, simplify_tolerance=None, simplify_levels=5, **kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and called == []
    assert 'clusters' in core.generate_mesh.last_simplify
    f.generate_mesh(simplify_tolerance=0.0, **kw)
    assert called == [1] and 'clusters_used' in core.generate_mesh.last_simplify


# ---- refusals ----
def test_refusals(eng):
    lib = eng.lib
    soup, origin, cell = host.case('tetrahedron')
    with core.adopted(soup) as mesh:
        o, c = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
        h, st = ctypes.c_void_p(), engine.SdfAdaptiveStats()
        for args in ((None, o, c, 1e-3, 0.1, 2, ctypes.byref(h), ctypes.byref(st)), (mesh.handle, None, c, 1e-3, 0.1, 2, ctypes.byref(h), ctypes.byref(st)),
                     (mesh.handle, o, None, 1e-3, 0.1, 2, ctypes.byref(h), ctypes.byref(st)), (mesh.handle, o, c, 1e-3, 0.1, 2, None, ctypes.byref(st)),
                     (mesh.handle, o, c, 1e-3, 0.1, 2, ctypes.byref(h), None)):
            assert lib.sdf_mesh_simplify_adaptive(*args) == 2 and b'NULL' in lib.sdf_last_error()
        for tol, levels, word in ((-1.0, 2, b'tolerance'), (float('nan'), 2, b'tolerance'), (0.1, -1, b'levels'), (0.1, 11, b'levels')):
            assert lib.sdf_mesh_simplify_adaptive(mesh.handle, o, c, 1e-3, tol, levels, ctypes.byref(h), ctypes.byref(st)) == 2
            assert word in lib.sdf_last_error()
        big = (ctypes.c_double * 3)(1e308, 1.0, 1.0)
        assert lib.sdf_mesh_simplify_adaptive(mesh.handle, o, big, 1e-3, 0.1, 1, ctypes.byref(h), ctypes.byref(st)) == 2 and b'levels' in lib.sdf_last_error()
        assert h.value is None
        for bad in (-0.1, np.nan, 'a', None, True):
            with pytest.raises(ValueError, match='tolerance'):
                mesh.simplify_adaptive(origin, cell, bad, 2)
        for bad in (-1, 11, 2.0, True):
            with pytest.raises(ValueError, match='levels'):
                mesh.simplify_adaptive(origin, cell, 0.1, bad)
        with pytest.raises(ValueError, match='cell'):
            mesh.simplify_adaptive(origin, np.zeros(3), 0.1, 2)
        with pytest.raises(ValueError, match='reg'):
            mesh.simplify_adaptive(origin, cell, 0.1, 2, reg=-1.0)
        with pytest.raises(ValueError, match='3 components'):
            mesh.simplify_adaptive(np.zeros(2), cell, 0.1, 2)
        with pytest.raises(engine.SdfHipError, match='span'):     # level 0 decides, after the coarser levels ran; nothing is written
            mesh.simplify_adaptive(origin, np.full(3, 2.0 ** -21), 0.1, 2)
        check(mesh, origin, np.full(3, 2.0 ** -20), 0.1, 2)
        ms = (ctypes.c_double * 11)(*([-1.0] * 11))
        total = lib.sdf_mesh_simplify_adaptive_last_kernel_ms(ms)
        assert all(ms[k] >= 0.0 for k in range(3)) and ms[3] == -1.0 and total >= sum(ms[k] for k in range(3))
