"""The definition of mesh simplification (tests/simplify_ref.py) on the example models and on hand-made meshes, `check_simplify` /
`resolve_cell`, and the ABI's new names: what can be checked without a device."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import components_ref
import measure_ref
import simplify_ref as ref
from sdf_amd import core, engine

simplify = importlib.import_module('sdf_amd.simplify')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = 2 ** 18


# ---- the example models, meshed once by the checker ----
def example(ns):
    f = ns['sphere'](1) & ns['box'](1.5)
    c = ns['cylinder'](0.5)
    return f - (c.orient(ns['X']) | c.orient(ns['Y']) | c.orient(ns['Z']))


@pytest.fixture(scope='module')
def models(ns, oracle_lib):
    out = {}
    for name, f, b in (('example', example(ns), 0.85), ('sphere', ns['sphere'](1), 1.1)):
        X, Y, Z, step = core.grid_axes(((-b, -b, -b), (b, b, b)), samples=SAMPLES)
        soup = oracle_lib.generate(f, X, Y, Z, 32, True).points.reshape(-1, 3, 3)
        pts, cells = ref.weld(soup)
        for a in (soup, pts, cells):
            a.setflags(write=False)
        out[name] = {'soup': soup, 'points': pts, 'cells': cells, 'grid': (X, Y, Z, step), 'done': {}}
    return out


def simplified(models, name, k):
    m = models[name]
    if k not in m['done']:
        origin, cell = simplify.resolve_cell(k, *m['grid'])
        m['done'][k] = ref.simplify(m['points'], m['cells'], origin, cell)
    return m['done'][k]


def volume(soup):
    return measure_ref.derive(measure_ref.moments(soup))['volume']


def live_clusters(r, cells):
    tc = r.vertex_cluster[cells]
    return tc[(tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])]


@pytest.mark.parametrize('k, want', ((2, 10844), (4, 3102), (8, 600)))
def test_example_counts(models, k, want):
    m = models['example']
    assert len(m['cells']) == 46288
    r = simplified(models, 'example', k)
    assert r.soup.shape == (want, 3, 3) and r.soup.dtype == np.float64
    assert r.stats['triangles_in'] == 46288 and r.stats['triangles_out'] == want and r.stats['collapsed'] == 46288 - want
    assert r.stats['clusters'] == len(r.vertices) and r.stats['flat'] == 0 and list(r.stats) == list(ref.STAT_KEYS)
    pts, cells = ref.weld(r.soup)
    census = measure_ref.edge_census(cells, len(pts))
    assert census['closed'] and census['oriented'] and census['collapsed'] == 0, census
    assert len(pts) == r.used.sum()                               # clusters that no survivor touches appear nowhere


@pytest.mark.parametrize('name', ('example', 'sphere'))
def test_the_quadric_vertex_keeps_the_volume_and_the_mean_does_not(models, name):
    """simplify=4: within 1 % of the unsimplified volume with the quadric vertices, outside it with the cluster means
    (measured: example 0.27 % / 3.3 %, sphere 0.38 % / 1.2 %)"""
    m = models[name]
    r = simplified(models, name, 4)
    v0 = volume(m['soup'])
    quadric = abs(volume(r.soup) - v0) / v0
    mean_only = abs(volume((r.centres + r.means)[live_clusters(r, m['cells'])]) - v0) / v0
    print('%s: quadric %.4f %%, mean only %.4f %%' % (name, 100 * quadric, 100 * mean_only))
    assert quadric <= 0.01 < mean_only, (quadric, mean_only)


@pytest.mark.parametrize('k', (2, 3.5, 8))
@pytest.mark.parametrize('name', ('example', 'sphere'))
def test_directed_edges_stay_balanced(models, name, k):
    """the input is closed and oriented: every directed edge A -> B of the output occurs as often as B -> A"""
    m = models[name]
    census = measure_ref.edge_census(m['cells'], len(m['points']))
    assert census['closed'] and census['oriented']
    r = simplified(models, name, k)
    tc = live_clusters(r, m['cells'])
    assert len(tc) == r.stats['triangles_out'] > 0
    a, b = tc.reshape(-1), tc[:, [1, 2, 0]].reshape(-1)
    n = int(r.stats['clusters'])
    fwd, back = np.unique(a * n + b, return_counts=True), np.unique(b * n + a, return_counts=True)
    assert np.array_equal(fwd[0], back[0]) and np.array_equal(fwd[1], back[1])
    assert np.array_equal(r.soup, r.vertices[tc])


# ---- constructed cases (shared with tests/test_simplify_gpu.py) ----
def sheet(z_of, x0, x1, y0=0.3, y1=0.7, n=4):
    xs, ys = np.linspace(x0, x1, n), np.linspace(y0, y1, n)
    v = lambda i, j: np.array([xs[i], ys[j], z_of(xs[i], ys[j])])
    t = []
    for i in range(n - 1):
        for j in range(n - 1):
            t += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
    return np.array(t)


PLANE = (0.3, 0.2, 0.2)                                           # z = 0.3 x + 0.2 y + 0.2


def case(name):
    """(soup (T, 3, 3), origin, cell) of a constructed case"""
    one = np.ones(3)
    if name == 'one_cluster':
        return np.array([[[0.1, 0.1, 0.1], [0.6, 0.2, 0.1], [0.2, 0.7, 0.3]]]), np.zeros(3), one
    if name == 'tetrahedron':
        return components_ref.tetrahedron(), np.full(3, -0.5), one
    if name == 'cell_faces':                                      # every coordinate a whole multiple of the cell, one of them -0.0
        soup = components_ref.cube(0.0, 1.0) * 0.5
        soup[soup[..., 2] == 0.0, 2] = -0.0
        return np.concatenate([soup, soup + np.array([1.0, -0.5, 0.0])]), np.zeros(3), np.full(3, 0.5)
    if name == 'straddles_the_origin':
        return np.concatenate([components_ref.cube(-0.5, 0.5), components_ref.tetrahedron(shift=(-3.25, -0.25, -1.75), scale=1.5)]), np.zeros(3), one
    if name == 'planar':
        return sheet(lambda x, y: PLANE[0] * x + PLANE[1] * y + PLANE[2], 0.1, 0.9, 0.1, 0.9, 5), np.zeros(3), one
    if name == 'zero_area':
        return np.array([[[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4]], [[0.2, 0.2, 0.2], [0.1, 0.1, 0.1], [0.4, 0.4, 0.4]]]), np.zeros(3), one
    if name == 'two_planes_meet_outside':                         # z = 0.4 and z = 0.48 + 0.1 (x - 0.5): they meet at x = -0.3
        return np.concatenate([sheet(lambda x, y: 0.4 + 0.0 * x, 0.4, 0.6), sheet(lambda x, y: 0.48 + 0.1 * (x - 0.5), 0.4, 0.6)]), np.zeros(3), one
    if name == 'two_planes_meet_inside':                          # ... z = 0.41 + 0.1 (x - 0.5): at x = 0.4
        return np.concatenate([sheet(lambda x, y: 0.4 + 0.0 * x, 0.4, 0.6), sheet(lambda x, y: 0.41 + 0.1 * (x - 0.5), 0.4, 0.6)]), np.zeros(3), one
    # the same three kinds of cluster spread over several cells, so that triangles survive and carry the representatives out
    if name == 'planar_across_cells':
        return sheet(lambda x, y: PLANE[0] * x + PLANE[1] * y + PLANE[2], 0.1, 2.9, 0.1, 2.9, 8), np.zeros(3), one
    if name == 'zero_area_across_cells':
        line = np.array([[0.1, 0.1, 0.1], [1.2, 1.2, 1.2], [2.4, 2.4, 2.4], [3.7, 3.7, 3.7]])
        return line[[[0, 1, 2], [1, 0, 2], [1, 2, 3]]], np.zeros(3), one
    if name == 'two_planes_across_cells':
        return np.concatenate([sheet(lambda x, y: 0.4 + 0.0 * x, 0.4, 2.6, 0.3, 1.7, 8),
                               sheet(lambda x, y: 0.48 + 0.1 * (x - 0.5), 0.4, 2.6, 0.3, 1.7, 8)]), np.zeros(3), one
    raise KeyError(name)


CASES = ('one_cluster', 'tetrahedron', 'cell_faces', 'straddles_the_origin', 'planar', 'zero_area', 'two_planes_meet_outside',
         'two_planes_meet_inside', 'planar_across_cells', 'zero_area_across_cells', 'two_planes_across_cells')


def run(name, **kw):
    soup, origin, cell = case(name)
    pts, cells = ref.weld(soup)
    return pts, cells, origin, cell, ref.simplify(pts, cells, origin, cell, **kw)


def test_a_triangle_inside_one_cluster_leaves_nothing():
    pts, cells, origin, cell, r = run('one_cluster')
    assert r.soup.shape == (0, 3, 3) and r.stats == {'clusters': 1, 'triangles_in': 1, 'triangles_out': 0, 'collapsed': 1, 'mean_fallback': 0, 'flat': 0}
    assert r.used.sum() == 0


def test_a_tetrahedron_over_four_cells_keeps_its_connectivity():
    pts, cells, origin, cell, r = run('tetrahedron')
    assert r.stats['clusters'] == 4 and r.stats['triangles_out'] == 4 and r.stats['collapsed'] == 0
    assert np.array_equal(r.vertex_cluster, np.arange(4))         # key order is welded order here
    assert np.array_equal(ref.weld(r.soup)[1], cells)
    # one vertex per cluster, three planes through it: the representative is the vertex, to rounding
    assert np.abs(r.vertices - pts).max() <= 1e-12 and r.stats['mean_fallback'] == 0 and r.stats['flat'] == 0


def test_cell_faces_and_negative_zero():
    origin, cell = np.zeros(3), np.full(3, 0.5)
    p = np.array([[0.0, 0.5, 1.0], [-0.0, 0.5, 1.0], [0.5, 0.0, -0.0], [-0.5, -1e-300, 0.5 - 1e-17]])
    vc, q, centres = ref.clusters(p, origin, cell)
    assert q[vc].tolist() == [[0, 1, 2], [0, 1, 2], [1, 0, 0], [-1, -1, 1]]      # a face belongs to the cell above; 0.5 - 1e-17 IS 0.5
    assert vc[0] == vc[1] and np.array_equal(centres[vc[3]], [-0.25, -0.25, 0.75])
    pts, cells, origin, cell, r = run('cell_faces')
    assert r.stats['clusters'] == 16 and r.stats['triangles_out'] == 24 and np.isfinite(r.soup).all()
    plus = ref.simplify(pts + 0.0, cells, origin, cell)           # (+ 0.0 turns -0.0 into +0.0)
    assert np.array_equal(plus.vertex_cluster, r.vertex_cluster) and np.array_equal(plus.soup, r.soup)


def test_negative_coordinates_go_through_floor():
    pts, cells, origin, cell, r = run('straddles_the_origin')
    assert r.stats['clusters'] == 12 and r.stats['triangles_out'] == 16      # truncation would put the cube into one cell
    q = np.floor(pts / cell).astype(np.int64)
    assert q.min() == -4 and np.array_equal(r.centres[r.vertex_cluster], (q + 0.5) * cell)
    assert (r.centres[:, 0] < 0).sum() == 8
    assert (np.abs(r.vertices - r.centres) <= cell / 2).all()


def test_a_planar_cluster_stays_on_its_plane():
    pts, cells, origin, cell, r = run('planar')
    assert r.stats['clusters'] == 1 and r.stats['flat'] == 0 and r.stats['mean_fallback'] == 0 and r.stats['triangles_out'] == 0
    q = ref.quadrics(pts, cells, r.vertex_cluster, r.centres)[0]
    a = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
    assert np.linalg.matrix_rank(a, tol=1e-9 * np.trace(a)) == 1
    v = r.vertices[0]
    extent = np.ptp(pts, axis=0).max()
    off = abs(PLANE[0] * v[0] + PLANE[1] * v[1] + PLANE[2] - v[2]) / np.sqrt(PLANE[0] ** 2 + PLANE[1] ** 2 + 1)
    print('planar: off the plane by %.3g, extent %.3g' % (off, extent))
    assert np.isfinite(v).all() and off <= 1e-12 * extent and (np.abs(v - r.centres[0]) <= cell / 2).all()


def test_a_cluster_of_zero_area_triangles_is_flat():
    pts, cells, origin, cell, r = run('zero_area')
    assert r.stats['flat'] == 1 and r.stats['mean_fallback'] == 0 and r.stats['clusters'] == 1
    assert np.array_equal(r.vertices, r.centres + r.means)
    assert np.allclose(r.vertices[0], pts.mean(axis=0), rtol=0, atol=1e-15)


def test_a_minimiser_outside_the_cell_falls_back_to_the_mean():
    pts, cells, origin, cell, r = run('two_planes_meet_outside')
    assert r.stats['clusters'] == 1 and r.stats['mean_fallback'] == 1 and r.stats['flat'] == 0
    assert np.array_equal(r.vertices, r.centres + r.means)
    pts, cells, origin, cell, r = run('two_planes_meet_inside')
    assert r.stats['mean_fallback'] == 0 and not np.array_equal(r.vertices, r.centres + r.means)
    assert (np.abs(r.vertices - r.centres) <= cell / 2).all()
    assert abs(r.vertices[0, 2] - 0.4) < 2e-3 and abs(r.vertices[0, 0] - 0.4) < 0.05      # near the line where the planes meet


def test_the_same_clusters_across_cells_leave_triangles():
    pts, cells, origin, cell, r = run('planar_across_cells')
    assert r.stats['triangles_out'] > 0 and r.stats['flat'] == 0 and r.stats['mean_fallback'] == 0
    v = r.soup.reshape(-1, 3)
    off = np.abs(PLANE[0] * v[:, 0] + PLANE[1] * v[:, 1] + PLANE[2] - v[:, 2]).max()
    assert off <= 1e-12 * np.ptp(pts, axis=0).max(), off
    pts, cells, origin, cell, r = run('zero_area_across_cells')
    assert r.stats == {'clusters': 4, 'triangles_in': 3, 'triangles_out': 3, 'collapsed': 0, 'mean_fallback': 0, 'flat': 4}
    assert np.array_equal(r.vertices, r.centres + r.means)
    pts, cells, origin, cell, r = run('two_planes_across_cells')
    assert r.stats['triangles_out'] > 0 and r.stats['mean_fallback'] > 0 and r.stats['flat'] == 0, r.stats
    assert r.used[(r.vertices == r.centres + r.means).all(axis=1)].any()          # a fallen-back vertex is in the soup


def huge(n, dtype):
    """n rows of three zeros that take 24 bytes"""
    return np.lib.stride_tricks.as_strided(np.zeros(3, dtype), shape=(n, 3), strides=(0, np.dtype(dtype).itemsize), writeable=False)


def test_refusals():
    soup, origin, cell = case('tetrahedron')
    pts, cells = ref.weld(soup)
    for bad in (0.0, -1.0, np.inf, np.nan, (1.0, 1.0, 0.0), (1.0, 1.0), 'a'):
        with pytest.raises(ValueError):
            ref.simplify(pts, cells, origin, np.broadcast_to(bad, (3,)) if np.isscalar(bad) and not isinstance(bad, str) else bad)
    for bad in ((0.0, np.nan, 0.0), (np.inf, 0.0, 0.0), (0.0, 0.0)):
        with pytest.raises(ValueError, match='origin'):
            ref.simplify(pts, cells, bad, cell)
    for bad in (-1e-300, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='reg'):
            ref.simplify(pts, cells, origin, cell, reg=bad)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[2, 1] = bad
        with pytest.raises(ValueError, match='not finite'):
            ref.simplify(p, cells, origin, cell)
    with pytest.raises(ValueError, match='span'):                 # 2^21 cells between the nearest and the farthest vertex
        ref.simplify(pts, cells, origin, np.full(3, 2.0 ** -21))
    assert ref.simplify(pts, cells, origin, np.full(3, 2.0 ** -20)).stats['clusters'] == 4
    with pytest.raises(ValueError, match='span'):                 # a floor beyond 2^53
        ref.simplify(pts * 1e300, cells, origin, np.full(3, 1e280))
    with pytest.raises(ValueError, match='2\\^31'):
        ref.simplify(huge(2 ** 31, np.float64), cells, origin, cell)
    with pytest.raises(ValueError, match='2\\^31'):
        ref.simplify(pts, huge((2 ** 31 + 2) // 3, np.int64), origin, cell)
    empty = ref.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int64), origin, cell)
    assert empty.soup.shape == (0, 3, 3) and set(empty.stats.values()) == {0}


# ---- the host side of the package ----
def test_check_simplify_and_resolve_cell():
    assert simplify.check_simplify(None) is None
    for ok in (2, 3.5, np.float32(4), np.int64(8), 1e-3, 1):
        assert simplify.check_simplify(ok) == float(ok) and isinstance(simplify.check_simplify(ok), float)
    for bad in (0, -2, 0.0, np.nan, np.inf, True, False, '4', (2, 2, 2), [4], 2 + 0j, {}):
        with pytest.raises(ValueError, match='simplify'):
            simplify.check_simplify(bad)
    X, Y, Z, step = core.grid_axes(((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)), step=(0.1, 0.2, 0.25))
    origin, cell = simplify.resolve_cell(3.5, X, Y, Z, step)
    assert origin.dtype == cell.dtype == np.float64
    assert np.array_equal(origin, [X[0], Y[0], Z[0]]) and np.array_equal(cell, [3.5 * 0.1, 3.5 * 0.2, 3.5 * 0.25])
    with pytest.raises(ValueError, match='simplify'):
        simplify.resolve_cell(None, X, Y, Z, step)
    with pytest.raises(ValueError, match='simplify'):
        simplify.resolve_cell(-1, X, Y, Z, step)


def test_simplify_is_refused_before_anything_is_meshed():
    """a simplify that is no positive number raises ValueError before the engine is asked for: this passes without a device"""
    import sdf_amd
    f = sdf_amd.sphere(1)
    for bad in (0, -1.5, 'fine', True):
        for call in (f.generate_mesh, f.measure, f.shells, f.measure_shells):
            with pytest.raises(ValueError, match='simplify'):
                call(simplify=bad, samples=2 ** 10, verbose=False)
        with pytest.raises(ValueError, match='simplify'):
            f.save('never_written.stl', simplify=bad, samples=2 ** 10, verbose=False)
    assert not os.path.exists('never_written.stl')


def test_the_public_names():
    measure = importlib.import_module('sdf_amd.measure')
    shells = importlib.import_module('sdf_amd.shells')
    mesh = importlib.import_module('sdf_amd.mesh')
    for fn in (core.save, core.generate_mesh, core.meshed.__wrapped__, measure.measure, shells.shells, shells.measure_shells):
        assert inspect.signature(fn).parameters['simplify'].default is None, fn
    assert 'simplify' not in inspect.signature(core.generate).parameters       # the reference's signature
    assert core.Meshed._fields[-1] == 'simplify_stats' and core.Meshed(1, 2, 3, 4, 5, 6).simplify_stats is None
    assert core.generate_mesh.last_simplify is None or isinstance(core.generate_mesh.last_simplify, dict)
    assert callable(engine.Mesh.simplify) and callable(mesh.Mesh.simplify)
    p = inspect.signature(mesh.Mesh.simplify).parameters
    assert list(p) == ['self', 'cell', 'origin', 'reg'] and p['origin'].default is None and p['reg'].default == 1e-3
    assert inspect.signature(engine.Mesh.simplify).parameters['reg'].default == 1e-3


def test_the_abi_names_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION == 17
    for name in ('sdf_mesh_simplify', 'sdf_mesh_simplify_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    lib = engine.load_library()
    assert lib.sdf_abi_version() == version and hasattr(lib, 'sdf_mesh_simplify') and all(hasattr(lib, n) for n in engine.ABI)
    fields = ['clusters', 'triangles_in', 'triangles_out', 'collapsed', 'mean_fallback', 'flat', 'kernel_ms']
    assert [k for k, _ in engine.SdfSimplifyStats._fields_] == fields
    m = re.search(r'typedef struct sdf_simplify_stats \{(.*?)\} sdf_simplify_stats;', hdr, re.S).group(1)
    assert re.findall(r'\b(%s)\b' % '|'.join(fields), m) == fields
    assert engine.SIMPLIFY_FIELDS == ref.STAT_KEYS
