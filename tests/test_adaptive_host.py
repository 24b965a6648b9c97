"""The definition of mesh simplification to a tolerance (tests/adaptive_ref.py) on hand-made welds and on the checker's meshes, the
checks of `simplify_tolerance=` / `simplify_levels=`, the public names and the ABI's new names: what can be checked without a device."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import adaptive_ref as aref
import measure_ref
import simplify_ref as ref
import test_simplify_host as host
from sdf_amd import core, engine

simplify = importlib.import_module('sdf_amd.simplify')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = 2 ** 18
LEVELS = 5
TOLERANCES = (0.0, 0.05, 0.1)                                     # in grid steps


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def volume(soup):
    return measure_ref.derive(measure_ref.moments(soup))['volume']


def census(soup):
    pts, cells = ref.weld(soup)
    return measure_ref.edge_census(cells, len(pts))


# ---- the two identities ----
def identities(pts, cells, origin, cell, levels):
    """levels = 0 is the uniform clustering on the cell, tolerance = inf the uniform clustering on cell * 2^levels, bit for bit"""
    fine = ref.simplify(pts, cells, origin, cell)
    for tol in (0.0, 0.3, np.inf):
        got = aref.simplify_adaptive(pts, cells, origin, cell, tol, 0)
        assert got.soup.shape == fine.soup.shape and np.array_equal(bits(got.soup), bits(fine.soup))
        assert got.stats['triangles_out'] == fine.stats['triangles_out'] and got.stats['collapsed'] == fine.stats['collapsed']
        assert got.stats['clusters_used'] == [fine.stats['clusters']] and got.stats['vertices'] == [len(pts)]
        assert (got.stats['mean_fallback'], got.stats['flat']) == (fine.stats['mean_fallback'], fine.stats['flat'])
    coarse = ref.simplify(pts, cells, origin, np.asarray(cell, dtype=np.float64) * 2.0 ** levels)
    got = aref.simplify_adaptive(pts, cells, origin, cell, np.inf, levels)
    assert got.soup.shape == coarse.soup.shape and np.array_equal(bits(got.soup), bits(coarse.soup))
    assert got.stats['clusters_used'] == [0] * levels + [coarse.stats['clusters']] and got.stats['vertices'] == [0] * levels + [len(pts)]
    assert (got.stats['mean_fallback'], got.stats['flat']) == (coarse.stats['mean_fallback'], coarse.stats['flat'])
    assert list(got.stats) == list(aref.STAT_KEYS) and got.stats['levels'] == levels


@pytest.mark.parametrize('name', host.CASES)
def test_the_identities_on_the_constructed_cases(name):
    soup, origin, cell = host.case(name)
    pts, cells = ref.weld(soup)
    identities(pts, cells, origin, cell / 4.0, 2)                 # (level 2 is the case's own grid)
    identities(pts, cells, origin, cell, 3)


def test_the_identities_on_the_example(ns, oracle_lib):
    X, Y, Z, step = core.grid_axes(((-0.85,) * 3, (0.85,) * 3), samples=2 ** 15)
    pts, cells = ref.weld(oracle_lib.generate(host.example(ns), X, Y, Z, 32, True).points.reshape(-1, 3, 3))
    origin, cell = simplify.resolve_cell(1, X, Y, Z, step)
    identities(pts, cells, origin, cell, 3)


# ---- the choice rule: a planar sheet over 4 x 4 level-0 cells and one tent vertex (shared with tests/test_adaptive_gpu.py) ----
TENT_H = 0.05
TENT_AT = (5, 5)                                                  # the lifted vertex: (1.375, 1.375), inside level-0 cell (1, 1) with its six neighbours


def tent(h=TENT_H, n=16, rows=None):
    """(points, cells, origin, cell) of a hand-built weld: n x `rows` vertices 0.25 apart from 0.125 on the plane z = 0, two triangles
    per square, the vertex TENT_AT lifted by h; on the grid of origin (0, 0, -0.5) and cell 1 the sheet covers 4 x 4 cells of level
    0 and one cell of level 2.  The points are in welded (lexicographic) order.  rows < n cuts a strip (tests/test_adaptive_gpu.py)"""
    rows = n if rows is None else rows
    i, j = np.meshgrid(np.arange(n), np.arange(rows), indexing='ij')
    pts = np.stack([0.125 + 0.25 * i, 0.125 + 0.25 * j, np.zeros((n, rows))], axis=-1).reshape(-1, 3)
    if h and rows > TENT_AT[1] + 1:
        pts[TENT_AT[0] * rows + TENT_AT[1], 2] = h
    v = lambda a, b: a * rows + b
    a, b = np.meshgrid(np.arange(n - 1), np.arange(rows - 1), indexing='ij')
    a, b = a.reshape(-1), b.reshape(-1)
    cells = np.concatenate([np.stack([v(a, b), v(a + 1, b), v(a + 1, b + 1)], axis=1), np.stack([v(a, b), v(a + 1, b + 1), v(a, b + 1)], axis=1)])
    return pts, cells.astype(np.int64).reshape(-1, 3), np.array([0.0, 0.0, -0.5]), np.ones(3)


def tent_thresholds(h=TENT_H):
    """(lo, hi) from the definition: with t_L = sqrt(err / w) of the tent's ancestor at level L = 1, 2 -- the tolerance at which that
    cluster's test err <= tolerance^2 w turns -- every tolerance >= hi = 2 max t_L accepts the level-2 cluster, and every tolerance
    <= lo = min t_L / 2 refuses both ancestors; lo is still far above the t of the planar clusters, which is rounding noise"""
    pts, cells, origin, cell = tent(h)
    pyr = aref.pyramid(pts, cells, origin, cell, 2)
    lifted = TENT_AT[0] * 16 + TENT_AT[1]
    t = []
    for lv in (1, 2):
        k = pyr[lv].vertex_cluster[lifted]
        t.append(float(np.sqrt(pyr[lv].err[k] / pyr[lv].weight[k])))
        others = np.delete(np.arange(len(pyr[lv].err)), k)
        assert (np.sqrt(pyr[lv].err[others] / pyr[lv].weight[others]) <= 1e-12).all()      # planar clusters
    assert len(pyr[2].err) == 1 and len(pyr[1].err) == 4 and len(pyr[0].err) == 16
    return min(t) / 2, 2 * max(t)


def test_the_choice_rule_on_a_sheet_with_a_tent():
    h = TENT_H
    pts, cells, origin, cell = tent(h)
    assert np.array_equal(ref.weld(pts[cells])[0], pts) and np.array_equal(ref.weld(pts[cells])[1], cells)      # it IS a weld
    lo, hi = tent_thresholds(h)
    print('tent of height %g: refused below %.6g, accepted above %.6g' % (h, lo, hi))
    # the residual of a point of the sheet's plane in a plane of the tent is at most h |n|, so no threshold can lie above h by much
    assert 1e-9 < lo < hi <= 2 * h
    # well above h: the one level-2 cluster is accepted, every vertex takes it and nothing survives
    r = aref.simplify_adaptive(pts, cells, origin, cell, hi, 2)
    assert (r.vertex_level == 2).all() and r.stats['vertices'] == [0, 0, 256] and r.stats['clusters_used'] == [0, 0, 1]
    assert r.stats['triangles_out'] == 0 and r.stats['collapsed'] == len(cells)
    # well below: the tent's ancestors are refused, and only they: the 64 vertices of its level-1 cluster stay on level 0, the
    # other three level-1 clusters are planar and accepted
    r = aref.simplify_adaptive(pts, cells, origin, cell, lo, 2)
    in_parent = (pts[:, 0] < 2.0) & (pts[:, 1] < 2.0)
    assert in_parent.sum() == 64 and np.array_equal(r.vertex_level, np.where(in_parent, 0, 1))
    assert r.stats['vertices'] == [64, 192, 0] and r.stats['clusters_used'] == [4, 3, 0]
    assert [a.tolist() for a in r.accepted[1:]] == [[False, True, True, True], [False]] and r.accepted[0].all()
    assert r.stats['triangles_out'] > 0 and r.stats['triangles_out'] + r.stats['collapsed'] == len(cells)
    assert len(np.unique(r.soup.reshape(-1, 3), axis=0)) == 7      # 4 + 3 clusters, each with its own representative
    # intermediate levels need not accept: with levels = 1 the same low tolerance gives the same choice
    r1 = aref.simplify_adaptive(pts, cells, origin, cell, lo, 1)
    assert np.array_equal(r1.vertex_level, r.vertex_level) and np.array_equal(bits(r1.soup), bits(r.soup))
    # tolerance 0: a planar cluster whose rounding noise is not exactly 0 is refused -- level 0 is still always accepted
    r0 = aref.simplify_adaptive(pts, cells, origin, cell, 0.0, 2)
    assert r0.stats['vertices'][0] >= 64 and sum(r0.stats['vertices']) == 256


# ---- models at 2^18 samples, meshed once by the checker ----
MODELS = {'box': (lambda ns: ns['box'](1).translate((0.013, 0.021, 0.008)), 0.7), 'plate': (lambda ns: ns['box']((2, 2, 0.12)), 1.1),
          'example': (host.example, 0.85)}
# triangles out at the tolerances 0, 0.05 and 0.1 step: what tests/adaptive_ref.py gives
COUNTS = {'box': (19828, 3136, 12), 'plate': (10722, 1796, 1796), 'example': (37230, 8578, 4808)}


@pytest.fixture(scope='module')
def models(ns, oracle_lib):
    out = {}
    for name, (make, b) in MODELS.items():
        X, Y, Z, step = core.grid_axes(((-b, -b, -b), (b, b, b)), samples=SAMPLES)
        soup = oracle_lib.generate(make(ns), X, Y, Z, 32, True).points.reshape(-1, 3, 3)
        pts, cells = ref.weld(soup)
        origin, cell = simplify.resolve_cell(1, X, Y, Z, step)
        pyr = aref.pyramid(pts, cells, origin, cell, LEVELS)
        for a in (soup, pts, cells):
            a.setflags(write=False)
        m = {'soup': soup, 'points': pts, 'cells': cells, 'grid': (X, Y, Z, step), 'volume': volume(soup)}
        m['done'] = [aref.simplify_adaptive(pts, cells, origin, cell, t * step[0], LEVELS, pyramid_of_it=pyr) for t in TOLERANCES]
        out[name] = m
    return out


def uniform(m, k):
    return ref.simplify(m['points'], m['cells'], *simplify.resolve_cell(k, *m['grid']))


@pytest.mark.parametrize('name', sorted(MODELS))
def test_models_stay_closed_and_oriented(models, name):
    m = models[name]
    c0 = measure_ref.edge_census(m['cells'], len(m['points']))
    assert c0['closed'] and c0['oriented'] and c0['nonmanifold'] == 0
    for tol, r, want in zip(TOLERANCES, m['done'], COUNTS[name]):
        c = census(r.soup)
        print('%s at %g step: %d -> %d triangles, volume %.5f (unsimplified %.5f), vertices per level %s, clusters used %s, mean_fallback %d'
              % (name, tol, len(m['cells']), len(r.soup), volume(r.soup), m['volume'], r.stats['vertices'], r.stats['clusters_used'],
                 r.stats['mean_fallback']))
        assert c['closed'] and c['oriented'] and c['nonmanifold'] == 0, (name, tol, c)
        assert r.stats['triangles_out'] == len(r.soup) == want and r.stats['collapsed'] == len(m['cells']) - want
        assert sum(r.stats['vertices']) == len(m['points']) and r.stats['flat'] == 0


def test_a_box_comes_down_to_its_twelve_triangles(models):
    m = models['box']
    r = m['done'][2]
    v = volume(r.soup)
    print('box: %d -> %d triangles, volume %.5f (unsimplified %.5f; uniform simplify=4: %d)' % (len(m['cells']), len(r.soup), v, m['volume'], len(uniform(m, 4).soup)))
    assert len(r.soup) == 12 and v >= 0.99
    c = census(r.soup)
    assert c['closed'] and c['oriented'] and c['vertices'] == 8 and c['euler'] == 2


def test_the_example_beats_uniform_clusters_of_two(models):
    m = models['example']
    r, u2 = m['done'][2], uniform(m, 2)
    print('example: to 0.1 step %d triangles, volume %.5f; uniform simplify=2 %d, %.5f; unsimplified %.5f'
          % (len(r.soup), volume(r.soup), len(u2.soup), volume(u2.soup), m['volume']))
    assert len(r.soup) < len(u2.soup) == 10844
    assert abs(volume(r.soup) - m['volume']) <= abs(volume(u2.soup) - m['volume'])


def test_a_thin_plate_keeps_its_volume_where_uniform_clusters_do_not(models):
    m = models['plate']
    r, u4 = m['done'][1], uniform(m, 4)
    rel = lambda s: abs(volume(s) - m['volume']) / m['volume']
    print('plate: to 0.05 step %d triangles, volume off by %.3g; uniform simplify=4 %d, off by %.3g' % (len(r.soup), rel(r.soup), len(u4.soup), rel(u4.soup)))
    assert rel(r.soup) <= 1e-3 < rel(u4.soup)


# ---- refusals, public names, ABI ----
def test_the_definition_refuses():
    pts, cells, origin, cell = tent()
    for bad in (-1e-300, -1.0, np.nan, -np.inf, '0.1', None, True, 1 + 0j):
        with pytest.raises(ValueError, match='tolerance'):
            aref.simplify_adaptive(pts, cells, origin, cell, bad, 2)
    for bad in (-1, 11, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='levels'):
            aref.simplify_adaptive(pts, cells, origin, cell, 0.1, bad)
    with pytest.raises(ValueError, match='levels'):
        aref.simplify_adaptive(pts, cells, origin, np.full(3, 1e308), 0.1, 1)
    with pytest.raises(ValueError, match='cell'):
        aref.simplify_adaptive(pts, cells, origin, np.zeros(3), 0.1, 1)
    with pytest.raises(ValueError, match='reg'):
        aref.simplify_adaptive(pts, cells, origin, cell, 0.1, 1, reg=-1.0)
    with pytest.raises(ValueError, match='span'):                 # level 0 has the widest key range: it decides
        aref.simplify_adaptive(pts, cells, origin, np.full(3, 2.0 ** -20), 0.1, 2)
    assert aref.simplify_adaptive(pts, cells, origin, cell, np.inf, 10).stats['triangles_out'] == 0
    empty = aref.simplify_adaptive(np.zeros((0, 3)), np.zeros((0, 3), np.int64), origin, cell, 0.1, 2)
    assert empty.soup.shape == (0, 3, 3) and empty.stats['clusters_used'] == [0, 0, 0] and empty.stats['triangles_in'] == 0


def test_check_tolerance_and_levels():
    assert simplify.check_tolerance(None) is None
    for ok in (0, 0.0, 1e-3, np.float32(0.5), np.int64(2), np.inf):
        assert simplify.check_tolerance(ok) == float(ok) and isinstance(simplify.check_tolerance(ok), float)
    for bad in (-1e-9, -1, np.nan, -np.inf, True, '0.1', (0.1,), 1j):
        with pytest.raises(ValueError, match='simplify_tolerance'):
            simplify.check_tolerance(bad)
    for ok in (0, 5, 10, np.int32(3)):
        assert simplify.check_levels(ok) == int(ok) and isinstance(simplify.check_levels(ok), int)
    for bad in (-1, 11, 2.5, 2.0, True, None, '3'):
        with pytest.raises(ValueError, match='simplify_levels'):
            simplify.check_levels(bad)
    assert simplify.check_adaptive(None, None, 5) == (None, None, None) and simplify.check_adaptive(3, None, 5) == (3.0, None, None)
    assert simplify.check_adaptive(None, 0.01, 5) == (1.0, 0.01, 5)          # only the tolerance: the finest cluster is a grid cell
    assert simplify.check_adaptive(2, np.inf, 0) == (2.0, np.inf, 0)
    with pytest.raises(ValueError, match='simplify_levels'):      # levels without a tolerance would do nothing
        simplify.check_adaptive(2, None, 3)
    with pytest.raises(ValueError, match='simplify'):             # check_simplify keeps refusing what it refuses
        simplify.check_adaptive(0, 0.01, 5)


def test_the_keywords_are_refused_before_anything_is_meshed():
    """a bad simplify_tolerance or simplify_levels raises ValueError before the engine is asked for: this passes without a device"""
    import sdf_amd
    f = sdf_amd.sphere(1)
    calls = (f.generate_mesh, f.measure, f.shells, f.measure_shells, f.overhangs, f.supports, f.thickness)
    for kw, match in (({'simplify_tolerance': -0.1}, 'simplify_tolerance'), ({'simplify_tolerance': np.nan}, 'simplify_tolerance'),
                      ({'simplify_tolerance': 'fine'}, 'simplify_tolerance'), ({'simplify_tolerance': True}, 'simplify_tolerance'),
                      ({'simplify_tolerance': 0.01, 'simplify_levels': 11}, 'simplify_levels'),
                      ({'simplify_tolerance': 0.01, 'simplify_levels': 2.5}, 'simplify_levels'),
                      ({'simplify_levels': 3}, 'simplify_levels'), ({'simplify': 2, 'simplify_levels': 0}, 'simplify_levels'),
                      ({'simplify': -2, 'simplify_tolerance': 0.01}, 'simplify')):
        for call in calls:
            with pytest.raises(ValueError, match=match):
                call(samples=2 ** 10, verbose=False, **kw)
        with pytest.raises(ValueError, match=match):
            f.save('never_written.stl', samples=2 ** 10, verbose=False, **kw)
    assert not os.path.exists('never_written.stl')


def test_the_public_names():
    measure = importlib.import_module('sdf_amd.measure')
    shells = importlib.import_module('sdf_amd.shells')
    mesh = importlib.import_module('sdf_amd.mesh')
    overhang = importlib.import_module('sdf_amd.overhang')
    supports = importlib.import_module('sdf_amd.supports')
    thickness = importlib.import_module('sdf_amd.thickness')
    for fn in (core.save, core.generate_mesh, core.meshed.__wrapped__, measure.measure, shells.shells, shells.measure_shells, overhang.overhangs,
               supports.supports, thickness.thickness):
        p = inspect.signature(fn).parameters
        assert p['simplify_tolerance'].default is None and p['simplify_levels'].default == 5 and p['simplify'].default is None, fn
    assert 'simplify_tolerance' not in inspect.signature(core.generate).parameters      # the reference's signature
    assert core.Meshed._fields == ('mesh', 'points', 'tape', 'engine', 'bounds', 'stats', 'simplify_stats')
    p = inspect.signature(engine.Mesh.simplify_adaptive).parameters
    assert list(p) == ['self', 'origin', 'cell', 'tolerance', 'levels', 'reg'] and p['levels'].default == 5 and p['reg'].default == 1e-3
    p = inspect.signature(mesh.Mesh.simplify_adaptive).parameters
    assert list(p) == ['self', 'cell', 'tolerance', 'levels', 'origin', 'reg']
    assert p['levels'].default == 5 and p['origin'].default is None and p['reg'].default == 1e-3
    assert list(inspect.signature(mesh.Mesh.simplify).parameters) == ['self', 'cell', 'origin', 'reg']
    assert list(inspect.signature(engine.Mesh.simplify).parameters) == ['self', 'origin', 'cell', 'reg']


def test_the_abi_names_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION == 17
    for name in ('sdf_mesh_simplify_adaptive', 'sdf_mesh_simplify_adaptive_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    lib = engine.load_library()
    assert lib.sdf_abi_version() == version and all(hasattr(lib, n) for n in engine.ABI)
    fields = ['triangles_in', 'triangles_out', 'collapsed', 'levels', 'mean_fallback', 'flat', 'clusters_used', 'vertices', 'kernel_ms']
    assert [k for k, _ in engine.SdfAdaptiveStats._fields_] == fields
    m = re.search(r'typedef struct sdf_adaptive_stats \{(.*?)\} sdf_adaptive_stats;', hdr, re.S).group(1)
    assert re.findall(r'\b(%s)\b' % '|'.join(fields), m) == fields
    assert int(re.search(r'#define\s+SDF_ADAPTIVE_MAX_LEVELS\s+(\d+)', hdr).group(1)) == engine.ADAPTIVE_MAX_LEVELS == aref.MAX_LEVELS == 10
    assert engine.SdfAdaptiveStats.clusters_used.size == engine.SdfAdaptiveStats.vertices.size == 8 * 11
    assert set(aref.STAT_KEYS) == set(fields) - {'kernel_ms'}
    # the uniform entry point and its statistics are what they were
    assert [k for k, _ in engine.SdfSimplifyStats._fields_] == list(ref.STAT_KEYS) + ['kernel_ms']
