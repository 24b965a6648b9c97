"""The definition of tests/overhang_ref.py against constructed cases (no GPU): the cube and the T with the numbers worked out by
hand, the tree sum against math.fsum, the directions, the record's methods, the refusals of the Python entry points, the ABI."""
import math
import os
import re

import numpy as np
import pytest

import measure_ref
import overhang_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def one(soup, d, angle, bed_tol=0.0):
    o = ref.overhangs(soup, d, angle, bed_tol)
    return {k: (v[0] if isinstance(v, np.ndarray) and k != 'directions' else v) for k, v in o.items()}


# ---- the constructed cases ----
def test_the_cube_upright():
    o = one(measure_ref.cube_soup(), Z, 45)
    assert o['height'] == 1.0 and o['lo'] == 0.5 and o['hi'] == 1.5
    assert o['contact_area'] == 1.0 and o['overhang_area'] == 0.0 and o['support_volume'] == 0.0
    assert o['overhang_triangles'] == 0 and o['contact_triangles'] == 2


def test_the_cube_on_its_corner():
    cube = measure_ref.cube_soup()
    o = one(cube, (1, 1, 1), 45)                                  # the three lower faces make 54.7 degrees with the vertical's plane: no overhang
    assert o['overhang_area'] == 0.0 and o['support_volume'] == 0.0 and o['overhang_triangles'] == 0
    assert abs(o['height'] - math.sqrt(3.0)) <= 1e-15 and o['contact_triangles'] == 0 and o['contact_area'] == 0.0
    o = one(cube, (1, 1, 1), 30)
    assert o['overhang_area'] == 3.0 and abs(o['support_volume'] - 1.0) <= 1e-12 and o['overhang_triangles'] == 6
    assert abs(o['lo'] - 1.5 / math.sqrt(3.0)) <= 1e-15 and abs(o['hi'] - 4.5 / math.sqrt(3.0)) <= 1e-15


def test_the_cube_on_its_edge():
    o = one(measure_ref.cube_soup(), (1, 0, 1), 30)
    assert o['overhang_area'] == 2.0 and abs(o['support_volume'] - 0.5) <= 1e-12 and o['overhang_triangles'] == 4
    assert abs(o['height'] - math.sqrt(2.0)) <= 1e-15


def test_the_t_in_three_directions():
    t = ref.t_soup()
    up, down, side = one(t, Z, 45), one(t, (0, 0, -1), 45), one(t, Y, 45)
    # upright: the whole underside of the bar overhangs, the 1 x 1 face hidden inside the soup included
    assert (up['height'], up['overhang_area'], up['support_volume'], up['contact_area']) == (3.0, 3.0, 6.0, 1.0)
    assert (up['lo'], up['hi'], up['overhang_triangles'], up['contact_triangles']) == (0.0, 3.0, 2, 2)
    assert (down['height'], down['overhang_area'], down['support_volume'], down['contact_area']) == (3.0, 1.0, 1.0, 3.0)
    assert (side['height'], side['overhang_area'], side['support_volume'], side['contact_area']) == (1.0, 0.0, 0.0, 5.0)
    assert side['contact_triangles'] == 4 and side['overhang_triangles'] == 0


def test_the_bed_tolerance_turns_low_overhangs_into_contact():
    """a chamfered foot: a face that looks down at 45 degrees and ends 0.25 above the bed"""
    a, b, c = np.array([0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([-0.25, 0.0, 0.25])
    soup = np.array([[a, c, b], [[0, 0, 0], [1, 0, 0], [0, 1, 0]][::-1]], dtype=np.float64)
    strict, loose = one(soup, Z, 30, 0.0), one(soup, Z, 30, 0.25)
    assert strict['overhang_triangles'] == 1 and strict['contact_triangles'] == 1
    assert loose['overhang_triangles'] == 0 and loose['contact_triangles'] == 2 and loose['overhang_area'] == 0.0


def test_classes_follow_the_predicates():
    t = ref.t_soup().copy()
    t[5, 1, 1] = np.nan
    r = ref.rate(t, ref.normalise(Z), ref.sin_limit_of(45), 0.0, classes=True)
    cls = r['classes'][0]
    assert cls.dtype == np.uint8 and cls.shape == (24,) and cls[5] == ref.NONFINITE
    assert (cls == ref.OVERHANG).sum() == r['overhang_triangles'][0] and (cls == ref.CONTACT).sum() == r['contact_triangles'][0]


# ---- the sum ----
def test_the_tree_sum_against_fsum():
    rng = np.random.RandomState(5)
    T = 3 * ref.C + 17
    soup = rng.uniform(-1.1, 1.1, size=(T, 3, 3)) + np.array([0.5, -2.0, 3.0])
    D = ref.normalise(rng.normal(size=(3, 3)))
    s, tol = ref.sin_limit_of(30), 0.05
    r = ref.rate(soup, D, s, tol, classes=True)
    tri, n, dbl, finite = ref.triangle_parts(soup)
    for k, d in enumerate(D):
        h = (tri[:, :, 0] * d[0] + tri[:, :, 1] * d[1]) + tri[:, :, 2] * d[2] - r['lo'][k]
        dn = (n[:, 0] * d[0] + n[:, 1] * d[1]) + n[:, 2] * d[2]
        over, contact = r['classes'][k] == ref.OVERHANG, r['classes'][k] == ref.CONTACT
        assert over.sum() > 100
        want = (math.fsum(dbl[over]), math.fsum(((-dn) * ((h[:, 0] + h[:, 1]) + h[:, 2]))[over]), math.fsum(dbl[contact]))
        for got, w in zip(r['sums'][k], want):
            assert abs(got - w) <= 1e-12 * abs(w), (k, got, w)
        assert r['lo'][k] == h.min() + r['lo'][k] and r['overhang_triangles'][k] == over.sum()


def test_the_chunk_tree_is_the_stated_one():
    """one accumulator per chunk in index order, then groups of 256 partials through the halving tree"""
    rng = np.random.RandomState(3)
    T = 257 * ref.C + 5                                           # 258 partials: a second level
    x = rng.uniform(0, 1, size=(T, 1))
    parts = []
    for c0 in range(0, T, ref.C):
        a = 0.0
        for v in x[c0:c0 + ref.C, 0]:
            a = a + v
        parts.append(a)
    def halve(v):
        v = list(v)
        h = 128
        while h >= 1:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]
    while len(parts) > 1:
        parts = [halve(parts[g:g + 256] + [0.0] * (256 - len(parts[g:g + 256]))) for g in range(0, len(parts), 256)]
    assert ref.chunk_tree_sum(x)[0].tobytes() == np.float64(parts[0]).tobytes()
    assert ref.chunk_tree_sum(x[:5])[0].tobytes() == np.float64((((x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0]) + x[4, 0]).tobytes()


def test_a_nan_triangle_and_a_zero_area_triangle_add_nothing():
    cube = measure_ref.cube_soup()
    bad = cube[3].copy()
    bad[1, 2] = np.nan
    flat = np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 0.5], [1.5, 1.5, 0.5]])          # collinear, on the bed
    high = flat + np.array([0.0, 0.0, 0.5])                                          # ... and above it
    soup = np.concatenate([cube[:5], [bad], cube[5:], [flat, high]])
    D = ref.normalise([Z, (1, 1, 1), (0, -1, 0)])
    got, want = ref.rate(soup, D, ref.sin_limit_of(30), 0.0, classes=True), ref.rate(cube, D, ref.sin_limit_of(30), 0.0)
    for k in ('lo', 'hi', 'sums'):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    for k in ('overhang_triangles', 'contact_triangles'):
        assert np.array_equal(got[k], want[k]), k
    assert (got['classes'][:, 5] == ref.NONFINITE).all() and (got['classes'][:, 13:] == ref.NEITHER).all()


def test_the_empty_soup():
    r = ref.overhangs(np.zeros((0, 3, 3)), [Z, X], 45)
    assert np.array_equal(r['lo'], [np.inf, np.inf]) and np.array_equal(r['hi'], [-np.inf, -np.inf])
    assert not r['sums'].any() and not r['overhang_triangles'].any() and not r['contact_triangles'].any()
    assert r['sums'].shape == (2, 3) and (r['height'] == -np.inf).all() and not r['overhang_area'].any()
    nothing = ref.overhangs(np.full((3, 3, 3), np.nan), Z, 45)
    assert nothing['lo'][0] == np.inf and not nothing['sums'].any()


# ---- directions, the record ----
@pytest.mark.parametrize('n', (0, 1, 58, 256))
def test_sphere_directions(n):
    from sdf_amd import overhang
    d = overhang.sphere_directions(n)
    assert d.shape == (n + 6, 3) and d.dtype == np.float64
    assert np.array_equal(d[:6], [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert (np.abs(length - 1.0) <= np.spacing(1.0)).all()
    assert len(np.unique(d, axis=0)) == n + 6
    assert np.array_equal(bits(d), bits(ref.sphere_directions(n)))            # the package restates the definition's
    if n >= 58:                                                   # ... and the points cover the sphere: none far from a direction
        probe = ref.normalise(np.random.RandomState(1).normal(size=(200, 3)))
        assert (probe @ d.T).max(axis=1).min() > math.cos(math.radians(35.0))


def test_normalise_is_the_written_formula():
    from sdf_amd import overhang
    d = np.array([[3.0, -4.0, 12.0], [1e-3, 2e-3, -5e-4], [0.0, 0.0, 7.0]])
    want = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    assert np.array_equal(bits(ref.normalise(d)), bits(want)) and np.array_equal(bits(overhang.normalise(d)), bits(want))
    assert overhang.normalise((0, 0, 2)).shape == (1, 3)
    assert overhang.sin_limit_of(30) == ref.sin_limit_of(30) == math.sin(math.radians(30.0))


def record(**kw):
    from sdf_amd import overhang
    K = len(kw['directions'])
    base = dict(lo=np.zeros(K), hi=np.ones(K), height=np.ones(K), overhang_area=np.zeros(K), support_volume=np.zeros(K),
                contact_area=np.zeros(K), overhang_triangles=np.zeros(K, np.int64), contact_triangles=np.zeros(K, np.int64),
                angle=45.0, bed_tolerance=0.0, sums=np.zeros((K, 3)), classes=None)
    base.update(kw)
    return overhang.Overhangs(**base)


def test_best_resolves_ties_to_the_first_index():
    d = ref.sphere_directions(0)
    o = record(directions=d, support_volume=np.array([2.0, 1.0, 3.0, 1.0, 1.0, 5.0]), contact_area=np.array([0.0, 4.0, 9.0, 9.0, 1.0, 2.0]))
    assert o.best() == 1 and type(o.best()) is int
    assert o.best('contact_area') == 0
    assert o.best(lambda r: -r.contact_area) == 2
    assert o.best(lambda r: r.support_volume - 1e-3 * r.contact_area) == 3
    with pytest.raises(ValueError):
        o.best(lambda r: r.support_volume[:2])
    with pytest.raises(AttributeError):
        o.angle = 30.0                                            # immutable


def test_rotation_takes_the_direction_to_z():
    rng = np.random.RandomState(2)
    d = ref.normalise(np.concatenate([ref.sphere_directions(58), rng.normal(size=(200, 3)), [[1e-9, 0, -1], [0, 1e-200, 1], [-1e-5, 1e-5, -1]]]))
    o = record(directions=d)
    for k in range(len(d)):
        R = o.rotation(k)
        assert np.abs(R @ d[k] - np.array([0.0, 0.0, 1.0])).max() <= 1e-15, (k, d[k])
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
    assert np.array_equal(o.rotation(4), np.eye(3))
    assert np.array_equal(o.rotation(5) @ np.array([0.0, 0.0, -1.0]), [0.0, 0.0, 1.0])


def test_derive_restates_the_definition():
    from sdf_amd import overhang
    r = ref.rate(ref.t_soup(), ref.sphere_directions(10), ref.sin_limit_of(40), 0.0)
    want, got = ref.derive(r), overhang.derive(r)
    assert sorted(want) == sorted(got) == ['contact_area', 'height', 'overhang_area', 'support_volume']
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k


# ---- refusals: decided in Python, before an engine is asked for ----
@pytest.mark.parametrize('kwargs,match', [
    (dict(directions=(0.0, 0.0, 0.0)), 'zero'),
    (dict(directions=[(0, 0, 1), (np.nan, 0, 1)]), 'not finite'),
    (dict(directions=(1.0, 0.0)), 'shape'),
    (dict(angle=90.0), 'angle'),
    (dict(angle=-1.0), 'angle'),
    (dict(angle=float('nan')), 'angle'),
    (dict(bed_tolerance=-0.1), 'bed_tolerance'),
    (dict(directions=[(0, 0, 1), (1, 0, 0)], classes=True), 'one direction'),
    (dict(directions=6, classes=True), 'one direction'),
])
def test_python_refusals(kwargs, match):
    import sdf_amd
    with pytest.raises(ValueError, match=match):
        sdf_amd.overhangs_soup(measure_ref.cube_soup(), **kwargs)
    with pytest.raises(ValueError, match=match):
        sdf_amd.sphere(1).overhangs(**kwargs)
    with pytest.raises(ValueError, match=match):
        sdf_amd.Mesh(np.zeros((3, 3)), np.array([[0, 1, 2]])).overhangs(**kwargs)


# ---- the ABI ----
NAMES = ('sdf_mesh_overhangs', 'sdf_mesh_overhang_classes', 'sdf_overhang_last_kernel_ms')


def test_the_abi_declares_the_overhang_entries_and_stays_17():
    from sdf_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION == 17
    for name in NAMES:
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    import sdf_amd
    for name in ('overhangs', 'overhangs_of_mesh', 'overhangs_soup', 'sphere_directions', 'Overhangs'):
        assert hasattr(sdf_amd, name), name
    assert hasattr(sdf_amd.SDF3, 'overhangs') and hasattr(sdf_amd.Mesh, 'overhangs')
    assert hasattr(engine.Mesh, 'overhangs') and hasattr(engine.Mesh, 'overhang_classes')


def test_the_built_library_exports_the_overhang_entries():
    from sdf_amd import engine
    lib = engine.load_library()
    assert lib.sdf_abi_version() == 17
    for name in NAMES:
        assert getattr(lib, name) is not None
    units = open(os.path.join(ROOT, 'sdf_amd', 'csrc', 'build.units')).read().splitlines()
    assert ['sdf_overhang', 'sdf_overhang.hip', 'plain'] in [ln.split() for ln in units]      # the flag class that rounds like NumPy
