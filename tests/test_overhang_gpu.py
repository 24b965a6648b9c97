"""Build directions rated on the device (csrc/sdf_overhang.hip, `Mesh.overhangs`, `Mesh.overhang_classes`, `overhangs`): lo, hi, the
three totals and both counts bit-identical to the definition (tests/overhang_ref.py) whatever the triangle count, the direction
count and the slabs; the classes exactly; end to end; the refusals and the leaks.  Every refusal is decided on the host before a
launch; no test repeats a device call that failed."""
import ctypes

import numpy as np
import pytest

import fixtures
import measure_ref
import overhang_ref as ref
from sdf_amd import core, engine, overhang
from test_measure_gpu import BOX, SAMPLES, Soup, _free, bits, device_mesh, meshed

pytestmark = pytest.mark.gpu

C = ref.C
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby')


def same_rating(got, want):
    for k in ('lo', 'hi', 'sums'):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), '%s: %d of %d values differ, first at %s: %r != %r' % (
            k, bad.sum(), bad.size, np.argwhere(bad)[0], got[k][bad][0], want[k][bad][0])
    for k in ('overhang_triangles', 'contact_triangles'):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, got[k], want[k])


def random_soup(n_tris, seed=11):
    """small triangles scattered through a box that lies off the origin (test_measure_gpu.random_soup's box; its triangles span the
    whole box, and a triangle that wide never lies on the bed)"""
    rng = np.random.RandomState(seed + n_tris % 1000)
    return rng.uniform(-1.1, 1.1, size=(n_tris, 1, 3)) + rng.uniform(-0.02, 0.02, size=(n_tris, 3, 3)) + np.array([0.5, -2.0, 3.0])


WIDE_BED = 0.6      # a tolerance at which a few triangles in a corner of the box are bed contact for any direction


def random_directions(k, seed=7):
    return ref.normalise(np.random.RandomState(seed + k).normal(size=(k, 3)))


def rated(eng, tris, D, angle=30.0, bed_tol=0.05, max_scratch_bytes=0, classes=False):
    """(the device's rating, the slabs it took[, the device's classes]) of an adopted soup"""
    s = Soup(eng, tris)
    try:
        got = s.mesh.overhangs(D, ref.sin_limit_of(angle), bed_tol, max_scratch_bytes)
        n_slabs = ctypes.c_int64(-1)
        eng.lib.sdf_overhang_last_kernel_ms(ctypes.byref(n_slabs))
        if classes:
            return got, n_slabs.value, s.mesh.overhang_classes(D[0], ref.sin_limit_of(angle), bed_tol)
        return got, n_slabs.value
    finally:
        s.close()


# ---- adopted soups against the definition ----
# one triangle, a wave / a tile of 256 less one, whole, plus one, a chunk less one / whole / plus one, two chunks and a bit, and
# 256 C + 1: 257 partials, a second level of the tree
@pytest.mark.parametrize('n_tris', (0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 256 * C + 1))
def test_adopted_soups_are_bit_identical_to_the_definition(n_tris, eng):
    tris, D = random_soup(n_tris), random_directions(3)
    got, n_slabs = rated(eng, tris, D)
    want = ref.rate(tris, D, ref.sin_limit_of(30.0), 0.05)
    same_rating(got, want)
    assert n_slabs == (1 if n_tris else 0)
    if n_tris >= 63:
        assert want['overhang_triangles'].min() > 0 and (want['sums'][:, :2] > 0).all()
    if n_tris == 0:
        assert (got['lo'] == np.inf).all() and (got['hi'] == -np.inf).all() and not got['sums'].any()


# one lane, a wave of directions less one / whole / plus one, a workgroup of 256 less one / whole / plus one (a second group), more
@pytest.mark.parametrize('k', (1, 2, 63, 64, 65, 130, 255, 256, 257, 600))
def test_direction_counts(k, eng):
    tris, D = random_soup(2 * C + 3), random_directions(k)
    got, n_slabs = rated(eng, tris, D, bed_tol=WIDE_BED)
    want = ref.rate(tris, D, ref.sin_limit_of(30.0), WIDE_BED)
    same_rating(got, want)
    assert n_slabs == 1 and got['lo'].shape == (k,) and want['contact_triangles'].sum() > 0


# the partials of one direction of 2 C + 3 triangles: 3 chunks x (3 doubles + a count word) + one second-level group x 3 doubles
PER_DIRECTION = 3 * (3 * 8 + 4) + 3 * 8


@pytest.mark.parametrize('k,cap,slabs', [(130, 50 * PER_DIRECTION, 3), (130, 1, 130), (600, 256 * PER_DIRECTION + 9, 3), (600, 100 * PER_DIRECTION, 10)])
def test_slabs_change_no_bit(k, cap, slabs, eng):
    """50 + 50 + 30 directions; one direction per slab (a cap below one direction's partials); 256 + 256 + 88; 64 x 9 + 24"""
    tris, D = random_soup(2 * C + 3), random_directions(k)
    whole, one = rated(eng, tris, D, bed_tol=WIDE_BED)
    cut, n_slabs = rated(eng, tris, D, bed_tol=WIDE_BED, max_scratch_bytes=cap)
    assert one == 1 and n_slabs == slabs
    same_rating(cut, whole)
    same_rating(cut, ref.rate(tris, D, ref.sin_limit_of(30.0), WIDE_BED))


@pytest.mark.parametrize('bed_tol', (0.0, 0.05))
@pytest.mark.parametrize('angle', (0.0, 30.0, 45.0, 89.0))
def test_angles_and_tolerances(angle, bed_tol, eng):
    tris, D = random_soup(2 * C + 3), random_directions(3)
    got, _ = rated(eng, tris, D, angle, bed_tol)
    want = ref.rate(tris, D, ref.sin_limit_of(angle), bed_tol)
    same_rating(got, want)
    assert want['overhang_triangles'].min() > 0 or angle == 89.0     # (sin 89 = 0.99985: a random face that steep is one in 13,000)


def test_a_nan_vertex_an_inf_vertex_and_a_zero_area_triangle(eng):
    tris = random_soup(C + 300)
    tris[700, 1, 2] = np.nan
    tris[C + 5, 0, 0] = np.inf
    tris[900, 2] = tris[900, 0]                                  # two equal vertices: no area
    D = random_directions(5)
    got, _, cls = rated(eng, tris, D, classes=True)
    want = ref.rate(tris, D, ref.sin_limit_of(30.0), 0.05, classes=True)
    assert np.isfinite(want['sums']).all() and np.isfinite(want['lo']).all()
    same_rating(got, want)
    assert np.array_equal(cls, want['classes'][0]) and cls[700] == cls[C + 5] == ref.NONFINITE and cls[900] == ref.NEITHER


def test_a_soup_of_nan_triangles(eng):
    tris, D = np.full((5, 3, 3), np.nan), random_directions(2)
    got, _, cls = rated(eng, tris, D, classes=True)
    same_rating(got, ref.rate(tris, D, ref.sin_limit_of(30.0), 0.05))
    assert (got['lo'] == np.inf).all() and (got['hi'] == -np.inf).all() and not got['sums'].any()
    assert not got['overhang_triangles'].any() and not got['contact_triangles'].any() and (cls == ref.NONFINITE).all()


# ---- the constructed cases ----
def derived(eng, tris, d, angle):
    D = ref.normalise(d)
    got, _ = rated(eng, tris, D, angle, 0.0)
    same_rating(got, ref.rate(tris, D, ref.sin_limit_of(angle), 0.0))
    return {k: v[0] for k, v in dict(got, **overhang.derive(got)).items()}


def test_the_cube_on_the_device(eng):
    cube = measure_ref.cube_soup()
    o = derived(eng, cube, Z, 45)
    assert (o['height'], o['contact_area'], o['overhang_area'], o['support_volume']) == (1.0, 1.0, 0.0, 0.0)
    assert (o['overhang_triangles'], o['contact_triangles'], o['lo'], o['hi']) == (0, 2, 0.5, 1.5)
    o = derived(eng, cube, (1, 1, 1), 45)
    assert o['overhang_area'] == 0.0 and o['support_volume'] == 0.0
    o = derived(eng, cube, (1, 1, 1), 30)
    assert o['overhang_area'] == 3.0 and abs(o['support_volume'] - 1.0) <= 1e-12 and o['overhang_triangles'] == 6
    o = derived(eng, cube, (1, 0, 1), 30)
    assert o['overhang_area'] == 2.0 and abs(o['support_volume'] - 0.5) <= 1e-12


def test_the_t_on_the_device(eng):
    t = ref.t_soup()
    up, down, side = derived(eng, t, Z, 45), derived(eng, t, (0, 0, -1), 45), derived(eng, t, Y, 45)
    assert (up['height'], up['overhang_area'], up['support_volume'], up['contact_area']) == (3.0, 3.0, 6.0, 1.0)
    assert (down['overhang_area'], down['support_volume'], down['contact_area']) == (1.0, 1.0, 3.0)
    assert (side['height'], side['overhang_area'], side['support_volume'], side['contact_area']) == (1.0, 0.0, 0.0, 5.0)


def test_the_translated_cube_has_the_same_areas(eng):
    for d, angle in ((Z, 45), ((1, 1, 1), 30), ((1, 0, 1), 30)):
        here = derived(eng, measure_ref.cube_soup(), d, angle)
        there = derived(eng, measure_ref.cube_soup(shift=(1024.0, -512.0, 256.0)), d, angle)
        for k in ('overhang_area', 'contact_area', 'overhang_triangles', 'contact_triangles'):
            assert here[k] == there[k], (d, k, here[k], there[k])


# ---- classes ----
@pytest.mark.parametrize('case', ('random', 't'))
def test_classes_equal_the_definition(case, eng):
    tris = random_soup(2 * C + 3) if case == 'random' else ref.t_soup()
    D = random_directions(1) if case == 'random' else ref.normalise(Z)
    angle, tol = (30.0, WIDE_BED) if case == 'random' else (45.0, 0.0)
    got, _, cls = rated(eng, tris, D, angle, tol, classes=True)
    want = ref.rate(tris, D, ref.sin_limit_of(angle), tol, classes=True)
    assert cls.dtype == np.uint8 and np.array_equal(cls, want['classes'][0])
    assert (cls == ref.OVERHANG).sum() == got['overhang_triangles'][0] > 0
    assert (cls == ref.CONTACT).sum() == got['contact_triangles'][0] > 0


# ---- generated meshes ----
@pytest.mark.parametrize('name', MODELS)
def test_generated_meshes(name, ns, eng):
    f, bounds, soup, pts, cells = meshed(name, ns, eng)
    assert len(soup) > C
    D = ref.sphere_directions(58)
    s, tol = ref.sin_limit_of(45.0), max(core.grid_axes(bounds, samples=SAMPLES)[3])
    m = device_mesh(name, ns, eng)
    try:
        got = m.overhangs(D, s, tol)
        again = m.overhangs(D, s, tol)
    finally:
        m.close()
    want = ref.rate(soup, D, s, tol)
    same_rating(got, want)
    same_rating(again, want)
    assert len(D) == 64 and (want['hi'] > want['lo']).all() and want['overhang_triangles'].max() > 0 and want['contact_triangles'].max() > 0


def test_a_record_mesh_gives_the_same_bits(ns, eng):
    f, bounds, soup, pts, cells = meshed('ex_example', ns, eng)
    D = ref.sphere_directions(58)
    warm = device_mesh('ex_example', ns, eng, records=True)       # (the first call of a model sizes the slab; the second uses it)
    warm.close()
    m = device_mesh('ex_example', ns, eng, records=True)
    try:
        got = m.overhangs(D, ref.sin_limit_of(45.0), 0.02)
        cls = m.overhang_classes(D[4], ref.sin_limit_of(45.0), 0.02)
    finally:
        m.close()
    want = ref.rate(soup, D, ref.sin_limit_of(45.0), 0.02)
    same_rating(got, want)
    assert np.array_equal(cls, ref.rate(soup, D[4:5], ref.sin_limit_of(45.0), 0.02, classes=True)['classes'][0])


# ---- end to end ----
def same_overhangs(got, want, angle, tol, classes=None):
    """an `Overhangs` against the dict of ref.overhangs"""
    assert isinstance(got, overhang.Overhangs) and got.angle == angle and got.bed_tolerance == tol
    for k in ('directions', 'lo', 'hi', 'height', 'overhang_area', 'support_volume', 'contact_area', 'sums'):
        g = getattr(got, k)
        assert g.dtype == np.float64 and not g.flags.writeable and np.array_equal(bits(g), bits(want[k])), (k, g, want[k])
    for k in ('overhang_triangles', 'contact_triangles'):
        g = getattr(got, k)
        assert g.dtype == np.int64 and not g.flags.writeable and np.array_equal(g, want[k]), (k, g, want[k])
    if classes is None:
        assert got.classes is None
    else:
        assert got.classes.dtype == np.uint8 and not got.classes.flags.writeable and np.array_equal(got.classes, classes)


def defined(soup, n, angle, tol, classes=False):
    """the definition's result for directions=n, an int: `sphere_directions(n)` as they are (they are normalised once)"""
    D = ref.sphere_directions(n)
    r = ref.rate(soup, D, ref.sin_limit_of(angle), tol, classes)
    return dict(r, directions=D, **ref.derive(r))


def test_overhangs_end_to_end(ns, eng):
    f, bounds, _, _, _ = meshed('ex_example', ns, eng)
    tol = float(max(core.grid_axes(bounds, samples=SAMPLES)[3]))   # the default: the largest step of the grid
    pts, cells, _ = f.generate_mesh(samples=SAMPLES, verbose=False)
    soup = pts[cells]
    got = f.overhangs(58, samples=SAMPLES, verbose=False)
    same_overhangs(got, defined(soup, 58, 45.0, tol), 45.0, tol)
    assert 0 <= got.best() < 64 and got.support_volume[got.best()] == got.support_volume.min()
    again = ns['overhangs'](f, [X, (1, 1, 1)], angle=30, bed_tolerance=0.0, samples=SAMPLES, verbose=False)
    same_overhangs(again, ref.overhangs(soup, [X, (1, 1, 1)], 30.0, 0.0), 30.0, 0.0)
    one = f.overhangs(angle=60, classes=True, samples=SAMPLES, verbose=False)              # the default direction: up
    want = ref.overhangs(soup, Z, 60.0, tol, classes=True)
    same_overhangs(one, want, 60.0, tol, want['classes'][0])
    assert (one.classes == ref.CONTACT).sum() == one.contact_triangles[0] > 0
    with pytest.raises(AttributeError):
        got.angle = 1.0                                           # immutable
    with pytest.raises(ValueError):
        got.support_volume[0] = 0.0


def test_keep_and_simplify(ns, eng):
    f = fixtures.build('ex_example', ns) | ns['sphere'](0.2).translate((0, 0, 1.6))
    kw = dict(bounds=((-1.2, -1.2, -1.2), (1.2, 1.2, 2.0)), samples=SAMPLES, verbose=False)
    D = ref.sphere_directions(0)
    for extra in (dict(keep='largest'), dict(simplify=2)):
        pts, cells, _ = f.generate_mesh(**dict(kw, **extra))
        got = f.overhangs(D, bed_tolerance=0.01, **dict(kw, **extra))
        same_overhangs(got, ref.overhangs(pts[cells], D, 45.0, 0.01), 45.0, 0.01)
    whole = f.overhangs(D, bed_tolerance=0.01, **kw)
    kept = f.overhangs(D, bed_tolerance=0.01, keep='largest', **kw)
    assert kept.height[4] < whole.height[4]                       # the small sphere above the part is gone


def test_a_model_with_a_closure(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    got = f.overhangs(6, angle=40, bed_tolerance=0.03, bounds=BOX, samples=SAMPLES, verbose=False)
    pts, cells, _ = f.generate_mesh(bounds=BOX, samples=SAMPLES, verbose=False)
    same_overhangs(got, defined(pts[cells], 6, 40.0, 0.03), 40.0, 0.03)
    assert len(cells) > 256 and got.overhang_area.min() > 0


def test_a_mesh_read_from_an_stl_file(tmp_path, ns):
    f = fixtures.build('ex_example', ns)
    f.save(str(tmp_path / 'a.stl'), samples=SAMPLES, verbose=False)
    mesh = ns['Mesh'].from_stl(str(tmp_path / 'a.stl'))
    got = mesh.overhangs(20, angle=50)
    soup = np.asarray(mesh.points)[np.asarray(mesh.triangles)]
    same_overhangs(got, defined(soup, 20, 50.0, 0.0), 50.0, 0.0)
    assert got.directions.shape == (26, 3) and (got.height > 1.0).all()


def test_a_t_of_boxes_lies_down(ns, eng):
    """a 3 x 1 x 1 bar on a 1 x 1 x 2 stem, meshed at 2^13 samples, over the six axes: lying on its flat side needs no support,
    upright it needs the bar's two wings held up.  The bounds come from the grid's step, not from the device's numbers."""
    box = ns['box']
    f = box((1, 1, 2)).translate((0, 0, 1)) | box((3, 1, 1)).translate((0, 0, 2.5))
    bounds = ((-1.75, -0.75, -0.25), (1.75, 0.75, 3.25))
    step = float(max(core.grid_axes(bounds, samples=SAMPLES)[3]))
    o = f.overhangs(0, bounds=bounds, samples=SAMPLES, verbose=False)
    assert o.bed_tolerance == step and np.array_equal(o.directions, ref.sphere_directions(0))
    assert o.best() in (2, 3)                                    # +y or -y
    for k in (2, 3):
        assert o.support_volume[k] < step * o.contact_area[k]
        assert o.contact_area[k] > 5.0 - 12.0 * step               # the T's flat side, 1 x 2 + 3 x 1, less a strip along its outline of 12
    # upright: the wings' underside, 2 x (1 x 1), give or take a strip one step wide along the perimeter of the underside, 2 (3 + 1)
    assert abs(o.overhang_area[4] - 2.0) <= step * 8.0
    assert o.support_volume[4] > (2.0 - 8.0 * step) * (2.0 - step) and abs(o.height[4] - 3.0) <= 2 * step


# ---- refusals and leaks ----
def test_abi_refusals(eng):
    lib = eng.lib
    tris = random_soup(C + 7)
    s = Soup(eng, tris)
    try:
        good = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
        values, counts, cls = np.zeros((2, 5)), np.zeros((2, 2), np.int64), np.zeros(len(tris), np.uint8)
        pd, pv, pc, pk = (good.ctypes.data_as(engine._f64p), values.ctypes.data_as(engine._f64p),
                          counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cls.ctypes.data_as(engine._u8p))
        h = s.mesh.handle

        def refused(rc, *words):
            msg = lib.sdf_last_error()
            assert rc == 2 and all(w in msg for w in words), (rc, msg)

        refused(lib.sdf_mesh_overhangs(None, pd, 2, 0.5, 0.0, 0, pv, pc), b'sdf_mesh_overhangs', b'NULL')
        refused(lib.sdf_mesh_overhangs(h, None, 2, 0.5, 0.0, 0, pv, pc), b'NULL')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, 0.5, 0.0, 0, None, pc), b'NULL')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, 0.5, 0.0, 0, pv, None), b'NULL')
        refused(lib.sdf_mesh_overhangs(h, pd, 0, 0.5, 0.0, 0, pv, pc), b'n_dirs')
        refused(lib.sdf_mesh_overhangs(h, pd, (1 << 20) + 1, 0.5, 0.0, 0, pv, pc), b'2^20')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, 1.0, 0.0, 0, pv, pc), b'sin_limit')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, -0.1, 0.0, 0, pv, pc), b'sin_limit')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, float('nan'), 0.0, 0, pv, pc), b'sin_limit')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, 0.5, -1e-9, 0, pv, pc), b'bed_tol')
        refused(lib.sdf_mesh_overhangs(h, pd, 2, 0.5, float('nan'), 0, pv, pc), b'bed_tol')
        for bad in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0), (0.0, 0.0, 1.0 + 1e-9), (0.6, 0.0, 0.8 - 1e-9)):
            d = np.array([[0.0, 0.0, 1.0], bad])
            refused(lib.sdf_mesh_overhangs(h, d.ctypes.data_as(engine._f64p), 2, 0.5, 0.0, 0, pv, pc), b'direction 1', b'unit length')
            refused(lib.sdf_mesh_overhang_classes(h, d[1:].ctypes.data_as(engine._f64p), 0.5, 0.0, pk), b'sdf_mesh_overhang_classes', b'direction 0')
        refused(lib.sdf_mesh_overhang_classes(None, pd, 0.5, 0.0, pk), b'NULL')
        refused(lib.sdf_mesh_overhang_classes(h, None, 0.5, 0.0, pk), b'NULL')
        refused(lib.sdf_mesh_overhang_classes(h, pd, 0.5, 0.0, None), b'NULL')
        refused(lib.sdf_mesh_overhang_classes(h, pd, 1.5, 0.0, pk), b'sin_limit')
        refused(lib.sdf_mesh_overhang_classes(h, pd, 0.5, -1.0, pk), b'bed_tol')
        assert not values.any() and not counts.any() and not cls.any()              # nothing was written
        # ... the binding turns a refusal into a ValueError, and the mesh serves the calls that are in order
        with pytest.raises(ValueError, match='unit length'):
            s.mesh.overhangs(2.0 * good, 0.5, 0.0)
        with pytest.raises(ValueError, match='sin_limit'):
            s.mesh.overhang_classes(good[0], 1.0, 0.0)
        want = ref.rate(tris, good, 0.5, 0.0, classes=True)
        same_rating(s.mesh.overhangs(good, 0.5, 0.0), want)
        assert np.array_equal(s.mesh.overhang_classes(good[1], 0.5, 0.0), want['classes'][1])
    finally:
        s.close()


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through sdf_mesh_overhangs on 400,000 random triangles x 64 directions (and through the classes):
    each failure carries the allocator's message, the free device memory is what it was, and the next call matches the definition"""
    lib = eng.lib
    warm = Soup(eng, random_soup(3))                            # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.overhangs(random_directions(2), 0.5, 0.0)
        warm.mesh.overhang_classes(Z, 0.5, 0.0)
    finally:
        warm.close()
    tris, D = random_soup(400000), random_directions(64)
    s = Soup(eng, tris)
    try:
        eng.synchronize()
        f0 = _free(lib)
        values, counts, cls = np.zeros((64, 5)), np.zeros((64, 2), np.int64), np.zeros(len(tris), np.uint8)
        pd, pv, pc, pk = (D.ctypes.data_as(engine._f64p), values.ctypes.data_as(engine._f64p),
                          counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cls.ctypes.data_as(engine._u8p))
        for call in (lambda: lib.sdf_mesh_overhangs(s.mesh.handle, pd, 64, 0.5, 0.05, 0, pv, pc),
                     lambda: lib.sdf_mesh_overhang_classes(s.mesh.handle, pd, 0.5, 0.05, pk)):
            failures = 0
            for n in range(1, 6):
                lib.sdf_test_fail_alloc(n)
                rc = call()
                lib.sdf_test_fail_alloc(0)
                assert _free(lib) == f0                          # every block is back, failed or not
                if rc == 0:
                    break
                failures += 1
                assert rc == 1 and b'emory' in lib.sdf_last_error(), lib.sdf_last_error()
            assert failures >= 1 and rc == 0
        want = ref.rate(tris, D, 0.5, 0.05)
        got = {'lo': values[:, 0], 'hi': values[:, 1], 'sums': values[:, 2:5], 'overhang_triangles': counts[:, 0],
               'contact_triangles': counts[:, 1]}
        same_rating({k: np.ascontiguousarray(v) for k, v in got.items()}, want)
        same_rating(s.mesh.overhangs(D, 0.5, 0.05), want)
        assert np.array_equal(cls, ref.rate(tris, D[:1], 0.5, 0.05, classes=True)['classes'][0])
        assert (cls == ref.OVERHANG).sum() == counts[0, 0] and _free(lib) == f0
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
