"""A mesh measured on the device (csrc/sdf_measure.hip, `Mesh.moments`, `Mesh.edge_census`, `measure`): the 11 totals, the box and
both counts bit-identical to the definition (tests/measure_ref.py), the census exactly; end to end; the refusals and the leaks.
Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
import ctypes

import numpy as np
import pytest

import fixtures
import measure_ref as ref
from sdf_amd import core, engine

pytestmark = pytest.mark.gpu

MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'slots_plain_8_8_p8d8')
SAMPLES = 2 ** 13
BOX = ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))
C = ref.C
_meshes = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_moments(got, want):
    for k in ('sums', 'origin', 'box'):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), '%s: %d of %d values differ, first at %s: %r != %r' % (
            k, bad.sum(), bad.size, np.argwhere(bad)[0], got[k][bad][0], want[k][bad][0])
    for k in ('triangles', 'zero_area', 'nonfinite'):
        assert got[k] == want[k], (k, got[k], want[k])


class Soup:
    """a float64 soup in device memory (torch owns it) and the Mesh that adopts it"""

    def __init__(self, eng, tris):
        import torch
        self.host = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 9)
        self.buf = torch.from_numpy(self.host.reshape(-1).copy()).to('cuda:0') if len(self.host) else None
        torch.cuda.synchronize()
        self.mesh = eng.adopt_soup(self.buf.data_ptr() if len(self.host) else 0, len(self.host))

    def close(self):
        self.mesh.close()


def random_soup(n_tris, seed=11):
    rng = np.random.RandomState(seed + n_tris % 1000)
    return rng.uniform(-1.1, 1.1, size=(n_tris, 3, 3)) + np.array([0.5, -2.0, 3.0])


def meshed(name, ns, eng):
    """(model, bounds, soup (T, 3, 3), welded points, cells) at 2^13 samples: meshed once per model, left unchanged"""
    if name not in _meshes:
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, _ = core.grid_axes(bounds, samples=SAMPLES)
        m = eng.generate(f, X, Y, Z, 32, True)
        try:
            soup = m.points().copy().reshape(-1, 3, 3)
            pts, cells = m.weld()
            pts, cells = pts.copy(), cells.copy()
        finally:
            m.close()
        for a in (soup, pts, cells):
            a.setflags(write=False)
        _meshes[name] = (f, bounds, soup, pts, cells)
    return _meshes[name]


def device_mesh(name, ns, eng, records=False):
    f, bounds, soup, pts, cells = meshed(name, ns, eng)
    X, Y, Z, _ = core.grid_axes(bounds, samples=SAMPLES)
    return eng.generate(f, X, Y, Z, 32, True, records=records)


# ---- moments ----
# one lane, a tile less one / whole / plus one, a chunk less one / whole / plus one, two chunks and a bit (two partials), and
# 256 C + 1: 257 partials, a third level of the tree (262,145 triangles)
@pytest.mark.parametrize('n_tris', (0, 1, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 256 * C + 1))
def test_moments_of_adopted_soups_are_bit_identical_to_the_definition(n_tris, eng):
    tris = random_soup(n_tris)
    s = Soup(eng, tris)
    try:
        got = s.mesh.moments()
    finally:
        s.close()
    same_moments(got, ref.moments(tris))
    assert got['triangles'] == n_tris


@pytest.mark.parametrize('name', MODELS)
def test_moments_of_generated_meshes(name, ns, eng):
    f, bounds, soup, pts, cells = meshed(name, ns, eng)
    assert len(soup) > C
    m = device_mesh(name, ns, eng)
    try:
        got = m.moments()
        again = m.moments()
        about = m.moments(origin=(0.25, -0.5, 0.125))
    finally:
        m.close()
    want = ref.moments(soup)
    same_moments(got, want)
    same_moments(again, want)
    same_moments(about, ref.moments(soup, origin=(0.25, -0.5, 0.125)))
    assert (bits(about['sums']) != bits(got['sums'])).any()
    d = ref.derive(got)
    assert d['volume'] > 0 and d['area'] > 0 and np.isfinite(d['inertia']).all()


def test_an_explicit_origin(eng):
    tris = random_soup(3 * C + 17)
    s = Soup(eng, tris)
    try:
        for o in ((0.0, 0.0, 0.0), (100.0, -3.5, 2.0 ** -20)):
            same_moments(s.mesh.moments(origin=o), ref.moments(tris, origin=o))
        with pytest.raises(ValueError, match='3 components'):
            s.mesh.moments(origin=(1.0, 2.0))
    finally:
        s.close()


def test_a_nan_vertex_and_a_zero_area_triangle(eng):
    tris = random_soup(C + 300)
    tris[700, 1, 2] = np.nan
    tris[C + 5, 0, 0] = np.inf
    tris[900, 2] = tris[900, 0]                                  # two equal vertices: no area
    s = Soup(eng, tris)
    try:
        got = s.mesh.moments()
    finally:
        s.close()
    want = ref.moments(tris)
    assert want['nonfinite'] == 2 and want['zero_area'] == 1 and np.isfinite(want['sums']).all()
    same_moments(got, want)
    nothing = Soup(eng, np.full((5, 3, 3), np.nan))              # no finite triangle: an empty box, the origin at 0
    try:
        got = nothing.mesh.moments()
    finally:
        nothing.close()
    same_moments(got, ref.moments(np.full((5, 3, 3), np.nan)))
    assert got['nonfinite'] == 5 and not got['sums'].any() and got['box'][0, 0] == np.inf


def test_a_record_mesh_gives_the_same_bits(ns, eng):
    f, bounds, soup, pts, cells = meshed('ex_example', ns, eng)
    warm = device_mesh('ex_example', ns, eng, records=True)       # (the first call of a model sizes the slab; the second uses it)
    warm.close()
    m = device_mesh('ex_example', ns, eng, records=True)
    try:
        got = m.moments()
        census = m.edge_census()
    finally:
        m.close()
    same_moments(got, ref.moments(soup))
    assert census == ref.edge_census(cells, len(pts))


def test_the_exact_cube_and_its_translation(eng):
    out = []
    for shift in ((0.0, 0.0, 0.0), (1024.0, -512.0, 256.0)):
        tris = ref.cube_soup(shift=shift)
        s = Soup(eng, tris)
        try:
            got = s.mesh.moments()
        finally:
            s.close()
        same_moments(got, ref.moments(tris))
        out.append((got, ref.derive(got)))
    (m0, d0), (m1, d1) = out
    assert d0['volume'] == 1.0 and d0['area'] == 6.0 and np.array_equal(d0['centroid'], [1.0, 1.0, 1.0])
    assert np.array_equal(bits(m0['sums']), bits(m1['sums']))
    assert np.array_equal(d1['centroid'], [1025.0, -511.0, 257.0])


# ---- census ----
def census_of(eng, tris):
    """(device census, the definition's on the device's own weld, sorted keys of the definition)"""
    s = Soup(eng, tris)
    try:
        got = s.mesh.edge_census()
        pts, cells = s.mesh.weld()
        pts, cells = pts.copy(), cells.copy()
    finally:
        s.close()
    return got, ref.edge_census(cells, len(pts)), np.sort(ref.edge_keys(cells)[0])


@pytest.mark.parametrize('name', MODELS)
def test_census_of_generated_meshes(name, ns, eng):
    f, bounds, soup, pts, cells = meshed(name, ns, eng)
    m = device_mesh(name, ns, eng)
    try:
        got = m.edge_census()                                     # welds on its own
        again = m.edge_census()
    finally:
        m.close()
    want = ref.edge_census(cells, len(pts))
    assert got == want and again == want
    assert all(type(got[k]) is type(want[k]) for k in want)


@pytest.mark.parametrize('name', sorted(ref.census_cases()))
def test_census_of_the_constructed_cases(name, eng):
    tris, expected = ref.census_cases()[name]
    got, want, _ = census_of(eng, tris)
    assert got == want
    for k, v in expected.items():
        assert got[k] == v, (name, k, got[k], v)


# k pages around one edge behind n_pad unrelated triangles: the edge's run of sorted keys is [3 n_pad, 3 n_pad + k)
@pytest.mark.parametrize('k,n_pad,boundary', [(k, p, b) for p, b in ((21, 64), (85, 256)) for k in (1, 2, 3, 4, 5)] +
                         [(4, 20, 64), (5, 20, 64), (4, 84, 256), (5, 84, 256)])
def test_books_across_wave_and_workgroup_boundaries(k, n_pad, boundary, eng):
    got, want, keys = census_of(eng, ref.book_soup(k, n_pad))
    und = keys >> np.uint64(1)
    run = np.flatnonzero(und == und[3 * n_pad])
    assert run[0] == 3 * n_pad and len(run) == k
    if 3 * n_pad + k > boundary:
        assert run[0] < boundary <= run[-1]                       # the run straddles the boundary
    else:
        assert run[-1] == boundary - 1                            # ... or ends on a wave's last lane
    assert got == want
    assert got[{1: 'boundary', 2: 'misoriented'}.get(k, 'nonmanifold')] >= 1 and got['nonmanifold'] == (1 if k >= 3 else 0)


def test_a_soup_of_coincident_triangles(eng):
    """one long run per edge: 3 edges, each used 3000 times"""
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    got, want, keys = census_of(eng, np.repeat(tri[None], 3000, axis=0))
    assert got == want
    assert got['nonmanifold'] == 3 and got['edges'] == 3 and got['vertices'] == 3 and got['faces'] == 3000 and not got['closed']


@pytest.mark.parametrize('n_tris', (1, 85, 86))
def test_ragged_key_counts(n_tris, eng):
    """255 and 258 keys: one below and two above a workgroup"""
    got, want, keys = census_of(eng, random_soup(n_tris))
    assert got == want and got['boundary'] == 3 * n_tris and got['vertices'] == 3 * n_tris


# ---- end to end ----
def as_measurement(want):
    return {k: want[k] for k in ('volume', 'area', 'centroid', 'inertia', 'triangles', 'zero_area_triangles', 'nonfinite_triangles',
                                 'vertices', 'faces', 'collapsed', 'edges', 'paired', 'boundary', 'misoriented', 'nonmanifold',
                                 'euler', 'closed', 'oriented', 'origin', 'sums')}


def same_measurement(got, want):
    for k, v in as_measurement(want).items():
        g = getattr(got, k)
        if isinstance(v, np.ndarray) or isinstance(v, float):
            assert np.array_equal(bits(g), bits(v)), (k, g, v)
        else:
            assert g == v and type(g) is type(v), (k, g, v)
    assert np.array_equal(bits(np.array(got.bounds)), bits(want['bounds']))


def test_measure_end_to_end(ns, eng):
    f = fixtures.build('ex_example', ns)
    got = f.measure(samples=SAMPLES, verbose=False)
    pts, cells, _ = f.generate_mesh(samples=SAMPLES, verbose=False)
    want = ref.measure(pts, cells)
    same_measurement(got, want)
    assert got.closed and got.oriented and got.volume > 0 and got.triangles == len(cells)
    again = ns['measure'](f, samples=SAMPLES, verbose=False)
    same_measurement(again, want)
    with pytest.raises(AttributeError):
        got.volume = 1.0                                          # immutable
    with pytest.raises(ValueError):
        got.centroid[0] = 0.0
    about = f.measure(origin=(0.0, 0.0, 0.0), samples=SAMPLES, verbose=False)
    same_measurement(about, ref.measure(pts, cells, origin=(0.0, 0.0, 0.0)))


def test_a_sphere_is_closed_and_oriented(ns):
    got = ns['sphere'](1).measure(samples=SAMPLES, verbose=False)
    assert got.closed and got.oriented and got.euler % 2 == 0 and got.boundary == 0 and got.collapsed == 0
    # a coarse grid decides its own topology and its own volume; the sphere's is 4.19, the mesh lies inside it
    assert 3.0 < got.volume < 4.2 and 9.0 < got.area < 12.6


def test_a_model_with_a_closure(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    got = f.measure(bounds=BOX, samples=SAMPLES, verbose=False)
    pts, cells, _ = f.generate_mesh(bounds=BOX, samples=SAMPLES, verbose=False)
    same_measurement(got, ref.measure(pts, cells))
    assert got.triangles > 256 and got.closed


def test_a_mesh_read_from_an_stl_file(tmp_path, ns):
    f = fixtures.build('ex_example', ns)
    f.save(str(tmp_path / 'a.stl'), samples=SAMPLES, verbose=False)
    mesh = ns['Mesh'].from_stl(str(tmp_path / 'a.stl'))
    got = mesh.measure()
    same_measurement(got, ref.measure(mesh.points, mesh.triangles))
    assert got.triangles == len(mesh.triangles) and got.volume > 0


# ---- refusals and leaks ----
def test_refusals(eng):
    lib = eng.lib
    s = Soup(eng, random_soup(4))
    try:
        census = engine.SdfEdgeCensus()
        mom = engine.SdfMoments()
        assert lib.sdf_mesh_edge_census(s.mesh.handle, ctypes.byref(census)) == 2        # before the weld
        assert b'sdf_mesh_edge_census: call sdf_mesh_weld first' in lib.sdf_last_error()
        assert lib.sdf_mesh_edge_census(None, ctypes.byref(census)) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_edge_census(s.mesh.handle, None) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_moments(None, None, ctypes.byref(mom)) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_moments(s.mesh.handle, None, None) == 2 and b'NULL' in lib.sdf_last_error()
        # ... and the mesh serves the calls that are in order
        assert s.mesh.edge_census()['boundary'] == 12
        same_moments(s.mesh.moments(), ref.moments(s.host.reshape(-1, 3, 3)))
    finally:
        s.close()


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through sdf_mesh_moments and sdf_mesh_edge_census on 400,000 random triangles: each failure carries
    the allocator's message, the free device memory is what it was, and the next call succeeds and matches the definition"""
    lib = eng.lib
    warm = Soup(eng, random_soup(3))                            # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.moments()
        warm.mesh.edge_census()
    finally:
        warm.close()
    tris = random_soup(400000)
    s = Soup(eng, tris)
    try:
        pts, cells = s.mesh.weld()
        want_census = ref.edge_census(cells, len(pts))
        del pts, cells
        eng.synchronize()
        f0 = _free(lib)
        mom, census = engine.SdfMoments(), engine.SdfEdgeCensus()
        for call in (lambda: lib.sdf_mesh_moments(s.mesh.handle, None, ctypes.byref(mom)),
                     lambda: lib.sdf_mesh_edge_census(s.mesh.handle, ctypes.byref(census))):
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
        same_moments(s.mesh.moments(), ref.moments(tris))
        assert s.mesh.edge_census() == want_census and census.boundary == want_census['boundary'] == 1200000
        assert mom.n_triangles == 400000 and _free(lib) == f0
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
