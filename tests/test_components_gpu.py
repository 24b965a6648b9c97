"""The connected shells of a mesh on the device (csrc/sdf_components.hip, `Mesh.components`, `Mesh.select`, sdf_amd/shells.py, `keep=`):
every array compared EXACTLY with the definition (tests/components_ref.py) on the mesh's own weld, the selection bit for bit with the
host subset, end to end, the refusals and the leaks.  Every refusal is decided on the host before a launch; no test repeats a device
call that failed."""
import ctypes
import importlib

import numpy as np
import pytest

import components_ref as ref
import fixtures
import measure_ref
import normals_ref
from sdf_amd import core, engine, stl

shells = importlib.import_module('sdf_amd.shells')
pytestmark = pytest.mark.gpu

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


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


def same_components(got, want, n_vertices):
    """the dict of Mesh.components against the definition's Components: values, shapes and types; and the rounds bound"""
    assert got['count'] == want.count, (got['count'], want.count)
    for k, dt in (('vertex_shell', np.int32), ('triangle_shell', np.int32), ('triangles', np.int64), ('vertices', np.int64)):
        w = getattr(want, k)
        assert got[k].dtype == dt and got[k].shape == w.shape, (k, got[k].dtype, got[k].shape, w.shape)
        bad = got[k] != w
        assert not bad.any(), '%s: %d of %d differ, first at %s: %r != %r' % (k, bad.sum(), bad.size, np.argwhere(bad)[0], got[k][bad][0], w[bad][0])
    assert got['bounds'].dtype == np.float64 and got['bounds'].shape == want.bounds.shape
    assert np.array_equal(bits(got['bounds']), bits(want.bounds)), 'bounds'
    assert 0 <= got['rounds'] <= ref.rounds_bound(n_vertices), (got['rounds'], ref.rounds_bound(n_vertices))
    print('shells %d, vertices %d, rounds %d (bound %d)' % (got['count'], n_vertices, got['rounds'], ref.rounds_bound(n_vertices)))


def check(mesh):
    """components() of a device mesh against the definition on the mesh's OWN weld; returns (got, want, points, cells)"""
    pts, cells = mesh.weld()
    pts, cells = pts.copy(), cells.copy()
    want = ref.components(pts, cells)
    got = mesh.components()
    same_components(got, want, len(pts))
    return got, want, pts, cells


def check_soup(eng, tris):
    s = Soup(eng, tris)
    try:
        return check(s.mesh)
    finally:
        s.close()


# ---- adopted soups: the smallest shapes where each kernel can go wrong ----
def disjoint_triangles(n, seed=3):
    """n triangles that share no vertex, standing in another order than they lie"""
    rng = np.random.RandomState(seed + n)
    tri = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.25], [0.0, 0.5, -0.25]])
    x = rng.permutation(n).astype(np.float64)
    return tri[None] + np.stack([x, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1)[:, None, :]


def strip(n_vertices, closed, seed=7):
    """a triangle strip over n_vertices vertices -- triangles (j, j + 1, j + 2): a path, as graphs go -- whose x positions are a seeded
    permutation, so that the welded order zigzags against the adjacency; the triangles are shuffled; closed: the two triangles
    that make it a ring"""
    rng = np.random.RandomState(seed)
    j = np.arange(n_vertices)
    pos = np.stack([rng.permutation(n_vertices).astype(np.float64), (j % 2).astype(np.float64), np.zeros(n_vertices)], axis=1)
    n_t = n_vertices if closed else n_vertices - 2
    idx = (np.arange(n_t)[:, None] + np.arange(3)[None, :]) % n_vertices
    return pos[idx][rng.permutation(n_t)]


def tetrahedra(n, seed=9):
    rng = np.random.RandomState(seed)
    soup = np.concatenate([ref.tetrahedron(shift=(3.0 * x, rng.uniform(-1, 1), rng.uniform(-1, 1)), scale=rng.uniform(0.5, 1.5))
                           for x in rng.permutation(n)])
    return soup[rng.permutation(len(soup))]


def striped_sheet(n=300, stripes=7):
    """an n x n vertex sheet, two triangles per quad, with the quad columns between the stripes left out"""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    cut = {(n - 1) * s // stripes for s in range(1, stripes)}
    live = ~np.isin(i, sorted(cut))
    i, j = i[live], j[live]
    v = lambda a, b: np.stack([a * 0.01, b * 0.01, np.sin(a * 0.1) * 0.05], axis=-1)
    return np.concatenate([np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1)], axis=1), np.stack([v(i, j), v(i + 1, j + 1), v(i, j + 1)], axis=1)])


@pytest.mark.parametrize('n', (0, 1, 2, 255, 256, 257))
def test_disjoint_triangles(n, eng):
    """K = T: every wave of the count kernels is mixed; 255 / 256 / 257 straddle a workgroup"""
    got, want, pts, cells = check_soup(eng, disjoint_triangles(n))
    assert got['count'] == n and len(pts) == 3 * n and got['bounds'].shape == (n, 2, 3)
    if n == 0:
        assert got['rounds'] == 0 and len(got['vertex_shell']) == 0 and len(got['triangle_shell']) == 0
    else:
        assert (got['triangles'] == 1).all() and (got['vertices'] == 3).all() and sorted(got['triangle_shell'].tolist()) == list(range(n))


def test_coincident_triangles(eng):
    """3000 times one triangle: one shell, three vertices, every lane at the same three words"""
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    got, want, pts, cells = check_soup(eng, np.repeat(tri[None], 3000, axis=0))
    assert got['count'] == 1 and got['triangles'].tolist() == [3000] and got['vertices'].tolist() == [3]


@pytest.mark.parametrize('closed', (False, True))
def test_a_long_strip_is_one_shell_within_the_rounds_bound(closed, eng):
    """2^16 + 1 vertices in a path (or a ring): one hop per round would need 2^16 rounds; the bound is 19"""
    n = 2 ** 16 + 1
    got, want, pts, cells = check_soup(eng, strip(n, closed))
    assert len(pts) == n and got['count'] == 1 and got['vertices'].tolist() == [n]
    assert got['triangles'].tolist() == [n if closed else n - 2]
    assert 1 <= got['rounds'] <= ref.rounds_bound(n) == 19


def test_a_thousand_tetrahedra(eng):
    got, want, pts, cells = check_soup(eng, tetrahedra(1000))
    assert got['count'] == 1000 and (got['triangles'] == 4).all() and (got['vertices'] == 4).all()


def test_a_sheet_cut_into_stripes(eng):
    """90,000 vertices: many workgroups, K = 7, long runs of one shell in the count kernels"""
    soup = striped_sheet()
    got, want, pts, cells = check_soup(eng, soup)
    assert len(pts) == 90000 and got['count'] == 7 and got['vertices'].sum() == 90000 and got['triangles'].sum() == len(soup)
    assert (np.diff(got['vertex_shell']) >= 0).all()              # the stripes lie along x: so do their numbers


def test_shells_that_touch_in_one_vertex_are_one(eng):
    got, want, pts, cells = check_soup(eng, np.concatenate([ref.tetrahedron(), ref.tetrahedron(shift=(1.0, 0.0, 0.0))]))
    assert got['count'] == 1 and got['vertices'].tolist() == [7] and got['triangles'].tolist() == [8]


def test_a_collapsed_cell_is_a_bridge(eng):
    soup = ref.collapsed_bridge()
    got, want, pts, cells = check_soup(eng, soup)
    assert got['count'] == 1 and got['triangles'].tolist() == [3]
    got, want, pts, cells = check_soup(eng, soup[:2])
    assert got['count'] == 2


# ---- generated models ----
def model(name, ns):
    if name == 'three_spheres':
        return ns['sphere'](0.5).translate((-2, 0, 0)) | ns['sphere'](0.7) | ns['sphere'](0.4).translate((2, 0, 0))
    if name == 'hollow_sphere':
        return ns['sphere'](1) - ns['sphere'](0.5)
    return fixtures.build(name, ns)


def device_mesh(name, samples, ns, eng, records=False):
    key = (name, samples)
    if key not in _cache:
        f = model(name, ns)
        bounds = eng.estimate_bounds(f)
        _cache[key] = (f, core.grid_axes(bounds, samples=samples)[:3])
    f, (X, Y, Z) = _cache[key]
    return f, eng.generate(f, X, Y, Z, 32, True, records=records)


@pytest.mark.parametrize('samples', (2 ** 13, 2 ** 15))
@pytest.mark.parametrize('name', ('three_spheres', 'hollow_sphere', 'ex_example', 'ex_gearlike', 'ex_knurling'))
def test_generated_models(name, samples, ns, eng):
    f, m = device_mesh(name, samples, ns, eng)
    try:
        got, want, pts, cells = check(m)
        again = m.components()                                    # a second call returns the same arrays
    finally:
        m.close()
    assert got['count'] >= 1 and got['triangles'].sum() == len(cells) and got['vertices'].sum() == len(pts)
    for k in got:
        assert np.array_equal(again[k], got[k]), k
    if name == 'three_spheres':
        assert got['count'] == 3 and got['triangles'][1] == got['triangles'].max()      # numbered along x: the large one in the middle
    if name == 'hollow_sphere':
        assert got['count'] == 2 and got['triangles'][0] > got['triangles'][1]           # the outer shell holds the smallest vertex
    warm = device_mesh(name, samples, ns, eng, records=True)[1]   # (the first record call of a model sizes the slab)
    warm.close()
    f, r = device_mesh(name, samples, ns, eng, records=True)
    try:
        rec = r.components()
    finally:
        r.close()
    same_components(rec, want, len(pts))


# ---- selection ----
def masks_of(k):
    single = [np.arange(k) == i for i in range(k)]
    return single + [np.arange(k) < 2] + ([np.arange(k) != 1] if k > 2 else [])


@pytest.mark.parametrize('name', ('hollow_sphere', 'three_spheres'))
def test_selection_is_the_host_subset_bit_for_bit(name, ns, eng):
    f, m = device_mesh(name, 2 ** 13, ns, eng)
    try:
        soup = m.points().copy().reshape(-1, 3, 3)
        c = m.components()
        ts, k = c['triangle_shell'], c['count']
        for mask in masks_of(k):
            sub = soup[mask[ts]]
            sel = m.select(mask)
            try:
                assert sel.n_triangles == len(sub) == c['triangles'][mask].sum()
                assert np.array_equal(bits(sel.points()), bits(sub.reshape(-1, 3)))
                assert np.array_equal(sel.stl_records(), stl.stl_records(sub.reshape(-1, 3)).view(np.uint8).reshape(-1))
                got, want = sel.moments(), measure_ref.moments(sub)
                for key in ('sums', 'origin', 'box'):
                    assert np.array_equal(bits(got[key]), bits(want[key])), key
                g, w, pts, cells = check(sel)
                assert g['count'] == mask.sum()
                wp, wc = ref.weld(sub)
                assert np.array_equal(pts, wp) and np.array_equal(cells, wc)
                assert sel.edge_census() == measure_ref.edge_census(cells, len(pts))
            finally:
                sel.close()
        none = m.select(np.zeros(k, bool))                        # nothing kept: a mesh of 0 triangles that every reader takes
        try:
            assert none.n_triangles == 0 and none.points().shape == (0, 3) and none.components()['count'] == 0
            assert len(none.stl_records()) == 0 and none.moments()['triangles'] == 0
        finally:
            none.close()
        for bad in (np.ones(k + 1, bool), np.ones(k - 1, bool), np.ones(0, bool)):
            with pytest.raises(ValueError, match='shells'):
                m.select(bad)
        assert np.array_equal(bits(m.points()), bits(soup.reshape(-1, 3)))      # the source is what it was
        same_components(m.components(), ref.components(*m.weld()), len(c['vertex_shell']))
    finally:
        m.close()


def test_selection_of_an_adopted_soup_and_of_a_record_mesh(ns, eng):
    tris = tetrahedra(50)
    s = Soup(eng, tris)
    try:
        c = s.mesh.components()
        mask = np.arange(50) % 3 == 0
        sel = s.mesh.select(mask)
        try:
            assert np.array_equal(bits(sel.points()), bits(tris[mask[c['triangle_shell']]].reshape(-1, 3)))
            assert check(sel)[0]['count'] == mask.sum()
        finally:
            sel.close()
    finally:
        s.close()
    warm = device_mesh('hollow_sphere', 2 ** 13, ns, eng, records=True)[1]
    warm.close()
    f, r = device_mesh('hollow_sphere', 2 ** 13, ns, eng, records=True)
    try:
        c = r.components()
        sel = r.select([False, True])
        try:
            soup = r.points().reshape(-1, 3, 3)
            assert np.array_equal(bits(sel.points()), bits(soup[c['triangle_shell'] == 1].reshape(-1, 3)))
        finally:
            sel.close()
    finally:
        r.close()


@pytest.mark.parametrize('n', (1, 256, 257))
def test_selection_pins_the_last_triangle(n, eng):
    """the count of a selection is the last triangle's position + its flag: with only the shell of the LAST soup triangle kept the
    sum ends on flag 1 over position 0, with every shell but that one on flag 0 over position n - 1; 256 / 257: the last triangle
    is the last lane of a workgroup / alone in the next one"""
    tris = disjoint_triangles(n)
    s = Soup(eng, tris)
    try:
        ts = s.mesh.components()['triangle_shell']
        only_last = np.arange(n) == ts[-1]
        for mask in (only_last, ~only_last):
            sub = tris[mask[ts]]
            assert len(sub) == (1 if mask is only_last else n - 1)
            sel = s.mesh.select(mask)
            try:
                assert sel.n_triangles == len(sub)
                assert sel.points().shape == (3 * len(sub), 3) and np.array_equal(bits(sel.points()), bits(sub.reshape(-1, 3)))
            finally:
                sel.close()
    finally:
        s.close()


def test_refusals(eng):
    lib = eng.lib
    s = Soup(eng, tetrahedra(3))
    try:
        out, h = engine.SdfComponents(), ctypes.c_void_p()
        keep = (ctypes.c_uint8 * 3)(1, 0, 1)
        assert lib.sdf_mesh_components(None, ctypes.byref(out)) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_components(s.mesh.handle, None) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_components_fetch(s.mesh.handle, None, None, None, None, None) == 2          # before the labelling
        assert b'call sdf_mesh_components first' in lib.sdf_last_error()
        assert lib.sdf_mesh_select_shells(s.mesh.handle, keep, 3, ctypes.byref(h)) == 2 and b'call sdf_mesh_components first' in lib.sdf_last_error()
        assert s.mesh.components()['count'] == 3
        assert lib.sdf_mesh_select_shells(s.mesh.handle, keep, 2, ctypes.byref(h)) == 2 and h.value is None
        assert lib.sdf_mesh_select_shells(s.mesh.handle, None, 3, ctypes.byref(h)) == 2 and b'NULL' in lib.sdf_last_error()
        assert lib.sdf_mesh_components_fetch(s.mesh.handle, None, None, None, None, None) == 0              # any pointer may be NULL
        sel = s.mesh.select([True, False, True])
        try:
            assert sel.n_triangles == 8
        finally:
            sel.close()
    finally:
        s.close()


# ---- end to end ----
SAMPLES = 2 ** 13


def as_fields(m):
    return [(k, bits(v).tolist() if isinstance(v, (np.ndarray, float)) else v) for k, v in m._asdict().items() if k != 'bounds'] + \
        [('bounds', bits(np.array(m.bounds)).tolist())]


def test_measure_shells_of_a_hollow_sphere(ns, eng):
    f = model('hollow_sphere', ns)
    got = f.measure_shells(samples=SAMPLES, verbose=False)
    assert len(got) == 2 and got[0].triangles > got[1].triangles
    outer, inner = got
    assert outer.volume > 0 and inner.volume < 0 and outer.closed and inner.closed and outer.oriented and inner.oriented
    whole = f.measure(samples=SAMPLES, verbose=False)
    # two summation orders of the same terms (about two origins): 1e-12 relative
    assert abs((outer.volume + inner.volume) - whole.volume) <= 1e-12 * abs(whole.volume), (outer.volume, inner.volume, whole.volume)
    assert outer.triangles + inner.triangles == whole.triangles
    assert len(ns['measure_shells'](f, limit=1, samples=SAMPLES, verbose=False)) == 1
    first = f.measure(keep='largest', samples=SAMPLES, verbose=False)
    assert as_fields(first) == as_fields(outer)
    sh = f.shells(samples=SAMPLES, verbose=False)
    assert isinstance(sh, shells.Shells) and sh.count == 2 and sh.triangles.tolist() == [outer.triangles, inner.triangles]
    assert not sh.triangles.flags.writeable and sh.rounds >= 1
    assert ns['shells'](f, samples=SAMPLES).count == 2


def test_save_and_generate_mesh_with_keep(tmp_path, ns, eng):
    f = model('three_spheres', ns)
    soup = f.generate(samples=SAMPLES, verbose=False).reshape(-1, 3, 3)
    sh = f.shells(samples=SAMPLES)
    assert sh.count == 3 and len(sh.triangle_shell) == len(soup)
    largest = soup[sh.triangle_shell == 1]
    f.save(tmp_path / 'a.stl', keep='largest', samples=SAMPLES, verbose=False)
    stl.write_binary_stl(str(tmp_path / 'want.stl'), largest.reshape(-1, 3))
    assert open(tmp_path / 'a.stl', 'rb').read() == open(tmp_path / 'want.stl', 'rb').read()
    wp, wc = ref.weld(largest)
    f.save(str(tmp_path / 'a.ply'), keep=1, writer='native', samples=SAMPLES, verbose=False)
    p, nn, c, head = normals_ref.parse_ply(str(tmp_path / 'a.ply'))
    assert nn is None and head == normals_ref.ply_header(len(wp), len(wc), False)
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32)) and np.array_equal(c, wc)
    pts, cells, n = f.generate_mesh(keep='largest', normals=True, samples=SAMPLES, verbose=False)
    assert np.array_equal(pts, wp) and np.array_equal(cells, wc) and n.shape == pts.shape
    bounds = eng.estimate_bounds(f)
    lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
    eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    want_n = normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), wp, eps)[0]
    assert np.array_equal(bits(n), bits(want_n))
    # two shells by a mask and by a callable
    two = soup[np.isin(sh.triangle_shell, (0, 2))]
    pts, cells, n = f.generate_mesh(keep=[True, False, True], samples=SAMPLES, verbose=False)
    assert np.array_equal(pts, ref.weld(two)[0]) and np.array_equal(cells, ref.weld(two)[1]) and n is None
    seen = []
    pts2, cells2, _ = f.generate_mesh(keep=lambda s: seen.append(s) or s.triangles < s.triangles.max(), samples=SAMPLES, verbose=False)
    assert np.array_equal(pts2, pts) and np.array_equal(cells2, cells) and isinstance(seen[0], shells.Shells)
    with pytest.raises(ValueError, match='keep'):
        f.generate_mesh(keep=[True, False], samples=SAMPLES, verbose=False)
    # keep=None is the call without the argument
    f.save(str(tmp_path / 'n.stl'), keep=None, samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 'm.stl'), samples=SAMPLES, verbose=False)
    assert open(tmp_path / 'n.stl', 'rb').read() == open(tmp_path / 'm.stl', 'rb').read()


def test_keep_none_makes_no_new_calls(tmp_path, monkeypatch, ns, eng):
    called = []
    for name in ('components', 'select', 'shell_summary'):
        monkeypatch.setattr(engine.Mesh, name, lambda self, *a, _n=name: called.append(_n))
    f = model('hollow_sphere', ns)
    f.save(str(tmp_path / 'a.stl'), samples=SAMPLES, verbose=False)
    f.generate_mesh(samples=SAMPLES, verbose=False)
    f.measure(samples=SAMPLES, verbose=False)
    assert called == []


def test_a_mesh_read_from_an_stl_file(tmp_path, ns):
    f = model('hollow_sphere', ns)
    f.save(str(tmp_path / 'a.stl'), samples=SAMPLES, verbose=False)
    mesh = ns['Mesh'].from_stl(str(tmp_path / 'a.stl'))
    got = mesh.shells()
    soup = np.asarray(mesh.points)[np.asarray(mesh.triangles)]
    want = ref.components(*ref.weld(soup))
    assert got.count == want.count == 2 and np.array_equal(got.triangle_shell, want.triangle_shell)
    assert np.array_equal(got.triangles, want.triangles) and np.array_equal(bits(got.bounds), bits(want.bounds))


# ---- leaks ----
def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through sdf_mesh_components (the scratch, then the block the mesh keeps) and sdf_mesh_select_shells
    (the scratch, then the selection's soup) on 500,000 tetrahedra -- 2,000,000 triangles, 500,000 shells, every block at least 16 MiB, welded beforehand (the weld's
    own blocks are walked by test_alloc_hook_gpu.py): each failure carries the allocator's message and the free device memory is
    what it was, the first call that gets through matches the definition, and closing the meshes returns the rest.  The hook injects
    a host-side allocation error: nothing faults."""
    lib = eng.lib
    warm = Soup(eng, tetrahedra(3))                             # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.components()
        warm.mesh.select([True, False, True]).close()
    finally:
        warm.close()
    n = 500000
    rng = np.random.RandomState(1)
    tris = (ref.tetrahedron()[None] + np.stack([3.0 * rng.permutation(n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1)[:, None, None, :]).reshape(-1, 3, 3)
    s = Soup(eng, tris)
    try:
        eng.trim()
        eng.synchronize()
        f00 = _free(lib)
        want = ref.components(*s.mesh.weld())
        eng.synchronize()
        f0 = _free(lib)
        out = engine.SdfComponents()
        failures, rc = 0, -1
        for nth in range(1, 5):
            lib.sdf_test_fail_alloc(nth)
            rc = lib.sdf_mesh_components(s.mesh.handle, ctypes.byref(out))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error(), (rc, lib.sdf_last_error())
            assert _free(lib) == f0, (nth, f0, _free(lib))
            assert lib.sdf_mesh_components_fetch(s.mesh.handle, None, None, None, None, None) == 2        # no labelling was left behind
        assert rc == 0 and failures == 2 and out.n_shells == n and out.n_triangles == 4 * n, (rc, failures, out.n_shells)
        c = s.mesh.components()
        assert c['count'] == n and (c['triangles'] == 4).all() and (c['vertices'] == 4).all()
        assert np.array_equal(c['triangle_shell'], want.triangle_shell) and np.array_equal(c['vertex_shell'], want.vertex_shell)
        eng.synchronize()
        f1 = _free(lib)
        mask = np.ascontiguousarray(np.arange(n) % 2 == 0, dtype=np.uint8)
        h = ctypes.c_void_p()
        failures, rc = 0, -1
        for nth in range(1, 5):
            lib.sdf_test_fail_alloc(nth)
            rc = lib.sdf_mesh_select_shells(s.mesh.handle, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, ctypes.byref(h))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error() and h.value is None, (rc, lib.sdf_last_error())
            assert _free(lib) == f1, (nth, f1, _free(lib))
        assert rc == 0 and failures == 2, (rc, failures)
        sel = engine.Mesh(eng, h)
        try:
            assert sel.n_triangles == 2 * n
            assert np.array_equal(bits(sel.points()), bits(tris[mask[c['triangle_shell']] != 0].reshape(-1, 3)))
            held = f1 - _free(lib)                                # the selection's soup, 72 B per triangle, and nothing else
            assert 72 * 2 * n <= held <= 72 * 2 * n + (8 << 20), held
        finally:
            sel.close()
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
    eng.trim()
    eng.synchronize()
    assert _free(lib) >= f00
