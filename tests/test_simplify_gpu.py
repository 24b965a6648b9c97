"""A mesh simplified on the device (csrc/sdf_simplify.hip, `engine.Mesh.simplify`, sdf_amd/simplify.py, `simplify=`): every soup
compared EXACTLY, as int64 bit patterns, with the definition (tests/simplify_ref.py) applied to the mesh's own weld, the statistics
as integers; end to end; the refusals and the leaks.  Every refusal is decided on the host or before any output exists; no test
repeats a device call that failed."""
import ctypes
import os

import numpy as np
import pytest

import components_ref
import measure_ref
import normals_ref
import simplify_ref as ref
import test_simplify_host as host
from sdf_amd import core, engine, simplify
from sdf_amd.shells import resolve_keep

pytestmark = pytest.mark.gpu

SAMPLES = 2 ** 18
BOUNDS = ((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85))
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


def same(small, want):
    """a simplified device mesh against the definition's Simplified: the soup bit for bit, the statistics as integers"""
    got = small.points()
    assert small.n_triangles == len(want.soup) and got.shape == (3 * len(want.soup), 3) and got.dtype == np.float64
    bad = bits(got) != bits(want.soup.reshape(-1, 3))
    assert not bad.any(), '%d of %d doubles differ, first at %s' % (bad.sum(), bad.size, np.argwhere(bad)[0])
    st = small.simplify_stats
    assert {k: st[k] for k in ref.STAT_KEYS} == want.stats and all(isinstance(st[k], int) for k in ref.STAT_KEYS)
    assert st['kernel_ms'] >= 0.0


def check(mesh, origin, cell, reg=1e-3):
    """mesh.simplify against the definition on the mesh's OWN weld; returns the definition's Simplified"""
    pts, cells = mesh.weld()
    want = ref.simplify(pts.copy(), cells.copy(), origin, cell, reg)
    small = mesh.simplify(origin, cell, reg)
    try:
        same(small, want)
    finally:
        small.close()
    print('triangles %d -> %d, clusters %d, mean_fallback %d, flat %d' % (len(cells), len(want.soup), want.stats['clusters'],
                                                                        want.stats['mean_fallback'], want.stats['flat']))
    return want


def check_soup(eng, tris, origin, cell, reg=1e-3):
    s = Soup(eng, tris)
    try:
        return check(s.mesh, origin, cell, reg)
    finally:
        s.close()


# ---- adopted soups: the smallest shapes where each kernel can go wrong ----
def apart(n, seed=5):
    """n triangles that share no vertex, 4 apart along x in shuffled order, each within [0.2, 1.8]^3 of its place with its corners in
    three cells of edge 1"""
    rng = np.random.RandomState(seed + n)
    tri = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    jitter = rng.uniform(-0.3, 0.3, (n, 3, 3))
    return tri[None] + jitter + np.stack([4.0 * rng.permutation(n), np.zeros(n), np.zeros(n)], axis=1)[:, None, :]


@pytest.mark.parametrize('n', (0, 1, 2, 255, 256, 257))
def test_disjoint_triangles_each_over_three_cells(n, eng):
    """T at a workgroup edge (K = 3 T: 768 is one too); every triangle survives"""
    want = check_soup(eng, apart(n), np.zeros(3), np.ones(3))
    assert want.stats['triangles_out'] == n and want.stats['clusters'] == 3 * n and want.stats['collapsed'] == 0


@pytest.mark.parametrize('n', (1, 255, 256, 257))
def test_disjoint_triangles_each_inside_one_cell(n, eng):
    """K = T at a workgroup edge; nothing survives, and nothing is emitted"""
    want = check_soup(eng, apart(n), np.zeros(3), np.full(3, 4.0))
    assert want.stats['triangles_out'] == 0 and want.stats['clusters'] == n and want.stats['collapsed'] == n


def wavy_sheet(n):
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    v = lambda a, b: np.stack([a * 1.0, b * 1.0, np.sin(a * 0.3) * 0.5 + np.cos(b * 0.2) * 0.4], axis=-1)
    return np.concatenate([np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1)], axis=1), np.stack([v(i, j), v(i + 1, j + 1), v(i, j + 1)], axis=1)])


@pytest.mark.parametrize('cx, cy', ((1, 1), (2, 2), (9, 7), (8, 8), (13, 5)))
def test_a_sheet_in_clusters_of_1_4_63_64_65_vertices(cx, cy, eng):
    n = 66
    want = check_soup(eng, wavy_sheet(n), np.array([-0.5, -0.5, -5.0]), np.array([float(cx), float(cy), 10.0]))
    assert np.bincount(want.vertex_cluster).max() == cx * cy and want.stats['clusters'] == (-(-n // cx)) * (-(-n // cy))


def test_a_fan_of_a_thousand_triangles(eng):
    """one cluster with 1000 items, its neighbours single-vertex clusters"""
    n = 1000
    a = 2 * np.pi * np.arange(n) / n
    rim = np.stack([50 * np.cos(a), 50 * np.sin(a), 3 * np.sin(7 * a)], axis=1)
    hub = np.array([0.01, 0.02, 0.03])
    soup = np.stack([np.broadcast_to(hub, (n, 3)), rim, np.roll(rim, -1, axis=0)], axis=1)
    want = check_soup(eng, soup, np.array([-0.05, -0.05, -0.05]), np.full(3, 0.1))
    counts = np.bincount(want.vertex_cluster)
    assert want.stats['clusters'] == n + 1 and counts.max() == 1 and want.stats['triangles_out'] == n


def test_soup_order_shuffled_against_welded_order(eng):
    rng = np.random.RandomState(7)
    n = 3000
    j = np.arange(n)
    pos = np.stack([rng.permutation(n).astype(np.float64), (j % 2).astype(np.float64), np.sin(j * 0.01)], axis=1)
    idx = (np.arange(n)[:, None] + np.arange(3)[None, :]) % n
    want = check_soup(eng, pos[idx][rng.permutation(n)], np.array([-0.3, -0.2, -1.5]), np.array([40.0, 0.7, 1.0]))
    assert 0 < want.stats['triangles_out'] < n


@pytest.mark.parametrize('name', host.CASES)
def test_constructed_numeric_cases(name, eng):
    soup, origin, cell = host.case(name)
    want = check_soup(eng, soup, origin, cell)
    expect = {'planar': (0, 0), 'zero_area': (1, 0), 'two_planes_meet_outside': (0, 1), 'two_planes_meet_inside': (0, 0)}
    if name in expect:
        assert (want.stats['flat'], want.stats['mean_fallback']) == expect[name]
    if name == 'cell_faces':
        assert np.signbit(soup).any()
    if name == 'straddles_the_origin':
        assert want.stats['clusters'] == 12
    if name.endswith('_across_cells'):                            # the representatives of such clusters are in the soup that was compared
        assert want.stats['triangles_out'] > 0
        assert {'planar': want.stats['flat'] + want.stats['mean_fallback'] == 0, 'zero_area': want.stats['flat'] == 4,
                'two_planes': want.stats['mean_fallback'] > 0}[name[:-len('_across_cells')]]


def test_no_triangles_no_launch(eng):
    s = Soup(eng, np.zeros((0, 3, 3)))
    try:
        small = s.mesh.simplify(np.zeros(3), np.ones(3))
        try:
            assert small.n_triangles == 0 and small.points().shape == (0, 3) and len(small.stl_records()) == 0
            assert {k: small.simplify_stats[k] for k in ref.STAT_KEYS} == dict.fromkeys(ref.STAT_KEYS, 0)
        finally:
            small.close()
    finally:
        s.close()


# ---- end to end on the example ----
def example(ns):
    return host.example(ns)


def grid():
    if 'grid' not in _cache:
        _cache['grid'] = core.grid_axes(BOUNDS, samples=SAMPLES)
    return _cache['grid']


def full_weld(ns):
    """generate_mesh() of the example without simplify: the weld every end-to-end case starts from (taken once, left unchanged)"""
    if 'weld' not in _cache:
        pts, cells, _ = example(ns).generate_mesh(bounds=BOUNDS, samples=SAMPLES, verbose=False)
        pts, cells = np.array(pts), np.array(cells)
        pts.setflags(write=False); cells.setflags(write=False)
        _cache['weld'] = (pts, cells)
    return _cache['weld']


def wanted(ns, k):
    if ('want', k) not in _cache:
        X, Y, Z, step = grid()
        pts, cells = full_weld(ns)
        want = ref.simplify(pts, cells, *simplify.resolve_cell(k, X, Y, Z, step))
        _cache['want', k] = (want,) + ref.weld(want.soup)
    return _cache['want', k]


@pytest.mark.parametrize('k', (2, 4))
def test_generate_mesh_with_simplify(k, ns, eng):
    f = example(ns)
    want, wp, wc = wanted(ns, k)
    pts, cells, n = f.generate_mesh(simplify=k, bounds=BOUNDS, samples=SAMPLES, verbose=False)
    assert n is None and np.array_equal(pts, wp) and np.array_equal(cells, wc)
    assert len(cells) == {2: 10844, 4: 3102}[k]
    st = core.generate_mesh.last_simplify
    assert {key: st[key] for key in ref.STAT_KEYS} == want.stats
    f.generate_mesh(bounds=BOUNDS, samples=2 ** 12, verbose=False)
    assert core.generate_mesh.last_simplify is None


def test_save_and_measure_with_simplify(tmp_path, ns, eng):
    f = example(ns)
    want, wp, wc = wanted(ns, 4)
    kw = dict(bounds=BOUNDS, samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 'a.stl'), simplify=4, **kw)
    data = open(tmp_path / 'a.stl', 'rb').read()
    assert len(data) == 84 + 50 * 3102 and int(np.frombuffer(data, '<u4', 1, 80)[0]) == 3102
    f.save(str(tmp_path / 'a.ply'), simplify=4, normals=True, **kw)
    p, nn, c, head = normals_ref.parse_ply(str(tmp_path / 'a.ply'))
    assert head == normals_ref.ply_header(len(wp), len(wc), True) and np.array_equal(c, wc)
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32))
    lo, hi = np.asarray(BOUNDS[0]), np.asarray(BOUNDS[1])
    eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    want_n = normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), wp, eps)[0]
    assert np.array_equal(nn.view(np.int32), want_n.astype(np.float32).view(np.int32))
    pts, cells, n = f.generate_mesh(simplify=4, normals=True, **kw)
    assert np.array_equal(pts, wp) and np.array_equal(bits(n), bits(want_n))
    m = f.measure(simplify=4, **kw)
    assert m.closed and m.oriented and m.triangles == 3102 and m.faces == 3102 and m.collapsed == 0
    v = measure_ref.derive(measure_ref.moments(want.soup))['volume']
    assert abs(m.volume - v) <= 1e-12 * abs(v)                    # (two origins, two summation orders)
    assert f.shells(simplify=4, **{k: v for k, v in kw.items() if k != 'verbose'}).triangles.sum() == 3102
    assert sum(s.triangles for s in f.measure_shells(simplify=4, **{k: v for k, v in kw.items() if k != 'verbose'})) == 3102


def test_the_closing_line_counts_what_is_yielded(capsys, ns, eng):
    example(ns).generate_mesh(simplify=4, bounds=BOUNDS, samples=SAMPLES)
    assert '\n3102 triangles in ' in capsys.readouterr().out


def test_keep_then_simplify_is_simplify_after_select(ns, eng):
    f = example(ns) | ns['sphere'](0.1).translate((0.7, 0.7, 0.7))          # a crumb of its own beside the example
    X, Y, Z, step = grid()
    origin, cell = simplify.resolve_cell(4, X, Y, Z, step)
    mesh = eng.generate(f, X, Y, Z, 32, True)
    try:
        counts = mesh.shell_summary()['triangles']
        assert len(counts) == 2
        sel = mesh.select(resolve_keep('largest', counts))
        try:
            pts, cells = sel.weld()
            want = ref.simplify(pts.copy(), cells.copy(), origin, cell)
            small = sel.simplify(origin, cell)
            try:
                same(small, want)                                 # a selection simplifies to the definition
                by_hand = [np.array(a) for a in small.weld()]
            finally:
                small.close()
        finally:
            sel.close()
    finally:
        mesh.close()
    pts, cells, _ = f.generate_mesh(keep='largest', simplify=4, bounds=BOUNDS, samples=SAMPLES, verbose=False)
    assert np.array_equal(pts, by_hand[0]) and np.array_equal(cells, by_hand[1]) and len(cells) == want.stats['triangles_out']
    whole = f.generate_mesh(simplify=4, bounds=BOUNDS, samples=SAMPLES, verbose=False)[1]
    assert len(whole) > len(cells)


@pytest.mark.parametrize('how', ('chunked', 'records'))
def test_other_kinds_of_mesh_simplify_to_the_definition(how, ns, eng):
    f = example(ns)
    X, Y, Z, step = grid()
    origin, cell = simplify.resolve_cell(4, X, Y, Z, step)
    if how == 'records':
        eng.generate(f, X, Y, Z, 32, True, records=True).close()  # (the first record call of a model sizes the slab)
    mesh = eng.generate(f, X, Y, Z, 64, True) if how == 'chunked' else eng.generate(f, X, Y, Z, 32, True, records=True)
    try:
        want = check(mesh, origin, cell)
        assert want.stats['triangles_out'] == 3102
    finally:
        mesh.close()


def test_a_mesh_read_from_an_stl_file(tmp_path, ns, eng):
    f = example(ns)
    f.save(str(tmp_path / 'a.stl'), bounds=BOUNDS, samples=2 ** 15, verbose=False)
    mesh = ns['Mesh'].from_stl(str(tmp_path / 'a.stl'))
    small = mesh.simplify(0.2)
    soup = np.asarray(mesh.points, dtype=np.float64)[np.asarray(mesh.triangles)]
    pts, cells = ref.weld(soup)
    want = ref.simplify(pts, cells, pts.min(axis=0), np.full(3, 0.2))
    wp, wc = ref.weld(want.soup)
    assert isinstance(small, ns['Mesh']) and np.array_equal(small.points, wp) and np.array_equal(small.triangles, wc)
    other = mesh.simplify((0.2, 0.3, 0.25), origin=(-1.0, -1.0, -1.0), reg=1e-2)
    want = ref.simplify(pts, cells, np.full(3, -1.0), np.array([0.2, 0.3, 0.25]), 1e-2)
    assert np.array_equal(other.points, ref.weld(want.soup)[0])


# ---- stability ----
def test_simplify_none_is_the_call_without_the_keyword(tmp_path, monkeypatch, ns, eng):
    f = example(ns)
    kw = dict(bounds=BOUNDS, samples=2 ** 15, verbose=False)
    called = []
    real = engine.Mesh.simplify
    monkeypatch.setattr(engine.Mesh, 'simplify', lambda self, *a, **k: called.append(1) or real(self, *a, **k))
    for ext in ('stl', 'ply'):
        f.save(str(tmp_path / ('n.' + ext)), simplify=None, **kw)
        f.save(str(tmp_path / ('m.' + ext)), **kw)
        assert open(tmp_path / ('n.' + ext), 'rb').read() == open(tmp_path / ('m.' + ext), 'rb').read()
    a, b = f.generate_mesh(simplify=None, **kw), f.generate_mesh(**kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    f.measure(**kw)
    assert called == []
    f.save(str(tmp_path / 's.stl'), simplify=2, **kw)
    assert called == [1] and os.path.getsize(tmp_path / 's.stl') < os.path.getsize(tmp_path / 'm.stl') / 3


def test_simplifying_twice_gives_identical_bits(ns, eng):
    X, Y, Z, step = grid()
    origin, cell = simplify.resolve_cell(2, X, Y, Z, step)
    mesh = eng.generate(example(ns), X, Y, Z, 32, True)
    try:
        before = mesh.points().copy()
        a = mesh.simplify(origin, cell)
        b = mesh.simplify(origin, cell)
        try:
            assert a.n_triangles == 10844 and np.array_equal(bits(a.points()), bits(b.points()))
            sa, sb = dict(a.simplify_stats, kernel_ms=0), dict(b.simplify_stats, kernel_ms=0)
            assert sa == sb
        finally:
            a.close()
            b.close()
        assert np.array_equal(bits(mesh.points()), bits(before))  # the source is what it was
    finally:
        mesh.close()


# ---- refusals and leaks ----
def test_refusals(eng):
    lib = eng.lib
    tris = components_ref.tetrahedron()
    s = Soup(eng, tris)
    try:
        o, c = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
        h, st = ctypes.c_void_p(), engine.SdfSimplifyStats()
        for args in ((None, o, c, 1e-3, ctypes.byref(h), ctypes.byref(st)), (s.mesh.handle, None, c, 1e-3, ctypes.byref(h), ctypes.byref(st)),
                     (s.mesh.handle, o, None, 1e-3, ctypes.byref(h), ctypes.byref(st)), (s.mesh.handle, o, c, 1e-3, None, ctypes.byref(st)),
                     (s.mesh.handle, o, c, 1e-3, ctypes.byref(h), None)):
            assert lib.sdf_mesh_simplify(*args) == 2 and b'NULL' in lib.sdf_last_error()
        for cell in (0.0, -1.0, np.inf, np.nan, (1.0, 0.0, 1.0)):
            with pytest.raises(ValueError, match='cell'):
                s.mesh.simplify(np.zeros(3), np.broadcast_to(cell, (3,)))
        for origin in ((np.nan, 0.0, 0.0), (0.0, 0.0, np.inf)):
            with pytest.raises(ValueError, match='origin'):
                s.mesh.simplify(origin, np.ones(3))
        for reg in (-1.0, np.nan, np.inf):
            with pytest.raises(ValueError, match='reg'):
                s.mesh.simplify(np.zeros(3), np.ones(3), reg)
        with pytest.raises(ValueError, match='3 components'):
            s.mesh.simplify(np.zeros(2), np.ones(3))
        assert h.value is None
        with pytest.raises(engine.SdfHipError, match='span'):     # found after the first pass, before any output
            s.mesh.simplify(np.zeros(3), np.full(3, 2.0 ** -21))
        check(s.mesh, np.zeros(3), np.full(3, 2.0 ** -20))
    finally:
        s.close()


@pytest.mark.parametrize('bad', (np.nan, np.inf))
def test_a_vertex_that_is_not_finite(bad, eng):
    tris = np.concatenate([components_ref.tetrahedron(), components_ref.tetrahedron(shift=(3.0, 0.0, 0.0))])
    tris[5, 1, 2] = bad
    s = Soup(eng, tris)
    try:
        with pytest.raises(engine.SdfHipError, match='not finite'):
            s.mesh.simplify(np.zeros(3), np.ones(3))
        assert s.mesh.n_triangles == 8 and np.array_equal(bits(s.mesh.points()), bits(tris.reshape(-1, 3)))      # the source is still usable
    finally:
        s.close()


@pytest.mark.parametrize('v', (1, 65, 257))
def test_the_refusal_counts_the_vertices_that_are_not_finite(v, eng):
    """1, 65 and 257 welded vertices -- one lane, a partial last wave, a partial last workgroup -- of a strip whose welded order is its
    own (x ascends); the vertices that are not finite lie in every wave and in both workgroups, and the refusal quotes how many the
    mesh's own weld holds"""
    x = np.arange(v, dtype=np.float64)
    p = np.stack([x, np.sin(x), np.cos(x)], axis=1)
    marks = [k for k in (0, 63, 64, 130, 200, 255, 256) if k < v]
    p[marks, 2] = np.where(np.arange(len(marks)) % 2, -np.inf, np.inf)      # (infinities weld like any value; a NaN equals nothing)
    i = np.arange(max(v - 2, 1))
    tris = np.stack([p[i], p[np.minimum(i + 1, v - 1)], p[np.minimum(i + 2, v - 1)]], axis=1)
    s = Soup(eng, tris)
    try:
        pts, cells = s.mesh.weld()
        assert len(pts) == v and list(np.flatnonzero(~np.isfinite(pts).all(axis=1))) == marks
        with pytest.raises(engine.SdfHipError, match=': %d vertices are not finite' % len(marks)):
            s.mesh.simplify(np.zeros(3), np.ones(3))
    finally:
        s.close()


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through sdf_mesh_simplify (the scratch, then the survivors' soup) on 100,000 tetrahedra -- 400,000
    triangles, both blocks above 16 MiB, welded beforehand: each failure carries the allocator's message, writes no mesh, and the free
    device memory is what it was; the first call that gets through matches the definition, and closing the meshes returns the rest.
    The hook injects a host-side allocation error: nothing faults."""
    lib = eng.lib
    warm = Soup(eng, components_ref.tetrahedron())                # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.simplify(np.full(3, -0.5), np.ones(3)).close()
    finally:
        warm.close()
    n = 100000
    rng = np.random.RandomState(1)
    tris = (components_ref.tetrahedron()[None] + np.stack([3.0 * rng.permutation(n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1)[:, None, None, :]).reshape(-1, 3, 3)
    origin, cell = np.array([-0.5, -1.5, -1.5]), np.full(3, 0.4)
    o, c = (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*cell)
    s = Soup(eng, tris)
    try:
        eng.trim()
        eng.synchronize()
        f00 = _free(lib)
        pts, cells = s.mesh.weld()
        want = ref.simplify(pts.copy(), cells.copy(), origin, cell)
        assert 72 * want.stats['triangles_out'] > (16 << 20)
        eng.synchronize()
        f0 = _free(lib)
        h, st = ctypes.c_void_p(), engine.SdfSimplifyStats()
        failures, rc = 0, -1
        for nth in range(1, 5):
            lib.sdf_test_fail_alloc(nth)
            rc = lib.sdf_mesh_simplify(s.mesh.handle, o, c, 1e-3, ctypes.byref(h), ctypes.byref(st))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error() and h.value is None, (rc, lib.sdf_last_error())
            assert _free(lib) == f0, (nth, f0, _free(lib))
        assert rc == 0 and failures == 2, (rc, failures)
        small = engine.Mesh(eng, h)
        try:
            small.simplify_stats = dict({k: int(getattr(st, k)) for k in ref.STAT_KEYS}, kernel_ms=float(st.kernel_ms))
            same(small, want)
            held = f0 - _free(lib)                                # the survivors' soup, 72 B per triangle, and nothing else
            assert 72 * small.n_triangles <= held <= 72 * small.n_triangles + (8 << 20), held
        finally:
            small.close()
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
    eng.trim()
    eng.synchronize()
    assert _free(lib) >= f00
