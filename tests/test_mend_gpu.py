"""A mesh mended on the device (csrc/sdf_mend.hip, `engine.Mesh.mend`, sdf_amd/mend.py, `mend=`): every soup compared EXACTLY, as
int64 bit patterns, with the definition (tests/mend_ref.py) applied to the mesh's own weld and its own soup, the statistics as
integers; end to end on the thin-plates model; the refusals and the leaks.  Every refusal is decided on the host; no test repeats a
device call that failed."""
import ctypes

import numpy as np
import pytest

import components_ref
import measure_ref
import mend_ref as ref
import normals_ref
from sdf_amd import core, engine, simplify
from sdf_amd.shells import resolve_keep

pytestmark = pytest.mark.gpu

BOUNDS = ((-1.3,) * 3, (1.3,) * 3)
STEP = 0.05
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


def same(mended, want):
    """a mended device mesh against the definition's Mended: the soup bit for bit, the statistics as integers"""
    got = mended.points()
    assert mended.n_triangles == len(want.soup) and got.shape == (3 * len(want.soup), 3) and got.dtype == np.float64
    bad = bits(got) != bits(want.soup.reshape(-1, 3))
    assert not bad.any(), '%d of %d doubles differ, first at %s' % (bad.sum(), bad.size, np.argwhere(bad)[0])
    st = mended.mend_stats
    assert {k: st[k] for k in ref.STAT_KEYS} == want.stats and all(isinstance(st[k], int) for k in ref.STAT_KEYS)
    assert st['kernel_ms'] >= 0.0


def check(mesh):
    """mesh.mend against the definition on the mesh's OWN weld and soup; returns the definition's Mended"""
    cells = mesh.weld()[1]
    want = ref.mend(np.array(cells), np.array(mesh.points()).reshape(-1, 3, 3))
    mended = mesh.mend()
    try:
        same(mended, want)
    finally:
        mended.close()
    print('mended: %s' % (want.stats,))
    return want


def check_soup(eng, tris):
    s = Soup(eng, tris)
    try:
        return check(s.mesh)
    finally:
        s.close()


# ---- adopted soups: the smallest shapes where each kernel can go wrong ----
@pytest.mark.parametrize('name', sorted(ref.mend_cases()))
def test_constructed_cases(name, eng):
    """T = 0 (no launch), T = 1, every cell collapsed, the cube unchanged, the cube and its flipped copy gone, one face repeated on
    either side among unrelated triangles, faces that agree in two of three indices"""
    soup, expect = ref.mend_cases()[name]
    want = check_soup(eng, soup)
    assert want.stats == expect
    if name == 'cube':
        assert np.array_equal(bits(want.soup), bits(soup))


def test_negative_zero_comes_from_the_source_soup(eng):
    """-0.0 and +0.0 weld to one vertex; the survivor is the first copy, and its doubles are the soup's, sign bits included"""
    cube = measure_ref.cube_soup(lo=0.0, hi=1.0)
    cube[cube == 0.0] = -0.0
    soup = np.concatenate([cube[:, [1, 2, 0]], cube + 0.0])
    want = check_soup(eng, soup)
    assert want.stats['duplicates'] == 12 and np.array_equal(bits(want.soup), bits(soup[:12])) and np.signbit(want.soup).any()


@pytest.mark.parametrize('n0, n1', ref.REPEATS)
def test_the_survivor_is_the_first_of_the_majority_side(n0, n1, eng):
    soup, survivor = ref.repeated_face(n0, n1)
    s = Soup(eng, soup)
    try:
        mended = s.mesh.mend()
        try:
            keep = (soup < 0).all(axis=(1, 2))                    # the unrelated ones are negative ...
            if survivor is not None:
                keep[survivor] = True                             # ... and of the repeated face, this one
            assert np.array_equal(bits(mended.points()), bits(soup[keep].reshape(-1, 3)))
        finally:
            mended.close()
    finally:
        s.close()


@pytest.mark.parametrize('k, flipped', ((63, 0), (64, 32), (65, 33), (255, 0), (256, 128), (257, 1), (1025, 512)))
def test_one_face_many_times_across_a_workgroup_edge(k, flipped, eng):
    """the run of the face is [n_pad, n_pad + k) of the sorted order and straddles position 256 (1025: five workgroups): the head's
    walk crosses waves and workgroups; side 0 wins, side 1 wins (65: 32 against 33) and nobody wins (64, 256)"""
    n_pad = 100 if k > 512 else 256 - k // 2
    want = check_soup(eng, ref.long_run(k, n_pad, flipped))
    one = k != 2 * flipped
    assert want.stats == dict(triangles_in=n_pad + k, triangles_out=n_pad + one, collapsed=0, duplicates=(k - 1) if one else 0,
                              cancelled=0 if one else k, faces=n_pad + 1)
    assert np.flatnonzero(want.keep[n_pad:]).tolist() == ([0 if k > 2 * flipped else k - flipped] if one else [])


def test_indices_beyond_two_to_the_seventeen(eng):
    """70,000 disjoint triangles, 210,000 welded vertices: the keys pass 2^16 and 2^17, every digit of both sorts carries
    information; a few of them again (duplicates), flipped (cancelled) and collapsed, everything shuffled"""
    rng = np.random.RandomState(17)
    base = ref.unrelated(70000)
    again = base[[5, 69999, 40000]][:, [1, 2, 0]]
    flipped = base[[7, 65000, 33000, 69998]][:, [0, 2, 1]]
    sliver = base[[9, 60000]][:, [0, 0, 1]]
    soup = np.concatenate([base, again, flipped, sliver])
    want = check_soup(eng, soup[rng.permutation(len(soup))])
    assert want.stats == dict(triangles_in=70009, triangles_out=69996, collapsed=2, duplicates=3, cancelled=8, faces=70000)
    assert want.face.max() >= 2 ** 17


def test_soup_order_shuffled_against_welded_order(eng):
    """a strip whose vertices are placed by a permutation, every third triangle also flipped and every seventh twice"""
    rng = np.random.RandomState(7)
    n = 3000
    j = np.arange(n)
    pos = np.stack([rng.permutation(n).astype(np.float64), (j % 2).astype(np.float64), np.sin(j * 0.01)], axis=1)
    strip = pos[(j[:, None] + np.arange(3)[None, :]) % n]
    soup = np.concatenate([strip, strip[::3][:, [2, 1, 0]], strip[::7][:, [1, 2, 0]]])
    want = check_soup(eng, soup[rng.permutation(len(soup))])
    assert want.stats['cancelled'] > 0 and want.stats['duplicates'] > 0 and 0 < want.stats['triangles_out'] < n


def test_mending_twice(eng):
    rng = np.random.RandomState(3)
    pts = rng.uniform(0, 1, (40, 3))
    s = Soup(eng, pts[rng.randint(0, 40, size=(2000, 3))])
    try:
        before = s.mesh.points().copy()
        a = s.mesh.mend()
        b = s.mesh.mend()
        try:
            assert 0 < a.n_triangles < 2000 and np.array_equal(bits(a.points()), bits(b.points()))
            assert dict(a.mend_stats, kernel_ms=0) == dict(b.mend_stats, kernel_ms=0)
            n = a.n_triangles
            want = check(a)                                       # a mended mesh mends to itself
            assert want.stats == dict(triangles_in=n, triangles_out=n, collapsed=0, duplicates=0, cancelled=0, faces=n)
            assert np.array_equal(bits(want.soup.reshape(-1, 3)), bits(a.points()))
        finally:
            a.close()
            b.close()
        assert np.array_equal(bits(s.mesh.points()), bits(before))            # the source is what it was
    finally:
        s.close()


# ---- the thin-plates model: other kinds of mesh, end to end ----
def plates(ns):
    plate = ns['box']((2, 2, 0.12))
    return plate | plate.translate((0, 0, 0.3))


def grid():
    if 'grid' not in _cache:
        _cache['grid'] = core.grid_axes(BOUNDS, STEP)
    return _cache['grid']


def wanted(ns, eng):
    """the definition applied to the device's own simplified mesh (simplify=4), taken once and left unchanged: (Mended, points,
    cells of its weld)"""
    if 'want' not in _cache:
        X, Y, Z, step = grid()
        mesh = eng.generate(plates(ns), X, Y, Z, 32, True)
        try:
            small = mesh.simplify(*simplify.resolve_cell(4, X, Y, Z, step))
            try:
                want = check(small)                               # a simplified mesh mends to the definition
            finally:
                small.close()
        finally:
            mesh.close()
        for a in (want.soup, want.keep):
            a.setflags(write=False)
        _cache['want'] = (want,) + ref.weld(want.soup)
    return _cache['want']


def test_a_simplified_mesh(ns, eng):
    want, wp, wc = wanted(ns, eng)
    assert want.stats['cancelled'] > 0 and want.stats['triangles_in'] > want.stats['triangles_out'] > 0


@pytest.mark.parametrize('how', ('records', 'selection', 'chunked'))
def test_other_kinds_of_mesh_mend_to_the_definition(how, ns, eng):
    f = plates(ns)
    X, Y, Z, step = grid()
    if how == 'records':
        eng.generate(f, X, Y, Z, 32, True, records=True).close()  # (the first record call of a model sizes the slab)
    mesh = eng.generate(f, X, Y, Z, 40 if how == 'chunked' else 32, True, records=how == 'records')
    try:
        if how == 'selection':
            counts = mesh.shell_summary()['triangles']
            assert len(counts) == 2
            sel = mesh.select(resolve_keep('largest', counts))
            try:
                want = check(sel)
            finally:
                sel.close()
        else:
            want = check(mesh)
        # (before the plates are simplified no face repeats; the plates' sides at x, y = +-1 lie on grid planes, where marching cubes emits
        # triangles with two equal corners: those go)
        assert want.stats['duplicates'] == want.stats['cancelled'] == 0 and want.stats['faces'] == want.stats['triangles_out'] > 0
    finally:
        mesh.close()


def test_generate_mesh_measure_and_save_with_mend(tmp_path, capsys, ns, eng):
    f = plates(ns)
    want, wp, wc = wanted(ns, eng)
    kw = dict(bounds=BOUNDS, step=STEP, simplify=4, mend=True)
    pts, cells, n = f.generate_mesh(verbose=False, **kw)
    assert n is None and np.array_equal(bits(pts), bits(wp)) and np.array_equal(cells, wc)
    st = core.generate_mesh.last_mend
    assert {k: st[k] for k in ref.STAT_KEYS} == want.stats and st['cancelled'] > 0
    m = f.measure(verbose=False, **kw)
    census = measure_ref.edge_census(wc, len(wp))
    assert {k: getattr(m, k) for k in census} == census and m.triangles == len(wc)
    folded = f.measure(verbose=False, bounds=BOUNDS, step=STEP, simplify=4)
    assert folded.triangles == want.stats['triangles_in'] and folded.nonmanifold > census['nonmanifold']
    v = measure_ref.derive(measure_ref.moments(want.soup))
    assert abs(m.volume - v['volume']) <= 1e-12 * abs(v['volume']) and abs(m.area - v['area']) <= 1e-12 * v['area']
    assert abs(m.volume - folded.volume) <= 1e-12 * abs(m.volume) and m.area < folded.area     # a cancelled pair encloses nothing
    nt = len(wc)
    f.save(str(tmp_path / 'a.stl'), verbose=False, **kw)
    data = open(tmp_path / 'a.stl', 'rb').read()
    assert len(data) == 84 + 50 * nt and int(np.frombuffer(data, '<u4', 1, 80)[0]) == nt
    f.save(str(tmp_path / 'a.ply'), verbose=False, writer='native', **kw)
    p, nn, c, head = normals_ref.parse_ply(str(tmp_path / 'a.ply'))
    assert head == normals_ref.ply_header(len(wp), nt, False) and np.array_equal(c, wc)
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32))
    assert f.shells(**kw).triangles.sum() == nt
    assert sum(s.triangles for s in f.measure_shells(**kw)) == nt
    capsys.readouterr()
    f.generate_mesh(**kw)
    assert '\n%d triangles in ' % nt in capsys.readouterr().out   # the closing line counts what is yielded


def test_mend_false_is_the_call_without_the_keyword(tmp_path, monkeypatch, ns, eng):
    f = plates(ns)
    kw = dict(bounds=BOUNDS, step=STEP, simplify=4, verbose=False)
    called = []
    real = engine.Mesh.mend
    monkeypatch.setattr(engine.Mesh, 'mend', lambda self: called.append(1) or real(self))
    for ext in ('stl', 'ply'):
        f.save(str(tmp_path / ('n.' + ext)), mend=False, **kw)
        f.save(str(tmp_path / ('m.' + ext)), **kw)
        assert open(tmp_path / ('n.' + ext), 'rb').read() == open(tmp_path / ('m.' + ext), 'rb').read()
    a, b = f.generate_mesh(mend=False, **kw), f.generate_mesh(**kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    f.measure(**kw)
    assert called == []
    f.save(str(tmp_path / 's.stl'), mend=True, **kw)
    assert called == [1] and len(open(tmp_path / 's.stl', 'rb').read()) < len(open(tmp_path / 'm.stl', 'rb').read())


def test_a_mesh_read_from_an_stl_file(tmp_path, ns, eng):
    """`Mesh.from_stl('thin.stl').simplify(cell).mend()`"""
    f = plates(ns)
    f.save(str(tmp_path / 'thin.stl'), bounds=BOUNDS, step=STEP, verbose=False)
    small = ns['Mesh'].from_stl(str(tmp_path / 'thin.stl')).simplify(4 * STEP)
    mended = small.mend()
    soup = np.asarray(small.points, dtype=np.float64)[np.asarray(small.triangles)]
    want = ref.mend_soup(soup)
    wp, wc = ref.weld(want.soup)
    assert isinstance(mended, ns['Mesh']) and np.array_equal(bits(mended.points), bits(wp)) and np.array_equal(mended.triangles, wc)
    assert want.stats['cancelled'] > 0


# ---- refusals and leaks ----
def test_refusals(eng):
    lib = eng.lib
    s = Soup(eng, components_ref.tetrahedron())
    try:
        h, st = ctypes.c_void_p(), engine.SdfMendStats()
        for args in ((None, ctypes.byref(h), ctypes.byref(st)), (s.mesh.handle, None, ctypes.byref(st)), (s.mesh.handle, ctypes.byref(h), None)):
            rc = lib.sdf_mesh_mend(*args)
            assert rc == 2 and b'NULL' in lib.sdf_last_error()
            with pytest.raises(ValueError, match='NULL'):         # what the binding makes of a refusal
                engine._check(lib, rc)
        assert h.value is None
        check(s.mesh)
    finally:
        s.close()
    with pytest.raises(ValueError, match='closed'):               # decided on the host: the handle is not touched
        s.mesh.mend()


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through sdf_mesh_mend (the scratch, then the survivors' soup) on 100,000 tetrahedra -- 400,000
    triangles, both blocks above 16 MiB, welded beforehand: each failure carries the allocator's message, writes no mesh, and the free
    device memory is what it was; the first call that gets through matches the definition, and closing the meshes returns the rest.
    The hook injects a host-side allocation error: nothing faults."""
    lib = eng.lib
    warm = Soup(eng, components_ref.tetrahedron())                # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.mend().close()
    finally:
        warm.close()
    n = 100000
    rng = np.random.RandomState(1)
    tris = (components_ref.tetrahedron()[None] + np.stack([3.0 * rng.permutation(n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1)[:, None, None, :]).reshape(-1, 3, 3)
    s = Soup(eng, tris)
    try:
        eng.trim()
        eng.synchronize()
        f00 = _free(lib)
        want = ref.mend(np.array(s.mesh.weld()[1]), tris)
        assert 72 * want.stats['triangles_out'] > (16 << 20)
        eng.synchronize()
        f0 = _free(lib)
        h, st = ctypes.c_void_p(), engine.SdfMendStats()
        failures, rc = 0, -1
        for nth in range(1, 5):
            lib.sdf_test_fail_alloc(nth)
            rc = lib.sdf_mesh_mend(s.mesh.handle, ctypes.byref(h), ctypes.byref(st))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error() and h.value is None, (rc, lib.sdf_last_error())
            assert _free(lib) == f0, (nth, f0, _free(lib))
        assert rc == 0 and failures == 2, (rc, failures)
        mended = engine.Mesh(eng, h)
        try:
            mended.mend_stats = dict({k: int(getattr(st, k)) for k in ref.STAT_KEYS}, kernel_ms=float(st.kernel_ms))
            same(mended, want)
            held = f0 - _free(lib)                                # the survivors' soup, 72 B per triangle, and nothing else
            assert 72 * mended.n_triangles <= held <= 72 * mended.n_triangles + (8 << 20), held
        finally:
            mended.close()
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
    eng.trim()
    eng.synchronize()
    assert _free(lib) >= f00
