"""Dual contouring on the device (csrc/sdf_dual.hip, `engine.Engine.generate_dual`, `sdf_amd.dual_of_grid`, `dual=` of everything
that meshes): every output -- the crossing points and normals, the vertices, the cells, the soup, the eight counters -- identical bit
for bit to the definition (tests/dual_ref.py) run over the same interpreter (`Engine.eval_points`), and for the tapes without libm
calls to the definition over the CPU checker; grids that straddle a workgroup boundary on the contiguous axis; the feature through
the pipeline.  Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
import ctypes
import os

import numpy as np
import pytest

import dual_ref as ref
import fixtures
import normals_ref
import probe_cases as pc
from conftest import GOLDEN
from sdf_amd import core, dist, dual, tape
from test_register_slots import is_trig

pytestmark = pytest.mark.gpu

REG = 1e-3


def cube_bounds(half, shift=0.0):
    return ((-half + shift,) * 3, (half + shift,) * 3)


def grid(bounds, samples):
    return core.grid_axes(bounds, None, samples)[:3]


def case(name, ns):
    """(model, X, Y, Z, eps) of a named case"""
    if name == 'box':
        b = cube_bounds(0.6, 0.013)
        return (ns['box'](1),) + grid(b, 2 ** 12) + (core.default_normal_eps(b),)
    if name == 'example':
        b = cube_bounds(0.85)
        return (fixtures.build('ex_example', ns),) + grid(b, 2 ** 15) + (core.default_normal_eps(b),)
    if name == 'sphere_open':                                          # the bounds cut the sphere: open_edges > 0
        b = cube_bounds(0.8)
        return (ns['sphere'](1),) + grid(b, 2 ** 12) + (core.default_normal_eps(b),)
    if name == 'anisotropic':
        return ns['sphere'](0.4).translate((0.01, -0.02, 0.015)), np.arange(-0.5, 0.5, 0.05), np.arange(-0.5, 0.5, 0.07), np.arange(-0.5, 0.5, 0.06), 1e-4
    if name == 'nz2':
        ax = np.arange(-8, 9) / 10.0
        return ns['sphere'](0.5).translate((0.0, 0.0, 0.3)), ax, ax, np.array([-0.05, 0.3]), 1e-4
    if name == 'empty':                                                # the bounds miss the model
        b = ((2.0, 2.0, 2.0), (3.0, 3.0, 3.0))
        return (ns['box'](1),) + grid(b, 2 ** 9) + (core.default_normal_eps(b),)
    return (pc.model(name, ns)[0],) + tuple(pc.axes(name, ns)) + (pc.NORMAL_EPS,)      # a fixture on its small grid


def same(mesh, want, what=''):
    """the device's mesh (made with parts=True) against the definition's Dual: types, shapes, bits, counters"""
    got = mesh.dual_parts
    assert list(mesh.dual_stats) == list(ref.STAT_KEYS) and mesh.dual_stats == want.stats, (what, mesh.dual_stats, want.stats)
    for key, w in (('points', want.points), ('normals', want.normals), ('vertices', want.vertices)):
        g = got[key]
        assert g.dtype == np.float64 and g.shape == w.shape, (what, key, g.shape, w.shape)
        bad = (ref.bits(g) != ref.bits(w)).any(axis=1)
        assert not bad.any(), '%s: %d of %d %s differ, first at %d: %r / %r' % (what, bad.sum(), bad.size, key, np.flatnonzero(bad)[0],
                                                                               g[np.flatnonzero(bad)[0]], w[np.flatnonzero(bad)[0]])
    assert got['cells'].dtype == np.int64 and got['cells'].shape == want.cells.shape and np.array_equal(got['cells'], want.cells), what
    soup = mesh.points()
    assert mesh.n_triangles == len(want.cells) and soup.shape == (3 * len(want.cells), 3), what
    assert np.array_equal(ref.bits(soup), ref.bits(want.soup.reshape(-1, 3))), what


@pytest.mark.parametrize('name', ('box', 'example', 'sphere_open', 'anisotropic', 'nz2', 'empty', 'twist', 'ellipsoid_flat'))
def test_every_output_is_the_definitions(name, ns, eng, oracle_lib):
    f, X, Y, Z, eps = case(name, ns)
    with np.errstate(all='ignore'):
        want = ref.dual(lambda P: eng.eval_points(f, P), X, Y, Z, eps, REG)
    mesh = eng.generate_dual(f, X, Y, Z, eps, REG, parts=True)
    try:
        same(mesh, want, name)
        st = mesh.stats()
        assert st['skipped'] == 0 and st['triangles'] == want.stats['triangles'] and st['nonempty'] + st['empty'] == st['batches']
        assert (st['nonempty'] > 0) == (want.stats['cells'] > 0)
    finally:
        mesh.close()
    print('%s: %s' % (name, want.stats))
    if name == 'sphere_open':
        assert want.stats['open_edges'] > 0 and want.stats['triangles'] > 0
    if name == 'nz2':
        assert want.stats['open_edges'] > 0 and (want.edges[:, 1] == 2).any() and want.stats['triangles'] > 0
    if name == 'empty':
        assert want.stats == dict.fromkeys(ref.STAT_KEYS, 0)
    if name == 'ellipsoid_flat':
        assert want.stats['nonfinite_edges'] > 0
    if name not in ('empty',):
        assert want.stats['crossings'] > 0
    assert is_trig(tape.lower(f)) == (name == 'twist')
    if name != 'twist':                                                # no libm call in the tape: the CPU checker gives the same bits
        with np.errstate(all='ignore'):
            cpu = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, eps, REG)
        assert cpu.stats == want.stats and np.array_equal(cpu.cells, want.cells), name
        for a, b in ((cpu.points, want.points), (cpu.normals, want.normals), (cpu.vertices, want.vertices)):
            assert np.array_equal(ref.bits(a), ref.bits(b)), name
    # the indexed result without the handle, and what the timing entry says
    v, c, stats = dual.dual_of_grid(f, X, Y, Z, eps, REG)
    assert np.array_equal(ref.bits(v), ref.bits(want.vertices)) and np.array_equal(c, want.cells) and stats == want.stats
    parts = np.zeros(5)
    total = eng.lib.sdf_generate_dual_last_kernel_ms(parts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert abs(total - parts.sum()) <= 1e-9 * total and total > 0 and (parts[2] > 0) == (want.stats['crossings'] > 0)


@pytest.mark.parametrize('nz', (255, 257))
def test_grids_that_straddle_a_workgroup_boundary(nz, ns, eng, oracle_lib):
    """256 lanes along the contiguous axis: with nz = 255 and 257 a row of samples starts anywhere in a workgroup, so a lane's +1
    neighbours along x and y, and the scan bases of the four samples a cell gathers from, lie in other workgroups"""
    f = ns['sphere'](0.45).translate((0.02, -0.03, 0.01))
    X, Y, Z = np.array([-0.5, -0.2, 0.1, 0.4]), np.array([-0.6, -0.3, 0.0, 0.3, 0.6]), np.linspace(-0.6, 0.6, nz)
    want = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, 1e-4, REG)
    assert want.stats['crossings'] > 500 and want.stats['triangles'] > 0 and np.bincount(want.edges[:, 1], minlength=3).min() > 0
    mesh = eng.generate_dual(f, X, Y, Z, 1e-4, REG, batch_size=7, parts=True)
    try:
        same(mesh, want, 'nz = %d' % nz)
        # the blocks of 7^3 cells that hold a vertex, counted on the host from the definition's active cells
        ci = np.stack(np.unravel_index(want.active, (len(X) - 1, len(Y) - 1, nz - 1)), axis=1) // 7
        st = mesh.stats()
        assert st['nonempty'] == len(np.unique(ci, axis=0)) and st['batches'] == 1 * 1 * -(-(nz - 1) // 7)
    finally:
        mesh.close()


# ---- through the pipeline ----

BOX_BOUNDS = cube_bounds(0.6, 0.013)
SAMPLES = 2 ** 12
CALL = dict(bounds=BOX_BOUNDS, samples=SAMPLES, verbose=False)


@pytest.fixture(scope='module')
def box(ns, eng):
    """(the model, its definition Dual over the device's interpreter, the axes and steps of the call)"""
    f = ns['box'](1)
    X, Y, Z, steps = core.grid_axes(BOX_BOUNDS, None, SAMPLES)
    want = ref.dual(lambda P: eng.eval_points(f, P), X, Y, Z, core.default_normal_eps(BOX_BOUNDS), REG)
    return f, want, (X, Y, Z), steps


def test_generate_measure_and_save_stl(box, tmp_path, ns):
    f, want, _, _ = box
    pts = f.generate(dual=True, **CALL)
    assert pts.shape == (3 * len(want.cells), 3) and np.array_equal(ref.bits(pts), ref.bits(want.soup.reshape(-1, 3)))
    assert core.generate.last_dual == want.stats and list(core.generate.last_dual) == list(ref.STAT_KEYS)
    assert core.generate.last_stats['skipped'] == 0 and core.generate.last_stats['triangles'] == len(want.cells)
    m = f.measure(dual=True, **CALL)
    assert m.closed and m.oriented and m.euler == 2 and m.triangles == len(want.cells) and m.vertices == len(want.vertices)
    assert abs(m.volume - ref.volume(want.soup)) <= 1e-10               # (two orders of summation over a few thousand terms below 1)
    f.save(str(tmp_path / 'a.stl'), dual=True, **CALL)
    back = ns['Mesh'].from_stl(str(tmp_path / 'a.stl'))
    soup32 = np.asarray(back.points)[np.asarray(back.triangles)].astype(np.float32)
    assert np.array_equal(soup32, want.soup.astype(np.float32))


def test_the_option_as_a_dict(box, eng):
    f, _, (X, Y, Z), _ = box
    want = ref.dual(lambda P: eng.eval_points(f, P), X, Y, Z, 1e-3, 0.0)
    pts = f.generate(dual={'eps': 1e-3, 'reg': 0.0}, **CALL)
    assert np.array_equal(ref.bits(pts), ref.bits(want.soup.reshape(-1, 3))) and core.generate.last_dual == want.stats


def test_the_stages_behind_it(box, tmp_path, ns, eng):
    """each stage of the pipeline behind dual=True gives what the same stage gives on the adopted soup of the definition"""
    from sdf_amd.deviation import snap_params
    from sdf_amd.shells import resolve_keep
    from sdf_amd.simplify import resolve_cell
    f, want, (X, Y, Z), steps = box
    eps = core.default_normal_eps(BOX_BOUNDS)

    def equal(got, points, cells, what):
        assert np.array_equal(ref.bits(got[0]), ref.bits(points)) and np.array_equal(got[1], cells), what

    with core.adopted(want.soup) as mesh:
        points, cells = mesh.weld()
        normals, n_flat = mesh.vertex_normals(f, eps)
        got = f.generate_mesh(dual=True, normals=True, **CALL)
        equal(got, points, cells, 'weld')
        assert np.array_equal(ref.bits(got[2]), ref.bits(normals))
        f.save(str(tmp_path / 'a.ply'), dual=True, normals=True, **CALL)
        p32, n32, c32, _ = normals_ref.parse_ply(str(tmp_path / 'a.ply'))
        assert np.array_equal(p32, points.astype(np.float32)) and np.array_equal(n32, normals.astype(np.float32)) and np.array_equal(c32, cells)

        small = mesh.simplify(*resolve_cell(2, X, Y, Z, steps))
        try:
            equal(f.generate_mesh(dual=True, simplify=2, **CALL), *small.weld(), 'simplify')
            assert core.generate_mesh.last_simplify['triangles_in'] == len(want.cells) and small.n_triangles < len(want.cells)
        finally:
            small.close()
        mended = mesh.mend()
        try:
            equal(f.generate_mesh(dual=True, mend=True, **CALL), *mended.weld(), 'mend')
            assert core.generate_mesh.last_mend['triangles_in'] == len(want.cells)
        finally:
            mended.close()
        snapped = mesh.snap(f, **snap_params({}, BOX_BOUNDS, steps))
        try:
            equal(f.generate_mesh(dual=True, snap=True, **CALL), *snapped.weld(), 'snap')
            assert core.generate_mesh.last_snap['vertices'] == len(want.vertices)
        finally:
            snapped.close()

    # keep: two shells, the larger one kept
    g = ns['sphere'](0.2).translate((-0.2, 0.0, 0.0)) | ns['sphere'](0.08).translate((0.35, 0.0, 0.0))       # (0.27 apart: two cell diagonals)
    two = ref.dual(lambda P: eng.eval_points(g, P), X, Y, Z, eps, REG)
    with core.adopted(two.soup) as mesh:
        counts = mesh.shell_summary()['triangles']
        assert len(counts) == 2
        kept = mesh.select(resolve_keep('largest', counts))
        try:
            equal(g.generate_mesh(dual=True, keep='largest', **CALL), *kept.weld(), 'keep')
            assert 0 < kept.n_triangles < len(two.cells)
        finally:
            kept.close()


def test_a_call_without_dual_is_the_parents(ns):
    f = fixtures.build('ex_example', ns)
    d = np.load(os.path.join(GOLDEN, 'gen_example_s15.npz'))
    before = core.generate.last_dual
    pts = f.generate(samples=2 ** 15, verbose=False)
    assert pts.shape == d['points'].shape and np.array_equal(pts, d['points'])
    st = core.generate.last_stats
    assert (st['skipped'], st['empty'], st['nonempty'], st['triangles']) == (0, 0, 1, len(d['points']) // 3)
    assert core.generate.last_dual is before                           # untouched by a call that did not ask


def test_refusals(ns, eng, monkeypatch):
    f = ns['sphere'](1)
    ax = np.arange(-6, 7) / 5.0
    for kw in ({'eps': 0.0}, {'eps': np.nan}, {'reg': -1.0}, {'reg': np.inf}):
        with pytest.raises(ValueError):
            eng.generate_dual(f, ax, ax, ax, **dict({'eps': 1e-4, 'reg': REG}, **kw))
    with pytest.raises(ValueError):
        eng.generate_dual(f, ax, np.array([0.0, np.nan, 1.0]), ax, 1e-4)
    # a model with user closures: refused like the normals kernel refuses it, before anything is launched
    @ns['sdf3']
    def ball(r):
        def field(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return field
    closure = ball(0.8) & ns['box'](1.4)
    with pytest.raises(ValueError, match='closures'):
        eng.generate_dual(closure, ax, ax, ax, 1e-4)
    with pytest.raises(ValueError, match='closures'):
        closure.generate(dual=True, bounds=cube_bounds(1.2), samples=2 ** 9, verbose=False)
    # more than one process: the soup would be gathered on the host
    monkeypatch.setattr(dist, 'world_size', lambda: 2)
    with pytest.raises(NotImplementedError, match='dual'):
        f.generate(dual=True, bounds=cube_bounds(1.2), samples=2 ** 9, verbose=False)
