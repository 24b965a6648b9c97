"""Dual contouring on the device (csrc/sdf_dual.hip, `engine.Engine.generate_dual`, `sdf_amd.dual_of_grid`, `dual=` of everything
that meshes): every output -- the crossing points and normals, the vertices, the cells, the soup, the eight counters -- identical bit
for bit to the definition (tests/dual_ref.py) run over the same interpreter (`Engine.eval_points`), and for the tapes without libm
calls to the definition over the CPU checker; with every comparison (`same`) the blocks that the closing line counts, from the
definition's active cells; grids that straddle a workgroup boundary on the contiguous axis; grids where the indexing can go wrong --
more than one sampling slab, crossings without a single quad, an axis of one sample, samples that are exactly zero, non-uniform
axes with ragged blocks --; the feature through the pipeline and behind the facades that probe a mesh.  tests/test_dual_sweep_gpu.py
runs the whole case table.  Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
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


def blocks(want, n, batch_size):
    """(batches, nonempty) of the closing line, from the definition: the blocks of batch_size^3 cells of a grid of n = (nx, ny, nz)
    samples, and those of them that hold an active cell.  A grid without a cell has no block"""
    nc = np.asarray(n, dtype=np.int64) - 1
    if nc.min() < 1:
        return 0, 0
    ci = np.stack(np.unravel_index(want.active, tuple(nc)), axis=1) // batch_size
    return int(np.prod(-(-nc // batch_size))), len(np.unique(ci, axis=0))


def same(mesh, want, what, n, batch_size=32):
    """the device's mesh (made with parts=True on a grid of n = (nx, ny, nz) samples, with this batch_size) against the definition's
    Dual: types, shapes, bits, counters, and what the closing line counts"""
    got = mesh.dual_parts
    st = mesh.stats()
    batches, nonempty = blocks(want, n, batch_size)
    assert (st['batches'], st['nonempty'], st['empty'], st['skipped']) == (batches, nonempty, batches - nonempty, 0), (what, st, batches, nonempty)
    assert st['triangles'] == want.stats['triangles'], (what, st['triangles'])
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
        same(mesh, want, name, (len(X), len(Y), len(Z)))
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
        same(mesh, want, 'nz = %d' % nz, (len(X), len(Y), nz), 7)
        # the blocks of 7^3 cells that hold a vertex, counted on the host from the definition's active cells
        ci = np.stack(np.unravel_index(want.active, (len(X) - 1, len(Y) - 1, nz - 1)), axis=1) // 7
        st = mesh.stats()
        assert st['nonempty'] == len(np.unique(ci, axis=0)) and st['batches'] == 1 * 1 * -(-(nz - 1) // 7)
    finally:
        mesh.close()


# ---- grids where the indexing can go wrong ----

SLAB = 2 ** 22                                                         # the samples of one sampling launch (csrc/sdf_dual.hip)


def test_more_than_one_sampling_slab(ns, eng, oracle_lib):
    """3 x 3 x 840001 samples: the sampling loop of dual_run runs twice -- k_dual_points with s0 = 2^22 and a partial second slab of
    3365705 points, the values written at V + s0.  With 4 nz <= 2^22 < 5 nz the seam lies in the CENTRE row (i, j) = (1, 1), at
    k = 2^22 - 4 nz = 834300, so the crossings round it have their four cells and emit quads whose vertices gather samples from both
    slabs.  Three small spheres: at the first samples, at the last ones, and about the seam's sample.  A sphere's tape has no libm
    call, so the definition runs over the CPU checker and the device is called once."""
    nz = 840001
    X, Y, Z = np.array([-0.05, 0.0, 0.05]) + 0.004, np.array([-0.05, 0.0, 0.05]) - 0.003, np.arange(nz) * 0.05
    n = 9 * nz
    assert SLAB < n < 2 * SLAB and n % SLAB and 4 * nz <= SLAB < 5 * nz
    k = SLAB - 4 * nz
    ball = ns['sphere'](0.06)
    f = ball.translate((0.0, 0.0, Z[2] + 0.01)) | ball.translate((0.0, 0.0, Z[nz - 3] - 0.02)) | ball.translate((0.0, 0.0, Z[k]))
    assert not is_trig(tape.lower(f))
    want = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, 1e-4, REG)
    print('slabs: %s' % (want.stats,))
    s = want.edges[:, 0]
    assert (s < SLAB).any() and (s >= SLAB).any() and want.stats['triangles'] > 0
    near = np.abs(s - SLAB) <= 2                                       # the crossings at the seam: on both sides of it, and they emit
    assert (s[near] < SLAB).any() and (s[near] >= SLAB).any() and (s % nz < 8).any() and (s % nz >= nz - 8).any()
    mesh = eng.generate_dual(f, X, Y, Z, 1e-4, REG, parts=True)
    try:
        same(mesh, want, 'slabs', (3, 3, nz))
    finally:
        mesh.close()


def readers(mesh):
    """what the readers of a mesh without a triangle give: the weld, the measurement, the shells, the STL records, the soup"""
    from sdf_amd.measure import measure_mesh
    pts, cells = mesh.weld()
    m = measure_mesh(mesh)._asdict()
    shells = mesh.shell_summary()
    return {'weld': (pts.shape, pts.dtype, cells.shape, cells.dtype), 'stl': len(mesh.stl_records()), 'soup': mesh.points().shape,
            'shells': (shells['count'], shells['triangles'].shape), 'measure': {k: np.asarray(v).tolist() for k, v in m.items()}}


def same_readers(got, want, what):
    assert list(got) == list(want), what
    for key in want:
        if key == 'measure':                                           # (the centroid and the inertia of nothing are NaN on both sides)
            for field, w in want[key].items():
                assert np.array_equal(np.asarray(got[key][field], dtype=np.float64), np.asarray(w, dtype=np.float64), equal_nan=True), (what, field)
        else:
            assert got[key] == want[key], (what, key, got[key], want[key])


@pytest.fixture(scope='module')
def no_triangles(ns, eng):
    """what the readers give on a marching-cubes mesh without a triangle: the grid misses the model"""
    far = np.linspace(5.0, 6.0, 9)
    mesh = eng.generate(ns['sphere'](0.5), far, far, far, 32, True)
    try:
        assert mesh.n_triangles == 0
        got = readers(mesh)
    finally:
        mesh.close()
    assert got['weld'][0] == (0, 3) and got['weld'][2] == (0, 3) and got['stl'] == 0 and got['soup'] == (0, 3) and got['shells'][0] == 0
    assert got['measure']['triangles'] == 0 and got['measure']['vertices'] == 0 and got['measure']['volume'] == 0.0
    return got


NO_QUADS = {                                                           # (X, Y): the sphere of radius 0.5 about the origin on Z = -0.8 .. 0.8 in steps of 0.2
    '2x2x9': (np.array([-0.1, 0.1]), np.array([-0.1, 0.1])),           # four rows along z, each enters and leaves the sphere
    '3x2x9': (np.array([-0.1, 0.1, 0.45]), np.array([-0.1, 0.1])),     # and a layer of rows that leave it sooner: crossings along x as well
    '2x3x9': (np.array([-0.1, 0.1]), np.array([-0.1, 0.1, 0.45])),     # the same along y
}


@pytest.mark.parametrize('name', sorted(NO_QUADS))
def test_crossings_without_a_quad(name, ns, eng, oracle_lib, no_triangles):
    """two samples on an axis: every crossing along another axis lies on the grid's border, so no crossing has its four cells --
    crossings, active cells and vertices, but no triangle: the soup is never allocated and the cells of the parts have no row"""
    X, Y = NO_QUADS[name]
    Z = np.linspace(-0.8, 0.8, 9)
    f = ns['sphere'](0.5)
    want = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, 1e-4, REG)
    print('%s: %s' % (name, want.stats))
    st = want.stats
    assert (st['crossings'], st['cells'], st['triangles']) == {'2x2x9': (8, 2, 0), '3x2x9': (20, 8, 0), '2x3x9': (20, 8, 0)}[name]
    assert st['open_edges'] == st['crossings'] and want.cells.shape == (0, 3) and want.soup.shape == (0, 3, 3) and len(want.vertices) == st['cells']
    mesh = eng.generate_dual(f, X, Y, Z, 1e-4, REG, parts=True)
    try:
        same(mesh, want, name, (len(X), len(Y), len(Z)))               # (the vertices among it: identical)
        assert mesh.n_triangles == 0 and mesh.points().shape == (0, 3)
        assert mesh.dual_parts['cells'].shape == (0, 3) and mesh.dual_parts['vertices'].shape == (st['cells'], 3)
        same_readers(readers(mesh), no_triangles, name)
    finally:
        mesh.close()
    assert dual.dual_of_grid(f, X, Y, Z, 1e-4, REG)[2] == st


@pytest.mark.parametrize('axis', (0, 1, 2))
def test_an_axis_of_one_sample(axis, ns, eng, no_triangles):
    """no cell: the empty mesh, every counter zero, nothing launched and nothing counted as a block"""
    axes = [np.arange(-8, 9) / 10.0] * 3
    axes[axis] = np.array([0.05])
    f = ns['sphere'](0.5)
    want = ref.dual(lambda P: eng.eval_points(f, P), *axes, 1e-4, REG)
    assert want.stats == dict.fromkeys(ref.STAT_KEYS, 0)
    mesh = eng.generate_dual(f, *axes, 1e-4, REG, parts=True)
    try:
        same(mesh, want, 'axis %d' % axis, tuple(len(a) for a in axes))
        assert mesh.stats()['batches'] == 0
        same_readers(readers(mesh), no_triangles, 'axis %d' % axis)
    finally:
        mesh.close()


@pytest.mark.parametrize('reg', (REG, 0.0))
def test_samples_that_are_exactly_zero(reg, ns, eng, oracle_lib):
    """the unit box on the nodes k / 8: its faces, edges and corners lie ON samples, whose value is 0.0 -- not inside, so the
    crossings run from them inwards with t = 0 / (0 - v1) = 0, or end in them with t = v0 / v0 = 1.  Every cell's crossings then lie in
    one plane or on one line, and without a regularisation the system is singular: the mean fallback"""
    ax = np.arange(-8, 9) / 8.0
    f = ns['box'](1)
    G = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), axis=-1).reshape(-1, 3)
    V = eng.eval_points(f, G)
    assert (V == 0.0).sum() == 386 and np.array_equal(ref.bits(V), ref.bits(oracle_lib.evaluate(f, G)))
    with np.errstate(all='ignore'):
        want = ref.dual(lambda P: eng.eval_points(f, P), ax, ax, ax, 1e-4, reg)
        cpu = ref.dual(lambda P: oracle_lib.evaluate(f, P), ax, ax, ax, 1e-4, reg)
    print('on the nodes, reg = %g: %s' % (reg, want.stats))
    stride = np.array([17 * 17, 17, 1])
    v0, v1 = V[want.edges[:, 0]], V[want.edges[:, 0] + stride[want.edges[:, 1]]]
    assert ((v0 == 0.0) & (v1 < 0.0)).any() and ((v1 == 0.0) & (v0 < 0.0)).any()      # both quotients occur
    assert (want.stats['crossings'], want.stats['triangles'], want.stats['open_edges']) == (294, 588, 0)
    assert (want.stats['mean_fallback'] > 0) == (reg == 0.0)
    assert cpu.stats == want.stats
    mesh = eng.generate_dual(f, ax, ax, ax, 1e-4, reg, parts=True)
    try:
        same(mesh, want, 'on the nodes', (17, 17, 17))
        same(mesh, cpu, 'on the nodes, over the checker', (17, 17, 17))
    finally:
        mesh.close()


def test_nonuniform_axes(ns, eng, oracle_lib):
    """every cell has its own lo, hi and half size on every axis (steps of 0.02 .. 0.11, drawn per axis), and blocks of 5^3 cells
    over 21 cells an axis: the last block is ragged on every axis"""
    rs = np.random.RandomState(5)
    X, Y, Z = (np.cumsum(rs.uniform(0.02, 0.11, 22)) - 0.7 for _ in range(3))
    assert len({tuple(np.diff(a)) for a in (X, Y, Z)}) == 3 and all(np.ptp(np.diff(a)) > 0.05 for a in (X, Y, Z))
    f = ns['sphere'](0.45).translate((-0.1, 0.05, 0.0)) | ns['box'](0.5).translate((0.15, -0.05, 0.1))
    want = ref.dual(lambda P: eng.eval_points(f, P), X, Y, Z, 1e-4, REG)
    cpu = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, 1e-4, REG)
    print('nonuniform: %s' % (want.stats,))
    assert want.stats['crossings'] > 1000 and want.stats['clamped'] > 0 and want.stats['open_edges'] == 0 and cpu.stats == want.stats
    census = ref.edge_census(want.cells)
    assert census['closed'] and census['oriented']
    batches, nonempty = blocks(want, (22, 22, 22), 5)
    assert batches == 5 ** 3 and 0 < nonempty < batches and 21 % 5
    mesh = eng.generate_dual(f, X, Y, Z, 1e-4, REG, batch_size=5, parts=True)
    try:
        same(mesh, want, 'nonuniform', (22, 22, 22), 5)
        same(mesh, cpu, 'nonuniform, over the checker', (22, 22, 22), 5)
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
    assert want.stats['mean_fallback'] > 0                             # a box without a regularisation: the fallback is taken
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


def alike(got, want, what):
    """two results of a reader, field by field: the same types and shapes, float64 by its bits, everything else exactly"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), what
        for key in want:
            alike(got[key], want[key], '%s.%s' % (what, key))
    elif isinstance(want, (tuple, list)):
        assert type(got) is type(want) and len(got) == len(want), what
        for k, (g, w) in enumerate(zip(got, want)):
            alike(g, w, '%s[%d]' % (what, k))
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
        assert np.array_equal(ref.bits(got), ref.bits(want)) if want.dtype == np.float64 else np.array_equal(got, want), what
    elif isinstance(want, float):
        assert isinstance(got, float) and ref.bits(got) == ref.bits(want), (what, got, want)
    elif hasattr(want, '__dict__'):
        assert type(got) is type(want), what
        alike(vars(got), vars(want), what)
    else:
        assert type(got) is type(want) and got == want, (what, got, want)


def test_the_probes_behind_it(box, ns):
    """the facades that probe a mesh -- overhangs, supports, thickness, curvature, deviation, shells -- with dual=True give exactly what
    the same reader gives on the adopted soup of the definition, with the parameters the facade resolves from the call's grid"""
    import sdf_amd
    from sdf_amd.curvature import Curvature, default_eps
    from sdf_amd.deviation import Deviation
    from sdf_amd.overhang import UP, overhangs_of_mesh
    from sdf_amd.shells import shells_of_mesh
    from sdf_amd.supports import supports_of_mesh
    from sdf_amd.thickness import Thickness, default_params
    f, want, _, steps = box
    tol, quarter = float(max(steps)), float(min(steps)) / 4
    assert len(want.cells) > 0
    with core.adopted(want.soup) as mesh:
        pts, cells = mesh.weld()
        assert len(pts) == len(want.vertices) and len(cells) == len(want.cells)
        alike(sdf_amd.overhangs(f, dual=True, **CALL), overhangs_of_mesh(mesh, UP, 45.0, tol), 'overhangs')
        alike(sdf_amd.supports(f, dual=True, **CALL), supports_of_mesh(mesh, f, UP, 45.0, tol, quarter, quarter), 'supports')
        par = dict(default_params(BOX_BOUNDS, steps), step_scale=1.0, max_steps=256, refine=16)
        got = sdf_amd.thickness(f, dual=True, **CALL)
        alike(got, Thickness(pts, cells, *mesh.vertex_thickness(f, **par), par), 'thickness')
        assert got.measured.any()
        eps = default_eps(steps)
        curv, status, _ = mesh.vertex_curvature(f, eps)
        alike(sdf_amd.curvature(f, dual=True, **CALL), Curvature(pts, cells, curv, status, {'eps': eps}), 'curvature')
        alike(sdf_amd.deviation(f, dual=True, **CALL), Deviation(pts, cells, *mesh.triangle_deviation(f, 2), 2), 'deviation')
        got = sdf_amd.shells(f, dual=True, **CALL)
        alike(got, shells_of_mesh(mesh), 'shells')
        assert got.count == 1 and got.triangles.tolist() == [len(want.cells)]
    assert core.generate.last_dual == want.stats                       # every one of them went through generate_dual


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
