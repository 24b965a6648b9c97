"""Contours on the device (csrc/sdf_contour.hip, sdf_amd/contour.py): every output array compared EXACTLY, as bit patterns, with the
definition (tests/contour_ref.py) -- the grid entry on constructed grids, ragged sizes, a random field and one loop that needs every
linking round; the tape entry and the slices of 3-D models on the samples the device took, which are Engine.eval_points' own; the
refusals, each decided on the host; the leaks.  No test repeats a device call that failed."""
import ctypes

import numpy as np
import pytest

import contour_cases as cases
import contour_ref as ref
import fixtures
from sdf_amd import contour, engine

pytestmark = pytest.mark.gpu

_f64p = ctypes.POINTER(ctypes.c_double)


def same(got, want, what=''):
    """a Contours of the device against the definition's dict: every array bit for bit, dtypes included, and the counts"""
    for k in ref.ARRAYS:
        g, w = getattr(got, k), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        bad = g.view(np.int64) != w.view(np.int64) if g.dtype == np.float64 else g != w
        assert not bad.any(), '%s %s: %d of %d differ, first at %s' % (what, k, bad.sum(), bad.size, np.argwhere(bad)[0])
    cnt = got.counts
    assert cnt['n_segments'] == want['n_segments'] and cnt['nonfinite_cells'] == want['nonfinite_cells'], (what, cnt)
    assert cnt['n_points'] == len(want['points']) and cnt['n_contours'] == len(want['closed'])
    assert cnt['rounds'] == int(np.ceil(np.log2(max(want['n_segments'], 1))))


def grid_points(X, Y, W=None):
    G = np.stack(np.meshgrid(X, Y, indexing='ij'), axis=-1).reshape(-1, 2)
    if W is None:
        return np.ascontiguousarray(G)
    return np.ascontiguousarray(np.concatenate([np.column_stack([G, np.full(len(G), h)]) for h in W]))


# ---- the grid entry ----
@pytest.mark.parametrize('name', sorted(cases.GRIDS))
def test_constructed_grids(eng, name):
    V, X, Y, level = cases.GRIDS[name]()
    same(contour.contour_grid(V, X, Y, level, eng=eng), ref.contours(V, X, Y, level), name)


def test_the_sixteen_cases(eng):
    X, Y = np.array([0.0, 1.0]), np.array([0.0, 1.5])
    for name, V, inside, centre in cases.two_by_two():
        same(contour.contour_grid(V, X, Y, 0.0, eng=eng), ref.contours(V, X, Y, 0.0), name)


@pytest.mark.parametrize('nw', [1, 3])
@pytest.mark.parametrize('nx,ny', [(2, 2), (3, 2), (2, 65), (65, 2), (33, 67), (129, 64)])
def test_ragged_sizes(eng, nx, ny, nw):
    V, X, Y, level = cases.random_field(nx, ny, nw, seed=nx * 1000 + ny * 10 + nw)
    V = np.round(V * 2) / 2                                           # (halves: plenty of samples equal to the second level)
    for lv in (level, 0.5):
        same(contour.contour_grid(V, X, Y, lv, eng=eng), ref.contours(V, X, Y, lv), '%dx%dx%d at %g' % (nw, nx, ny, lv))


def test_a_random_field(eng):
    """67 x 131 normal samples: hundreds of contours, closed and open, saddles of both decisions, more than one linking round"""
    V, X, Y, level = cases.random_field()
    want = ref.contours(V, X, Y, level)
    case, centre_inside, _ = ref.cell_codes(V, level)
    saddle = (case == 5) | (case == 10)
    assert (saddle & centre_inside).any() and (saddle & ~centre_inside).any()
    assert len(want['closed']) > 100 and want['closed'].any() and not want['closed'].all()
    got = contour.contour_grid(V, X, Y, level, eng=eng)
    assert got.counts['rounds'] > 1
    same(got, want, 'random')
    V[0, 5, 7] = np.inf                                               # ... and with non-finite samples in it
    V[0, 40, 0] = np.nan
    want = ref.contours(V, X, Y, level)
    assert want['nonfinite_cells'] == 6
    same(contour.contour_grid(V, X, Y, level, eng=eng), want, 'random with non-finite samples')


@pytest.mark.parametrize('ny', (2, 66, 258))
def test_nonfinite_cells_are_counted_at_ragged_sizes(eng, ny):
    """1, 65 and 257 cells -- one lane, a partial last wave, a partial last workgroup -- with non-finite samples at both ends: the
    workgroup's count is the definition's"""
    V, X, Y, level = cases.random_field(2, ny, 1, seed=ny)
    V[0, 0, ny - 1] = np.nan
    V[0, 1, 0] = np.inf
    want = ref.contours(V, X, Y, level)
    assert want['nonfinite_cells'] == (1 if ny == 2 else 2)
    same(contour.contour_grid(V, X, Y, level, eng=eng), want, '2 x %d with non-finite samples' % ny)


def test_one_contour_that_needs_every_round(eng):
    """a comb drawn into 257 x 257 samples: ONE closed loop of tens of thousands of segments, so the last doubling round still moves
    information -- a round count that is one short, or a round that reads what it writes, changes the leader or the positions"""
    V, X, Y, level = cases.comb()
    want = ref.contours(V, X, Y, level)
    assert len(want['closed']) == 1 and want['closed'][0] and want['n_segments'] > 20000
    got = contour.contour_grid(V, X, Y, level, eng=eng)
    assert 2 ** (got.counts['rounds'] - 1) < want['n_segments'] <= 2 ** got.counts['rounds']
    same(got, want, 'comb')
    V2 = np.concatenate([V, -V])                                      # the complement as a second layer: its loops are holes in a full sheet
    same(contour.contour_grid(V2, X, Y, level, eng=eng), ref.contours(V2, X, Y, level), 'comb and its complement')


# ---- the tape entry ----
def models(ns):
    return {
        'circle': ns['circle'](1),
        'plate': ns['rectangle']((2, 1)) - ns['circle'](0.3),
        'rounded_x': ns['rounded_x'](1, 0.2),
        'polygon': ns['polygon']([(-1, -1), (1, -1), (1, 1), (0, 0.2), (-1, 1)]),
        'hexagon_shell': ns['hexagon'](1).shell(0.1),
    }


@pytest.mark.parametrize('nx,ny', [(64, 64), (200, 150)])
@pytest.mark.parametrize('name', ['circle', 'plate', 'rounded_x', 'polygon', 'hexagon_shell'])
def test_2d_models(eng, ns, name, nx, ny):
    """the samples the device took are Engine.eval_points' at the same points, bit for bit, and the contours are the definition's
    over those samples"""
    f = models(ns)[name]
    X, Y = np.linspace(-1.6, 1.6, nx), np.linspace(-1.3, 1.3, ny)
    got, V = contour.contour_tape(f, X, Y, eng=eng, return_values=True)
    direct = eng.eval_points(f, grid_points(X, Y)).reshape(1, nx, ny)
    assert (V.view(np.int64) == direct.view(np.int64)).all()
    want = ref.contours(V, X, Y, 0.0)
    assert want['closed'].all() and len(want['closed']) >= (2 if name in ('plate', 'hexagon_shell') else 1)
    same(got, want, name)
    assert got.z is None and got.n_layers == 1


def test_more_samples_than_one_slab_of_points(eng, ns):
    """4100 x 4100 samples are more than the 2^24 points the tape entry evaluates at a time: the second slab starts in the middle of
    a row, and its samples and the contours across the seam are what one pass gives"""
    f = ns['rectangle']((4, 1)) - ns['circle'](0.3)                  # wider than the grid: its long edges run through every row
    n = 4100
    assert n * n > 2 ** 24 and (2 ** 24) % n != 0
    X, Y = np.linspace(-0.9, 0.9, n), np.linspace(-0.8, 0.8, n)
    got, V = contour.contour_tape(f, X, Y, eng=eng, return_values=True)
    direct = eng.eval_points(f, grid_points(X, Y)).reshape(1, n, n)
    assert (V.view(np.int64) == direct.view(np.int64)).all()
    want = ref.contours(V, X, Y, 0.0)
    ix = (2 ** 24) // n                                               # the row the seam lies in: the two open chains cross it
    assert want['closed'].tolist().count(False) == 2 and want['closed'].any()
    for p in (want['points'][want['offsets'][i]:want['offsets'][i + 1]] for i in np.flatnonzero(~want['closed'])):
        assert (p[:, 0] < X[ix]).any() and (p[:, 0] > X[ix + 1]).any()
    same(got, want, 'two slabs')


def test_a_float32_engine_takes_the_fall_back(eng, ns):
    """the tape entry is float64 only: with the engine set to float32 the samples are Engine.eval_points' float32 ones and the grid
    entry contours them"""
    f = ns['rectangle']((2, 1)) - ns['circle'](0.3)
    eng.precision = engine.PRECISION_F32
    try:
        c = f.contours(step=0.03, bounds=((-1.2, -0.7), (1.2, 0.7)))
        V = eng.eval_points(f, grid_points(c.X, c.Y)).reshape(1, len(c.X), len(c.Y))
    finally:
        eng.precision = engine.PRECISION_F64
    assert (V == V.astype(np.float32)).all()                          # float32 values, held in float64
    V64 = eng.eval_points(f, grid_points(c.X, c.Y)).reshape(V.shape)
    assert (V != V64).any()
    same(c, ref.contours(V, c.X, c.Y, 0.0), 'float32')
    assert c.closed.tolist() == [True, True]


def check_slices(eng, c, f):
    direct = eng.eval_points(f, grid_points(c.X, c.Y, c.z)).reshape(len(c.z), len(c.X), len(c.Y))
    same(c, ref.contours(direct, c.X, c.Y, 0.0))
    return direct


def test_slices_of_the_example(eng, ns):
    f = fixtures.build('ex_example', ns)
    z = np.linspace(-0.9, 0.9, 7)
    c = f.slices(z, samples=2 ** 14)
    assert (c.z == z).all() and c.n_layers == 7 and 100 < len(c.X) < 170
    check_slices(eng, c, f)
    # z = -0.9 and 0.9 lie outside the box of half-width 0.75: layers without a contour, at either end
    assert set(c.layer.tolist()) == set(range(1, 6)) and (np.diff(c.layer) >= 0).all() and c.closed.all()
    assert sum(1 for _ in c.loops(3)) == int((c.layer == 3).sum()) >= 2
    assert any(a < 0 for _, _, a in c.loops(5)) and any(a > 0 for _, _, a in c.loops(5))     # z = 0.6: the bore along z is a hole


def test_slices_of_a_model_of_the_trig_family(eng, ns):
    f = fixtures.build('ex_gearlike', ns)
    assert eng.tape_for(f).tape.dim == 3
    c = f.slices((-0.3, 0.0, 0.3), samples=2 ** 14)
    check_slices(eng, c, f)
    assert len(c) >= 3 * 2


def test_two_routes_to_the_same_slice(eng, ns):
    """f.slices(0.25) against the 2-D model f.translate((0, 0, -0.25)).slice() contoured on the same axes.  The two tapes differ --
    the 2-D one goes through a translation and the op `slice`, which picks between two intersections with a thin slab -- so their
    samples may differ in the last bits and the comparison is to 1e-12 of the extent, not bit for bit; the structure (which contours,
    how many points each, closed or not) must be the same"""
    f = fixtures.build('ex_example', ns)
    a = f.slices(0.25, bounds=((-1.1, -1.1), (1.1, 1.1)), step=0.02)
    b = contour.contour_tape(f.translate((0, 0, -0.25)).slice(), a.X, a.Y, eng=eng)
    assert a.offsets.tolist() == b.offsets.tolist() and a.closed.tolist() == b.closed.tolist() and len(a) >= 2
    extent = a.X[-1] - a.X[0]
    assert np.abs(a.points - b.points).max() <= 1e-12 * extent
    assert np.abs(a.area - b.area).max() <= 1e-11 * extent * extent
    assert a.z.tolist() == [0.25] and b.z is None


def test_a_model_with_a_user_closure_takes_the_fall_back(eng, ns):
    @ns['sdf2']
    def my_circle(radius):
        def f(p):
            return np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) - radius
        return f
    f = my_circle(0.9) - ns['circle'](0.4)
    assert eng.tape_for(f).tape.externs
    c = f.contours(step=0.04, bounds=((-1, -1), (1, 1)))
    V = eng.eval_points(f, grid_points(c.X, c.Y)).reshape(1, len(c.X), len(c.Y))
    want = ref.contours(V, c.X, c.Y, 0.0)
    same(c, want, 'closure')
    assert want['closed'].tolist() == [True, True] and want['area'][0] > 0 > want['area'][1]


def test_bounds_are_estimated_and_files_written(eng, ns, tmp_path):
    f = ns['rounded_x'](1, 0.2)
    c = f.save(str(tmp_path / 'x.svg'), samples=2 ** 12)
    (x0, y0), (x1, y1) = c.bounds                                     # the estimate holds the model: one closed loop inside it
    assert c.closed.all() and len(c) == 1 and c.area[0] > 0
    assert x0 < c.points[:, 0].min() and c.points[:, 0].max() < x1 and y0 < c.points[:, 1].min() and c.points[:, 1].max() < y1
    same(c, ref.contours(eng.eval_points(f, grid_points(c.X, c.Y)).reshape(1, len(c.X), len(c.Y)), c.X, c.Y, 0.0))
    assert open(str(tmp_path / 'x.svg')).read().count('M') == 1
    f.save(str(tmp_path / 'x.dxf'), step=0.05, bounds=((-1.3, -1.3), (1.3, 1.3)))
    assert open(str(tmp_path / 'x.dxf')).read().count('POLYLINE') == 1


# ---- refusals and leaks ----
def test_refusals(eng, ns):
    lib = eng.lib
    X = np.array([0.0, 1.0, 2.0])
    V = np.zeros((1, 3, 3))
    V[0, 1, 1] = -1.0
    h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
    p = lambda a: a.ctypes.data_as(_f64p)

    def grid(ctx=eng.ctx, v=V, nw=1, nx=3, ny=3, x=X, y=X, level=0.0, out=ctypes.byref(h), counts=ctypes.byref(cnt)):
        return lib.sdf_contour_grid_host(ctx, None if v is None else p(v), nw, nx, ny, None if x is None else p(x), None if y is None else p(y),
                                         level, out, counts)

    def refused(rc, word):
        assert rc == 2 and word.encode() in lib.sdf_last_error(), (rc, lib.sdf_last_error())
        with pytest.raises(ValueError, match=word):                   # what the binding makes of a refusal
            engine._check(lib, rc)
        assert h.value is None

    for kw in ({'ctx': None}, {'v': None}, {'x': None}, {'y': None}, {'out': None}, {'counts': None}):
        refused(grid(**kw), 'NULL')
    refused(grid(nx=1), 'nx and ny')
    refused(grid(ny=1), 'nx and ny')
    refused(grid(nw=0), 'nw')
    refused(grid(nw=2, nx=1 << 14, ny=1 << 14), 'samples')            # 2^29 of them (refused before an axis is read)
    for bad in (np.nan, np.inf, -np.inf):
        refused(grid(level=bad), 'level')
        refused(grid(x=np.array([0.0, bad, 2.0])), 'X value')
        refused(grid(y=np.array([0.0, 1.0, bad])), 'Y value')
    refused(grid(x=np.array([0.0, 1.0, 1.0])), 'X is not strictly')
    refused(grid(y=np.array([0.0, 2.0, 1.0])), 'Y is not strictly')

    f2, f3 = ns['circle'](1), ns['sphere'](1)
    t2, t3 = eng.tape_for(f2), eng.tape_for(f3)

    def tape(t=t2.handle, dim=2, x=X, y=X, w=None, nw=1, level=0.0, out=ctypes.byref(h), counts=ctypes.byref(cnt)):
        return lib.sdf_contour_host(t, dim, None if x is None else p(x), 3, None if y is None else p(y), 3, None if w is None else p(w), nw, level,
                                    None, out, counts)

    for kw in ({'t': None}, {'x': None}, {'y': None}, {'out': None}, {'counts': None}, {'t': t3.handle, 'dim': 3, 'w': None}):
        refused(tape(**kw), 'NULL')
    refused(tape(dim=4), 'dim')
    refused(tape(dim=2, nw=2), 'nw must be 1')
    refused(tape(t=t3.handle, dim=3, w=np.array([0.0, np.nan]), nw=2), 'W value')
    refused(tape(level=np.nan), 'level')
    refused(tape(x=np.array([0.0, 0.0, 1.0])), 'X is not strictly')

    @ns['sdf2']
    def mine():
        return lambda q: q[:, 0]
    tc = eng.tape_for(mine() & f2)
    refused(tape(t=tc.handle), 'closures')
    # a dim that does not match the tape: the C side has no notion of a tape's dimension, the binding has
    with pytest.raises(ValueError, match='2-D model'):
        contour.contour_tape(f2, X, X, W=np.array([0.0]), eng=eng)
    with pytest.raises(ValueError, match='3-D model'):
        contour.contour_tape(f3, X, X, eng=eng)
    # and after all that the entry points work
    same(contour.contour_grid(V, X, X, 0.0, eng=eng), ref.contours(V, X, X, 0.0))


def _free(lib):
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


def test_failed_allocations_leak_nothing(eng):
    """sdf_test_fail_alloc walked through one small sdf_contour_grid_host: the grid's scratch, the segments' scratch, the result's
    block.  Each failure carries the allocator's message and writes no handle, and the free device memory is what it was; the
    fourth call gets through and matches the definition; destroying its handle returns the rest.  The hook injects a host-side
    allocation error: nothing faults."""
    lib = eng.lib
    V, X, Y, level = cases.annulus()
    want = ref.contours(V, X, Y, level)
    same(contour.contour_grid(V, X, Y, level, eng=eng), want)        # (code objects and the like are loaded before anything is compared)
    eng.trim()
    eng.synchronize()
    f0 = _free(lib)
    p = lambda a: a.ctypes.data_as(_f64p)
    h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
    failures, rc = 0, -1
    try:
        for nth in range(1, 6):
            lib.sdf_test_fail_alloc(nth)
            rc = lib.sdf_contour_grid_host(eng.ctx, p(V), 1, len(X), len(Y), p(X), p(Y), level, ctypes.byref(h), ctypes.byref(cnt))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error() and h.value is None, (rc, lib.sdf_last_error())
            eng.synchronize()
            assert _free(lib) == f0, (nth, f0, _free(lib))
        assert rc == 0 and failures == 3, (rc, failures)
        same(contour._fetch(eng, h, cnt, None, X, Y), want)           # (fetches, then destroys the handle)
    finally:
        lib.sdf_test_fail_alloc(0)
    eng.synchronize()
    assert _free(lib) == f0
