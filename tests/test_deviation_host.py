"""The definition of a mesh held to the field (tests/deviation_ref.py) over the CPU checker, and the host side of the feature: the ABI
entries, the package's restatement of the definition, the `Deviation` object, the refusals that need no device, the ISA check of the
built library.  No GPU.  Meshes: `oracle.generate` at 2^13 samples welded by np.unique."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import deviation_ref as ref
from sdf_amd import core, d3, engine
from sdf_amd import mesh as mesh_module
from sdf_amd.deviation import (Deviation, check_order, check_snap, check_snap_option, sample_points, snap_params, triangle_deviation,
                               vertex_snap)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = 2 ** 13
_cache = {}


def checker_mesh(name, f, oracle):
    """(soup (T, 3, 3), welded points, grid steps, bounds) of the checker's mesh at 2^13 samples: once per model"""
    if name not in _cache:
        bounds = oracle.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=SAMPLES)
        soup = np.ascontiguousarray(oracle.generate(f, X, Y, Z, 32, True).points, dtype=np.float64).reshape(-1, 3, 3)
        pts = np.unique(soup.reshape(-1, 3), axis=0)
        soup.setflags(write=False)
        pts.setflags(write=False)
        _cache[name] = (soup, pts, step, bounds)
    return _cache[name]


def preview_eps(bounds):
    lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
    return 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)


@pytest.mark.parametrize('order', (1, 2, 3, 4, 5, 6, 7, 8))
def test_sphere_mesh_lies_within_h_squared_and_inside(order, ns, oracle_lib):
    """marching cubes of the unit sphere, no simplification: max |dev| <= h^2 with h the largest grid step.  A chord as long as a
    cell's diagonal (h sqrt 3) sags (h sqrt 3)^2 / 8 = 3 h^2 / 8 on a unit sphere, and marching cubes' own vertex error along an edge
    (linear interpolation of a field whose second derivative along the edge is at most 1) is below h^2 / 8: together h^2 / 2 <= h^2.
    The worst sample lies inside the sphere: chords cut it off."""
    f = ns['sphere'](1)
    soup, pts, step, bounds = checker_mesh('sphere', f, oracle_lib)
    h = max(step)
    dev, at, sumsq = ref.deviation(lambda P: oracle_lib.evaluate(f, P), soup, order)
    worst = int(np.argmax(np.abs(dev)))
    print('sphere order %d: %d triangles, h = %.6g, max |dev| = %.6g = %.3f h^2 at triangle %d sample %d, dev there %.6g'
          % (order, len(soup), h, np.abs(dev).max(), np.abs(dev).max() / h ** 2, worst, at[worst], dev[worst]))
    assert dev.shape == at.shape == sumsq.shape == (len(soup),) and at.dtype == np.int32
    assert np.abs(dev).max() <= h * h
    assert dev[worst] < 0
    assert (at >= 0).all() and (at < ref.n_samples(order)).all() and (sumsq >= dev * dev).all()


def test_deviation_definition_details(ns, oracle_lib):
    f = ns['sphere'](1)
    ev = lambda P: oracle_lib.evaluate(f, P)
    tri = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]]])
    W = ref.weights(2)
    assert W.shape == (6, 3) and W[0].tolist() == [1.0, 0.0, 0.0] and W[2].tolist() == [0.0, 0.0, 1.0] and W[5].tolist() == [0.0, 1.0, 0.0]
    Q = ref.sample_points(tri, 2)
    assert np.array_equal(Q[:, 0], tri[:, 0]) and np.array_equal(Q[:, 2], tri[:, 2]) and np.array_equal(Q[:, 5], tri[:, 1])     # sample 0 is corner A
    dev, at, sumsq = ref.deviation(ev, tri, 2)
    V = ev(Q.reshape(-1, 3)).reshape(2, 6)
    # the first triangle: the corners are on the sphere, the edge midpoints inside, all three alike: the FIRST of them stays
    assert at[0] == 1 and dev[0] == V[0, 1] and dev[0] < 0
    # the second: corner A is the centre (-1), corners B and C are +1 outside: not strictly greater, A stays
    assert at[1] == 0 and dev[1] == -1.0
    want = np.zeros(2)
    for s in range(6):
        want = want + V[:, s] * V[:, s]
    assert np.array_equal(ref.bits(sumsq), ref.bits(want))
    # the first NaN replaces the value and stays
    nan_ev = lambda P: np.where(np.asarray(P)[:, 2] == 0.5, np.nan, ev(P).reshape(-1))
    dev, at, sumsq = ref.deviation(nan_ev, tri, 2)
    assert np.isnan(dev[0]) and at[0] == 1 and np.isnan(sumsq[0]) and dev[1] == -1.0
    with pytest.raises(ValueError):
        ref.weights(0)
    with pytest.raises(ValueError):
        ref.weights(9)
    e = ref.deviation(ev, np.zeros((0, 3, 3)), 3)
    assert [len(x) for x in e] == [0, 0, 0]


def test_snap_puts_displaced_sphere_vertices_back(ns, oracle_lib):
    """the mesh's vertices moved off the sphere by up to two grid steps: four Newton steps with tol = 1e-3 x the grid step leave every
    one SNAPPED (the field is the exact distance: one step lands within rounding and the central difference's error)"""
    f = ns['sphere'](1)
    soup, pts, step, bounds = checker_mesh('sphere', f, oracle_lib)
    h = min(step)
    rs = np.random.RandomState(11)
    P = pts + rs.uniform(-1.0, 1.0, size=pts.shape) * (2 * h / np.sqrt(3.0))
    assert np.sqrt(((P - pts) ** 2).sum(axis=1)).max() <= 2 * h
    tol = 1e-3 * h
    q, status, residual, evals = ref.snap(lambda Q: oracle_lib.evaluate(f, Q), P, preview_eps(bounds), tol, 4 * max(step), 4)
    print('sphere snap: %d vertices, %s, |residual| <= %.3g (tol %.3g), evals <= %d, lockstep share %.2f'
          % (len(P), dict(zip(ref.NAMES, np.bincount(status, minlength=5))), np.abs(residual).max(), tol, evals.max(), ref.lockstep_share(evals, 4)))
    assert q.dtype == np.float64 and status.dtype == np.uint8 and residual.dtype == np.float64 and evals.dtype == np.int32
    assert (status == ref.SNAPPED).all() and (np.abs(residual) <= tol).all()
    assert np.abs(np.sqrt((q * q).sum(axis=1)) - 1).max() <= 2 * tol
    assert (evals >= 1).all() and (evals <= 4 * 7 + 1).all() and (evals % 7 <= 1).all()


def test_snap_leaves_the_medial_plane_of_a_plate_alone(ns, oracle_lib):
    """on the medial plane of box((2, 2, 0.12)) the central difference across the plate is 0: away from the rim the vertex is FLAT;
    near the rim the gradient points at the side face, 0.02 and more away, and with max_move = 0.01 the vertex is HELD.  Either way
    it keeps its position."""
    f = ns['box']((2, 2, 0.12))
    rs = np.random.RandomState(5)
    P = np.zeros((400, 3))
    P[:, :2] = rs.uniform(-0.98, 0.98, size=(400, 2))
    q, status, residual, evals = ref.snap(lambda Q: oracle_lib.evaluate(f, Q), P, 1e-4, 1e-5, 0.01, 4)
    print('plate:', dict(zip(ref.NAMES, np.bincount(status, minlength=5))))
    assert set(status.tolist()) == {ref.HELD, ref.FLAT}
    assert np.array_equal(ref.bits(q), ref.bits(P)) and (evals == 7).all()
    assert np.array_equal(ref.bits(residual), ref.bits(oracle_lib.evaluate(f, P).reshape(-1)))


def test_snap_definition_statuses(ns, oracle_lib):
    f = ns['sphere'](1)
    ev = lambda Q: oracle_lib.evaluate(f, Q).reshape(-1)
    P = np.array([[1.2, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.6, 0.0], [0.0, 0.0, 1.0]])
    # the centre of a sphere has no central difference: FLAT; a vertex on the surface is SNAPPED at once, with one evaluation
    q, status, residual, evals = ref.snap(ev, P, 1e-4, 1e-9, 0.3, 4)
    assert status.tolist() == [ref.SNAPPED, ref.FLAT, ref.HELD, ref.SNAPPED] and evals[3] == 1 and evals[1] == 7 and evals[2] == 7
    assert np.array_equal(q[1:], P[1:]) and abs(q[0, 0] - 1) <= 1e-9 and residual[1] == -1.0
    # tol = 0: nothing but an exact zero is SNAPPED
    q, status, residual, evals = ref.snap(ev, P[:1] * np.array([[1.0, 0, 0]]) + np.array([[0.0, 0.3, 0.1]]), 1e-4, 0.0, 1.0, 2)
    assert status[0] in (ref.LEFT, ref.SNAPPED) and evals[0] == 15
    # a field that is NaN beyond a radius: the vertex goes back to where it began
    nan_ev = lambda Q: np.where((np.asarray(Q) ** 2).sum(axis=1) > 1.5, np.nan, ev(Q))
    q, status, residual, evals = ref.snap(nan_ev, np.array([[1.3, 0.0, 0.0], [0.5, 0.0, 0.0]]), 1e-4, 1e-9, 1.0, 4)
    assert status.tolist() == [ref.NAN, ref.SNAPPED] and np.array_equal(q[0], [1.3, 0.0, 0.0]) and np.isnan(residual[0]) and evals[0] == 1
    e = ref.snap(ev, np.zeros((0, 3)), 1e-4, 1e-9, 1.0, 4)
    assert [len(x) for x in e] == [0, 0, 0, 0]


def test_package_restatement_equals_the_definition(ns, oracle_lib):
    f = ns['sphere'](1) & ns['box'](1.5)
    soup, pts, step, bounds = checker_mesh('sphere_box', f, oracle_lib)
    ev = lambda Q: oracle_lib.evaluate(f, Q).reshape(-1)
    nan_ev = lambda Q: np.where(np.asarray(Q)[:, 0] > 0.6, np.nan, ev(Q))
    for e in (ev, nan_ev):
        for order in (1, 2, 5, 8):
            a, b = ref.deviation(e, soup[::3], order), triangle_deviation(e, soup[::3], order)
            assert b[0].dtype == np.float64 and b[1].dtype == np.int32 and b[2].dtype == np.float64
            assert all(ref.same_bits(x, y).all() for x, y in zip(a, b)), order
        assert np.array_equal(ref.sample_points(soup[:5], 3), sample_points(soup[:5], 3))
    rs = np.random.RandomState(3)
    P = np.vstack([pts[::2] + rs.uniform(-0.05, 0.05, size=pts[::2].shape), np.zeros((1, 3)), rs.uniform(-0.9, 0.9, size=(200, 3))])
    h = min(step)
    seen = set()
    for e, par in ((ev, (1e-4, 1e-3 * h, 2 * h, 4)), (ev, (1e-4, 1e-3 * h, 2 * h, 1)), (ev, (1e-4, 1e-3 * h, 0.01 * h, 4)), (ev, (1e-4, 0.0, 2 * h, 4)),
                   (nan_ev, (1e-4, 1e-3 * h, 2 * h, 4))):
        a, b = ref.snap(e, P, *par), vertex_snap(e, P, *par)
        assert b[0].dtype == np.float64 and b[1].dtype == np.uint8 and b[2].dtype == np.float64 and b[3].dtype == np.int32
        assert all(ref.same_bits(x, y).all() for x, y in zip(a, b)), par
        seen |= set(a[1].tolist())
    assert seen == {ref.LEFT, ref.SNAPPED, ref.HELD, ref.FLAT, ref.NAN}
    assert [len(x) for x in triangle_deviation(ev, np.zeros((0, 3, 3)), 2)] == [0, 0, 0]
    assert [len(x) for x in vertex_snap(ev, np.zeros((0, 3)), 1e-4, 0.0, 1.0)] == [0, 0, 0, 0]


def test_abi_and_surface():
    names = ('sdf_mesh_triangle_deviation', 'sdf_mesh_deviation_last_kernel_ms', 'sdf_mesh_snap')
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    lib = engine.load_library()
    for name in names:
        assert name in engine.ABI and re.search(r'\b(int|double)\s+%s\s*\(' % name, hdr) and getattr(lib, name)
    assert engine.ABI_VERSION == 17 and lib.sdf_abi_version() == 17
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == 17
    units = [l.split() for l in open(os.path.join(ROOT, 'sdf_amd', 'csrc', 'build.units')) if l.strip() and not l.lstrip().startswith('#')]
    # the kernels' unit with the interpreters' flags, the last of the kernel units; behind it only the probes' host entries (plain)
    assert units[-2:] == [['sdf_deviation', 'sdf_deviation.hip', 'interp'], ['sdf_probe_out', 'sdf_probe_out.hip', 'plain']]
    import sdf_amd
    assert callable(sdf_amd.deviation) and callable(sdf_amd.deviation_of_soup) and sdf_amd.Deviation is Deviation
    assert callable(d3.SDF3.deviation) and callable(mesh_module.Mesh.deviation) and callable(mesh_module.Mesh.snap)
    assert callable(engine.Mesh.triangle_deviation) and callable(engine.Mesh.snap)
    import ctypes
    assert ctypes.sizeof(engine.SdfSnapStats) == 7 * 8


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = engine.load_library()
    assert lib.sdf_mesh_triangle_deviation(None, None, 2, None, None, None) == 2 and b'sdf_mesh_triangle_deviation' in lib.sdf_last_error()
    assert lib.sdf_mesh_snap(None, None, None, 4, None, None, None, None, None, None) == 2 and b'sdf_mesh_snap' in lib.sdf_last_error()


def test_refusals_without_a_device(tmp_path, monkeypatch):
    for bad in (0, 9, -1, 2.0, True, None, '2'):
        with pytest.raises(ValueError):
            check_order(bad)
    assert check_order(1) == 1 and check_order(np.int64(8)) == 8
    good = dict(eps=1e-4, tol=1e-5, max_move=0.1, iters=4)
    assert check_snap(**good) == [1e-4, 1e-5, 0.1, 4] and check_snap(1e-4, 0.0, 0.0, 1) == [1e-4, 0.0, 0.0, 1]
    for bad in ({'eps': 0.0}, {'eps': -1.0}, {'tol': -1e-9}, {'max_move': -1.0}, {'iters': 0}, {'iters': 2.5}, {'iters': True}, {'eps': float('nan')},
                {'tol': float('inf')}, {'max_move': float('nan')}):
        with pytest.raises(ValueError):
            check_snap(**dict(good, **bad))
    assert check_snap_option(False) is None and check_snap_option(None) is None and check_snap_option(True) == {}
    assert check_snap_option({'tol': 0.0, 'iters': 2}) == {'tol': 0.0, 'iters': 2}
    for bad in ({'tolerance': 1.0}, {'tol': -1.0}, {'iters': 0}, {'eps': 0.0}, 'yes', 1, 2.0):
        with pytest.raises(ValueError):
            check_snap_option(bad)
    # the defaults: the preview's eps, a thousandth of the smallest step, the diagonal of one cluster cell, four passes
    par = snap_params({}, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (0.1, 0.2, 0.2), 4)
    assert par == {'eps': 1e-4 * float(np.sqrt(12.0) / 2), 'tol': 1e-3 * 0.1, 'max_move': float(np.sqrt(np.dot([0.4, 0.8, 0.8], [0.4, 0.8, 0.8]))), 'iters': 4}
    assert snap_params({'iters': 2, 'tol': 0.0}, ((0, 0, 0), (1, 1, 1)), (0.1, 0.1, 0.1))['max_move'] == float(np.sqrt(np.dot([0.1] * 3, [0.1] * 3)))
    # the pipeline refuses a bad snap= before it asks for an engine, and writes no file
    def no_engine(*a, **k):
        raise AssertionError('the engine was reached')
    monkeypatch.setattr(engine, 'get_engine', no_engine)
    for bad in ({'tolerance': 1.0}, {'iters': 0}, 'yes'):
        with pytest.raises(ValueError):
            core.generate_mesh('model', snap=bad)
        with pytest.raises(ValueError):
            core.save(str(tmp_path / 'x.ply'), 'model', snap=bad)
        assert not (tmp_path / 'x.ply').exists()
    from sdf_amd.deviation import deviation
    with pytest.raises(ValueError):
        deviation('model', order=0)
    with pytest.raises(ValueError):
        mesh_module.Mesh(np.zeros((3, 3)), np.array([[0, 1, 2]])).snap('model')                    # no step, no tol


def test_deviation_object():
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]])
    cells = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    dev = np.array([0.25, -0.5, np.nan, 0.125])
    d = Deviation(pts, cells, dev, np.array([0, 4, 1, 2], np.int32), np.array([0.1, 0.6, np.nan, 0.06]), 2)
    assert d.max == 0.5 and d.argmax == 1 and d.outside_max == 0.25 and d.inside_max == -0.5
    # sample 4 of order 2 is i = 1, j = 1: the midpoint of B and C of triangle (0, 1, 3)
    assert np.array_equal(d.worst_point, [1.0, 0.0, 1.0])
    assert d.farther_than(0.2).tolist() == [True, True, False, False] and d.counts == {'finite': 3, 'nan': 1}
    assert d.percentile(100) == 0.5 and d.percentile(0) == 0.125
    area = np.array([2.0, 2.0, 2.0 * np.sqrt(3.0)])
    want = np.sqrt((area * np.array([0.1, 0.6, 0.06]) / 6).sum() / area.sum())
    assert abs(d.rms - want) <= 1e-15 and not d.dev.flags.writeable and d.snap_stats is None
    none = Deviation(pts, cells[:1], [np.nan], np.zeros(1, np.int32), [np.nan], 1)
    assert np.isnan(none.max) and none.argmax is None and none.worst_point is None and none.outside_max == 0.0 and none.inside_max == 0.0
    with pytest.raises(ValueError):
        Deviation(pts, cells, dev[:3], np.zeros(4, np.int32), np.zeros(4), 2)
    with pytest.raises(ValueError):
        Deviation(pts, cells, dev, np.zeros(4, np.int32), np.zeros(4), 9)


def test_built_library_passes_the_isa_check_with_the_new_interpreters():
    """as build() runs it: the two kernels are there, classed as interpreters, with their jump-table dispatch"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_check.py'), engine.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if 'was NOT checked' in r.stderr:      # (nothing to check WITH is not a failed check: build() goes on as well)
        print(r.stderr.strip())
        return
    sys.path.insert(0, ROOT)
    from tools import isa_check
    assert 'k_triangle_deviation' in isa_check.INTERP and 'k_vertex_snap' in isa_check.INTERP
    for k in ('k_triangle_deviation', 'k_vertex_snap'):
        lines = [l for l in r.stdout.split('\n') if k + '<' in l]
        assert len(lines) == 2 and all(l.startswith('interp') for l in lines), (k, lines)          # <double, false> and <double, true>
        assert all(int(re.search(r's_setpc_b64\s+(\d+)', l).group(1)) > 0 for l in lines), lines
    assert [l for l in r.stdout.split('\n') if 'k_gather_soup' in l and l.startswith('plain')]
