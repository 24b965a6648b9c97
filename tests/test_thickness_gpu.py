"""The wall-thickness probe on the device (csrc/sdf_thickness.hip, `engine.Mesh.vertex_thickness`, sdf_amd/thickness.py, `save(...,
thickness=True)`): thickness bits, status and steps identical to the definition (tests/thickness_ref.py) run over the same
interpreter (`Engine.eval_points`) and, for the models without libm calls, over the CPU checker; ragged vertex counts through adopted
soups; every status; the files; the refusals.  Every refusal is decided on the host before a launch; no test repeats a device call
that failed."""
import ctypes

import numpy as np
import pytest

import fixtures
import normals_ref
import thickness_ref as ref
from sdf_amd import core, engine
from sdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu

# plain family, trig family (twice), smooth unions, the largest register files
# (opcode coverage lives in the sweep, tests/test_probe_sweep_gpu.py: every tape of the suite goes through this kernel there; these few
# models walk the kernel's own states)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'slots_plain_8_8_p8d8')
LIBM_FREE = ('ex_example', 'ex_blobby', 'torus')
SAMPLES = 2 ** 13
RUNS = ({}, {'t_far': 0.3}, {'max_steps': 4}, {'refine': 0})
_meshes = {}


def meshed(name, ns, eng):
    """(model, parameters, welded points, grid axes) at 2^13 samples: meshed and welded once per model; start = min_step = a quarter
    of the grid step, t_far = the diagonal of the bounds, normal_eps = the preview's"""
    if name not in _meshes:
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
        diagonal = float(np.sqrt(np.dot(hi - lo, hi - lo)))
        X, Y, Z, step = core.grid_axes(bounds, samples=SAMPLES)
        m = eng.generate(f, X, Y, Z, 32, True)
        try:
            pts = m.weld()[0].copy()
        finally:
            m.close()
        pts.setflags(write=False)
        par = dict(normal_eps=1e-4 * float(diagonal / 2), start=min(step) / 4, min_step=min(step) / 4, t_far=diagonal)
        _meshes[name] = (f, par, pts, (X, Y, Z))
    return _meshes[name]


def same(got, want, what=''):
    for g, w, dtype in zip(got, want, (np.float64, np.uint8, np.int32)):
        assert g.dtype == dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    bad = (ref.bits(got[0]) != ref.bits(want[0])) | (got[1] != want[1]) | (got[2] != want[2])
    assert not bad.any(), '%s: %d of %d vertices differ, first at %d: %r / %r' % (
        what, bad.sum(), bad.size, np.flatnonzero(bad)[0], [a[np.flatnonzero(bad)[0]] for a in got], [a[np.flatnonzero(bad)[0]] for a in want])


def counts(status):
    return dict(zip(ref.NAMES, np.bincount(status, minlength=5).tolist()))


class Soup:
    """a float64 soup in device memory (torch owns it) and the Mesh that adopts it"""

    def __init__(self, eng, tris):
        import torch
        self.host = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 9)
        self.buf = torch.from_numpy(self.host.reshape(-1).copy()).to('cuda:0') if len(self.host) else None
        torch.cuda.synchronize()
        self.mesh = eng.adopt_soup(self.buf.data_ptr() if len(self.host) else 0, len(self.host))

    def welded(self):
        return np.unique(self.host.reshape(-1, 3), axis=0)

    def close(self):
        self.mesh.close()


def random_soup(n_tris, seed=7):
    return np.random.RandomState(seed + n_tris).uniform(-1.1, 1.1, size=(n_tris, 9))


@pytest.mark.parametrize('name', MODELS)
def test_thickness_is_bit_identical_to_the_definition(name, ns, eng):
    f, par, pts, (X, Y, Z) = meshed(name, ns, eng)
    assert len(pts) > 256 and len(pts) % 64 != 0
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        got = m.vertex_thickness(f, **par)
    finally:
        m.close()
    want = ref.thickness(lambda P: eng.eval_points(f, P), pts, **par)
    print(name, len(pts), counts(want[1]), 'steps <= %d' % want[2].max(), 'lockstep share %.2f' % ref.lockstep_share(want[2]))
    same(got, want, name)
    assert (want[1] == ref.THICK).any()


@pytest.mark.parametrize('name', LIBM_FREE)
def test_thickness_is_bit_identical_to_the_definition_over_the_checker(name, ns, eng, oracle_lib):
    f, par, pts, (X, Y, Z) = meshed(name, ns, eng)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        got = m.vertex_thickness(f, **par)
    finally:
        m.close()
    same(got, ref.thickness(lambda P: oracle_lib.evaluate(f, P), pts, **par), name)


_seen = {}


@pytest.mark.parametrize('n_tris', (1, 21, 22, 86, 333))
def test_ragged_vertex_counts_through_adopted_soups(n_tris, ns, eng):
    """U = 3, 63, 66, 258, 999: a partial wave, a wave less one lane, a wave plus two lanes, a workgroup plus two lanes, many workgroups;
    each with the defaults, a near t_far, few steps and no refinement.  One vertex of the largest soup is the model's centre (FLAT)."""
    f, par, _, _ = meshed('ex_example', ns, eng)
    tris = random_soup(n_tris)
    if n_tris == 333:
        tris[100, 3:6] = 0.0
    s = Soup(eng, tris)
    try:
        pts = s.welded()
        assert len(pts) == 3 * n_tris
        ev = lambda P: eng.eval_points(f, P)
        for over in RUNS:
            p = dict(par, **over)
            want = ref.thickness(ev, pts, **p)
            same(s.mesh.vertex_thickness(f, **p), want, '%d %r' % (n_tris, over))
            _seen.setdefault(n_tris, []).append((over, want))
    finally:
        s.close()
    if n_tris == 333:
        by_run = {tuple(o): set(w[1].tolist()) for o, w in _seen[333]}
        print({k: sorted(v) for k, v in by_run.items()})
        assert {ref.THICK, ref.THIN, ref.FLAT} <= by_run[()] and ref.OPEN not in by_run[()]
        far = [w for o, w in _seen[333] if o == {'t_far': 0.3}][0]
        assert ((far[1] == ref.OPEN) & (far[2] < 256)).any()                 # OPEN beyond t_far
        few = [w for o, w in _seen[333] if o == {'max_steps': 4}][0]
        assert ((few[1] == ref.OPEN) & (few[2] == 4)).any()                  # OPEN out of steps
        raw = [w for o, w in _seen[333] if o == {'refine': 0}][0]
        full = [w for o, w in _seen[333] if o == {}][0]
        k = full[1] == ref.THICK
        assert np.array_equal(raw[1], full[1]) and np.array_equal(raw[2], full[2]) and (raw[0][k] >= full[0][k]).all() and (raw[0][k] > full[0][k]).any()


def test_a_ray_that_meets_a_nan_is_nan(ns, eng, oracle_lib):
    """`ellipsoid` divides 0 by 0 at its centre and nowhere else, and its field on the x axis inside is |x| - 1.  From (a, 0, 0) the
    direction is exactly (-1, -0, -0).  With start = a the first evaluation of the march is AT the centre; from (0.75, 0, 0) with
    start = 0.25 the first one is at x = 0.5, the field there is -0.5 and the second one is at the centre."""
    f = ns['ellipsoid']((1, 1, 1))
    assert np.isnan(oracle_lib.evaluate(f, np.zeros((1, 3)))[0]) and np.isnan(eng.eval_points(f, np.zeros((1, 3)))[0])
    tris = random_soup(30)
    tris[:, :] = np.where(np.abs(tris) < 0.05, 0.05, tris)
    tris[7, 0:3] = (0.5, 0.0, 0.0)
    tris[8, 0:3] = (0.75, 0.0, 0.0)
    tris[19, 6:9] = (0.0, -0.25, 0.0)
    s = Soup(eng, tris)
    nan_steps = set()
    try:
        pts = s.welded()
        for par in (dict(normal_eps=1e-4, start=0.5, min_step=0.5, t_far=4.0), dict(normal_eps=1e-4, start=0.25, min_step=0.125, t_far=4.0)):
            want = ref.thickness(lambda P: eng.eval_points(f, P), pts, **par)
            assert (want[1] == ref.NAN).sum() >= 1 and (want[1] != ref.NAN).sum() >= 80, counts(want[1])
            nan_steps |= set(want[2][want[1] == ref.NAN].tolist())
            same(s.mesh.vertex_thickness(f, **par), want, repr(par))
            same(want, ref.thickness(lambda P: oracle_lib.evaluate(f, P), pts, **par), 'checker')
    finally:
        s.close()
    assert nan_steps == {1, 2}, nan_steps                      # on the first pass and on a later one


def test_empty_mesh(ns, eng):
    s = Soup(eng, np.zeros((0, 9)))
    try:
        th, status, steps = s.mesh.vertex_thickness(ns['sphere'](1), 1e-4, 0.01, 0.01, 4.0)
        assert th.shape == status.shape == steps.shape == (0,)
    finally:
        s.close()


def test_simplified_and_mended_meshes_are_served(ns, eng):
    f, par, pts, (X, Y, Z) = meshed('ex_example', ns, eng)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        small = m.simplify(np.array([X[0], Y[0], Z[0]]), np.full(3, 2 * (X[1] - X[0])))
        try:
            mended = small.mend()
            try:
                for mesh in (small, mended):
                    p = dict(par, start=4 * par['start'])         # (the vertices of a simplified mesh lie off the surface)
                    same(mesh.vertex_thickness(f, **p), ref.thickness(lambda P: eng.eval_points(f, P), mesh.weld()[0], **p))
            finally:
                mended.close()
        finally:
            small.close()
    finally:
        m.close()


def test_plate_end_to_end(tmp_path, ns, eng):
    f = ns['box']((2, 2, 0.12))
    t = f.thickness(step=0.05, verbose=False)
    assert t.thickness.shape == (len(t.points),) and t.cells.shape[1] == 3 and t.params['start'] == t.params['min_step'] == 0.0125
    bounds = eng.estimate_bounds(f)
    lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
    assert t.params['t_far'] == float(np.sqrt(np.dot(hi - lo, hi - lo))) and t.params['normal_eps'] == 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    same((t.thickness, t.status, t.steps), ref.thickness(lambda P: eng.eval_points(f, P), t.points, **t.params))
    face = (np.abs(t.points[:, 0]) < 0.85) & (np.abs(t.points[:, 1]) < 0.85)
    assert face.sum() > 256 and (t.status[face] == ref.THICK).all()
    err = np.abs(t.thickness[face] - 0.12).max()
    print('plate: %d vertices, %d on the faces, largest |thickness - 0.12| there %.3g; %r' % (len(t.points), face.sum(), err, t))
    assert err <= 0.12 * 2.0 ** -16 + 1e-12 and abs(t.thickness[face].min() - 0.12) <= 0.12 * 2.0 ** -16 + 1e-12
    assert t.counts['THICK'] == (t.status == ref.THICK).sum() and t.min <= 0.12 + 0.12 * 2.0 ** -16 + 1e-12

    # the file: the quality column is the float32 cast of the same numbers, with and without normals
    f.save(str(tmp_path / 'q.ply'), thickness=True, step=0.05, verbose=False)
    p, n, q, c, head = ref.parse_ply(str(tmp_path / 'q.ply'))
    assert n is None and head == ref.ply_header(len(t.points), len(t.cells), False, True) and np.array_equal(c, t.cells)
    assert np.array_equal(p.view(np.int32), t.points.astype(np.float32).view(np.int32))
    assert np.array_equal(q.view(np.int32), t.thickness.astype(np.float32).view(np.int32))
    f.save(str(tmp_path / 'qn.ply'), thickness=True, normals=True, step=0.05, verbose=False)
    p, n, q2, c, head = ref.parse_ply(str(tmp_path / 'qn.ply'))
    nrm = normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), t.points, t.params['normal_eps'])[0]
    assert head == ref.ply_header(len(t.points), len(t.cells), True, True) and np.array_equal(q2.view(np.int32), q.view(np.int32))
    assert np.array_equal(n.view(np.int32), nrm.astype(np.float32).view(np.int32))
    t.save(str(tmp_path / 't.ply'))
    assert (tmp_path / 't.ply').read_bytes() == (tmp_path / 'q.ply').read_bytes()

    # a FILE measured in the field: the STL holds float32 vertices, and the definition is taken at those
    f.save(str(tmp_path / 's.stl'), step=0.05, verbose=False)
    file_mesh = Mesh.from_stl(str(tmp_path / 's.stl'))
    ft = file_mesh.thickness(f, step=0.05)
    assert np.array_equal(ft.points, file_mesh.points) and ft.params['start'] == 0.0125
    same((ft.thickness, ft.status, ft.steps), ref.thickness(lambda P: eng.eval_points(f, P), file_mesh.points, **ft.params))
    with pytest.raises(ValueError, match='step'):
        file_mesh.thickness(f)


def test_save_with_normals_is_unchanged_by_a_thickness_call(tmp_path, ns, eng):
    f, par, pts, (X, Y, Z) = meshed('ex_example', ns, eng)
    f.save(str(tmp_path / 'a.ply'), normals=True, samples=SAMPLES, verbose=False)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        eps = par['normal_eps']
        m.vertex_normals(f, eps)
        before = [a.copy() for a in m.ply_records(normals=True)]
        m.vertex_thickness(f, **par)
        after = m.ply_records(normals=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        m.close()
    f.thickness(samples=SAMPLES, verbose=False)
    f.save(str(tmp_path / 'b.ply'), normals=True, samples=SAMPLES, verbose=False)
    assert (tmp_path / 'a.ply').read_bytes() == (tmp_path / 'b.ply').read_bytes()
    assert (tmp_path / 'a.ply').read_bytes().endswith(before[0].tobytes() + before[1].tobytes())


def test_a_model_with_closures_takes_the_definition_on_the_host(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    X, Y, Z, step = core.grid_axes(((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), samples=SAMPLES)
    par = dict(normal_eps=1e-4, start=min(step) / 4, min_step=min(step) / 4, t_far=4.0)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        pts = m.weld()[0]
        dt = eng.tape_for(f)
        out = (np.zeros(len(pts)), np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.int32))
        p6 = np.array([par['normal_eps'], par['start'], par['min_step'], par['t_far'], 1.0, 0.0])
        rc = eng.lib.sdf_mesh_vertex_thickness(m.handle, dt.handle, p6.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 256, 16,
                                               out[0].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out[1].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                               out[2].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc == 2 and b'closures' in eng.lib.sdf_last_error() and b'sdf_mesh_vertex_thickness' in eng.lib.sdf_last_error()
        got = m.vertex_thickness(f, **par)
        same(got, ref.thickness(lambda P: eng.eval_points(f, P), pts, **par))
        assert (got[1] == ref.THICK).all() and np.isfinite(got[0]).all()
    finally:
        m.close()


def test_refusals(ns, eng):
    f = ns['sphere'](1)
    lib = eng.lib
    s = Soup(eng, random_soup(4))
    other = engine.Engine(0)                                    # a second context on the same device
    odt = other.tape_for(f)
    try:
        dt = eng.tape_for(f)
        th, status, steps = np.zeros(12), np.zeros(12, np.uint8), np.zeros(12, np.int32)
        f64p, u8p, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)

        def call(mesh, tape, p6, max_steps=256, refine=16):
            p6 = np.array(p6, np.float64)
            return lib.sdf_mesh_vertex_thickness(mesh, tape, p6.ctypes.data_as(f64p), max_steps, refine, th.ctypes.data_as(f64p),
                                                 status.ctypes.data_as(u8p), steps.ctypes.data_as(i32p))
        good = [1e-4, 0.01, 0.01, 4.0, 1.0, 0.0]
        assert call(s.mesh.handle, dt.handle, good) == 2 and b'sdf_mesh_weld first' in lib.sdf_last_error()      # before the weld
        assert s.mesh._welded() == 12
        for bad, word in (([0.0, 0.01, 0.01, 4.0, 1.0, 0.0], b'normal_eps'), ([1e-4, 0.0, 0.01, 4.0, 1.0, 0.0], b'start'),
                          ([1e-4, 0.01, -1.0, 4.0, 1.0, 0.0], b'min_step'), ([1e-4, 0.01, 0.01, 4.0, 2.0, 0.0], b'step_scale'),
                          ([1e-4, 0.01, 0.01, 4.0, 0.0, 0.0], b'step_scale'), ([1e-4, 0.01, 0.01, 0.005, 1.0, 0.0], b't_far'),
                          ([1e-4, 0.01, 0.01, float('inf'), 1.0, 0.0], b'finite'), ([float('nan'), 0.01, 0.01, 4.0, 1.0, 0.0], b'finite'),
                          ([1e-4, 0.01, 0.01, 4.0, 1.0, float('nan')], b'finite')):
            assert call(s.mesh.handle, dt.handle, bad) == 2 and word in lib.sdf_last_error(), (bad, lib.sdf_last_error())
            assert b'sdf_mesh_vertex_thickness' in lib.sdf_last_error()
        assert call(s.mesh.handle, dt.handle, good, max_steps=0) == 2 and b'max_steps' in lib.sdf_last_error()
        assert call(s.mesh.handle, dt.handle, good, refine=-1) == 2 and b'refine' in lib.sdf_last_error()
        assert call(s.mesh.handle, None, good) == 2 and call(None, dt.handle, good) == 2
        assert lib.sdf_mesh_vertex_thickness(s.mesh.handle, dt.handle, None, 256, 16, th.ctypes.data_as(f64p), status.ctypes.data_as(u8p), steps.ctypes.data_as(i32p)) == 2
        assert call(s.mesh.handle, odt.handle, good) == 2 and b'different contexts' in lib.sdf_last_error()
        assert not th.any() and not status.any() and not steps.any()
        for bad in ({'start': 0.0}, {'step_scale': 2.0}, {'t_far': 0.005}, {'max_steps': 0}, {'refine': -1}, {'min_step': float('nan')}):
            with pytest.raises(ValueError):
                s.mesh.vertex_thickness(f, **dict(dict(normal_eps=1e-4, start=0.01, min_step=0.01, t_far=4.0), **bad))
        eng.precision = engine.PRECISION_F32
        try:
            with pytest.raises(ValueError, match='float32'):
                s.mesh.vertex_thickness(f, 1e-4, 0.01, 0.01, 4.0)
        finally:
            eng.precision = engine.PRECISION_F64
        with pytest.raises(ValueError):
            f.thickness(start=0.0, samples=SAMPLES, verbose=False)
        # ... and the mesh serves the call that is in order
        same(s.mesh.vertex_thickness(f, 1e-4, 0.01, 0.01, 4.0), ref.thickness(lambda P: eng.eval_points(f, P), s.welded(), 1e-4, 0.01, 0.01, 4.0))
        assert lib.sdf_mesh_thickness_last_kernel_ms() > 0
    finally:
        s.close()
        odt._fin()
        other._fin()
