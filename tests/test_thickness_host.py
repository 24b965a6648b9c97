"""The definition of the wall-thickness probe (tests/thickness_ref.py) over the CPU checker, and the host side of the feature: the ABI
entries, the package's restatement of the definition, the `quality` column of the PLY writer, the `Thickness` object, the refusals of
`save`.  No GPU.  Meshes: `oracle.generate` at 2^13 samples welded by np.unique; start = min_step = a quarter of the grid step,
t_far = the diagonal of the bounds, normal_eps = the preview's (1e-4 x the half-diagonal)."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixtures
import normals_ref
import thickness_ref as ref
from sdf_amd import core, engine, meshfile
from sdf_amd.thickness import Thickness, vertex_thickness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = 2 ** 13
REFINE = 16
_cache = {}


def model(name, ns):
    if name == 'plate':
        return ns['box']((2, 2, 0.12))
    return ns['sphere'](1) if name == 'sphere' else fixtures.build(name, ns)


def probed(name, ns, oracle):
    """the welded checker mesh of a model, the default parameters and the definition's result with its debug values: once per model"""
    if name not in _cache:
        f = model(name, ns)
        bounds = oracle.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=SAMPLES)
        pts = np.unique(oracle.generate(f, X, Y, Z, 32, True).points, axis=0)
        lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
        diagonal = float(np.sqrt(np.dot(hi - lo, hi - lo)))
        par = dict(normal_eps=1e-4 * diagonal / 2, start=min(step) / 4, min_step=min(step) / 4, t_far=diagonal)
        ev = lambda P: oracle.evaluate(f, P)
        th, status, steps, dbg = ref.thickness(ev, pts, refine=REFINE, debug=True, **par)
        for a in (pts, th, status, steps) + tuple(dbg.values()):
            a.setflags(write=False)
        _cache[name] = dict(f=f, ev=ev, pts=pts, par=par, diagonal=diagonal, th=th, status=status, steps=steps, dbg=dbg)
    return _cache[name]


def test_abi_has_the_entry_points():
    assert 'sdf_mesh_vertex_thickness' in engine.ABI and 'sdf_mesh_thickness_last_kernel_ms' in engine.ABI
    assert engine.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_mesh_vertex_thickness\s*\(', hdr) and re.search(r'\bdouble\s+sdf_mesh_thickness_last_kernel_ms\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == 17
    lib = engine.load_library()
    assert lib.sdf_abi_version() == 17
    assert lib.sdf_mesh_vertex_thickness and lib.sdf_mesh_thickness_last_kernel_ms       # (the library exports both)
    assert callable(getattr(engine.Mesh, 'vertex_thickness'))


def test_entry_point_refuses_null_arguments_without_a_device():
    lib = engine.load_library()
    assert lib.sdf_mesh_vertex_thickness(None, None, None, 256, 16, None, None, None) == 2
    assert b'sdf_mesh_vertex_thickness' in lib.sdf_last_error()


def test_sphere_thickness_is_the_chord_through_the_centre(ns, oracle_lib):
    m = probed('sphere', ns, oracle_lib)
    assert len(m['pts']) == 1722 and (m['status'] == ref.THICK).all() and m['steps'].max() <= 9
    # the ray from p runs through the centre to the far side: 1 + |p|.  The last bracket of the march is no longer than one advance,
    # an advance is below t_far (the diagonal), and `refine` bisections halve it each time
    err = np.abs(m['th'] - (1 + np.sqrt((m['pts'] ** 2).sum(axis=1)))).max()
    print('sphere: largest |thickness - (1 + |p|)| = %.3g, bound %.3g' % (err, 2.0 ** -REFINE * m['diagonal']))
    assert err <= 2.0 ** -REFINE * m['diagonal']


def test_plate_thickness_at_the_face_vertices(ns, oracle_lib):
    m = probed('plate', ns, oracle_lib)
    face = (np.abs(m['pts'][:, 0]) < 0.85) & (np.abs(m['pts'][:, 1]) < 0.85)
    assert len(m['pts']) == 2870 and face.sum() == 1800 and (m['status'][face] == ref.THICK).all()
    err = np.abs(m['th'][face] - 0.12).max()
    print('plate: largest |thickness - 0.12| at the face vertices = %.3g, bound %.3g; steps there <= %d, overall <= %d'
          % (err, 0.12 * 2.0 ** -16 + 1e-12, m['steps'][face].max(), m['steps'].max()))
    assert err <= 0.12 * 2.0 ** -16 + 1e-12              # the bracket is at most the thickness
    assert m['steps'][face].max() <= 5


@pytest.mark.parametrize('name', ('sphere', 'torus', 'ex_example', 'ex_blobby', 'twist', 'ex_knurling'))
def test_definition_is_consistent(name, ns, oracle_lib):
    m = probed(name, ns, oracle_lib)
    P, th, status, steps, dbg, ev = m['pts'], m['th'], m['status'], m['steps'], m['dbg'], m['ev']
    U = len(P)
    assert th.dtype == np.float64 and status.dtype == np.uint8 and steps.dtype == np.int32
    assert th.shape == status.shape == steps.shape == (U,) and dbg['D'].shape == (U, 3)
    assert (steps <= 256).all() and (steps >= 0).all() and (status <= ref.NAN).all()
    k = status == ref.THICK
    assert k.any()
    D, lo, hi = dbg['D'], dbg['lo'], dbg['hi']
    assert np.array_equal(ref.bits(th[k]), ref.bits(hi[k]))
    assert (ev(P[k] + th[k][:, None] * D[k]) >= 0).all()                       # outside again at the thickness
    assert (ev(P[k] + lo[k][:, None] * D[k]) < 0).all()                        # still solid at lo
    # `refine` bisections of the march's bracket.  Each midpoint 0.5 * (lo + hi) is rounded once, by at most half a unit of hi in the
    # last place, so a half can exceed the exact half by that much: `refine` units are allowed over bracket * 2^-refine.
    assert (hi[k] - lo[k] <= dbg['bracket'][k] * 2.0 ** -REFINE + REFINE * np.spacing(hi[k])).all()
    assert (dbg['bracket'][k] > 0).all() and (steps[k] >= 2).all()
    assert np.isposinf(th[status == ref.OPEN]).all()
    assert np.isnan(th[(status == ref.FLAT) | (status == ref.NAN)]).all() and (steps[status == ref.FLAT] == 0).all()
    assert (th[status == ref.THIN] == m['par']['start']).all() and (steps[status == ref.THIN] == 1).all()
    print('%s: %d vertices, %s, steps <= %d, thickness %.4g .. %.4g, lockstep share %.2f'
          % (name, U, dict(zip(ref.NAMES, np.bincount(status, minlength=5))), steps.max(), th[k].min(), th[k].max(), ref.lockstep_share(steps)))


def test_every_status_occurs(ns, oracle_lib):
    m = probed('ex_example', ns, oracle_lib)
    P = np.random.RandomState(7).uniform(-1.1, 1.1, size=(999, 3))
    runs = {'default': {}, 't_far': {'t_far': 0.3}, 'max_steps': {'max_steps': 4}}
    got = {}
    for key, over in runs.items():
        th, status, steps = ref.thickness(m['ev'], P, **dict(m['par'], **over))
        got[key] = (th, status, steps)
        print(key, dict(zip(ref.NAMES, np.bincount(status, minlength=5))))
    th, status, steps = got['default']
    assert (status == ref.THICK).any() and (status == ref.THIN).any() and not (status == ref.OPEN).any()
    th, status, steps = got['t_far']                            # OPEN because the ray passed t_far ...
    far = status == ref.OPEN
    assert far.any() and (steps[far] < 256).all() and np.isposinf(th[far]).all()
    th, status, steps = got['max_steps']                        # ... and OPEN because the steps ran out
    out = status == ref.OPEN
    assert out.any() and (steps[out] == 4).all() and np.isposinf(th[out]).all() and (steps <= 4).all()
    # no gradient at the centre of a box
    g = ns['box'](1)
    th, status, steps = ref.thickness(lambda Q: oracle_lib.evaluate(g, Q), np.array([[0.0, 0.0, 0.0], [0.5, 0.1, 0.2]]), 1e-4, 0.01, 0.01, 4.0)
    assert status.tolist() == [ref.FLAT, ref.THICK] and np.isnan(th[0]) and steps[0] == 0 and abs(th[1] - 1.0) <= 4.0 * 2.0 ** -16
    # a field that is NaN beyond a radius: the ray from inside runs into it
    s = ns['sphere'](1)
    ev = lambda Q: np.where((np.asarray(Q) ** 2).sum(axis=1) > 0.36, np.nan, oracle_lib.evaluate(s, Q).reshape(-1))
    th, status, steps = ref.thickness(ev, np.array([[0.3, 0.0, 0.0], [0.0, 0.0, 0.5]]), 1e-4, 0.01, 0.01, 4.0)
    assert status.tolist() == [ref.NAN, ref.NAN] and np.isnan(th).all() and (steps >= 2).all()


def test_package_restatement_equals_the_definition(ns, oracle_lib):
    m = probed('ex_example', ns, oracle_lib)
    P = np.vstack([m['pts'][::3], np.zeros((1, 3)), np.random.RandomState(7).uniform(-1.1, 1.1, size=(200, 3))])
    nan_ev = lambda Q: np.where(np.asarray(Q)[:, 0] > 0.7, np.nan, m['ev'](Q).reshape(-1))
    seen = set()
    for ev, over in ((m['ev'], {}), (m['ev'], {'t_far': 0.3}), (m['ev'], {'max_steps': 4}), (m['ev'], {'refine': 0}),
                     (m['ev'], {'step_scale': 0.5}), (nan_ev, {})):
        par = dict(m['par'], **over)
        a = ref.thickness(ev, P, **par)
        b = vertex_thickness(ev, P, **par)
        assert b[0].dtype == np.float64 and b[1].dtype == np.uint8 and b[2].dtype == np.int32
        assert np.array_equal(ref.bits(a[0]), ref.bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), over
        seen |= set(a[1].tolist())
    assert seen == {ref.OPEN, ref.THICK, ref.THIN, ref.FLAT, ref.NAN}
    e = vertex_thickness(m['ev'], np.zeros((0, 3)), **m['par'])
    assert [len(x) for x in e] == [0, 0, 0]
    for bad in ({'start': 0.0}, {'min_step': -1.0}, {'normal_eps': 0.0}, {'step_scale': 2.0}, {'step_scale': 0.0}, {'t_far': 1e-9},
                {'t_far': float('inf')}, {'start': float('nan')}, {'max_steps': 0}, {'refine': -1}):
        with pytest.raises(ValueError):
            vertex_thickness(m['ev'], P, **dict(m['par'], **bad))


PTS = np.array([[0.1, -0.2, 0.3], [1.0 / 3.0, 2.0 ** -30, -0.0], [1e6 + 0.015625, -7.25, 3.0], [0.7, 0.7, -123456.789]])
CELLS = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
NRM = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [1.0 / 3.0, 2.0 / 3.0, -2.0 / 3.0], [0.0, 0.0, 0.0]])
QUAL = np.array([0.12, np.inf, np.nan, 1.0 / 3.0])


@pytest.mark.parametrize('with_normals', (False, True))
def test_ply_quality_column(tmp_path, with_normals):
    nrm = NRM if with_normals else None
    w = 7 if with_normals else 4
    vb, fb = meshfile.ply_records(PTS, CELLS, nrm, quality=QUAL)
    assert vb.dtype == np.uint8 and len(vb) == 4 * 4 * w
    v = vb.view('<f4').reshape(4, w)
    assert np.array_equal(v[:, :3].view(np.int32), PTS.astype(np.float32).view(np.int32))
    if with_normals:
        assert np.array_equal(v[:, 3:6].view(np.int32), NRM.astype(np.float32).view(np.int32))
    assert np.array_equal(v[:, w - 1].view(np.int32), QUAL.astype(np.float32).view(np.int32))       # inf and nan as they are
    want = ['ply', 'format binary_little_endian 1.0', 'comment sdf_amd', 'element vertex 4', 'property float x', 'property float y',
            'property float z'] + (['property float nx', 'property float ny', 'property float nz'] if with_normals else []) + \
           ['property float quality', 'element face 2', 'property list uchar int vertex_indices', 'end_header']
    assert meshfile.ply_header(4, 2, with_normals, quality=True) == ('\n'.join(want) + '\n').encode()
    assert meshfile.ply_header(4, 2, with_normals, quality=True) == ref.ply_header(4, 2, with_normals, True)
    # without quality: byte for byte what the export's definition says, as before
    for q in ({}, {'quality': None}):
        assert meshfile.ply_header(4, 2, with_normals, **q) == normals_ref.ply_header(4, 2, with_normals)
        pv, pf = meshfile.ply_records(PTS, CELLS, nrm, **q)
        wv, wf = normals_ref.ply_records(PTS, CELLS, nrm)
        assert np.array_equal(pv, wv) and np.array_equal(pf, wf) and np.array_equal(pf, fb)
    path = str(tmp_path / 'q.ply')
    meshfile.write_ply(path, vb, fb, 4, 2, with_normals, quality=True)
    p, n, q, c, head = ref.parse_ply(path)
    assert head == ref.ply_header(4, 2, with_normals, True) and np.array_equal(c, CELLS)
    assert np.array_equal(q.view(np.int32), QUAL.astype(np.float32).view(np.int32)) and (n is not None) == with_normals
    with pytest.raises(ValueError):
        meshfile.write_ply(path, vb, fb, 4, 2, with_normals)                  # the records are too long for a file without quality
    with pytest.raises(ValueError):
        meshfile.ply_records(PTS, CELLS, nrm, quality=QUAL[:3])


def test_save_refuses_thickness_in_other_formats_before_meshing(tmp_path, monkeypatch):
    def no_meshing(*a, **k):
        raise AssertionError('meshed was reached')
    monkeypatch.setattr(core, 'meshed', no_meshing)
    for name, kw in (('x.stl', {}), ('x.obj', {}), ('x.obj', {'normals': True}), ('x.ply', {'writer': 'meshio'}), ('x.off', {}),
                     ('x.ply', {'thickness': {'start': 0.0}}), ('x.ply', {'thickness': {'begin': 1.0}})):
        with pytest.raises(ValueError):
            core.save(str(tmp_path / name), 'model', **dict({'thickness': True}, **kw))
        assert not (tmp_path / name).exists()
    assert meshfile.choose_writer('a.ply', None, False, True) == 'native' and meshfile.choose_writer('a.PLY', 'native', True, True) == 'native'


def test_thickness_object():
    pts = np.arange(21, dtype=np.float64).reshape(7, 3)
    th = np.array([0.5, np.inf, 0.25, np.nan, 0.125, np.nan, 0.75])
    status = np.array([ref.THICK, ref.OPEN, ref.THIN, ref.FLAT, ref.THICK, ref.NAN, ref.THICK], np.uint8)
    t = Thickness(pts, np.array([[0, 1, 2]]), th, status, np.arange(7, dtype=np.int32), {'start': 0.25})
    assert t.min == 0.125 and t.argmin == 4 and np.array_equal(t.thinnest_point, pts[4])
    assert t.thinner_than(0.5).tolist() == [False, False, True, False, True, False, False]
    assert t.thinner_than(10.0).tolist() == [True, False, True, False, True, False, True]
    assert t.counts == {'OPEN': 1, 'THICK': 3, 'THIN': 1, 'FLAT': 1, 'NAN': 1}
    assert t.percentile(0) == 0.125 and t.percentile(100) == 0.75 and t.percentile(50) == 0.375
    assert t.params == {'start': 0.25} and not t.thickness.flags.writeable
    none = Thickness(pts[:2], np.zeros((0, 3), np.int64), [np.inf, np.nan], np.array([ref.OPEN, ref.FLAT], np.uint8), np.zeros(2, np.int32), {})
    assert np.isnan(none.min) and none.argmin is None and none.thinnest_point is None and not none.thinner_than(1.0).any()
    with pytest.raises(ValueError):
        Thickness(pts, np.zeros((0, 3)), th[:3], status, np.zeros(7, np.int32), {})


def test_thickness_object_saves_the_quality_column(tmp_path):
    t = Thickness(PTS, CELLS, QUAL, np.array([ref.THICK, ref.OPEN, ref.FLAT, ref.THICK], np.uint8), np.zeros(4, np.int32), {})
    t.save(str(tmp_path / 't.ply'))
    p, n, q, c, head = ref.parse_ply(str(tmp_path / 't.ply'))
    assert n is None and head == ref.ply_header(4, 2, False, True) and np.array_equal(c, CELLS)
    assert np.array_equal(p.view(np.int32), PTS.astype(np.float32).view(np.int32))
    assert np.array_equal(q.view(np.int32), QUAL.astype(np.float32).view(np.int32))
    with pytest.raises(ValueError):
        t.save(str(tmp_path / 't.obj'))
