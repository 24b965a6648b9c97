"""The definition of the curvature probe (tests/curvature_ref.py) held to analytic truth over analytic evaluators, its statuses, and the
host side of the feature: the package's restatement of the definition, the refusals, the `Curvature` object, the refusals of `save`,
the ABI entries.  No GPU.

The bounds.  The second differences of a smooth field lose O(eps^2) times its fourth derivatives, which for a distance field of
curvature radius R is (eps / R)^2 relative: 1e-6 for R = 1 and 1.6e-5 for R = 0.25 at eps = 1e-3; the rounding of the 19 float64
values adds about 1e-16 / eps^2 = 1e-10.  The bounds below (1e-4 relative for the spheres, 1e-3 absolute for the torus) carry the
constant in front of that; the prints show what is reached."""
import os
import re

import numpy as np
import pytest

import curvature_ref as ref
import probe_cases as pc
from sdf_amd import core, engine, meshfile
from sdf_amd.curvature import Curvature, check_params, quality_of, vertex_curvature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


def unit(n, seed):
    d = np.random.RandomState(seed).normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def sphere_ev(R):
    return lambda P: np.sqrt((P * P).sum(axis=1)) - R


def box_ev(b):
    def ev(P):
        q = np.abs(P) - b
        return np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=1)) + np.minimum(q.max(axis=1), 0.0)
    return ev


def test_abi_has_the_entry_points():
    assert 'sdf_mesh_vertex_curvature' in engine.ABI and 'sdf_mesh_curvature_last_kernel_ms' in engine.ABI
    assert engine.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_mesh_vertex_curvature\s*\(', hdr) and re.search(r'\bdouble\s+sdf_mesh_curvature_last_kernel_ms\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == 17
    lib = engine.load_library()
    assert lib.sdf_abi_version() == 17
    assert lib.sdf_mesh_vertex_curvature and lib.sdf_mesh_curvature_last_kernel_ms       # (the library exports both)
    assert callable(getattr(engine.Mesh, 'vertex_curvature'))
    import sdf_amd
    from sdf_amd import d3, mesh as mesh_module
    assert callable(sdf_amd.curvature) and callable(sdf_amd.curvature_of_soup) and sdf_amd.Curvature is Curvature
    assert callable(d3.SDF3.curvature) and callable(mesh_module.Mesh.curvature)
    units = [l.split() for l in open(os.path.join(ROOT, 'sdf_amd', 'csrc', 'build.units')) if l.strip() and not l.lstrip().startswith('#')]
    assert ['sdf_curvature', 'sdf_curvature.hip', 'interp'] in units and units[-1][0] == 'sdf_probe_out'


def test_entry_point_refuses_null_arguments_without_a_device():
    lib = engine.load_library()
    assert lib.sdf_mesh_vertex_curvature(None, None, 1e-3, None, None, None) == 2
    assert b'sdf_mesh_vertex_curvature' in lib.sdf_last_error()


@pytest.mark.parametrize('R', (1.0, 0.25))
def test_sphere(R):
    P = R * unit(1000, 3)
    curv, status = ref.curvature(sphere_ev(R), P, EPS)
    assert curv.shape == (1000, 4) and curv.dtype == np.float64 and status.dtype == np.uint8 and (status == ref.CURVED).all()
    want = np.array([1 / R, 1 / R ** 2, 1 / R, 1 / R])
    err = np.abs(curv / want - 1).max(axis=0)
    print('sphere R = %g: largest relative error of mean, gauss, k1, k2 = %s' % (R, err))
    assert (err <= 1e-4).all()
    assert (curv[:, 2] >= curv[:, 3]).all()


def test_torus():
    R, r = 1.0, 0.25
    rs = np.random.RandomState(5)
    th, ph = rs.uniform(0, 2 * np.pi, 1000), rs.uniform(0, 2 * np.pi, 1000)
    P = np.stack([(R + r * np.cos(th)) * np.cos(ph), (R + r * np.cos(th)) * np.sin(ph), r * np.sin(th)], axis=1)
    ev = lambda Q: np.sqrt((np.sqrt(Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]) - R) ** 2 + Q[:, 2] * Q[:, 2]) - r
    curv, status = ref.curvature(ev, P, EPS)
    assert (status == ref.CURVED).all()
    k2 = np.cos(th) / (R + r * np.cos(th))
    e1, e2 = np.abs(curv[:, 2] - 1 / r).max(), np.abs(curv[:, 3] - k2).max()
    print('torus (1, 0.25): largest |k1 - 1/r| = %.3g, |k2 - cos t / (R + r cos t)| = %.3g' % (e1, e2))
    assert e1 <= 1e-3 and e2 <= 1e-3
    assert np.abs(curv[:, 0] - 0.5 * (1 / r + k2)).max() <= 1e-3 and np.abs(curv[:, 1] - k2 / r).max() <= 4e-3 + 1e-3     # (k1 dk2 + k2 dk1)
    assert (k2 < 0).any() and (curv[:, 1][k2 < -0.1] < 0).all()          # the inner half of a torus is a saddle


def test_infinite_cylinder():
    r = 0.5
    rs = np.random.RandomState(9)
    a = rs.uniform(0, 2 * np.pi, 1000)
    P = np.stack([r * np.cos(a), r * np.sin(a), rs.uniform(-3, 3, 1000)], axis=1)
    curv, status = ref.curvature(lambda Q: np.sqrt(Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]) - r, P, EPS)
    assert (status == ref.CURVED).all()
    print('cylinder r = 0.5: largest |gauss| = %.3g, |k1 - 1/r| = %.3g, |k2| = %.3g' % (
        np.abs(curv[:, 1]).max(), np.abs(curv[:, 2] - 1 / r).max(), np.abs(curv[:, 3]).max()))
    assert np.abs(curv[:, 1]).max() <= 1e-6 and np.abs(curv[:, 2] - 1 / r).max() <= 1e-4


def test_box_faces_are_exactly_flat():
    b, rs = 0.5, np.random.RandomState(11)
    P = rs.uniform(-b + 2 * EPS, b - 2 * EPS, (600, 3))                  # farther than eps from every edge ...
    face = np.arange(600) % 6
    P[np.arange(600), face // 2] = np.where(face % 2 == 0, b, -b)        # ... on one of the six faces
    curv, status = ref.curvature(box_ev(b), P, EPS)
    assert (status == ref.CURVED).all() and (curv == 0.0).all()
    # within eps of an edge the stencil sees the crease: about 1 / eps
    edge = np.array([[b, b - 0.01, 0.1]])
    c, s = ref.curvature(box_ev(b), edge, 0.05)
    print('box edge at eps = 0.05: k1 = %.4g (1 / eps = 20)' % c[0, 2])
    assert s[0] == ref.CURVED and 5.0 <= c[0, 2] <= 40.0 and abs(c[0, 3]) <= 1e-9


def test_a_cavity_is_negative():
    R = 0.5
    P = R * unit(200, 13)
    curv, status = ref.curvature(lambda Q: R - np.sqrt((Q * Q).sum(axis=1)), P, EPS)
    assert (status == ref.CURVED).all() and (curv[:, 2] < 0).all() and (curv[:, 3] < 0).all() and (curv[:, 0] < 0).all() and (curv[:, 1] > 0).all()
    assert np.abs(curv[:, 2:] * -R - 1).max() <= 1e-4


def test_statuses(ns, oracle_lib):
    f = ns['sphere'](1)
    ev = lambda Q: oracle_lib.evaluate(f, Q)
    P = np.array([[0.0, 0.0, 0.0], [1e200, 0.0, 0.0], [0.6, 0.0, 0.8], [0.0, -1e200, 1e200]])
    curv, status, dbg = ref.curvature(ev, P, EPS, debug=True)
    assert status.tolist() == [ref.FLAT, ref.NAN, ref.CURVED, ref.NAN]
    assert np.isfinite(dbg['values'][:, 0]).all() and np.isinf(dbg['values'][:, 1]).all()       # FLAT: no gradient; NAN: through infinite values
    nan_bits = np.array(np.nan).view(np.uint64)
    assert nan_bits == ref.NAN_BITS == 0x7ff8000000000000
    assert (curv.view(np.uint64)[[0, 1, 3]] == nan_bits).all() and np.isfinite(curv[2]).all()
    g, _ = pc.model('capsule_same_ends', ns)                            # a model that is NaN at every point
    curv, status = ref.curvature(lambda Q: oracle_lib.evaluate(g, Q), P[2:3], EPS)
    assert status.tolist() == [ref.NAN] and (curv.view(np.uint64) == nan_bits).all()
    # a gradient too small to square: L2 == 0 although the values differ -> FLAT; a gradient whose square overflows: L = inf -> FLAT;
    # a denormal L2: (2 L2) L underflows to 0 and the results are 0 / 0 -> NAN again
    curv, status = ref.curvature(lambda Q: 1e-170 * Q[:, 0], P[2:3], EPS)
    assert status.tolist() == [ref.FLAT]
    curv, status = ref.curvature(lambda Q: 1e300 * (Q * Q).sum(axis=1), P[2:3], EPS)
    assert status.tolist() == [ref.FLAT]
    curv, status, dbg = ref.curvature(lambda Q: 1e-160 * (Q[:, 0] + (Q * Q).sum(axis=1)), P[2:3], EPS, debug=True)
    assert np.isfinite(dbg['values']).all() and 0 < (dbg['G'] ** 2).sum() < 1e-300
    assert status.tolist() == [ref.NAN] and (curv.view(np.uint64) == nan_bits).all()
    assert ref.counts(np.array([0, 2, 2, 1, 0, 0], np.uint8)).tolist() == [3, 1, 2]
    e = ref.curvature(ev, np.zeros((0, 3)), EPS)
    assert e[0].shape == (0, 4) and e[1].shape == (0,)


@pytest.mark.parametrize('name', ('ex_example', 'twist', 'ex_blobby', 'grid_torus', 'capsule_same_ends'))
def test_package_restatement_equals_the_definition(name, ns, oracle_lib):
    """over the CPU checker: two smooth models, a trigonometric one, a sampled leaf, a model that is NaN everywhere"""
    f, _ = pc.model(name, ns)
    pts = pc.inputs(name, ns)[1]
    ev = lambda Q: oracle_lib.evaluate(f, Q)
    for eps in (pc.NORMAL_EPS, pc.START):
        a = ref.curvature(ev, pts, eps)
        b = vertex_curvature(ev, pts, eps)
        assert b[0].dtype == np.float64 and b[1].dtype == np.uint8 and b[0].shape == (len(pts), 4)
        assert np.array_equal(ref.bits(a[0]), ref.bits(b[0])) and np.array_equal(a[1], b[1]), (name, eps)
        if name == 'capsule_same_ends':
            assert (a[1] == ref.NAN).all()
        else:
            assert (a[1] == ref.CURVED).any()
    e = vertex_curvature(ev, np.zeros((0, 3)), 1e-3)
    assert e[0].shape == (0, 4) and e[1].shape == (0,)


def test_check_params_refusals():
    assert check_params(1) == 1.0 and isinstance(check_params(1), float)
    for bad in (0.0, -1e-3, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            check_params(bad)
        with pytest.raises(ValueError):
            vertex_curvature(sphere_ev(1.0), np.ones((2, 3)), bad)


def test_curvature_object():
    pts = np.arange(18, dtype=np.float64).reshape(6, 3)
    nan = np.nan
    k1 = np.array([2.0, 0.5, nan, -0.25, 4.0, nan])
    k2 = np.array([1.0, -8.0, nan, -0.5, 4.0, nan])
    curv = np.stack([0.5 * (k1 + k2), k1 * k2, k1, k2], axis=1)
    status = np.array([ref.CURVED, ref.CURVED, ref.FLAT, ref.CURVED, ref.CURVED, ref.NAN], np.uint8)
    c = Curvature(pts, np.array([[0, 1, 2]]), curv, status, {'eps': 0.01})
    assert c.measured.tolist() == [True, True, False, True, True, False]
    assert c.counts == {'CURVED': 4, 'FLAT': 1, 'NAN': 1}
    assert c.min_convex_radius == 0.25 and c.min_concave_radius == 0.125
    assert c.argsharpest == 1 and np.array_equal(c.sharpest_point, pts[1])
    assert c.tighter_than(0.3).tolist() == [False, True, False, False, True, False]           # max(|k1|, |k2|) > 1 / 0.3
    assert c.tighter_than(1e-9).tolist() == [False] * 6 and c.tighter_than(1e9).tolist() == c.measured.tolist()
    assert c.percentile(100) == 4.0 and c.percentile(0) == -0.25 and c.percentile(0, of='k2') == -8.0 and c.percentile(50, of='gauss') == 1.0625      # (gauss: 2, -4, 0.125, 16)
    with pytest.raises(ValueError):
        c.percentile(50, of='k3')
    assert c.params == {'eps': 0.01} and not c.k1.flags.writeable and not c.points.flags.writeable and not c.status.flags.writeable
    assert np.array_equal(c.mean[c.measured], curv[c.measured, 0]) and np.array_equal(c.gauss[c.measured], curv[c.measured, 1])
    q = c.quality('max')
    assert q[[0, 1, 3, 4]].tolist() == [2.0, -8.0, -0.5, 4.0] and np.isnan(q[[2, 5]]).all()
    assert np.array_equal(c.quality('k2')[c.measured], k2[c.measured]) and np.array_equal(quality_of(curv, 'mean')[c.measured], curv[c.measured, 0])
    none = Curvature(pts[:2], np.zeros((0, 3), np.int64), np.full((2, 4), nan), np.array([ref.FLAT, ref.NAN], np.uint8), {})
    assert none.min_convex_radius == np.inf and none.min_concave_radius == np.inf and none.sharpest_point is None
    assert not none.tighter_than(1.0).any() and np.isnan(none.percentile(50))
    with pytest.raises(ValueError):
        Curvature(pts, np.zeros((0, 3)), curv[:3], status, {})


def test_curvature_object_saves_the_quality_column(tmp_path):
    import thickness_ref
    pts = np.array([[0.1, -0.2, 0.3], [1.0 / 3.0, 2.0 ** -30, -0.0], [1e6 + 0.015625, -7.25, 3.0], [0.7, 0.7, -123456.789]])
    cells = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
    curv = np.array([[1.5, 2.0, 2.0, 1.0], [np.nan] * 4, [-1.0 / 3.0, 0.0, 0.0, -2.0 / 3.0], [0.0, -1.0, 1.0, -1.0]])
    c = Curvature(pts, cells, curv, np.array([0, 1, 0, 0], np.uint8), {})
    for which, col in (('mean', curv[:, 0]), ('k2', curv[:, 3]), ('max', np.array([2.0, np.nan, -2.0 / 3.0, 1.0]))):
        c.save(str(tmp_path / 'c.ply'), which)
        p, n, q, cc, head = thickness_ref.parse_ply(str(tmp_path / 'c.ply'))
        assert n is None and head == thickness_ref.ply_header(4, 2, False, True) and np.array_equal(cc, cells)
        assert np.array_equal(q.view(np.int32), col.astype(np.float32).view(np.int32)), which
    with pytest.raises(ValueError):
        c.save(str(tmp_path / 'c.obj'))
    with pytest.raises(ValueError):
        c.save(str(tmp_path / 'c.ply'), 'k3')


def test_save_refuses_curvature_before_meshing(tmp_path, monkeypatch):
    def no_meshing(*a, **k):
        raise AssertionError('meshed was reached')
    monkeypatch.setattr(core, 'meshed', no_meshing)
    for name, kw in (('x.stl', {}), ('x.obj', {}), ('x.off', {}), ('x.ply', {'writer': 'meshio'}), ('x.ply', {'thickness': True}),
                     ('x.ply', {'curvature': 'k3'}), ('x.ply', {'curvature': {'quality': 'mean', 'begin': 1.0}}),
                     ('x.ply', {'curvature': {'eps': 0.0}}), ('x.ply', {'curvature': {'quality': 'sharp'}})):
        with pytest.raises(ValueError):
            core.save(str(tmp_path / name), 'model', **dict({'curvature': 'mean'}, **kw))
        assert not (tmp_path / name).exists()
    with pytest.raises(AssertionError, match='meshed was reached'):     # what is in order gets as far as the meshing
        core.save(str(tmp_path / 'x.ply'), 'model', curvature={'quality': 'max', 'eps': 1e-3})
    assert meshfile.choose_writer('a.ply', None, False, False, True) == 'native' and meshfile.choose_writer('a.PLY', 'native', True, curvature=True) == 'native'
    assert meshfile.choose_writer('a.ply', None, False, True) == 'native' and meshfile.choose_writer('a.stl') == 'stl'      # as before
    with pytest.raises(ValueError, match='not both'):
        meshfile.choose_writer('a.ply', None, False, True, True)
