"""The definition of tests/supports_ref.py against constructed cases, over the CPU checker (no GPU): the shelf
with the numbers worked out by hand, the inequalities that hold for every model, hidden faces, every status, the empty cases, the
package's restatement bit for bit, the `Supports` record, the refusals of the Python entry points, the ABI."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import fixtures
import overhang_ref
import supports_ref as ref
from sdf_amd import core

pkg = importlib.import_module('sdf_amd.supports')      # (the package's attribute `supports` is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
SAMPLES = 2 ** 13
NAMES = ('sdf_mesh_support_rays', 'sdf_support_rays_fetch', 'sdf_support_rays_destroy', 'sdf_mesh_supports_last_kernel_ms')
_meshes = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def shelf(ns, base=True):
    """a plate 0.2 thick on the bed, a post 0.5 x 0.5, and a second plate whose underside is at z = 1.0, 0.8 above the first"""
    box = ns['box']
    f = box((0.5, 0.5, 1.0)).translate((0, 0, 0.6)) | box((2, 2, 0.2)).translate((0, 0, 1.1))
    return f | box((2, 2, 0.2)).translate((0, 0, 0.1)) if base else f


def meshed(key, f, oracle_lib):
    """(soup (T, 3, 3), start = min_step, bed_tol) of a model at 2^13 samples over the checker, once per model"""
    if key not in _meshes:
        bounds = oracle_lib.estimate_bounds(f)
        Xs, Ys, Zs, step = core.grid_axes(bounds, samples=SAMPLES)
        soup = oracle_lib.generate(f, Xs, Ys, Zs, 32, True).points.reshape(-1, 3, 3).copy()
        soup.setflags(write=False)
        _meshes[key] = (soup, float(min(step)) / 4, float(max(step)))
    return _meshes[key]


def run(oracle_lib, f, soup, d, angle, bed_tol, start, **kw):
    d = overhang_ref.normalise(d)[0]
    return ref.supports(lambda P: oracle_lib.evaluate(f, P), soup, d, overhang_ref.sin_limit_of(angle), bed_tol, start, kw.pop('min_step', start), **kw)


def proxy_terms(r):
    """proj * tb over the rays that are not buried, +0.0 for the others"""
    return np.where(r['status'] != ref.BURIED, r['proj'] * r['tb'], 0.0)[:, None]


# ---- the ABI ----
def test_abi_names_are_bound_declared_and_exported():
    from sdf_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    lib = engine.load_library()
    for name in NAMES:
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name), name
    assert engine.ABI_VERSION == 17 and lib.sdf_abi_version() == 17
    assert re.search(r'typedef struct sdf_support_rays sdf_support_rays;', hdr)


def test_null_arguments_are_refused_without_a_device():
    from sdf_amd import engine
    lib = engine.load_library()
    h = ctypes.c_void_p()
    assert lib.sdf_mesh_support_rays(None, None, None, 1, None, 256, 16, ctypes.byref(h), None, None) == 2
    assert b'sdf_mesh_support_rays' in lib.sdf_last_error() and b'NULL' in lib.sdf_last_error() and not h.value
    assert lib.sdf_support_rays_fetch(None, 0, None, None, None, None, None) == 2 and b'sdf_support_rays_fetch' in lib.sdf_last_error()
    assert lib.sdf_support_rays_destroy(None) == 0
    assert lib.sdf_mesh_supports_last_kernel_ms(None) == 0.0


# ---- the shelf ----
def test_the_shelf_upright(ns, oracle_lib):
    f = shelf(ns)
    soup, start, tol = meshed('shelf', f, oracle_lib)
    r = run(oracle_lib, f, soup, Z, 45, tol, start)
    v = ref.derive(r)
    counts = dict(zip(ref.NAMES, r['counts'].tolist()))
    o = r['origin']
    margin = 2 * tol                                              # two grid steps
    under = (np.abs(o[:, 0]) < 1 - margin) & (np.abs(o[:, 1]) < 1 - margin) & (np.maximum(np.abs(o[:, 0]), np.abs(o[:, 1])) > 0.25 + margin)
    err = np.abs(r['height'][under] - 0.8).max()
    print('shelf +z: %r, volume %.6g (on the part %.6g), proxy %.6g; %d rays under the plate, largest |height - 0.8| %.3g'
          % (counts, v['support_volume'], v['on_part_volume'], overhang_ref.overhangs(soup, Z, 45, tol)['support_volume'][0], under.sum(), err))
    assert counts['BED'] == 0 and counts['NAN'] == 0 and counts['UNRESOLVED'] == 0 and r['counts'].sum() == len(r['triangle'])
    assert under.sum() > 100 and (r['status'][under] == ref.PART).all()
    assert err <= 0.8 * 2.0 ** -16 + 1e-12
    assert v['on_bed_volume'] == 0.0 and v['support_volume'] == v['on_part_volume'] > 0
    assert v['support_volume'] < overhang_ref.overhangs(soup, Z, 45, tol)['support_volume'][0]


def test_the_shelf_without_its_base_rests_on_the_bed(ns, oracle_lib):
    f = shelf(ns, base=False)
    soup, start, tol = meshed('shelf_nobase', f, oracle_lib)
    r = run(oracle_lib, f, soup, Z, 45, tol, start)
    v = ref.derive(r)
    assert r['counts'][ref.PART] == 0 and r['counts'][ref.BED] > 100 and v['on_part_volume'] == 0.0
    want = overhang_ref.chunk_tree_sum(proxy_terms(r))[0] / 2.0
    assert bits(v['support_volume']) == bits(want) and want > 0


def test_the_shelf_sideways_is_all_bed(ns, oracle_lib):
    f = shelf(ns)
    soup, start, tol = meshed('shelf', f, oracle_lib)
    r = run(oracle_lib, f, soup, X, 45, tol, start)
    v = ref.derive(r)
    assert len(r['triangle']) > 100 and r['counts'][ref.BED] == len(r['triangle'])
    assert bits(v['support_volume']) == bits(overhang_ref.chunk_tree_sum(proxy_terms(r))[0] / 2.0)
    assert v['buried_area'] == 0.0 and v['touch_area'] == 0.0


# ---- what holds for every model ----
def model(name, ns):
    return ns['torus'](1, 0.25) if name == 'torus_x' else fixtures.build(name, ns)


@pytest.mark.parametrize('angle', (45, 0))
@pytest.mark.parametrize('name', ('sphere', 'torus_x', 'ex_example', 'ex_blobby', 'twist', 'ex_knurling'))
def test_inequalities(name, angle, ns, oracle_lib):
    f = model(name, ns)
    soup, start, tol = meshed(name, f, oracle_lib)
    r = run(oracle_lib, f, soup, X if name == 'torus_x' else Z, angle, tol, start)
    ok = r['status'] != ref.NAN
    print(name, angle, dict(zip(ref.NAMES, r['counts'].tolist())), ref.derive(r))
    assert len(r['triangle']) > 0 and (r['height'][ok] <= r['tb'][ok]).all() and (r['height'][ok] >= 0).all()
    assert ref.derive(r)['support_volume'] <= overhang_ref.chunk_tree_sum((r['proj'] * r['tb'])[:, None])[0] / 2.0
    t = r['terms']
    assert (t >= 0).all() and (t[:, 3] >= t[:, 2] + t[:, 4]).all() and r['sums'][3] >= r['sums'][2] + r['sums'][4] * (1 - 2.0 ** -40)
    assert r['counts'].sum() == len(r['triangle']) and (r['proj'] > 0).all()
    assert np.array_equal(r['counts'], np.bincount(r['status'], minlength=5))


# ---- hidden faces ----
def test_faces_hidden_inside_a_union_are_buried(ns, oracle_lib):
    """the T of overhang_ref.t_soup in the field of the same two boxes as a union.  The bar's underside is z = 2 over x in [-1, 2],
    y in [0, 1], and `overhangs` counts all of it: 3.0, the 1 x 1 over the stem included.  The model is axis-aligned and every proj,
    tb and height below is a small dyadic number: the areas and volumes are exact.

    t_soup ITSELF cannot show the hidden part: its underside is two triangles, (-1,0) (-1,1) (2,1) and (-1,0) (2,1) (2,0), whose
    centroids have x = (-1 - 1 + 2) / 3 = 0 and (-1 + 2 + 2) / 3 = 1 -- they lie ON the stem's side faces x = 0 and x = 1, where the
    union's field is 0, never < 0, so both rays run down along the stem to the bed: one ray per face is all or nothing.  (The
    issue's "projected_area - buried_area is 2.0" is not reachable with faces of area 1.5 each.)  With the underside cut along
    the stem's outline the hidden 1 x 1 is BURIED and the difference is 2.0 exactly."""
    box = ns['box']
    f = box((1, 1, 2)).translate((0.5, 0.5, 1.0)) | box((3, 1, 1)).translate((0.5, 0.5, 2.5))
    soup = overhang_ref.t_soup()
    assert overhang_ref.overhangs(soup, Z, 45)['overhang_area'][0] == 3.0
    r = run(oracle_lib, f, soup, Z, 45, 0.0, 0.01)
    v = ref.derive(r)
    assert len(r['triangle']) == 2 and r['origin'][:, 0].tolist() == [0.0, 1.0] and r['status'].tolist() == [ref.BED, ref.BED]
    assert v['projected_area'] == 3.0 and v['buried_area'] == 0.0 and v['support_volume'] == 6.0 and r['height'].tolist() == [2.0, 2.0]
    # one ray per face is all or nothing: cut the underside along the stem's outline and the buried area is the hidden 1 x 1
    a, b = np.array([[0, 0, 2], [0, 1, 2], [1, 1, 2]], float), np.array([[0, 0, 2], [1, 1, 2], [1, 0, 2]], float)
    cut = np.concatenate([soup, [a, b, a - (1, 0, 0), b - (1, 0, 0), a + (1, 0, 0), b + (1, 0, 0)]])
    cut = np.delete(cut, r['triangle'], axis=0)
    rc = run(oracle_lib, f, cut, Z, 45, 0.0, 0.01)
    vc = ref.derive(rc)
    assert vc['projected_area'] == 3.0 and vc['buried_area'] == 1.0 and vc['projected_area'] - vc['buried_area'] == 2.0
    assert vc['support_volume'] == 4.0 and vc['on_part_volume'] == 0.0      # two 1 x 1 columns of height 2


# ---- every status ----
def down_triangle(c, r=0.01):
    """a small triangle that faces -z with its centroid at c (up to rounding)"""
    c = np.asarray(c, dtype=np.float64)
    return np.array([c + (r, 0, 0), c + (-r / 2, -r, 0), c + (-r / 2, r, 0)])


def test_every_status_is_reached(ns, oracle_lib):
    f = ns['sphere'](1)
    anchor = down_triangle((0, 0, -3.0))                          # the lowest point: the bed is at z = -3
    soup = np.array([anchor, down_triangle((0, 0, 2.0)), down_triangle((3, 0, 2.0)), down_triangle((0, 0, 0.5)), down_triangle((0, 0, -2.995))])
    r = run(oracle_lib, f, soup, Z, 45, 0.0, 0.01)
    assert r['triangle'].tolist() == [1, 2, 3, 4]                  # the anchor lies on the bed: contact
    assert r['status'].tolist() == [ref.PART, ref.BED, ref.BURIED, ref.BED]
    assert abs(r['height'][0] - 1.0) <= 2.0 ** -16 + 1e-12 and r['height'][1] == r['tb'][1] == 5.0 and bits(r['height'][2]) == 0
    assert r['steps'][3] == 0 and r['height'][3] == r['tb'][3] < 0.01 and r['steps'][2] == 1     # start >= tb: BED with no evaluation
    few = run(oracle_lib, f, soup, Z, 45, 0.0, 0.01, max_steps=4, step_scale=0.25)
    assert few['status'].tolist() == [ref.UNRESOLVED, ref.UNRESOLVED, ref.BURIED, ref.BED] and few['steps'].tolist() == [4, 4, 1, 0]
    assert few['height'][0] == few['tb'][0] == 5.0 and few['terms'][0, 0] == few['proj'][0] * 5.0 and few['terms'][0, 1] == 0.0
    raw = run(oracle_lib, f, soup, Z, 45, 0.0, 0.01, refine=0)
    assert np.array_equal(raw['status'], r['status']) and np.array_equal(raw['steps'], r['steps']) and raw['height'][0] > r['height'][0]


def nan_soup():
    """triangles over the centre of `ellipsoid((1, 1, 1))`, whose field is |p| - 1 and NaN at the centre and nowhere else: the
    vertices are chosen so that the centroids are (0, 0, 0.5), (0, 0, 1.5) and (0, 0, 3) exactly.  Triangle 0 lies on the bed (z = -3)."""
    def tri(z):
        return np.array([[0.5, 0.0, z], [-0.25, -0.5, z], [-0.25, 0.5, z]])
    return np.array([down_triangle((0, 0, -3.0)), tri(0.5), tri(1.5), tri(3.0), down_triangle((2, 0, 0.5))])


def test_a_ray_that_meets_a_nan_is_nan(ns, oracle_lib):
    f = ns['ellipsoid']((1, 1, 1))
    assert np.isnan(oracle_lib.evaluate(f, np.zeros((1, 3)))[0])
    soup = nan_soup()
    # start = 0.5: the first evaluation of the ray from (0, 0, 0.5) is AT the centre; the one from (0, 0, 1.5) meets the value 0 at
    # z = 1 (not inside), advances by min_step to z = 0.75 and is inside there
    r = run(oracle_lib, f, soup, Z, 45, 0.0, 0.5, min_step=0.25)
    assert np.array_equal(r['origin'][:3], [[0, 0, 0.5], [0, 0, 1.5], [0, 0, 3.0]]) and r['triangle'].tolist() == [1, 2, 3, 4]
    assert r['status'].tolist() == [ref.NAN, ref.PART, ref.PART, ref.BED] and r['steps'][:2].tolist() == [1, 2] and np.isnan(r['height'][0])
    # start = 1, min_step = 2: the ray from (0, 0, 3) meets the value 1 at z = 2, advances by max(1, 2) and its second evaluation is
    # AT the centre; the two rays below it begin inside
    r2 = run(oracle_lib, f, soup, Z, 45, 0.0, 1.0, min_step=2.0)
    assert r2['status'].tolist() == [ref.BURIED, ref.BURIED, ref.NAN, ref.BED] and r2['steps'].tolist() == [1, 1, 2, 2] and np.isnan(r2['height'][2])
    for rr, k in ((r, 0), (r2, 2)):
        assert rr['terms'][k].tolist() == [0.0, 0.0, 0.0, rr['proj'][k], 0.0] and rr['counts'][ref.NAN] == 1
        assert np.isfinite(rr['sums']).all() and rr['sums'][3] == rr['proj'].sum()


# ---- the empty cases ----
def test_empty_cases(ns, oracle_lib):
    f = ns['sphere'](1)
    calls = []

    def ev(P):
        calls.append(len(P))
        return oracle_lib.evaluate(f, P)
    d = np.array(Z)
    r = ref.supports(ev, np.zeros((0, 3, 3)), d, 0.5, 0.0, 0.01, 0.01)
    assert r['lo'] == np.inf and r['hi'] == -np.inf and not r['sums'].any() and not r['counts'].any() and r['height'].shape == (0,)
    assert r['origin'].shape == (0, 3) and r['triangle'].dtype == np.int32 and r['status'].dtype == np.uint8 and r['steps'].dtype == np.int32
    bad = np.array([down_triangle((0, 0, 2.0)), down_triangle((0, 0, 2.0))])
    bad[0, 1, 1] = np.nan
    bad[1, 2] = bad[1, 1]                                         # zero area
    r = ref.supports(ev, bad[:1], d, 0.5, 0.0, 0.01, 0.01)
    assert r['lo'] == np.inf and len(r['triangle']) == 0
    r = ref.supports(ev, bad, d, 0.5, 0.0, 0.01, 0.01)
    assert r['lo'] == 2.0 and len(r['triangle']) == 0 and not r['sums'].any()
    up = down_triangle((0, 0, 2.0))[::-1]                         # faces +z: no overhang
    assert len(ref.supports(ev, np.array([up, up + (0, 0, 1.0)]), d, 0.5, 0.0, 0.01, 0.01)['triangle']) == 0
    assert calls == []                                            # M = 0: no evaluation
    for soup in (np.zeros((0, 3, 3)), bad[:1], bad):
        got = pkg.support_rays_host(ev, soup, d, 0.5, 0.0, 0.01, 0.01)
        assert got['lo'] == ref.supports(ev, soup, d, 0.5, 0.0, 0.01, 0.01)['lo'] and len(got['triangle']) == 0 and not got['sums'].any()
    assert calls == []


# ---- the restatement ----
@pytest.mark.parametrize('name', ('shelf', 'ex_example', 'ex_knurling', 'ellipsoid_nan', 'mixed'))
def test_the_restatement_is_the_definition(name, ns, oracle_lib):
    runs = [dict(angle=45), dict(angle=0, max_steps=4), dict(angle=30, refine=0, step_scale=0.5)]
    if name == 'ellipsoid_nan':
        f, soup, start, tol = ns['ellipsoid']((1, 1, 1)), nan_soup(), 0.5, 0.0
    elif name == 'mixed':
        f, (soup, start, tol) = ns['sphere'](1), meshed('ex_example', fixtures.build('ex_example', ns), oracle_lib)
        soup = soup[:3000].copy()
        soup[5, 0, 0] = np.inf
        soup[7, 1] = soup[7, 0]
    else:
        f = shelf(ns) if name == 'shelf' else fixtures.build(name, ns)
        soup, start, tol = meshed(name, f, oracle_lib)
    ev = lambda P: oracle_lib.evaluate(f, P)
    for kw in runs:
        kw = dict(kw)
        s = overhang_ref.sin_limit_of(kw.pop('angle'))
        for d in (Z, (0.3, -0.5, 0.8), (-1.0, 0.0, 0.0)):
            d = overhang_ref.normalise(d)[0]
            want, got = ref.supports(ev, soup, d, s, tol, start, start, **kw), pkg.support_rays_host(ev, soup, d, s, tol, start, start, **kw)
            for k in ('triangle', 'status', 'steps', 'counts'):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, kw, k)
            for k in ('height', 'origin', 'sums', 'lo', 'hi'):
                assert np.array_equal(bits(got[k]), bits(want[k])), (name, kw, k)
            gd, wd = pkg.derive({k: np.array([got[k]]) for k in ('sums', 'lo', 'hi')}), ref.derive(want)
            assert all(bits(gd[k])[0] == bits(wd[k]) for k in wd)


def test_the_tree_is_over_the_rays():
    rng = np.random.RandomState(11)
    x = rng.uniform(0, 1, size=(257 * 1024 + 5, 2))
    assert np.array_equal(bits(pkg.chunk_tree_sum(x)), bits(overhang_ref.chunk_tree_sum(x)))
    assert np.array_equal(pkg.chunk_tree_sum(np.zeros((0, 5))), np.zeros(5))


# ---- the record ----
def fake_raw(K=3):
    rng = np.random.RandomState(2)
    rays = []
    for k in range(K):
        M = 4 + k
        h = rng.uniform(0, 1, M)
        h[0] = np.nan
        rays.append((np.arange(M, dtype=np.int32), h, np.full(M, ref.BED, np.uint8), np.ones(M, np.int32), rng.uniform(-1, 1, (M, 3))))
    sums = np.array([[4.0, 2.0, 1.0, 6.0, 1.0], [1.0, 1.0, 1.0, 6.0, 0.0], [1.0, 1.0, 0.5, 6.0, 2.0]])[:K]
    return {'lo': np.zeros(K), 'hi': np.arange(1.0, K + 1), 'sums': sums, 'counts': np.ones((K, 5), np.int64), 'rays': rays}


def test_the_record():
    D = overhang_ref.normalise([Z, (1, 1, 0), (0, -1, -1)])
    s = pkg.Supports(D, fake_raw(), 45.0, 0.1, dict(start=0.01))
    assert s.support_volume.tolist() == [3.0, 1.0, 1.0] and s.on_bed_volume.tolist() == [2.0, 0.5, 0.5] and s.on_part_volume.tolist() == [1.0, 0.5, 0.5]
    assert s.touch_area.tolist() == [0.5, 0.5, 0.25] and s.projected_area.tolist() == [3.0] * 3 and s.buried_area.tolist() == [0.5, 0.0, 1.0]
    assert s.height.tolist() == [1.0, 2.0, 3.0] and s.best() == 1 and s.best('buried_area') == 1 and s.best(lambda r: -r.height) == 2
    assert s.proxy is None and s.traced is None and not s.support_volume.flags.writeable and not s.rays(0)[1].flags.writeable
    with pytest.raises(ValueError):
        s.best(lambda r: np.zeros(2))
    for k in range(3):
        R = s.rotation(k)
        assert np.allclose(R @ D[k], Z, atol=1e-15) and np.allclose(R @ R.T, np.eye(3), atol=1e-15)
        tri, h, st, steps, o = s.rays(k)
        c = s.columns(k)
        assert c.shape == (len(h) - 1, 2, 3) and np.array_equal(c[:, 0], o[1:])
        assert np.array_equal(bits(c[:, 1]), bits(o[1:] + h[1:, None] * (-D[k])))
    empty = pkg.Supports(D[:1], {'lo': [np.inf], 'hi': [-np.inf], 'sums': np.zeros((1, 5)), 'counts': np.zeros((1, 5), np.int64),
                                 'rays': [(np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros((0, 3)))]},
                         45.0, 0.0, {})
    assert empty.columns(0).shape == (0, 2, 3) and empty.support_volume[0] == 0.0 and empty.best() == 0


class FakeMesh:
    """what `supports_of_mesh` needs of an `engine.Mesh`: the two device calls, answered by the definitions over the checker"""

    def __init__(self, soup, ev):
        self.soup, self.ev, self.calls = soup, ev, []

    def overhangs(self, d, sin_limit, bed_tol, max_scratch_bytes=0):
        return overhang_ref.rate(self.soup, d, sin_limit, bed_tol)

    def support_rays(self, sdf, d, sin_limit, bed_tol, start, min_step, step_scale=1.0, max_steps=256, refine=16):
        d, p = pkg.check_params(d, sin_limit, bed_tol, start, min_step, step_scale, max_steps, refine)
        self.calls.append(d.copy())
        got = [ref.supports(self.ev, self.soup, x, *p) for x in d]
        return {'lo': [g['lo'] for g in got], 'hi': [g['hi'] for g in got], 'sums': np.array([g['sums'] for g in got]),
                'counts': np.array([g['counts'] for g in got]), 'rays': [(g['triangle'], g['height'], g['status'], g['steps'], g['origin']) for g in got]}


def test_an_int_rates_first_and_traces_the_top(ns, oracle_lib):
    f = shelf(ns)
    soup, start, tol = meshed('shelf', f, oracle_lib)
    mesh = FakeMesh(soup, lambda P: oracle_lib.evaluate(f, P))
    s = pkg.supports_of_mesh(mesh, f, 20, 45, tol, start, start, top=3)
    proxy = overhang_ref.overhangs(soup, overhang_ref.sphere_directions(20), 45, tol)
    order = np.argsort(proxy['support_volume'], kind='stable')[:3]
    assert np.array_equal(s.traced, order) and np.array_equal(s.directions, proxy['directions'][order]) and len(mesh.calls) == 1 and np.array_equal(mesh.calls[0], s.directions)
    assert np.array_equal(bits(s.proxy.support_volume), bits(proxy['support_volume'])) and len(s.proxy.directions) == 26
    by_hand = mesh.support_rays(f, proxy['directions'][order], overhang_ref.sin_limit_of(45), tol, start, start)
    assert np.array_equal(bits(by_hand['sums']), bits(s.sums)) and np.array_equal(by_hand['counts'], s.counts)
    for k in range(3):
        assert all(np.array_equal(ref.bits(a), ref.bits(b)) for a, b in zip(s.rays(k), by_hand['rays'][k]))
    assert s.params == dict(start=start, min_step=start, step_scale=1.0, max_steps=256, refine=16) and s.angle == 45.0 and s.bed_tolerance == tol
    one = pkg.supports_of_mesh(mesh, f, (0, 0, 2.0), 45, tol, start, start)
    assert one.directions.tolist() == [[0, 0, 1.0]] and one.on_bed_volume[0] == 0.0 and one.on_part_volume[0] > 0


def test_python_refusals(ns):
    f = ns['sphere'](1)
    good = dict(directions=Z, sin_limit=0.5, bed_tol=0.0, start=0.01, min_step=0.01, step_scale=1.0, max_steps=256, refine=16)
    pkg.check_params(**good)
    for bad in ({'start': 0.0}, {'min_step': -1.0}, {'step_scale': 0.0}, {'step_scale': 2.0}, {'sin_limit': 1.0}, {'sin_limit': -0.1},
                {'bed_tol': -1.0}, {'bed_tol': float('nan')}, {'max_steps': 0}, {'refine': -1}, {'start': float('inf')},
                {'directions': (0, 0, 0)}, {'directions': (0, 0, 2.0)}, {'directions': (0, float('nan'), 1)}, {'directions': np.zeros((0, 3))},
                {'directions': np.tile(Z, (1025, 1))}, {'directions': (1.0, 0.0)}):
        with pytest.raises(ValueError):
            pkg.check_params(**dict(good, **bad))
    # ... and `supports` refuses before anything is meshed (no engine is asked for: this passes without a device)
    for bad in ({'angle': 90}, {'angle': -1}, {'bed_tolerance': -1.0}, {'start': 0.0}, {'min_step': 0.0}, {'step_scale': 1.5}, {'max_steps': 0},
                {'refine': -1}, {'directions': (0, 0, 0)}, {'directions': -1}, {'directions': 10, 'top': 0}):
        with pytest.raises(ValueError):
            f.supports(**dict(dict(samples=SAMPLES, verbose=False), **bad))
    with pytest.raises(ValueError, match='step'):
        pkg.supports_soup(np.zeros((0, 3, 3)), f)
