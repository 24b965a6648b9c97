"""Support rays on the device (csrc/sdf_supports.hip, the driver in csrc/sdf_overhang.hip, `engine.Mesh.support_rays`,
sdf_amd/supports.py): every output -- triangle, height bits, status, steps, origin, sums, counts, lo, hi --
identical to the definition (tests/supports_ref.py) run over the same interpreter (`Engine.eval_points`) and, for the models without
libm calls, over the CPU checker; ragged ray counts through adopted soups; every status; the shelf end to end; the other routes; the
refusals; the allocation sweep.  Every refusal is decided on the host before a launch; no test repeats a device call that failed."""
import ctypes
import importlib

import numpy as np
import pytest

import fixtures
import overhang_ref
import supports_ref as ref
from sdf_amd import core, engine
from sdf_amd.mesh import Mesh
from test_measure_gpu import Soup, _free
from test_supports_host import nan_soup, shelf

pkg = importlib.import_module('sdf_amd.supports')

pytestmark = pytest.mark.gpu

# plain family, trig family (twice), smooth unions, the largest register files
# (opcode coverage lives in the sweep, tests/test_probe_sweep_gpu.py: every tape of the suite goes through this kernel there; these few
# models walk the kernel's own states)
MODELS = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'slots_plain_8_8_p8d8')
LIBM_FREE = ('ex_example', 'ex_blobby', 'torus')
SAMPLES = 2 ** 13
X, Z = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
DIRS = overhang_ref.normalise([Z, (0.3, -0.5, 0.8), (-1.0, 0.0, 0.0)])
S45, S30 = overhang_ref.sin_limit_of(45), overhang_ref.sin_limit_of(30)
_meshes = {}


def meshed(name, ns, eng):
    """(model, grid axes, soup (T, 3, 3), start = min_step, bed_tol) at 2^13 samples: meshed once per model, left unchanged"""
    if name not in _meshes:
        f = shelf(ns) if name == 'shelf' else fixtures.build(name, ns)
        Xs, Ys, Zs, step = core.grid_axes(eng.estimate_bounds(f), samples=SAMPLES)
        m = eng.generate(f, Xs, Ys, Zs, 32, True)
        try:
            soup = m.points().copy().reshape(-1, 3, 3)
        finally:
            m.close()
        soup.setflags(write=False)
        _meshes[name] = (f, (Xs, Ys, Zs), soup, float(min(step)) / 4, float(max(step)))
    return _meshes[name]


def same(raw, k, want, what=''):
    """direction k of what `engine.Mesh.support_rays` returned against the definition's dict"""
    tri, height, status, steps, origin = raw['rays'][k]
    for g, w, dtype in ((tri, want['triangle'], np.int32), (height, want['height'], np.float64), (status, want['status'], np.uint8),
                        (steps, want['steps'], np.int32), (origin, want['origin'], np.float64)):
        assert g.dtype == dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    assert np.array_equal(tri, want['triangle']), what
    bad = (ref.bits(height) != ref.bits(want['height'])) | (status != want['status']) | (steps != want['steps']) \
        | (ref.bits(origin) != ref.bits(want['origin'])).any(axis=1)
    assert not bad.any(), '%s: %d of %d rays differ, first at %d: %r / %r' % (
        what, bad.sum(), bad.size, np.flatnonzero(bad)[0], [a[np.flatnonzero(bad)[0]] for a in (height, status, steps, origin)],
        [want[n][np.flatnonzero(bad)[0]] for n in ('height', 'status', 'steps', 'origin')])
    assert np.array_equal(ref.bits(raw['sums'][k]), ref.bits(want['sums'])), (what, raw['sums'][k], want['sums'])
    assert np.array_equal(raw['counts'][k], want['counts']) and raw['counts'].dtype == np.int64, (what, raw['counts'][k], want['counts'])
    assert ref.bits(raw['lo'][k:k + 1])[0] == ref.bits(np.array([want['lo']]))[0] and ref.bits(raw['hi'][k:k + 1])[0] == ref.bits(np.array([want['hi']]))[0]


def counts(r):
    return dict(zip(ref.NAMES, np.asarray(r['counts']).tolist()))


# ---- constructed soups in the field of sphere(1) ----
def constructed(m, seed=5):
    """m small triangles that face down -- tilted by up to 40 degrees, scattered above, beside and inside the unit sphere, every
    tenth one just above the bed -- with, after every third, one that is no overhang at 45 degrees: facing up, not finite, of zero
    area, tilted by 50 degrees.  Triangle 0 is the anchor on the bed at z = -3.  Returns (T, 3, 3) with T = 1 + m + m // 3."""
    rng = np.random.RandomState(seed + m % 1000)
    c = rng.uniform((-1.6, -1.6, -1.4), (1.6, 1.6, 2.5), size=(m, 3))
    c[9::10, 2] = -3.0 + rng.uniform(0.02, 0.04, size=len(c[9::10]))
    r = rng.uniform(0.005, 0.02, size=(m, 1))
    th = np.radians(rng.uniform(0.0, 40.0, size=(m, 1)))

    def tris(c, r, th):
        base = np.array([[1.0, 0.0], [-0.5, -1.0], [-0.5, 1.0]])                   # faces -z
        x, y = base[None, :, 0] * r, base[None, :, 1] * r
        return c[:, None, :] + np.stack([x * np.cos(th), y, x * np.sin(th)], axis=2)

    down = tris(c, r, th)
    out = [np.array([[[0.01, 0, -3.0], [-0.005, -0.01, -3.0], [-0.005, 0.01, -3.0]]])]
    n_extra = m // 3
    steep = tris(rng.uniform(-1.5, 1.5, size=(n_extra, 3)), np.full((n_extra, 1), 0.01), np.full((n_extra, 1), np.radians(50.0)))
    for i in range(0, m, 3):
        out.append(down[i:i + 3])
        e = i // 3
        if e < n_extra:
            kind = e % 4
            t = down[i:i + 1].copy()
            if kind == 0:
                t = t[:, ::-1]
            elif kind == 1:
                t[0, e % 3, (e // 3) % 3] = (np.nan, np.inf, -np.inf)[e % 3]
            elif kind == 2:
                t[0, 2] = t[0, 1]
            else:
                t = steep[e:e + 1]
            out.append(t)
    return np.concatenate(out)


RUNS = (dict(), dict(max_steps=4), dict(refine=0), dict(sin_limit=S30), dict(bed_tol=0.05), dict(sin_limit=S30, bed_tol=0.05, step_scale=0.5))


@pytest.mark.parametrize('m', (0, 1, 63, 65, 257, 1023, 1025))
def test_ragged_ray_counts_through_adopted_soups(m, ns, eng):
    """M = 0, 1, a wave less one lane, a wave plus one, a workgroup plus one, a chunk less one, a chunk plus one (two partials); each
    with the defaults, few steps, no refinement, two angles and two bed tolerances"""
    f = ns['sphere'](1)
    tris = constructed(m)
    ev = lambda P: eng.eval_points(f, P)
    s = Soup(eng, tris)
    try:
        seen = set()
        for over in RUNS:
            p = dict(dict(sin_limit=S45, bed_tol=0.0, start=0.01, min_step=0.01), **over)
            want = ref.supports(ev, tris, DIRS[0], **p)
            got = s.mesh.support_rays(f, DIRS[:1], **p)
            same(got, 0, want, '%d %r' % (m, over))
            seen |= set(want['status'].tolist())
            if not over:
                assert len(want['triangle']) == m and (m < 4 or not np.array_equal(want['triangle'], np.arange(1, m + 1)))
            if over == dict(sin_limit=S30) and m >= 63:
                assert len(want['triangle']) > m
            if over == dict(bed_tol=0.05) and m >= 63:
                assert len(want['triangle']) < m
            if over == dict(max_steps=4) and m >= 63:
                assert (want['status'] == ref.UNRESOLVED).any() and (want['steps'][want['status'] == ref.UNRESOLVED] == 4).all()
        if m >= 257:
            assert {ref.BED, ref.PART, ref.BURIED, ref.UNRESOLVED} <= seen
    finally:
        s.close()


def test_the_second_level_of_the_tree(ns, eng):
    """M = 256 * 1024 + 1 rays: 257 chunk partials, two levels of the halving tree; a few steps per ray"""
    m = 256 * 1024 + 1
    f = ns['sphere'](1)
    tris = constructed(m)
    p = dict(sin_limit=S45, bed_tol=0.0, start=0.01, min_step=0.01, max_steps=8)
    s = Soup(eng, tris)
    try:
        got = s.mesh.support_rays(f, DIRS[:1], **p)
    finally:
        s.close()
    want = ref.supports(lambda P: eng.eval_points(f, P), tris, DIRS[0], **p)
    assert len(want['triangle']) == m
    same(got, 0, want, 'second level')
    print(counts(want), 'lockstep share %.2f' % ref.lockstep_share(want['steps']))


# ---- generated meshes ----
@pytest.mark.parametrize('name', MODELS)
def test_generated_meshes_are_bit_identical_to_the_definition(name, ns, eng):
    f, (Xs, Ys, Zs), soup, start, tol = meshed(name, ns, eng)
    assert len(soup) > 256 and len(soup) % 64 != 0
    p = dict(sin_limit=S45, bed_tol=tol, start=start, min_step=start)
    m = eng.generate(f, Xs, Ys, Zs, 32, True)
    try:
        got = m.support_rays(f, DIRS, **p)
        again = m.support_rays(f, DIRS, **p)                      # a second call on the same mesh: identical bits
        singles = [m.support_rays(f, DIRS[k:k + 1], **p) for k in range(3)]
    finally:
        m.close()
    ev = lambda P: eng.eval_points(f, P)
    for k in range(3):
        want = ref.supports(ev, soup, DIRS[k], **p)
        print(name, k, len(soup), counts(want), 'steps <= %d' % (want['steps'].max() if len(want['steps']) else 0),
              'lockstep share %.2f' % ref.lockstep_share(want['steps']))
        same(got, k, want, '%s %d' % (name, k))
        same(again, k, want, '%s %d again' % (name, k))
        same(singles[k], 0, want, '%s %d alone' % (name, k))      # K = 3 directions in one call equal three calls
    assert sum(len(r[0]) for r in got['rays']) > 256


@pytest.mark.parametrize('name', LIBM_FREE)
def test_generated_meshes_against_the_checker(name, ns, eng, oracle_lib):
    f, (Xs, Ys, Zs), soup, start, tol = meshed(name, ns, eng)
    p = dict(sin_limit=S45, bed_tol=tol, start=start, min_step=start)
    m = eng.generate(f, Xs, Ys, Zs, 32, True)
    try:
        got = m.support_rays(f, DIRS, **p)
    finally:
        m.close()
    for k in range(3):
        same(got, k, ref.supports(lambda P: oracle_lib.evaluate(f, P), soup, DIRS[k], **p), '%s %d' % (name, k))


def test_a_ray_that_meets_a_nan_is_nan(ns, eng, oracle_lib):
    """`ellipsoid` divides 0 by 0 at its centre and nowhere else: rays that meet the centre on the first and on the second pass
    (test_supports_host.nan_soup says how)"""
    f = ns['ellipsoid']((1, 1, 1))
    assert np.isnan(eng.eval_points(f, np.zeros((1, 3)))[0])
    soup = nan_soup()
    s = Soup(eng, soup)
    nan_steps = set()
    try:
        for p in (dict(start=0.5, min_step=0.25), dict(start=1.0, min_step=2.0)):
            p = dict(p, sin_limit=S45, bed_tol=0.0)
            want = ref.supports(lambda P: eng.eval_points(f, P), soup, DIRS[0], **p)
            assert want['counts'][ref.NAN] == 1
            nan_steps |= set(want['steps'][want['status'] == ref.NAN].tolist())
            got = s.mesh.support_rays(f, DIRS[:1], **p)
            same(got, 0, want, repr(p))
            same(got, 0, ref.supports(lambda P: oracle_lib.evaluate(f, P), soup, DIRS[0], **p), 'checker')
            assert np.isfinite(got['sums']).all()
    finally:
        s.close()
    assert nan_steps == {1, 2}


def test_empty_meshes(ns, eng):
    f = ns['sphere'](1)
    p = dict(sin_limit=S45, bed_tol=0.0, start=0.01, min_step=0.01)
    bad = np.array([[[0.01, 0, 2.0], [-0.005, -0.01, 2.0], [-0.005, 0.01, 2.0]]] * 2)
    bad[0, 1, 1] = np.nan
    bad[1, 2] = bad[1, 1]
    for soup in (np.zeros((0, 3, 3)), bad[:1], bad, bad[1:, ::-1]):
        s = Soup(eng, soup)
        try:
            got = s.mesh.support_rays(f, DIRS[:2], **p)
        finally:
            s.close()
        for k in range(2):
            want = ref.supports(lambda P: eng.eval_points(f, P), soup, DIRS[k], **p)
            assert len(want['triangle']) == 0
            same(got, k, want, 'empty')
    assert got['rays'][0][4].shape == (0, 3)


# ---- the shelf, end to end ----
def test_the_shelf_end_to_end(ns, eng):
    f, (Xs, Ys, Zs), soup, start, tol = meshed('shelf', ns, eng)
    s = f.supports(samples=SAMPLES, verbose=False)
    assert s.params == dict(start=start, min_step=start, step_scale=1.0, max_steps=256, refine=16) and s.bed_tolerance == tol and s.angle == 45.0
    want = ref.supports(lambda P: eng.eval_points(f, P), soup, DIRS[0], S45, tol, start, start)
    same({'rays': [s.rays(0)], 'sums': s.sums, 'counts': s.counts, 'lo': s.lo, 'hi': s.hi}, 0, want, 'shelf')
    tri, height, status, steps, o = s.rays(0)
    margin = 2 * tol
    under = (np.abs(o[:, 0]) < 1 - margin) & (np.abs(o[:, 1]) < 1 - margin) & (np.maximum(np.abs(o[:, 0]), np.abs(o[:, 1])) > 0.25 + margin)
    err = np.abs(height[under] - 0.8).max()
    print('shelf: %r; %d rays under the plate, largest |height - 0.8| %.3g' % (s, under.sum(), err))
    assert under.sum() > 100 and (status[under] == ref.PART).all() and err <= 0.8 * 2.0 ** -16 + 1e-12
    assert s.counts[0, ref.BED] == 0 and s.on_bed_volume[0] == 0.0 and s.support_volume[0] == s.on_part_volume[0] > 0
    assert s.support_volume[0] < f.overhangs(samples=SAMPLES, verbose=False).support_volume[0]
    c = s.columns(0)
    assert c.shape == (len(tri), 2, 3) and np.array_equal(c[:, 0], o) and np.allclose(c[under, 1, 2], 0.2, atol=1e-4)

    # an int: rate 64 + 6 directions, trace the 4 with the smallest proxy -- against the two steps by hand on one device mesh
    top = f.supports(64, top=4, samples=SAMPLES, verbose=False)
    m = eng.generate(f, Xs, Ys, Zs, 32, True)
    try:
        proxy = pkg.overhangs_of_mesh(m, 64, 45, tol)
        order = np.argsort(proxy.support_volume, kind='stable')[:4]
        raw = m.support_rays(f, proxy.directions[order], S45, tol, start, start)
    finally:
        m.close()
    assert np.array_equal(top.traced, order) and np.array_equal(top.directions, proxy.directions[order]) and len(top.proxy.directions) == 70
    assert np.array_equal(ref.bits(top.proxy.support_volume), ref.bits(proxy.support_volume))
    assert np.array_equal(ref.bits(top.sums), ref.bits(raw['sums'])) and np.array_equal(top.counts, raw['counts'])
    for k in range(4):
        assert all(np.array_equal(ref.bits(a), ref.bits(b)) for a, b in zip(top.rays(k), raw['rays'][k]))
    assert top.best() == int(np.argmin(top.support_volume)) and np.allclose(top.rotation(top.best()) @ top.directions[top.best()], Z, atol=1e-15)


# ---- the other routes ----
def test_a_model_with_closures_takes_the_definition_on_the_host(ns, eng):
    @ns['sdf3']
    def ball(r):
        def f(p):
            return np.sqrt((p * p).sum(axis=1)) - r
        return f
    f = ball(0.8) & ns['box'](1.4)
    Xs, Ys, Zs, step = core.grid_axes(((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), samples=SAMPLES)
    p = dict(sin_limit=S45, bed_tol=max(step), start=min(step) / 4, min_step=min(step) / 4)
    m = eng.generate(f, Xs, Ys, Zs, 32, True)
    try:
        soup = m.points().copy().reshape(-1, 3, 3)
        dt = eng.tape_for(f)
        h = ctypes.c_void_p()
        values, cnt = np.zeros((1, 7)), np.zeros((1, 6), np.int64)
        p8 = np.array([p['sin_limit'], p['bed_tol'], p['start'], p['min_step'], 1.0, 0, 0, 0])
        rc = eng.lib.sdf_mesh_support_rays(m.handle, dt.handle, DIRS.ctypes.data_as(engine._f64p), 1, p8.ctypes.data_as(engine._f64p), 256, 16,
                                           ctypes.byref(h), values.ctypes.data_as(engine._f64p), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        assert rc == 2 and b'closures' in eng.lib.sdf_last_error() and b'sdf_mesh_support_rays' in eng.lib.sdf_last_error() and not h.value
        got = m.support_rays(f, DIRS[:2], **p)
    finally:
        m.close()
    for k in range(2):
        want = ref.supports(lambda P: eng.eval_points(f, P), soup, DIRS[k], **p)
        same(got, k, want, 'closure %d' % k)
    assert got['counts'][0, ref.BED] > 0
    s = f.supports(DIRS[:2], samples=SAMPLES, bounds=((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), verbose=False)
    for k in range(2):                                            # (`supports` normalises what it is given: its own directions count)
        want = ref.supports(lambda P: eng.eval_points(f, P), soup, s.directions[k], **p)
        same({'rays': [s.rays(k)], 'sums': s.sums[k:k + 1], 'counts': s.counts[k:k + 1], 'lo': s.lo[k:k + 1], 'hi': s.hi[k:k + 1]}, 0, want, 'closure')


def test_a_file_in_a_field_and_keep(tmp_path, ns, eng):
    f = shelf(ns)
    f.save(str(tmp_path / 's.stl'), samples=SAMPLES, verbose=False)
    file_mesh = Mesh.from_stl(str(tmp_path / 's.stl'))
    s = file_mesh.supports(f, DIRS[:2], step=0.08)
    soup = np.asarray(file_mesh.points, dtype=np.float64)[np.asarray(file_mesh.triangles)]
    assert s.params['start'] == s.params['min_step'] == 0.02 and s.bed_tolerance == 0.0
    for k in range(2):
        want = ref.supports(lambda P: eng.eval_points(f, P), soup, s.directions[k], S45, 0.0, 0.02, 0.02)
        same({'rays': [s.rays(k)], 'sums': s.sums[k:k + 1], 'counts': s.counts[k:k + 1], 'lo': s.lo[k:k + 1], 'hi': s.hi[k:k + 1]}, 0, want, 'file')
    with pytest.raises(ValueError, match='step'):
        file_mesh.supports(f)
    # keep=: two separate balls, the larger one kept -- the rays of the smaller one are gone
    g = ns['sphere'](0.5) | ns['sphere'](0.3).translate((0, 0, 1.2))
    both, kept = g.supports(samples=SAMPLES, verbose=False), g.supports(samples=SAMPLES, keep='largest', verbose=False)
    alone = ns['sphere'](0.5).supports(samples=SAMPLES, bounds=eng.estimate_bounds(g), verbose=False)
    assert len(kept.rays(0)[0]) < len(both.rays(0)[0]) and both.counts[0, ref.PART] > 0 and kept.counts[0, ref.PART] == 0
    assert len(kept.rays(0)[0]) == len(alone.rays(0)[0]) and np.array_equal(ref.bits(kept.rays(0)[4]), ref.bits(alone.rays(0)[4]))


# ---- refusals ----
def test_refusals(ns, eng):
    f = ns['sphere'](1)
    lib = eng.lib
    tris = constructed(30)
    s = Soup(eng, tris)
    other = engine.Engine(0)                                    # a second context on the same device
    odt = other.tape_for(f)
    try:
        dt = eng.tape_for(f)
        values, cnt = np.full((2, 7), 7.0), np.full((2, 6), 7, np.int64)
        f64p, i64p = engine._f64p, ctypes.POINTER(ctypes.c_int64)
        h = ctypes.c_void_p()

        def call(mesh, tape, p8, dirs=DIRS[:1], n_dirs=None, max_steps=256, refine=16, out=True):
            p8, dirs = np.array(p8, np.float64), np.ascontiguousarray(dirs, dtype=np.float64)
            return lib.sdf_mesh_support_rays(mesh, tape, dirs.ctypes.data_as(f64p), len(dirs) if n_dirs is None else n_dirs, p8.ctypes.data_as(f64p),
                                             max_steps, refine, ctypes.byref(h) if out else None, values.ctypes.data_as(f64p), cnt.ctypes.data_as(i64p))
        good = [0.5, 0.0, 0.01, 0.01, 1.0, 0.0, 0.0, 0.0]

        def bad_p(i, v):
            return good[:i] + [v] + good[i + 1:]
        for p8, word in ((bad_p(2, 0.0), b'start'), (bad_p(2, -1.0), b'start'), (bad_p(3, 0.0), b'min_step'), (bad_p(4, 0.0), b'step_scale'),
                         (bad_p(4, 2.0), b'step_scale'), (bad_p(0, 1.0), b'sin_limit'), (bad_p(0, -0.1), b'sin_limit'), (bad_p(1, -1.0), b'bed_tol'),
                         (bad_p(1, float('nan')), b'finite'), (bad_p(2, float('inf')), b'finite'), (bad_p(7, float('nan')), b'finite')):
            assert call(s.mesh.handle, dt.handle, p8) == 2 and word in lib.sdf_last_error(), (p8, lib.sdf_last_error())
            assert b'sdf_mesh_support_rays' in lib.sdf_last_error() and not h.value
        assert call(s.mesh.handle, dt.handle, good, max_steps=0) == 2 and b'max_steps' in lib.sdf_last_error()
        assert call(s.mesh.handle, dt.handle, good, refine=-1) == 2 and b'refine' in lib.sdf_last_error()
        for d in ((0, 0, 0), (0, 0, 2.0), (0, float('nan'), 1.0), (0, 0, 1 + 1e-9)):
            assert call(s.mesh.handle, dt.handle, good, dirs=[Z, d]) == 2 and b'direction 1' in lib.sdf_last_error()
        assert call(s.mesh.handle, dt.handle, good, n_dirs=0) == 2 and b'n_dirs' in lib.sdf_last_error()
        assert call(s.mesh.handle, dt.handle, good, dirs=np.tile(Z, (1025, 1))) == 2 and b'1024' in lib.sdf_last_error()
        assert call(s.mesh.handle, None, good) == 2 and call(None, dt.handle, good) == 2 and call(s.mesh.handle, dt.handle, good, out=False) == 2
        assert lib.sdf_mesh_support_rays(s.mesh.handle, dt.handle, None, 1, None, 256, 16, ctypes.byref(h), None, None) == 2
        assert call(s.mesh.handle, odt.handle, good) == 2 and b'different contexts' in lib.sdf_last_error()
        assert (values == 7.0).all() and (cnt == 7).all() and not h.value
        for bad in ({'start': 0.0}, {'step_scale': 2.0}, {'max_steps': 0}, {'refine': -1}, {'min_step': float('nan')}, {'sin_limit': 1.0},
                    {'bed_tol': -1.0}, {'directions': [(0, 0, 2.0)]}):
            with pytest.raises(ValueError):
                s.mesh.support_rays(f, **dict(dict(directions=DIRS[:1], sin_limit=0.5, bed_tol=0.0, start=0.01, min_step=0.01), **bad))
        eng.precision = engine.PRECISION_F32
        try:
            with pytest.raises(ValueError, match='float32'):
                s.mesh.support_rays(f, DIRS[:1], 0.5, 0.0, 0.01, 0.01)
        finally:
            eng.precision = engine.PRECISION_F64
        # ... and the mesh serves the call that is in order; the fetch refuses a direction it does not have
        assert call(s.mesh.handle, dt.handle, good, dirs=DIRS[:2]) == 0 and h.value
        try:
            assert lib.sdf_support_rays_fetch(h, 2, None, None, None, None, None) == 2 and b'sdf_support_rays_fetch' in lib.sdf_last_error()
            assert lib.sdf_support_rays_fetch(h, -1, None, None, None, None, None) == 2
            assert lib.sdf_support_rays_fetch(h, 1, None, None, None, None, None) == 0
        finally:
            lib.sdf_support_rays_destroy(h)
        want = ref.supports(lambda P: eng.eval_points(f, P), tris, DIRS[1], 0.5, 0.0, 0.01, 0.01)
        assert np.array_equal(ref.bits(values[1, 2:]), ref.bits(want['sums'])) and cnt[1, 5] == len(want['triangle'])
        parts = np.zeros(4)
        assert lib.sdf_mesh_supports_last_kernel_ms(parts.ctypes.data_as(f64p)) > 0 and (parts > 0).all()
    finally:
        s.close()
        odt._fin()
        other._fin()


def test_failed_allocations_leak_nothing(ns, eng):
    """sdf_test_fail_alloc walked through sdf_mesh_support_rays on 100,000 rays x 2 directions -- the scratch block and a block per
    direction: each failure carries the allocator's message, the free device memory is what it was, and the next call matches"""
    lib = eng.lib
    f = ns['sphere'](1)
    dt = eng.tape_for(f)
    warm = Soup(eng, constructed(30))                             # (code objects and the like are loaded before anything is compared)
    try:
        warm.mesh.support_rays(f, DIRS[:1], S45, 0.0, 0.01, 0.01)
    finally:
        warm.close()
    tris = constructed(100000)
    D = np.ascontiguousarray(DIRS[[0, 2]])
    s = Soup(eng, tris)
    try:
        eng.synchronize()
        f0 = _free(lib)
        values, cnt = np.zeros((2, 7)), np.zeros((2, 6), np.int64)
        p8 = np.array([S45, 0.0, 0.01, 0.01, 1.0, 0, 0, 0])
        h = ctypes.c_void_p()
        failures = 0
        for n in range(1, 8):
            lib.sdf_test_fail_alloc(n)
            rc = lib.sdf_mesh_support_rays(s.mesh.handle, dt.handle, D.ctypes.data_as(engine._f64p), 2, p8.ctypes.data_as(engine._f64p), 8, 4,
                                           ctypes.byref(h), values.ctypes.data_as(engine._f64p), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
            lib.sdf_test_fail_alloc(0)
            if rc == 0:
                break
            failures += 1
            assert rc == 1 and b'emory' in lib.sdf_last_error() and not h.value, lib.sdf_last_error()
            assert _free(lib) == f0                              # every block is back
        assert failures == 3 and rc == 0 and h.value              # the scratch, and one block per direction
        assert _free(lib) < f0
        lib.sdf_support_rays_destroy(h)
        assert _free(lib) == f0
        for k in range(2):
            want = ref.supports(lambda P: eng.eval_points(f, P), tris, D[k], S45, 0.0, 0.01, 0.01, max_steps=8, refine=4)
            assert np.array_equal(ref.bits(values[k, 2:]), ref.bits(want['sums'])) and np.array_equal(cnt[k, :5], want['counts'])
            assert cnt[k, 5] == len(want['triangle']) > 0
    finally:
        lib.sdf_test_fail_alloc(0)
        s.close()
