"""The definition of dual contouring (tests/dual_ref.py) over the CPU checker -- what it gains over marching cubes on the same grid,
constructed grids where its indexing can go wrong -- and the host side of the feature: the option's checker, the refusals, the ABI
entries.  No GPU.

The bounds against marching cubes are the issue's: a tenth of marching cubes' maximum deviation and volume error on the off-centre
box (a prototype measured a hundredth), below marching cubes on the example and on the rotated box, at most 1 % of the example's
faces against the gradient (a cap; the definition sits at 0.52 %).  The prints show what is reached."""
import functools
import os
import re

import numpy as np
import pytest

import dual_ref as ref
import fixtures
from sdf_amd import core, dual, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cube_bounds(half, shift=0.0):
    return ((-half + shift,) * 3, (half + shift,) * 3)


def weld_cells(soup):
    inv = np.unique(np.asarray(soup, dtype=np.float64).reshape(-1, 3), axis=0, return_inverse=True)[1]
    return np.asarray(inv, dtype=np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _both(name, samples):
    """(ev, the Dual, the marching-cubes soup (T, 3, 3)) of a model on its grid, made once"""
    import oracle
    import sdf_amd
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    f, bounds = {
        'box': lambda: (ns['box'](1), cube_bounds(0.6, 0.013)),
        'example': lambda: (fixtures.build('ex_example', ns), cube_bounds(0.85)),
        'rotated': lambda: (ns['box'](1).rotate(0.5, np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)), cube_bounds(0.95)),
    }[name]()
    X, Y, Z, _ = core.grid_axes(bounds, None, samples)
    ev = lambda P: oracle.evaluate(f, P)
    d = ref.dual(ev, X, Y, Z, core.default_normal_eps(bounds))
    mc = np.asarray(oracle.generate(f, X, Y, Z).points, dtype=np.float64).reshape(-1, 3, 3)
    return ev, d, mc


def test_off_centre_box(oracle_lib):
    ev, d, mc = _both('box', 2 ** 15)
    st = d.stats
    assert list(st) == list(ref.STAT_KEYS)
    census = ref.edge_census(d.cells)
    assert census['closed'] and census['oriented'] and census['euler'] == 2
    assert st['clamped'] == st['mean_fallback'] == st['flat'] == st['open_edges'] == st['nonfinite_edges'] == 0
    assert st['triangles'] == 2 * st['crossings'] == len(d.cells) and st['cells'] == len(d.vertices) == len(np.unique(d.cells))
    assert np.array_equal(d.soup, d.vertices[d.cells])
    assert ref.against_gradient(ev, d.soup, min_area=0.0)[0] == 0
    dev, dev_mc = ref.deviation(ev, d.soup), ref.deviation(ev, mc)
    vol, vol_mc = ref.volume(d.soup), ref.volume(mc)
    print('box at 2^15: max deviation %.3g (marching cubes %.3g), rms %.3g (%.3g), |1 - volume| %.3g (%.3g), %d triangles (%d)' % (
        dev[0], dev_mc[0], dev[1], dev_mc[1], abs(1 - vol), abs(1 - vol_mc), len(d.cells), len(mc)))
    assert dev[0] <= 0.1 * dev_mc[0]
    assert abs(1 - vol) <= 0.1 * abs(1 - vol_mc)


def test_example(oracle_lib):
    ev, d, mc = _both('example', 2 ** 18)
    census = ref.edge_census(d.cells)
    assert census['closed'] and census['oriented']
    dev, dev_mc = ref.deviation(ev, d.soup), ref.deviation(ev, mc)
    print('example at 2^18: max deviation %.3g (marching cubes %.3g), rms %.3g (%.3g), volume %.5f (%.5f), %d triangles (%d), stats %s' % (
        dev[0], dev_mc[0], dev[1], dev_mc[1], ref.volume(d.soup), ref.volume(mc), len(d.cells), len(mc), d.stats))
    assert dev[0] < dev_mc[0] and dev[1] < dev_mc[1]
    against, faces = ref.against_gradient(ev, d.soup, min_area=1e-12)
    print('example at 2^18: %d of %d faces of area > 1e-12 against the gradient: %.2f %%' % (against, faces, 100.0 * against / faces))
    assert against <= 0.01 * faces


def test_rotated_box(oracle_lib):
    ev, d, mc = _both('rotated', 2 ** 16)
    census = ref.edge_census(d.cells)
    assert census['oriented'] and census['boundary'] == 0
    dev, dev_mc = ref.deviation(ev, d.soup), ref.deviation(ev, mc)
    print('rotated box at 2^16: max deviation %.3g (marching cubes %.3g), rms %.3g (%.3g), volume %.5f (%.5f), %d non-manifold edges, '
          '%d faces against the gradient, stats %s' % (dev[0], dev_mc[0], dev[1], dev_mc[1], ref.volume(d.soup), ref.volume(mc),
                                                      census['nonmanifold'], ref.against_gradient(ev, d.soup)[0], d.stats))
    assert dev[1] < dev_mc[1]


# ---- constructed grids ----

def sphere_ev(r, centre=(0.0, 0.0, 0.0)):
    c = np.asarray(centre, dtype=np.float64)
    return lambda P: np.sqrt(((P - c) ** 2).sum(axis=1)) - r


def test_one_inside_corner_of_a_single_cell():
    ax = np.array([0.0, 1.0])
    d = ref.dual(sphere_ev(0.5), ax, ax, ax, 1e-4)
    assert d.stats == dict(dict.fromkeys(ref.STAT_KEYS, 0), crossings=3, cells=1, open_edges=3)
    assert d.edges.tolist() == [[0, 0], [0, 1], [0, 2]] and d.cells.shape == (0, 3) and d.soup.shape == (0, 3, 3)
    assert np.array_equal(d.points, 0.5 * np.eye(3))
    assert np.abs(d.vertices - 0.5).max() <= 0.5                       # inside its cell, whose centre is (0.5, 0.5, 0.5)


def test_only_the_centre_sample_inside():
    ax = np.array([-1.0, 0.0, 1.0])
    d = ref.dual(sphere_ev(0.5), ax, ax, ax, 1e-4)
    st = d.stats
    assert (st['crossings'], st['cells'], st['triangles'], st['open_edges']) == (6, 8, 12, 0)
    # the crossings by ascending (s, a): the three edges that END at the centre sample 13 first, then its own three
    assert d.edges.tolist() == [[4, 0], [10, 1], [12, 2], [13, 0], [13, 1], [13, 2]]
    census = ref.edge_census(d.cells)
    assert census['closed'] and census['oriented'] and census['euler'] == 2
    assert ref.volume(d.soup) > 0 and ref.against_gradient(sphere_ev(0.5), d.soup)[0] == 0
    assert d.active.tolist() == list(range(8))


def test_an_axis_of_two_samples():
    ax = np.arange(-8, 9) / 10.0
    Z = np.array([-0.05, 0.05])
    d = ref.dual(sphere_ev(0.5), ax, ax, Z, 1e-4)
    along = np.bincount(d.edges[:, 1], minlength=3)
    assert along[0] > 0 and along[1] > 0 and along[2] == 0            # the slab lies inside |z| < 0.5: no crossing along z
    assert d.stats['open_edges'] == d.stats['crossings'] == along[0] + along[1] and d.stats['triangles'] == 0
    # turned round: the two samples along x; the crossings along x have their four cells in (y, z) and emit, the others are open
    d = ref.dual(sphere_ev(0.5, (0.05, 0.0, 0.0)), np.array([0.0, 0.6]), ax, ax, 1e-4)
    along = np.bincount(d.edges[:, 1], minlength=3)
    assert along.min() > 0
    assert d.stats['open_edges'] >= along[1] + along[2] and d.stats['triangles'] == 2 * (d.stats['crossings'] - d.stats['open_edges'])
    assert d.stats['triangles'] <= 2 * along[0] and d.stats['triangles'] > 0
    for short in (np.array([0.0]), np.zeros(0)):
        e = ref.dual(sphere_ev(0.5), short, ax, ax, 1e-4)
        assert e.stats == dict.fromkeys(ref.STAT_KEYS, 0) and e.vertices.shape == (0, 3) and e.cells.shape == (0, 3) and e.cells.dtype == np.int64


def test_anisotropic_grid():
    X, Y, Z = np.arange(-0.5, 0.5, 0.05), np.arange(-0.5, 0.5, 0.07), np.arange(-0.5, 0.5, 0.06)
    ev = sphere_ev(0.4, (0.01, -0.02, 0.015))
    d = ref.dual(ev, X, Y, Z, 1e-4)
    census = ref.edge_census(d.cells)
    assert census['closed'] and census['oriented'] and census['euler'] == 2 and d.stats['open_edges'] == 0
    n = np.array([len(X), len(Y), len(Z)])
    ci = np.stack(np.unravel_index(d.active, tuple(n - 1)), axis=1)
    lo = np.stack([X[ci[:, 0]], Y[ci[:, 1]], Z[ci[:, 2]]], axis=1)
    hi = np.stack([X[ci[:, 0] + 1], Y[ci[:, 1] + 1], Z[ci[:, 2] + 1]], axis=1)
    ulp = np.spacing(1.0)                                              # (lo + h) + h is the cell's far face to a rounding or two
    assert ((d.vertices >= lo - 2 * ulp) & (d.vertices <= hi + 2 * ulp)).all()
    # The bound.  The corners of a triangle lie in cells that share a grid edge, so they are at most two cell diagonals apart, and a
    # chord of length L sags L^2 / (8 R) below a sphere of radius R; a vertex is the meet of tangent planes whose points lie within
    # half a diagonal of it, which stands (D / 2)^2 / (2 R) above the sphere.  The volume can be off by no more than the sphere's area
    # times that.
    R, D = 0.4, float(np.sqrt(0.05 ** 2 + 0.07 ** 2 + 0.06 ** 2))
    bound = (2 * D) ** 2 / (8 * R) + (D / 2) ** 2 / (2 * R)
    dev = ref.deviation(ev, d.soup)
    print('anisotropic sphere: max deviation %.3g (bound %.3g), volume %.5f of %.5f' % (dev[0], bound, ref.volume(d.soup), 4.0 / 3.0 * np.pi * R ** 3))
    assert dev[0] <= bound
    assert abs(ref.volume(d.soup) - 4.0 / 3.0 * np.pi * R ** 3) <= 4.0 * np.pi * R ** 2 * bound


def test_nonfinite_samples_next_to_a_sign_change():
    ax = np.arange(-6, 7) / 10.0
    base = sphere_ev(0.35)
    n = len(ax)
    at = lambda i, j, k: np.array([ax[i], ax[j], ax[k]])
    # +inf at (0.4, 0, 0), outside beside the inside sample (0.3, 0, 0); -inf, which counts as inside, at (0, 0.3, 0) beside the outside
    # (0, 0.4, 0); NaN, which does not, at (0, 0, -0.4) beside the inside (0, 0, -0.3)
    bad = {(10, 6, 6): np.inf, (6, 9, 6): -np.inf, (6, 6, 2): np.nan}

    def ev(P):
        v = base(P)
        for (i, j, k), value in bad.items():
            v[(P == at(i, j, k)).all(axis=1)] = value
        return v
    d = ref.dual(ev, ax, ax, ax, 1e-4)
    G = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), axis=-1).reshape(-1, 3)
    V = ev(G).reshape(n, n, n)
    want = 0
    for a in range(3):
        lo, hi = np.moveaxis(V, a, 0)[:-1], np.moveaxis(V, a, 0)[1:]
        want += int((((lo < 0) != (hi < 0)) & ~(np.isfinite(lo) & np.isfinite(hi))).sum())
    assert d.stats['nonfinite_edges'] == want and want >= 3
    bad_s = {(i * n + j) * n + k for i, j, k in bad}
    stride = np.array([n * n, n, 1])
    ends = set(d.edges[:, 0].tolist()) | set((d.edges[:, 0] + stride[d.edges[:, 1]]).tolist())
    assert not (ends & bad_s)                                          # no crossing, so no triangle, at a non-finite sample
    assert np.isfinite(d.points).all() and np.isfinite(d.vertices).all()
    clean = ref.dual(base, ax, ax, ax, 1e-4)
    assert d.stats['crossings'] < clean.stats['crossings'] and clean.stats['nonfinite_edges'] == 0


def test_zero_samples_are_not_inside():
    X = np.array([-0.2, -0.1, 0.0, 0.1, 0.2])
    Y = np.arange(4) * 0.1
    for ev, zero in ((lambda P: 0.0 - P[:, 0], 0.0), (lambda P: -P[:, 0], -0.0)):
        v0 = ev(np.array([[0.0, 0.0, 0.0]]))[0]
        assert v0 == 0.0 and np.signbit(v0) == np.signbit(zero)
        d = ref.dual(ev, X, Y, Y, 1e-4)
        # inside is x > 0: the sample at x = 0 is outside, the crossing runs from it to x = 0.1 and t = 0 puts it ON the sample
        assert d.stats['crossings'] == 16 and (d.edges[:, 1] == 0).all() and (d.edges[:, 0] // 16 == 2).all()
        assert (d.points[:, 0] == 0.0).all()
        assert np.array_equal(d.normals, np.tile([-1.0, 0.0, 0.0], (16, 1)))
        assert np.abs(d.vertices[:, 0]).max() <= 1e-12


# ---- the host side of the feature ----

def test_refusals_without_a_device(tmp_path, monkeypatch):
    assert dual.check_dual_option(False) is None and dual.check_dual_option(None) is None and dual.check_dual_option(True) == {}
    assert dual.check_dual_option({'eps': 1e-3}) == {'eps': 1e-3} and dual.check_dual_option({'reg': 0, 'eps': 1}) == {'reg': 0, 'eps': 1}
    for bad in ('yes', 1, 1.0, [], {'eps': 0.0}, {'eps': -1.0}, {'eps': float('nan')}, {'eps': float('inf')}, {'reg': -1e-9},
                {'reg': float('inf')}, {'reg': float('nan')}, {'tolerance': 1.0}, {'eps': 'small'}):
        with pytest.raises(ValueError):
            dual.check_dual_option(bad)
    assert dual.STAT_KEYS == ref.STAT_KEYS
    bounds = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    assert dual.dual_params({}, bounds) == (core.default_normal_eps(bounds), 1e-3) and dual.dual_params({'reg': 0.5, 'eps': 2}, bounds) == (2.0, 0.5)
    # a default is left out of the keywords a facade passes on
    assert core.pipeline_kwargs({'samples': 8}) == {'samples': 8} and core.pipeline_kwargs({}, dual=True) == {'dual': True}
    assert core.pipeline_kwargs({}, dual={'eps': 1.0}) == {'dual': {'eps': 1.0}} and core.pipeline_kwargs({'dual': True}) == {'dual': True}
    # the definition refuses what the device entry refuses
    ax = np.arange(4.0)
    ev = sphere_ev(1.0)
    for kw in ({'eps': 0.0}, {'eps': -1e-4}, {'eps': np.nan}, {'eps': np.inf}, {'reg': -1.0}, {'reg': np.nan}, {'reg': np.inf}):
        with pytest.raises(ValueError):
            ref.dual(ev, ax, ax, ax, **dict({'eps': 1e-4}, **kw))
        with pytest.raises(ValueError):
            dual.check_params(**dict({'eps': 1e-4, 'reg': 1e-3}, **kw))
    for bad in (np.array([0.0, np.inf]), np.array([np.nan, 1.0])):
        with pytest.raises(ValueError):
            ref.dual(ev, ax, bad, ax, 1e-4)
        with pytest.raises(ValueError):
            dual.check_axes(ax, bad, ax)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(2 ** 11,), strides=(0,))
    with pytest.raises(ValueError, match='2\\^31'):
        ref.dual(ev, huge, huge, np.zeros(2 ** 9), 1e-4)
    with pytest.raises(ValueError, match='2\\^31'):
        dual.check_axes(huge, huge, np.zeros(2 ** 9))
    # the pipeline refuses a bad dual= before it asks for an engine, and writes no file
    def no_engine(*a, **k):
        raise AssertionError('the engine was reached')
    monkeypatch.setattr(engine, 'get_engine', no_engine)
    from sdf_amd.measure import measure
    for bad in ({'tolerance': 1.0}, {'eps': 0}, 'yes', 3):
        with pytest.raises(ValueError):
            core.generate('model', dual=bad)
        with pytest.raises(ValueError):
            core.generate_mesh('model', dual=bad)
        with pytest.raises(ValueError):
            core.save(str(tmp_path / 'x.stl'), 'model', dual=bad)
        with pytest.raises(ValueError):
            measure('model', dual=bad)
        assert not (tmp_path / 'x.stl').exists()
    with pytest.raises(AssertionError, match='the engine was reached'):      # what is in order gets as far as the engine
        core.generate('model', dual={'eps': 1e-3, 'reg': 0.0})


def test_every_facade_hands_dual_to_meshed(monkeypatch):
    """the stand-in for `meshed` sees the keyword from every facade that meshes; without it, no facade passes one"""
    import sdf_amd
    seen = []

    class Reached(Exception):
        pass

    def stand_in(*args, **kwargs):
        seen.append(kwargs)
        raise Reached()
    monkeypatch.setattr(core, 'meshed', stand_in)
    calls = [lambda **kw: core.generate('model', **kw), lambda **kw: core.generate_mesh('model', **kw), lambda **kw: core.save('x.stl', 'model', **kw),
             lambda **kw: sdf_amd.measure('model', **kw), lambda **kw: sdf_amd.shells('model', **kw), lambda **kw: sdf_amd.measure_shells('model', **kw),
             lambda **kw: sdf_amd.overhangs('model', **kw), lambda **kw: sdf_amd.supports('model', **kw), lambda **kw: sdf_amd.thickness('model', **kw),
             lambda **kw: sdf_amd.curvature('model', **kw), lambda **kw: sdf_amd.deviation('model', **kw)]
    for call in calls:
        for option in (True, {'eps': 1e-3}):
            with pytest.raises(Reached):
                call(dual=option)
            assert seen[-1]['dual'] == option
        with pytest.raises(Reached):
            call()
        assert 'dual' not in seen[-1]


def test_abi_has_the_entry_points():
    names = ('sdf_generate_dual', 'sdf_dual_parts_fetch', 'sdf_dual_parts_destroy', 'sdf_generate_dual_last_kernel_ms')
    assert all(n in engine.ABI for n in names) and engine.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    assert re.search(r'\bint\s+sdf_generate_dual\s*\(', hdr) and re.search(r'\bdouble\s+sdf_generate_dual_last_kernel_ms\s*\(', hdr)
    assert re.search(r'\bint\s+sdf_dual_parts_fetch\s*\(', hdr) and re.search(r'\bint\s+sdf_dual_parts_destroy\s*\(', hdr)
    assert int(re.search(r'#define SDF_ABI_VERSION (\d+)', hdr).group(1)) == 17
    lib = engine.load_library()
    assert lib.sdf_abi_version() == 17 and all(getattr(lib, n) for n in names)
    assert callable(getattr(engine.Engine, 'generate_dual'))
    import sdf_amd
    assert callable(sdf_amd.dual_of_grid) and callable(dual.check_dual_option)
    units = [l.split() for l in open(os.path.join(ROOT, 'sdf_amd', 'csrc', 'build.units')) if l.strip() and not l.lstrip().startswith('#')]
    assert ['sdf_dual', 'sdf_dual.hip', 'plain'] in units
    assert [u[0] for u in units[-4:]] == ['sdf_dual', 'sdf_curvature', 'sdf_deviation', 'sdf_probe_out']


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = engine.load_library()
    assert lib.sdf_generate_dual(None, None, None, 2, None, 2, None, 2, 1e-4, 1e-3, 32, None, None, None) == 2
    assert b'sdf_generate_dual' in lib.sdf_last_error()
    assert lib.sdf_dual_parts_fetch(None, None, None, None, None) == 2 and b'sdf_dual_parts_fetch' in lib.sdf_last_error()
    assert lib.sdf_dual_parts_destroy(None) == 0
    assert lib.sdf_generate_dual_last_kernel_ms(None) == 0.0
