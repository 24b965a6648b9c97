"""The definitions of tests/measure_ref.py against closed forms (no GPU): dyadic coordinates, so the expected values are exact or
within 4 ulp; the constructed cases of the edge census; the ABI."""
import os
import re

import numpy as np
import pytest

import measure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def within_ulp(got, want, n=4):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= n * np.spacing(np.abs(want))).all())


def measured(soup, origin=None):
    m = ref.moments(soup, origin)
    return m, ref.derive(m)


def test_unit_cube_is_exact():
    m, d = measured(ref.cube_soup())
    assert d['volume'] == 1.0 and d['area'] == 6.0
    assert np.array_equal(d['centroid'], [1.0, 1.0, 1.0])
    assert np.array_equal(m['origin'], [1.0, 1.0, 1.0]) and np.array_equal(m['box'], [[0.5] * 3, [1.5] * 3])
    assert within_ulp(np.diag(d['inertia']), [1 / 6] * 3)
    off = d['inertia'][~np.eye(3, dtype=bool)]
    assert (off == 0).all(), off
    assert m['triangles'] == 12 and m['zero_area'] == 0 and m['nonfinite'] == 0


def test_translation_changes_no_bit_of_volume_area_inertia():
    """the reference point at work: the midpoint of the box moves with the cube, the relative coordinates are the same"""
    m0, d0 = measured(ref.cube_soup())
    shift = (1024.0, -512.0, 256.0)
    m1, d1 = measured(ref.cube_soup(shift=shift))
    assert np.array_equal(bits(m0['sums']), bits(m1['sums']))
    for k in ('volume', 'area', 'inertia'):
        assert np.array_equal(bits(d0[k]), bits(d1[k])), k
    assert np.array_equal(d1['centroid'], np.array([1.0, 1.0, 1.0]) + shift)
    # about the world's origin the same cube does not come out exact: that is what the reference point is for
    far = ref.derive(ref.moments(ref.cube_soup(shift=shift), origin=(0, 0, 0)))
    assert not np.array_equal(bits(far['inertia']), bits(d0['inertia']))


def test_right_tetrahedron():
    m, d = measured(ref.tetrahedron_soup())
    assert within_ulp(d['volume'], 1 / 6) and within_ulp(d['centroid'], [0.25] * 3)
    assert within_ulp(d['area'], (3 + np.sqrt(3.0)) / 2)
    # about the centroid: I_xx = I_yy = I_zz = 1/80 (3 V / 40 ...): checked against the closed form of the right tetrahedron
    assert np.allclose(np.diag(d['inertia']), [1 / 80] * 3, rtol=0, atol=1e-15)
    assert np.allclose(d['inertia'][0, 1], 1 / 480, rtol=0, atol=1e-15)


def test_inside_out_cube():
    m, d = measured(ref.cube_soup()[:, [0, 2, 1]])
    assert d['volume'] == -1.0 and d['area'] == 6.0
    assert np.isnan(d['centroid']).all() and np.isnan(d['inertia']).all()


def test_nonfinite_and_zero_area_triangles_are_counted_and_add_nothing():
    cube = ref.cube_soup()
    bad = cube[3].copy()
    bad[1, 2] = np.nan
    flat = np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]])           # collinear, inside the box
    soup = np.concatenate([cube[:5], [bad], cube[5:], [flat]])
    m = ref.moments(soup)
    assert m['nonfinite'] == 1 and m['zero_area'] == 1 and m['triangles'] == 14
    assert np.array_equal(m['box'], [[0.5] * 3, [1.5] * 3])
    assert np.array_equal(bits(m['sums']), bits(ref.moments(cube)['sums']))
    d = ref.derive(m)
    assert d['volume'] == 1.0 and np.isnan(d['centroid']).all() and np.isnan(d['inertia']).all()


def test_empty_soup():
    m = ref.moments(np.zeros((0, 3, 3)))
    assert not m['sums'].any() and m['triangles'] == 0 and np.array_equal(m['origin'], [0, 0, 0])
    assert np.array_equal(m['box'], [[np.inf] * 3, [-np.inf] * 3])
    d = ref.derive(m)
    assert d['volume'] == 0 and d['area'] == 0 and np.isnan(d['centroid']).all()


def test_the_tree_is_the_stated_one():
    """the same terms summed by hand: lanes in index order, then halving, then groups of 256 partials"""
    rng = np.random.RandomState(3)
    T = 256 * ref.C + 1                                          # three levels
    x = rng.uniform(-1, 1, size=(T, 1))
    got = ref.tree_sum(x)[0]
    def halve(v):
        v = list(v)
        h = 128
        while h >= 1:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]
    parts = []
    for c0 in range(0, T, ref.C):
        chunk = list(x[c0:c0 + ref.C, 0]) + [0.0] * (ref.C - len(x[c0:c0 + ref.C]))
        lanes = []
        for l in range(256):
            a = 0.0
            for s in range(ref.C // 256):
                a = a + chunk[s * 256 + l]
            lanes.append(a)
        parts.append(halve(lanes))
    while len(parts) > 1:
        parts = [halve(parts[g:g + 256] + [0.0] * (256 - len(parts[g:g + 256]))) for g in range(0, len(parts), 256)]
    assert got.tobytes() == np.float64(parts[0]).tobytes()
    # ... and it depends on the order of the triangles
    assert abs(got - ref.tree_sum(x[::-1])[0]) <= 1e-9 and np.isfinite(got)


@pytest.mark.parametrize('name', sorted(ref.census_cases()))
def test_census_cases(name):
    soup, want = ref.census_cases()[name]
    pts, cells = ref.weld(soup)
    got = ref.edge_census(cells, len(pts))
    for k, v in want.items():
        assert got[k] == v and type(got[k]) is type(v), (name, k, got[k], v)
    assert got['edges'] == got['paired'] + got['boundary'] + got['misoriented'] + got['nonmanifold']
    assert got['euler'] == got['vertices'] - got['edges'] + got['faces']


@pytest.mark.parametrize('k', (1, 2, 3, 4, 5))
def test_books(k):
    pts, cells = ref.weld(ref.book_soup(k, 21))
    got = ref.edge_census(cells, len(pts))
    # the shared edge, and per page two edges of its own; per padding triangle three
    want_shared = {1: 'boundary', 2: 'misoriented'}.get(k, 'nonmanifold')
    assert got[want_shared] >= 1 and got['boundary'] == 63 + 2 * k + (1 if k == 1 else 0)
    assert got['misoriented'] == (1 if k == 2 else 0) and got['nonmanifold'] == (1 if k >= 3 else 0) and got['paired'] == 0
    keys = np.sort(ref.edge_keys(cells)[0])
    run = np.flatnonzero((keys >> np.uint64(1)) == (keys[63] >> np.uint64(1)))
    assert run[0] == 63 and len(run) == k


def test_abi_15_declares_the_measurements():
    from sdf_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION and version >= 15
    for name in ('sdf_mesh_moments', 'sdf_mesh_edge_census', 'sdf_mesh_measure_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    import ctypes
    assert ctypes.sizeof(engine.SdfMoments) == (11 + 3 + 6 + 3) * 8 and ctypes.sizeof(engine.SdfEdgeCensus) == 11 * 8


def test_measure_result_restates_the_definition():
    """sdf_amd/measure.py derives the public values from the device's totals with the definition's operations"""
    import importlib
    measure = importlib.import_module('sdf_amd.measure')
    for soup in (ref.cube_soup(shift=(3.0, 0.25, -7.0)), ref.tetrahedron_soup(), ref.cube_soup()[:, [0, 2, 1]]):
        m = ref.moments(soup)
        want, got = ref.derive(m), measure.derive(m)
        for k in ('area', 'volume', 'centroid', 'inertia'):
            assert np.array_equal(bits(got[k]), bits(want[k])), k
