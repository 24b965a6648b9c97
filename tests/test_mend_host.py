"""The definition of mesh mending (tests/mend_ref.py) against a dictionary version and on constructed cases, its invariants, the
thin-plates model it was made for, `check_mend` and the keyword through every entry point, and the ABI's new names: what can be checked
without a device."""
import importlib
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import measure_ref
import mend_ref as ref
import simplify_ref
from sdf_amd import core, engine

mend = importlib.import_module('sdf_amd.mend')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition against a loop over the triangles ----
def brute(cells):
    """(keep (T,) bool, stats): the four steps of the definition, one triangle at a time"""
    groups, collapsed = {}, 0
    for t, (i, j, k) in enumerate(np.asarray(cells).reshape(-1, 3).tolist()):
        if i == j or j == k or i == k:
            collapsed += 1
            continue
        a, b, c = min(((i, j, k), (j, k, i), (k, i, j)))          # the rotation that starts with the smallest index
        groups.setdefault((a, min(b, c), max(b, c)), ([], []))[1 if b > c else 0].append(t)
    keep = np.zeros(len(cells), bool)
    duplicates = cancelled = 0
    for side0, side1 in groups.values():
        if len(side0) == len(side1):
            cancelled += 2 * len(side0)
        else:
            keep[(side0 if len(side0) > len(side1) else side1)[0]] = True
            duplicates += len(side0) + len(side1) - 1
    return keep, {'triangles_in': len(cells), 'triangles_out': int(keep.sum()), 'collapsed': collapsed, 'duplicates': duplicates,
                  'cancelled': cancelled, 'faces': len(groups)}


def agree(cells):
    got = ref.mend(cells)
    keep, stats = brute(cells)
    assert np.array_equal(got.keep, keep) and got.stats == stats and list(got.stats) == list(ref.STAT_KEYS)
    assert all(isinstance(v, int) for v in got.stats.values())
    s = got.stats
    assert s['triangles_in'] == s['triangles_out'] + s['collapsed'] + s['duplicates'] + s['cancelled']
    return got


@pytest.mark.parametrize('n_vertices, n_tris', ((3, 40), (4, 60), (5, 200), (9, 500), (40, 300)))
def test_random_index_soups(n_vertices, n_tris):
    """few vertices, many triangles: faces repeat in every order and many cells are collapsed"""
    rng = np.random.RandomState(n_vertices * 1000 + n_tris)
    got = agree(rng.randint(0, n_vertices, size=(n_tris, 3)).astype(np.int64))
    if n_vertices <= 9:                                           # (more triangles than there are faces and sides)
        assert got.stats['collapsed'] > 0 and got.stats['duplicates'] + got.stats['cancelled'] > 0


def test_one_face_in_all_six_orders():
    orders = list(itertools.permutations((7, 3, 5)))
    face, side, collapsed = ref.faces_and_sides(np.array(orders))
    assert (face == [3, 5, 7]).all() and not collapsed.any()
    # (3, 5, 7) and its rotations are side 0; (3, 7, 5) and its rotations side 1
    assert side.tolist() == [0 if o in ((3, 5, 7), (5, 7, 3), (7, 3, 5)) else 1 for o in orders]
    assert agree(np.array(orders)).stats == dict(triangles_in=6, triangles_out=0, collapsed=0, duplicates=0, cancelled=6, faces=1)
    for r in range(1, 7):
        for pick in itertools.combinations(range(6), r):
            agree(np.array([orders[i] for i in pick]))


# ---- the constructed cases (shared with tests/test_mend_gpu.py) ----
@pytest.mark.parametrize('name', sorted(ref.mend_cases()))
def test_constructed_cases(name):
    soup, want = ref.mend_cases()[name]
    got = ref.mend_soup(soup)
    assert got.stats == want, (name, got.stats)
    assert got.soup.shape == (want['triangles_out'], 3, 3) and got.soup.dtype == np.float64
    agree(ref.weld(soup)[1])
    if name == 'cube':
        assert np.array_equal(got.soup.view(np.int64), soup.view(np.int64))


@pytest.mark.parametrize('n0, n1', ref.REPEATS)
def test_the_survivor_is_the_first_of_the_majority_side(n0, n1):
    soup, survivor = ref.repeated_face(n0, n1)
    got = ref.mend_soup(soup)
    shared = np.flatnonzero(got.face[:, 0] == got.face[:, 0].max())          # the repeated face's vertices sort last
    assert len(shared) == n0 + n1
    assert np.flatnonzero(got.keep[shared]).tolist() == ([] if survivor is None else [shared.tolist().index(survivor)])
    assert got.keep.sum() == 7 + (survivor is not None)


def test_negative_zero_stays_and_the_winding_is_unchanged():
    cube = measure_ref.cube_soup(lo=0.0, hi=1.0)
    cube[cube == 0.0] = -0.0
    soup = np.concatenate([cube[:, [1, 2, 0]], cube + 0.0])       # (+ 0.0 turns -0.0 into +0.0: the second copy welds onto the first)
    got = ref.mend_soup(soup)
    assert got.stats['duplicates'] == 12 and np.array_equal(got.soup.view(np.int64), soup[:12].view(np.int64)) and np.signbit(got.soup).any()


@pytest.mark.parametrize('k, flipped, n_pad', ((63, 0, 200), (64, 32, 255), (65, 32, 190), (66, 40, 10), (257, 128, 100)))
def test_long_runs(k, flipped, n_pad):
    soup = ref.long_run(k, n_pad, flipped)
    got = ref.mend_soup(soup)
    one = k != 2 * flipped
    assert got.stats == dict(triangles_in=n_pad + k, triangles_out=n_pad + one, collapsed=0, duplicates=(k - 1) if one else 0,
                             cancelled=0 if one else k, faces=n_pad + 1)
    assert np.flatnonzero(got.keep[n_pad:]).tolist() == ([0 if k > 2 * flipped else k - flipped] if one else [])


# ---- invariants ----
def test_mending_a_mended_mesh_removes_nothing():
    rng = np.random.RandomState(4)
    pts = rng.uniform(0, 1, (12, 3))
    soup = pts[rng.randint(0, 12, size=(400, 3))]
    first = ref.mend_soup(soup)
    assert 0 < first.stats['triangles_out'] < 400
    again = ref.mend_soup(first.soup)
    n = first.stats['triangles_out']
    assert again.stats == dict(triangles_in=n, triangles_out=n, collapsed=0, duplicates=0, cancelled=0, faces=n)
    assert np.array_equal(again.soup.view(np.int64), first.soup.view(np.int64))


def test_survivors_are_in_soup_order_under_a_shuffle():
    rng = np.random.RandomState(5)
    cells = rng.randint(0, 8, size=(300, 3)).astype(np.int64)
    soup = rng.uniform(0, 1, (8, 3))[cells]
    base = ref.mend(cells, soup)
    for seed in range(3):
        perm = np.random.RandomState(seed).permutation(len(cells))
        got = agree(cells[perm])
        assert {k: v for k, v in got.stats.items()} == base.stats                   # what survives is a set of faces and sides ...
        key = lambda m: sorted(map(tuple, np.c_[m.face[m.keep], m.side[m.keep]].tolist()))
        assert key(got) == key(base)
        out = ref.mend(cells[perm], soup[perm]).soup                                 # ... and it comes out in the order it went in
        assert np.array_equal(out, soup[perm][np.flatnonzero(got.keep)]) and (np.diff(np.flatnonzero(got.keep)) > 0).all()


def test_refusals_of_the_definition():
    with pytest.raises(ValueError, match='2\\^31'):
        ref.mend(np.array([[0, 1, 2 ** 31]]))
    with pytest.raises(ValueError, match='2\\^31'):
        ref.mend(np.lib.stride_tricks.as_strided(np.zeros(3, np.int64), shape=((2 ** 31 + 2) // 3, 3), strides=(0, 8), writeable=False))
    with pytest.raises(ValueError, match='negative'):
        ref.mend(np.array([[0, 1, -2]]))
    with pytest.raises(ValueError, match='soup'):
        ref.mend(np.array([[0, 1, 2]]), np.zeros((2, 3, 3)))


# ---- the model the feature was made for ----
def test_two_thin_plates_simplified_and_mended(ns, oracle_lib):
    """`box((2, 2, 0.12)) | box((2, 2, 0.12)).translate((0, 0, 0.3))` on X = Y = Z = arange(-1.3, 1.3 + 0.025, 0.05), meshed by the
    checker, simplified by the definition at k = 4 and mended by the definition.  The definition gives: 880 triangles after
    simplify, 280 non-manifold edges, not closed; 400 cancelled, 0 duplicates, 0 collapsed; 480 triangles after mending, 0
    non-manifold edges, closed and oriented; the area falls from 16.95 to 8.827 and the volume stays 0.470075."""
    step, ext = 0.05, 1.3
    plate = ns['box']((2, 2, 0.12))
    f = plate | plate.translate((0, 0, 0.3))
    X = np.arange(-ext, ext + step / 2, step)
    soup = oracle_lib.generate(f, X, X, X, 32, True).points.reshape(-1, 3, 3)
    pts, cells = ref.weld(soup)
    before = measure_ref.edge_census(cells, len(pts))
    assert before['closed'] and before['oriented']
    small = simplify_ref.simplify(pts, cells, np.full(3, X[0]), np.full(3, 4 * step)).soup
    sp, sc = ref.weld(small)
    folded = measure_ref.edge_census(sc, len(sp))
    got = ref.mend(sc, small)
    mp, mc = ref.weld(got.soup)
    after = measure_ref.edge_census(mc, len(mp))
    m0, m1 = (measure_ref.derive(measure_ref.moments(s)) for s in (small, got.soup))
    print('simplified %d triangles, nonmanifold %d; mended %s; nonmanifold %d; area %.4g -> %.4g, volume %.6g -> %.6g' % (
        len(small), folded['nonmanifold'], got.stats, after['nonmanifold'], m0['area'], m1['area'], m0['volume'], m1['volume']))
    assert got.stats['cancelled'] > 0
    assert not folded['closed'] and folded['nonmanifold'] > 0
    assert after['closed'] and after['oriented'] and after['nonmanifold'] == 0 and after['boundary'] == 0
    assert (len(small), folded['nonmanifold'], got.stats['cancelled'], len(got.soup)) == (880, 280, 400, 480)
    assert got.stats['duplicates'] == 0 and got.stats['collapsed'] == 0
    assert abs(m1['volume'] - m0['volume']) <= 1e-12 * abs(m0['volume']) and m1['area'] < 0.6 * m0['area']
    assert ref.mend(mc, got.soup).stats['triangles_out'] == len(got.soup)


# ---- the host side of the package ----
def test_check_mend():
    assert mend.check_mend(False) is False and mend.check_mend(True) is True
    assert mend.check_mend(np.bool_(True)) is True and mend.check_mend(np.bool_(False)) is False
    for bad in (None, 0, 1, 1.0, 'yes', 'True', (), [True], np.int64(1), np.array([True])):
        with pytest.raises(ValueError, match='mend'):
            mend.check_mend(bad)


def test_mend_is_refused_before_anything_is_meshed():
    """a mend that is no boolean raises ValueError before the engine is asked for: this passes without a device"""
    import sdf_amd
    f = sdf_amd.sphere(1)
    for bad in (None, 1, 0, 'yes', 2.0):
        for call in (f.generate_mesh, f.measure, f.shells, f.measure_shells):
            with pytest.raises(ValueError, match='mend'):
                call(mend=bad, samples=2 ** 10, verbose=False)
        with pytest.raises(ValueError, match='mend'):
            f.save('never_mended.stl', mend=bad, samples=2 ** 10, verbose=False)
    assert not os.path.exists('never_mended.stl')


def test_the_public_names():
    measure = importlib.import_module('sdf_amd.measure')
    shells = importlib.import_module('sdf_amd.shells')
    mesh = importlib.import_module('sdf_amd.mesh')
    for fn in (core.save, core.generate_mesh, core.meshed.__wrapped__, measure.measure, shells.shells, shells.measure_shells):
        assert inspect.signature(fn).parameters['mend'].default is False, fn
    assert 'mend' not in inspect.signature(core.generate).parameters          # the reference's signature
    assert core.Meshed._fields[-1] == 'simplify_stats' and 'mend_stats' not in core.Meshed._fields
    assert core.generate_mesh.last_mend is None or isinstance(core.generate_mesh.last_mend, dict)
    assert callable(engine.Mesh.mend) and callable(mesh.Mesh.mend)
    assert list(inspect.signature(mesh.Mesh.mend).parameters) == ['self'] and list(inspect.signature(engine.Mesh.mend).parameters) == ['self']


def test_the_abi_names_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION == 17                    # added under ABI 17
    assert 'added under ABI 17' in hdr
    for name in ('sdf_mesh_mend', 'sdf_mesh_mend_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    lib = engine.load_library()
    assert lib.sdf_abi_version() == version and hasattr(lib, 'sdf_mesh_mend') and all(hasattr(lib, n) for n in engine.ABI)
    fields = ['triangles_in', 'triangles_out', 'collapsed', 'duplicates', 'cancelled', 'faces', 'kernel_ms']
    assert [k for k, _ in engine.SdfMendStats._fields_] == fields
    m = re.search(r'typedef struct sdf_mend_stats \{(.*?)\} sdf_mend_stats;', hdr, re.S).group(1)
    assert re.findall(r'\b(%s)\b' % '|'.join(fields), m) == fields
    assert engine.MEND_FIELDS == ref.STAT_KEYS
