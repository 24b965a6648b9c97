"""The host side of tests/test_mesh_readers_gpu.py: the constructed soups (tests/soups_ref.py) are what the golden was recorded for and
hold what they are there for, `stl.stl_records` writes the reference's bytes for them (tests/golden/stl_soups.npz, made by
tools/make_golden_stl.py from the unmodified reference), the two lattice models keep their degenerate triangles, the PLY packer of
tests/normals_ref.py reads back at every face count of the device test, and the weld's expectation is right on an example whose
answer is written out.  Nothing here needs a device."""
import hashlib
import os

import numpy as np
import pytest

import normals_ref
import soups_ref
from conftest import GOLDEN
from sdf_amd import core, stl

NEG_QNAN = 0xffc00000                    # what 0/0 gives in float32 on x86-64, and so in the reference's file
LATTICE = dict(step=0.125, bounds=((-1, -1, -1), (1, 1, 1)), sparse=False)
LATTICE_MODELS = ('box', 'octahedron')
# triangles and records with a NaN normal, (a) of the recorded files -- the reference's grid, np.arange(-1, 1, 0.125), 16 samples an
# axis, which cuts the octahedron's tips at +1 off -- and (b) on the closed lattice np.arange(-1, 1.0001, 0.125) of
# test_gpu.py::test_weld_handles_signed_zeros_and_empty, where these counts were first taken
RECORDED_COUNTS = {'box': (968, 200), 'octahedron': (1640, 1140)}
CLOSED_LATTICE_COUNTS = {'box': (968, 200), 'octahedron': (1712, 1200)}

_golden = {}
STL_CASES = [(key, cls) for key, cls, soup in soups_ref.stl_cases()]
CLASS_A_KEYS = [k for k, c in STL_CASES if c == 'A']
CLASS_B_KEYS = [k for k, c in STL_CASES if c == 'B']


def golden():
    if not _golden:
        d = np.load(os.path.join(GOLDEN, 'stl_soups.npz'))
        _golden.update({k: d[k] for k in d.files})
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def stl_soup(key):
    """the soup of a golden key, checked against the sha256 the golden tool took of it"""
    name, T = key.rsplit('_', 1)
    soup = soups_ref.class_b(name[2:]) if name.startswith('b_') else soups_ref.class_a(name, int(T))
    assert len(soup) == 3 * int(T)
    assert hashlib.sha256(soup.tobytes()).digest() == golden()['sha_' + key].tobytes(), 'the builder of %s drifted from the golden' % key
    return soup


def record_words(rec):
    """(T, 12) uint32: the float32 words of T 50-byte records; the attribute (2 bytes) is returned apart"""
    r = np.ascontiguousarray(np.asarray(rec).view(np.uint8).reshape(-1, 50))
    return r[:, :48].copy().view('<u4'), r[:, 48:].copy()


def is_nan_word(w):
    return ((w & 0x7f800000) == 0x7f800000) & ((w & 0x007fffff) != 0)


def same_records(got, want, cls):
    """class A: every byte.  Class B: NaN in the same 32-bit words, every other word and the attribute bit-equal"""
    got, want = np.asarray(got).view(np.uint8).reshape(-1), np.asarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    if cls == 'A':
        bad = np.flatnonzero(got != want)
        if len(bad):
            t = int(bad[0]) // 50
            gw, ww = record_words(got)[0][t], record_words(want)[0][t]
            raise AssertionError('%d bytes of %d records differ, first in record %d:\n got  %s\n want %s' % (
                len(bad), len(np.unique(bad // 50)), t, ' '.join('%08x' % x for x in gw), ' '.join('%08x' % x for x in ww)))
        return
    (gw, ga), (ww, wa) = record_words(got), record_words(want)
    gn, wn = is_nan_word(gw), is_nan_word(ww)
    assert np.array_equal(gn, wn), 'NaN in other words: first at %s' % (np.argwhere(gn != wn)[0],)
    assert np.array_equal(gw[~wn], ww[~wn]) and np.array_equal(ga, wa)


def weld_expectation(rows):
    """(unique rows (U, 3) float64, cells (T, 3) int64): np.unique(rows, axis=0, return_inverse=True) with the signs of zero that the
    header of csrc/sdf_weld.hip documents -- a class of rows that differ only in them is represented by its first row of the soup"""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
    pts, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = np.asarray(inv, dtype=np.int64).reshape(-1)
    first = np.full(len(pts), len(rows), dtype=np.int64)
    np.minimum.at(first, inv, np.arange(len(rows), dtype=np.int64))
    rep = rows[first]
    assert np.array_equal(rep, pts)                      # (==: the same rows up to the signs of zero)
    return rep, inv.reshape(-1, 3)


# ---- the soups hold what they are there for ----
def normal_words(soup):
    return record_words(stl.stl_records(soup))[0][:, :3]


def test_the_golden_holds_every_case_and_count():
    g = golden()
    assert list(g['keys']) == [k for k, c in STL_CASES]
    want = ['%s_%d' % (n, T) for n in soups_ref.CLASS_A for T in soups_ref.COUNTS] + ['wide_exponent_513']
    assert CLASS_A_KEYS == want and CLASS_B_KEYS == ['b_%s_64' % n for n in soups_ref.CLASS_B]
    assert soups_ref.COUNTS == (1, 255, 256, 257)
    for k, c in STL_CASES:
        assert len(g['rec_' + k]) == 50 * int(k.rsplit('_', 1)[1])


@pytest.mark.parametrize('name', soups_ref.CLASS_A)
def test_class_a_soups_are_what_their_names_say(name):
    soup = stl_soup('%s_257' % name)
    tri32 = soup.astype(np.float32).reshape(-1, 3, 3)
    assert np.isfinite(tri32).all() and np.abs(tri32).max() <= 2.0 ** 60
    w = normal_words(soup)
    nan = is_nan_word(w)
    assert (w[nan] == NEG_QNAN).all()                    # the only NaN of class A is 0/0, whose bits do not depend on the operands
    with np.errstate(all='ignore'):
        e1, e2 = tri32[:, 1] - tri32[:, 0], tri32[:, 2] - tri32[:, 0]
        cross = np.cross(e1, e2)
    if name in ('duplicate', 'collinear', 'f32_collapse', 'tiny'):
        assert nan.all() and not cross.any()
    if name == 'duplicate':
        t = soup.reshape(-1, 3, 3)
        eq = np.stack([(t[:, 0] == t[:, 1]).all(axis=1), (t[:, 0] == t[:, 2]).all(axis=1), (t[:, 1] == t[:, 2]).all(axis=1)], axis=1)
        assert {tuple(r) for r in eq.tolist()} == {(True, False, False), (False, True, False), (False, False, True), (True, True, True)}
    if name == 'collinear':
        t = soup.reshape(-1, 3, 3)
        assert e1.any(axis=1).all() and e2.any(axis=1).all() and np.array_equal(t.astype(np.float32).astype(np.float64), t)
        s = (e1.astype(np.float64) * e2).sum(axis=1)
        assert (s > 0).any() and (s < 0).any()            # both orientations
    if name == 'f32_collapse':
        t = soup.reshape(-1, 3, 3)
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (tri32[:, 0] == tri32[:, 1]).all() and (tri32[:, 0] == tri32[:, 2]).all()
    if name == 'tiny':
        assert e1.all() and e2.all()                      # the edges are there; their products are not
    if name == 'denormal':
        tiny32 = np.finfo(np.float32).tiny
        assert cross.all() and (np.abs(cross) < tiny32).all()                   # every component a float32 denormal
        assert not nan.any() and np.isinf(w.view('<f4')).all()                  # ... a flushed one would give 0/0 here
    if name == 'wide_exponent':
        # the components themselves are normal numbers (the smallest product of two edges is of the order 2^-120) or cancel to
        # zero; it is their squares, the terms of the length, that are normal, denormal, zero behind a non-zero component, or inf
        with np.errstate(all='ignore'):
            sq = cross * cross
        tiny32 = np.finfo(np.float32).tiny
        assert (cross == 0).any() and ((sq == 0) & (cross != 0)).any() and ((sq > 0) & (sq < tiny32)).any()
        assert ((sq >= tiny32) & np.isfinite(sq)).any() and np.isinf(sq).any()
        f = w.view('<f4')
        assert np.isinf(f).any() and (f == 0).any() and (np.isfinite(f) & (f != 0)).any()
    if name == 'signed_zero':
        neg0 = np.uint32(0x80000000)
        assert (tri32.view(np.uint32) == neg0).any() and (w == neg0).any() and (w == 0).any()
        planar = (tri32 == 0).all(axis=1)                 # (T, 3): a whole column of a triangle is zero
        assert planar.any(axis=1).all() and planar[:, 0].any() and planar[:, 1].any() and planar[:, 2].any()
    if name == 'ordinary':
        ln = np.sqrt((w.view('<f4').astype(np.float64) ** 2).sum(axis=1))
        assert not nan.any() and (np.abs(ln - 1) < 1e-6).all()


@pytest.mark.parametrize('name', soups_ref.CLASS_B)
def test_class_b_soups_are_what_their_names_say(name):
    soup = stl_soup('b_%s_64' % name)
    with np.errstate(all='ignore'):
        f = soup.astype(np.float32)
    if name == 'nan':
        assert np.isnan(soup).any(axis=1).any() and not np.signbit(soup[np.isnan(soup)]).any()
    if name == 'inf':
        assert (soup == np.inf).any() and (soup == -np.inf).any()
    if name == 'overflow':
        assert np.isfinite(soup).all() and (f == np.inf).any() and (f == -np.inf).any()
    if name == 'huge':
        assert np.isfinite(f).all() and (np.abs(f) > 1e18).any()
    with np.errstate(all='ignore'):
        assert is_nan_word(record_words(stl.stl_records(soup))[0]).any()


# ---- stl.stl_records against the reference's bytes ----
@pytest.mark.parametrize('key,cls', STL_CASES, ids=[k for k, c in STL_CASES])
def test_host_stl_records_are_the_reference_bytes(key, cls):
    soup = stl_soup(key)
    with np.errstate(all='ignore'):
        got = stl.stl_records(soup).tobytes()
    same_records(np.frombuffer(got, np.uint8), golden()['rec_' + key], cls)


def lattice_file(name):
    """(records (T x 50 uint8), T) of a recorded file, its header checked"""
    raw = golden()['stl_' + name].tobytes()
    T = int(np.frombuffer(raw, '<u4', 1, 80)[0])
    assert raw[:80] == b'\x00' * 80 and len(raw) == 84 + 50 * T
    return np.frombuffer(raw, np.uint8, 50 * T, 84), T


def nan_normals(rec):
    """(records with a NaN normal, the set of NaN words among the normals)"""
    w = record_words(rec)[0][:, :3]
    nan = is_nan_word(w)
    return int(nan.any(axis=1).sum()), set(w[nan].tolist())


@pytest.mark.parametrize('name', LATTICE_MODELS)
def test_lattice_models_keep_their_degenerate_triangles(name, ns, oracle_lib):
    rec, T = lattice_file(name)
    assert (T, nan_normals(rec)[0]) == RECORDED_COUNTS[name] and nan_normals(rec)[1] == {NEG_QNAN}
    f = ns[name](1)
    X, Y, Z, _ = core.grid_axes(LATTICE['bounds'], LATTICE['step'])
    soup = oracle_lib.generate(f, X, Y, Z, 32, False).points
    with np.errstate(all='ignore'):
        same_records(stl.stl_records(soup).view(np.uint8).reshape(-1), rec, 'A')
    # the closed lattice, where the counts were first taken: a fifth of the box's records, most of the octahedron's
    A = np.arange(-1.0, 1.0001, 0.125)
    soup = oracle_lib.generate(f, A, A, A, 32, False).points
    with np.errstate(all='ignore'):
        n, words = nan_normals(stl.stl_records(soup))
    assert (len(soup) // 3, n) == CLOSED_LATTICE_COUNTS[name] and words == {NEG_QNAN}
    t = soup.reshape(-1, 3, 3)
    two_equal = (t[:, 0] == t[:, 1]).all(axis=1) | (t[:, 0] == t[:, 2]).all(axis=1) | (t[:, 1] == t[:, 2]).all(axis=1)
    assert int(two_equal.sum()) == n


# ---- the PLY packer reads back at every face count of the device test ----
@pytest.mark.parametrize('T', soups_ref.PLY_COUNTS)
@pytest.mark.parametrize('with_normals', (False, True), ids=('plain', 'normals'))
def test_ply_records_parse_back_at_every_face_count(T, with_normals, tmp_path):
    assert sorted({(13 * t) % 4 for t in soups_ref.PLY_COUNTS if t < 256}) == [0, 1, 2, 3]
    assert sorted({(13 * (t - 256 * (t // 256))) % 4 for t in soups_ref.PLY_COUNTS if t > 256}) == [1, 3]
    pts, cells = weld_expectation(soups_ref.class_a('ordinary', T))
    assert len(pts) == 3 * T and cells.shape == (T, 3)
    n = np.random.RandomState(T).standard_normal(pts.shape) if with_normals else None
    vb, fb = normals_ref.ply_records(pts, cells, n)
    assert len(vb) == len(pts) * (24 if with_normals else 12) and len(fb) == 13 * T
    path = str(tmp_path / 'a.ply')
    head = normals_ref.ply_header(len(pts), T, with_normals)
    with open(path, 'wb') as fp:
        fp.write(head + vb.tobytes() + fb.tobytes())
    p, nn, c, h = normals_ref.parse_ply(path)
    assert h == head and np.array_equal(p.view(np.int32), pts.astype(np.float32).view(np.int32)) and np.array_equal(c, cells)
    if with_normals:
        assert np.array_equal(nn.view(np.int32), n.astype(np.float32).view(np.int32))
    else:
        assert nn is None


# ---- the weld's expectation ----
def test_weld_expectation_on_a_written_out_example():
    rows = np.array([[1.0, -0.0, 2.0],       # class b, first member: -0.0 in column 1, +0.0 nowhere
                     [-1.0, 5.0, 0.0],       # class a
                     [1.0, 0.0, 2.0],        # class b again, with the other zero
                     [1.0, 0.0, -2.0],       # class c: below b in the last column only
                     [-1.0, 5.0, 0.0],       # class a again
                     [1.0, 0.0, 2.0]])
    pts, cells = weld_expectation(rows)
    want = np.array([[-1.0, 5.0, 0.0], [1.0, 0.0, -2.0], [1.0, -0.0, 2.0]])
    assert np.array_equal(pts, want) and np.array_equal(np.signbit(pts), np.signbit(want))
    assert cells.dtype == np.int64 and cells.tolist() == [[2, 0, 2], [1, 0, 2]]
    assert np.array_equal(pts[cells.reshape(-1)], rows)


@pytest.mark.parametrize('name', soups_ref.WELD)
def test_weld_rows_are_what_their_names_say(name):
    for T in soups_ref.WELD_COUNTS:
        rows = soups_ref.weld_rows(name, T)
        pts, cells = weld_expectation(rows)
        assert rows.shape == (3 * T, 3) and np.array_equal(pts[cells.reshape(-1)], rows)
    assert [3 * T for T in soups_ref.WELD_COUNTS] == [3, 255, 258, 513, 771]
    U = len(pts)                                                                # (of the 771 rows)
    if name == 'all_equal':
        assert U == 1
    if name == 'all_distinct':
        assert U == 771
    if name == 'z_neighbours':
        assert len(np.unique(rows[:, :2], axis=0)) == 1
        z = pts[:, 2]
        assert U == 31 and (np.diff(z) > 0).all()
        assert int((np.nextafter(z[:-1], np.inf) == z[1:]).sum()) == 26           # neighbours one ulp apart: five runs of them
        assert {-soups_ref.TINY, 0.0, soups_ref.TINY} <= set(z.tolist()) and np.signbit(rows[rows[:, 2] == 0, 2]).any()
        assert np.nextafter(soups_ref.MIN_NORMAL, 0) in z and soups_ref.MIN_NORMAL in z
    if name == 'mixed_signs':
        assert all((rows[:, k] < 0).any() and (rows[:, k] > 0).any() for k in range(3)) and U < 771
    if name == 'signed_zeros':
        # a class whose first member has -0.0 in one column and +0.0 in another, and classes whose members differ in the signs
        z = (pts == 0)
        sb = np.signbit(pts)
        assert ((z & sb).any(axis=1) & (z & ~sb).any(axis=1)).any()
        zero_rows = rows[(rows == 0).all(axis=1)]
        assert len({tuple(r) for r in np.signbit(zero_rows).tolist()}) == 8
    if name == 'extremes':
        for v in (soups_ref.TINY, -soups_ref.TINY, 1e308, -1e308, np.inf, -np.inf):
            assert all((rows[:, k] == v).any() for k in range(3))
