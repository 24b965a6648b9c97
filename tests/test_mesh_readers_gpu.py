"""The three oldest readers of a finished mesh on constructed soups (tests/soups_ref.py), bit for bit: k_stl against the bytes the
unmodified reference wrote (tests/golden/stl_soups.npz) and against `stl.stl_records` -- degenerate triangles whose normal is 0/0,
denormal cross products, exponents from 2^-60 to 2^59, signed zeros, at 1 / 255 / 256 / 257 / 513 triangles; two lattice models a
fifth and two thirds of whose triangles are degenerate, through every kind of producer and through `save`; k_ply_faces and
k_ply_vertices at every length of the file's tail, alone and behind full workgroups, and at the edges of the float64 -> float32 cast;
the weld (csrc/sdf_weld.hip) against np.unique on ties, neighbours one ulp apart, both zeros and the ends of the float64 range, with
the documented representative of a class of +-0.  tests/test_mesh_readers_host.py holds the helpers and checks on the host that each
soup reaches what it is there for.  Soups go in through `Engine.adopt_soup` on a torch tensor.  No test repeats a device call that
failed."""
import numpy as np
import pytest

import normals_ref
import soups_ref
from sdf_amd import core, stl
from test_export_gpu import Soup, bits, same_normals
from test_mesh_readers_host import (LATTICE, LATTICE_MODELS, RECORDED_COUNTS, STL_CASES, golden, is_nan_word, lattice_file, nan_normals,
                                    record_words, same_records, stl_soup, weld_expectation)

pytestmark = pytest.mark.gpu


def adopted(eng, rows, read):
    """read(mesh) of the (3T, 3) rows adopted as a soup on the device; arrays are copied out of the mesh's pinned blocks"""
    s = Soup(eng, np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 9))
    try:
        got = read(s.mesh)
        return tuple(np.array(a) for a in got) if isinstance(got, tuple) else np.array(got)
    finally:
        s.close()


# ---- STL ----
@pytest.mark.parametrize('key,cls', STL_CASES, ids=[k for k, c in STL_CASES])
def test_device_stl_records_are_the_reference_bytes(key, cls, eng):
    soup = stl_soup(key)
    got = adopted(eng, soup, lambda m: m.stl_records())
    w = record_words(got)[0]
    print('%s: NaN words the device wrote: %s' % (key, sorted('%08x' % x for x in set(w[is_nan_word(w)].tolist()))))
    same_records(got, golden()['rec_' + key], cls)
    with np.errstate(all='ignore'):
        same_records(got, stl.stl_records(soup).view(np.uint8).reshape(-1), cls)


def lattice_axes():
    return core.grid_axes(LATTICE['bounds'], LATTICE['step'])[:3]


def produce(how, f, eng, T):
    """the STL records of the lattice model's mesh from one kind of producer (test_large_batch_gpu.PRODUCERS, on a grid of 16^3)"""
    import torch
    X, Y, Z = lattice_axes()
    buf = None
    if how in ('caller_buffer', 'caller_buffer_not_waited_for'):
        buf = torch.full((9 * T + 9,), -7.0, dtype=torch.float64, device='cuda:0')
        torch.cuda.synchronize()
    if how == 'b8_three_shards':                                # every rank's part of the work list, in order
        out = []
        for r in range(3):
            m = eng.generate(f, X, Y, Z, 8, False, shard=(r, 3))
            try:
                out.append(np.array(m.stl_records()))
            finally:
                m.close()
        return np.concatenate(out)
    if how == 'b32_two_pass':
        eng.set_twopass(1)
    try:
        if how == 'caller_buffer':
            m = eng.generate(f, X, Y, Z, 32, False, out_ptr=buf.data_ptr(), out_cap=T)
            assert m.emitted
        elif how == 'caller_buffer_not_waited_for':
            m = eng.generate(f, X, Y, Z, 32, False, out_ptr=buf.data_ptr(), out_cap=T, wait=False)
        else:
            bs, records = {'b32': (32, False), 'b8': (8, False), 'b32_two_pass': (32, False), 'b32_records': (32, True),
                           'b40': (40, False), 'b33': (33, False), 'b40_records': (40, True)}[how]
            m = eng.generate(f, X, Y, Z, bs, False, records=records)
        try:
            return np.array(m.stl_records())
        finally:
            m.close()
    finally:
        if how == 'b32_two_pass':
            eng.set_twopass(-1)


LATTICE_PRODUCERS = ('b32', 'b8', 'b32_two_pass', 'b8_three_shards', 'caller_buffer', 'caller_buffer_not_waited_for', 'b32_records',
                     'b40', 'b33', 'b40_records')


@pytest.mark.parametrize('how', LATTICE_PRODUCERS)
@pytest.mark.parametrize('name', LATTICE_MODELS)
def test_lattice_models_give_the_reference_records_from_every_producer(name, how, ns, oracle_lib, eng):
    """the grid has 16 samples an axis: one batch at batch_size 32 and above, whose soup is the recorded file's; 2 x 2 x 2 batches at 8,
    whose soup (another order, and other triangles along the seams) is the checker's"""
    f = ns[name](1)
    rec, T = lattice_file(name)
    n_nan = RECORDED_COUNTS[name][1]
    if how.startswith('b8'):
        soup = oracle_lib.generate(f, *lattice_axes(), 8, False).points
        with np.errstate(all='ignore'):
            rec = stl.stl_records(soup).view(np.uint8).reshape(-1)
        T, n_nan = len(soup) // 3, nan_normals(rec)[0]
        assert n_nan > T // 6 and nan_normals(rec)[1] == {0xffc00000}
    got = produce(how, f, eng, T)
    assert len(got) == 50 * T and nan_normals(got)[0] == n_nan
    same_records(got, rec, 'A')


@pytest.mark.parametrize('kw', ({}, {'batch_size': 40}, {'batch_size': 16}), ids=('b32', 'b40', 'b16'))
@pytest.mark.parametrize('name', LATTICE_MODELS)
def test_save_writes_the_reference_file_of_a_lattice_model(name, kw, tmp_path, ns, eng):
    path = str(tmp_path / 'a.stl')
    ns[name](1).save(path, verbose=False, **dict(LATTICE, **kw))
    with open(path, 'rb') as fp:
        raw = fp.read()
    want = golden()['stl_' + name].tobytes()
    assert raw[:84] == want[:84]
    same_records(np.frombuffer(raw[84:], np.uint8), np.frombuffer(want[84:], np.uint8), 'A')
    assert raw == want


# ---- PLY ----
@pytest.mark.parametrize('T', soups_ref.PLY_COUNTS)
def test_ply_records_at_every_tail_length(T, ns, eng):
    """13 T mod 4 = 1, 2, 3, 0 in one workgroup (T = 1 .. 4); 3, 0, 1, 3 in the second (255 .. 259: 255 ends one byte short of the
    first workgroup's 3328) and 3 in the third (515)"""
    f = ns['sphere'](1)
    rows = soups_ref.class_a('ordinary', T)
    pts, cells = weld_expectation(rows)
    assert len(pts) == 3 * T

    def read(m):
        plain = tuple(np.array(a) for a in m.ply_records())
        n, n_flat = m.vertex_normals(f, 1e-3)
        return plain + (np.array(n), np.array(n_flat)) + tuple(np.array(a) for a in m.ply_records(normals=True))

    vb, fb, n, n_flat, vbn, fbn = adopted(eng, rows, read)
    wv, wf = normals_ref.ply_records(pts, cells)
    assert vb.dtype == np.uint8 and fb.dtype == np.uint8 and len(fb) == 13 * T
    assert np.array_equal(fb, wf), 'faces: first differing byte %d of %d' % (np.flatnonzero(fb != wf)[0], len(wf))
    assert np.array_equal(vb, wv)
    same_normals((n, int(n_flat)), normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), pts, 1e-3))
    wvn = normals_ref.ply_records(pts, cells[:0], n)[0]
    assert np.array_equal(vbn, wvn) and np.array_equal(fbn, wf)


PLY_VERTEX_SOUPS = {
    'wide_exponent': lambda: soups_ref.class_a('wide_exponent', 257),
    'signed_zero': lambda: soups_ref.class_a('signed_zero', 257),
    'cast_edges': lambda: soups_ref.cast_edges(86),
    'extremes': lambda: soups_ref.weld_rows('extremes', 86),
}


@pytest.mark.parametrize('name', sorted(PLY_VERTEX_SOUPS))
def test_ply_vertex_records_at_the_edges_of_the_float32_cast(name, eng):
    rows = PLY_VERTEX_SOUPS[name]()
    pts, cells = weld_expectation(rows)                         # (the signs of zero are the first soup row's: the weld's rule)
    with np.errstate(all='ignore'):
        wv, wf = normals_ref.ply_records(pts, cells)
    w = wv.view('<u4')
    if name == 'signed_zero':
        assert (w == 0x80000000).any() and (w == 0).any()
    if name in ('cast_edges', 'extremes'):
        assert (w == 0x80000000).any() and (w == 0x7f800000).any() and (w == 0xff800000).any()
    if name == 'cast_edges':
        assert (((w & 0x7f800000) == 0) & ((w & 0x007fffff) != 0)).any()                    # float32 denormals
    vb, fb = adopted(eng, rows, lambda m: tuple(np.array(a) for a in m.ply_records()))
    assert np.array_equal(vb, wv), 'vertices: first differing word %d' % (np.flatnonzero(vb.view('<u4') != w)[0],)
    assert np.array_equal(fb, wf)


# ---- weld ----
def same_weld(eng, rows):
    pts, cells = adopted(eng, rows, lambda m: m.weld())
    want_pts, want_inv = np.unique(rows, axis=0, return_inverse=True)
    assert pts.dtype == np.float64 and cells.dtype == np.int64
    assert pts.shape == want_pts.shape and (pts == want_pts).all()
    assert np.array_equal(cells, np.asarray(want_inv, dtype=np.int64).reshape(-1, 3))
    assert (pts[cells.reshape(-1)] == rows).all()
    # the signs of zero of a unique row are those of the first soup row of its class (header of csrc/sdf_weld.hip)
    rep = weld_expectation(rows)[0]
    bad = np.flatnonzero((bits(pts) != bits(rep)).any(axis=1))
    assert len(bad) == 0, '%d unique rows carry another sign of zero, first %d: %r, the first soup row of its class is %r' % (
        len(bad), bad[0], pts[bad[0]], rep[bad[0]])
    return pts


@pytest.mark.parametrize('T', soups_ref.WELD_COUNTS)
@pytest.mark.parametrize('name', soups_ref.WELD)
def test_weld_of_constructed_rows_is_numpy_unique(name, T, eng):
    pts = same_weld(eng, soups_ref.weld_rows(name, T))
    if name == 'all_equal':
        assert len(pts) == 1
    if name == 'all_distinct':
        assert len(pts) == 3 * T


@pytest.mark.parametrize('key', [k for k, c in STL_CASES if c == 'A'])
def test_weld_of_the_class_a_soups_is_numpy_unique(key, eng):
    same_weld(eng, stl_soup(key))
