"""batch_size > 32 (csrc/sdf_chunked.hip generate_big / march_chunk: k_eval_tiles, k_field_rows / k_scan_rows / k_field_emit) and the
mesh readers behind it, against the CPU checker and the readers' host definitions: every model family and both tape families,
every chunk length, a tile whose rows fill every row slot, a soup regrown while it holds triangles, ragged and degenerate grids,
every reader on meshes of every producer, the public entry points, and the count of ambiguous cells on both paths.
tests/test_large_batch_host.py holds the tables and checks on the checker alone that each case reaches what it is there for.
No test repeats a device call that failed."""
import importlib
import os

import numpy as np
import pytest

import components_ref
import fixtures
import measure_ref
import normals_ref
from conftest import GOLDEN
from sdf_amd import core, stl, tape
from test_components_gpu import as_fields, bits, same_components
from test_gpu import TRIG
from test_large_batch_host import AMBIGUOUS, CHUNK_CASES, CHUNK_IDS, MODEL_CASES, axes, model_case
from test_measure_gpu import same_measurement, same_moments
from test_register_slots import is_trig

shells = importlib.import_module('sdf_amd.shells')
pytestmark = pytest.mark.gpu

BOX = ((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85))
_oracle = {}


def checker(oracle_lib, key, f, X, Y, Z, bs, sparse):
    """the checker's generate, computed once per case and left unchanged"""
    k = (key, bs, sparse)
    if k not in _oracle:
        o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
        o.points.setflags(write=False); o.kinds.setflags(write=False)
        _oracle[k] = o
    return _oracle[k]


def same_as_checker(mesh, o, trig=False, extent=None, ambiguous=True):
    """the assertions of test_gpu.py::test_generate_matches_oracle_and_reference and of test_batch_size_above_32_...: classification,
    counts, soup (bit for bit and in order; the libm models to that test's bound), batch offsets; and the ambiguous cells"""
    pts, kinds, st, offs = mesh.points(), mesh.kinds(), mesh.stats(), mesh.batch_offsets()
    assert np.array_equal(kinds, o.kinds)
    assert (st['skipped'], st['empty'], st['nonempty']) == tuple(int((o.kinds == k).sum()) for k in (0, 1, 2))
    assert st['n_eval_voxels'] == o.n_eval and st['triangles'] == len(o.points) // 3 == mesh.n_triangles
    assert pts.shape == o.points.shape
    if trig:
        assert np.abs(pts - o.points).max() <= 1e-5 * extent
        assert (pts == o.points).mean() > 0.999
    else:
        assert np.array_equal(bits(pts), bits(o.points))
    assert offs[0] == 0 and offs[-1] == len(o.points) // 3 and np.array_equal(np.diff(offs) > 0, o.kinds == 2)
    print('triangles %d, ambiguous cells %d (checker %d)' % (st['triangles'], st['n_ambiguous_cells'], o.n_ambiguous))
    if ambiguous:
        assert st['n_ambiguous_cells'] == o.n_ambiguous
    return pts


# ---- 1. model families through k_eval_tiles and the MC33 branch of k_field_* ----
@pytest.mark.parametrize('name,samples,bs', MODEL_CASES, ids=['%s-b%d' % (n, b) for n, s, b in MODEL_CASES])
def test_model_families_match_the_checker(name, samples, bs, ns, oracle_lib, eng):
    f, X, Y, Z, bounds = model_case(name, samples, ns, oracle_lib)
    o = checker(oracle_lib, (name, samples), f, X, Y, Z, bs, True)
    if name in AMBIGUOUS:
        assert o.n_ambiguous > 0
    trig = name in TRIG or is_trig(tape.lower(f))
    m = eng.generate(f, X, Y, Z, bs, True)
    try:
        same_as_checker(m, o, trig, np.ptp(np.array(bounds), axis=0).max())
    finally:
        m.close()


# ---- 6. sdf_stats::n_ambiguous_cells on the fused path: k_mesh counts what the checker counts ----
@pytest.mark.parametrize('name,samples', sorted({(n, s) for n, s, b in MODEL_CASES}))
def test_the_fused_path_counts_the_ambiguous_cells_of_the_checker(name, samples, ns, oracle_lib, eng):
    f, X, Y, Z, bounds = model_case(name, samples, ns, oracle_lib)
    o = checker(oracle_lib, (name, samples), f, X, Y, Z, 32, True)
    m = eng.generate(f, X, Y, Z, 32, True)
    try:
        st = m.stats()
    finally:
        m.close()
    print(name, st['n_ambiguous_cells'], o.n_ambiguous)
    assert st['triangles'] == len(o.points) // 3 and st['n_ambiguous_cells'] == o.n_ambiguous
    if name in AMBIGUOUS:
        assert o.n_ambiguous > 0


@pytest.mark.parametrize('bs', (32, 255))
def test_the_callback_path_counts_them_too(bs, ns, oracle_lib, eng):
    """sdf_generate_field shares march_chunk: the README's sphere as a user closure in the example, whose values are the library
    sphere's, on the coarse grid of section 2 whose cells are ambiguous"""
    f, g = fixtures.build('custom_leaf_in_example', ns), fixtures.build('ex_example', ns)
    X, Y, Z = axes((600, 7, 6))
    o = checker(oracle_lib, ('ex_example', (600, 7, 6)), g, X, Y, Z, bs, True)
    assert o.n_ambiguous > 0
    m = eng.generate(f, X, Y, Z, bs, True)
    try:
        st = m.stats()
        assert np.array_equal(bits(m.points()), bits(o.points)) and np.array_equal(m.kinds(), o.kinds)
        assert st['n_ambiguous_cells'] == o.n_ambiguous
    finally:
        m.close()


# ---- 2. every chunk length, a full row-slot table, soup growth ----
def example_golden(ns, eng):
    d = np.load(os.path.join(GOLDEN, 'gen_example_s17.npz'))
    X, Y, Z, _ = core.grid_axes(tuple(map(tuple, d['bounds'])), d['step'].tolist())
    m = eng.generate(fixtures.build('ex_example', ns), X, Y, Z, 32, True)
    try:
        return np.array_equal(bits(m.points()), bits(d['points']))
    finally:
        m.close()


@pytest.mark.parametrize('bs,shape,sparse', CHUNK_CASES, ids=CHUNK_IDS)
def test_every_chunk_length_matches_the_checker(bs, shape, sparse, ns, oracle_lib, eng):
    f = fixtures.build('ex_example', ns)
    X, Y, Z = axes(shape)
    o = checker(oracle_lib, ('ex_example', shape), f, X, Y, Z, bs, sparse)
    m = eng.generate(f, X, Y, Z, bs, sparse)
    try:
        same_as_checker(m, o)
    finally:
        m.close()
    if bs >= 255:
        eng.trim()                                              # the chunk's buffers go back; the fused path allocates its own again
        assert example_golden(ns, eng)


# ---- 3. ragged and degenerate grids above 32 ----
def edge_grids(bs):
    return [(bs + 1, bs + 1, bs + 1), (bs + 2, bs + 1, 2 * bs + 1), (2, 2, 2), (1, 40, 40), (64, 1, 3), (3, 3, 4 * bs + 2)]


@pytest.mark.parametrize('sparse', [True, False], ids=['sparse', 'dense'])
@pytest.mark.parametrize('bs,shape', [(bs, s) for bs in (33, 64) for s in edge_grids(bs)],
                         ids=['b%d-%s' % (bs, 'x'.join(map(str, s))) for bs in (33, 64) for s in edge_grids(bs)])
def test_ragged_and_degenerate_grids_above_32(bs, shape, sparse, ns, oracle_lib, eng):
    f = fixtures.build('ex_example', ns)
    X, Y, Z = axes(shape)
    o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
    if shape == (bs + 1, bs + 1, bs + 1):
        assert len(o.kinds) == 8 and (o.kinds[1:] != 2).all()    # the one-sample batches behind the tile have no cells
    m = eng.generate(f, X, Y, Z, bs, sparse)
    try:
        same_as_checker(m, o)
    finally:
        m.close()


# ---- 4. every reader on meshes that no reader test has seen ----
def multi_shell(ns):
    return ns['sphere'](0.055).repeat(0.17) & ns['box'](1.7)


class Produced:
    """a mesh of one of the producers and what keeps it alive; `with` closes it and restores what the producer changed"""

    def __init__(self, which, ns, oracle_lib, eng):
        import torch
        self.eng, self.buf, self.twopass = eng, None, False
        f = self.f = multi_shell(ns) if which == 'i' else fixtures.build('ex_example', ns)
        if which == 'c':
            X, Y, Z = axes((660, 330, 7))
        elif which == 'i':
            X, Y, Z, _ = core.grid_axes(((-1, -1, -1), (1, 1, 1)), samples=2 ** 18)
        else:
            X, Y, Z, _ = core.grid_axes(BOX, samples=2 ** 20 if which == 'b' else 2 ** 18)
        self.eps = 1e-4 * float(np.sqrt((X[-1] - X[0]) ** 2 + (Y[-1] - Y[0]) ** 2 + (Z[-1] - Z[0]) ** 2) / 2)
        if which in 'fg':
            n = len(checker(oracle_lib, ('ex_example', 'box18'), f, X, Y, Z, 32, True).points) // 3
            self.buf = torch.full((9 * n + 9,), -7.0, dtype=torch.float64, device='cuda:0')
            torch.cuda.synchronize()
        if which == 'a':
            self.mesh = eng.generate(f, X, Y, Z, 40, True)
        elif which == 'b':
            self.mesh = eng.generate(f, X, Y, Z, 33, False)
        elif which == 'c':
            self.mesh = eng.generate(f, X, Y, Z, 322, True)
        elif which == 'd':
            eng.set_twopass(1)
            self.twopass = True
            self.mesh = eng.generate(f, X, Y, Z, 32, True)
        elif which == 'e':
            self.mesh = eng.generate(f, X, Y, Z, 32, True, shard=(1, 3))
        elif which == 'f':
            self.mesh = eng.generate(f, X, Y, Z, 32, True, out_ptr=self.buf.data_ptr(), out_cap=n)
            assert self.mesh.emitted
        elif which == 'g':
            self.mesh = eng.generate(f, X, Y, Z, 32, True, out_ptr=self.buf.data_ptr(), out_cap=n, wait=False)
        elif which == 'h':
            self.mesh = eng.generate(f, X, Y, Z, 40, True, records=True)
        elif which == 'i':
            self.mesh = eng.generate(f, X, Y, Z, 40, True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            if getattr(self, 'mesh', None) is not None:
                self.mesh.close()
        finally:
            if self.twopass:
                self.eng.set_twopass(-1)


def hold_every_reader(mesh, f, eps, eng):
    """every reader of `mesh` against its host definition on P = mesh.points(), taken once"""
    import torch
    P = mesh.points().copy()
    P.setflags(write=False)
    T = len(P) // 3
    assert T == mesh.n_triangles and T > 1000
    soup = P.reshape(-1, 3, 3)
    kinds, offs = mesh.kinds(), mesh.batch_offsets()
    assert offs[0] == 0 and offs[-1] == T and np.array_equal(np.diff(offs) > 0, kinds == 2)
    # weld, STL and PLY records, normals
    wp, inv = np.unique(P, axis=0, return_inverse=True)
    wc = np.asarray(inv, dtype=np.int64).reshape(-1, 3)
    pts, cells = mesh.weld()
    assert pts.dtype == np.float64 and cells.dtype == np.int64
    assert np.array_equal(bits(pts), bits(wp)) and np.array_equal(cells, wc)
    assert np.array_equal(mesh.stl_records(), stl.stl_records(P).view(np.uint8).reshape(-1))
    vb, fb = mesh.ply_records(normals=False)
    wv, wf = normals_ref.ply_records(wp, wc)
    assert np.array_equal(vb, wv) and np.array_equal(fb, wf)
    n, n_flat = mesh.vertex_normals(f, eps)
    wn, wflat = normals_ref.vertex_normals(lambda Q: eng.eval_points(f, Q), wp, eps)
    assert np.array_equal(bits(n), bits(wn)) and n_flat == wflat
    vb, fb = mesh.ply_records(normals=True)
    wv = normals_ref.ply_records(wp, wc[:0], wn)[0]
    assert np.array_equal(vb, wv) and np.array_equal(fb, wf)
    # moments, census, shells
    same_moments(mesh.moments(), measure_ref.moments(soup))
    assert mesh.edge_census() == measure_ref.edge_census(wc, len(wp))
    want = components_ref.components(wp, wc)
    got = mesh.components()
    same_components(got, want, len(wp))
    summary = mesh.shell_summary()
    assert summary['count'] == want.count and np.array_equal(summary['triangles'], want.triangles)
    assert np.array_equal(summary['vertices'], want.vertices) and np.array_equal(bits(summary['bounds']), bits(want.bounds))
    # selections: the largest shell, all of them, none
    k = want.count
    for mask in (np.arange(k) == np.argmax(want.triangles), np.ones(k, bool), np.zeros(k, bool)):
        sub = soup[mask[want.triangle_shell]]
        sel = mesh.select(mask)
        try:
            assert sel.n_triangles == len(sub)
            assert np.array_equal(bits(sel.points()), bits(sub.reshape(-1, 3)))
            same_moments(sel.moments(), measure_ref.moments(sub))
        finally:
            sel.close()
    # ranges: the first triangle, across the boundary of the first two non-empty work items, the last triangle
    ranges = [(0, 1), (T - 1, 1), (T // 2, 257)]
    starts = offs[:-1][kinds == 2]
    if len(starts) >= 2:
        ranges.append((int(starts[1]) - 2, 5))
    for first, count in ranges:
        assert np.array_equal(bits(mesh.points_range(first, count)), bits(P[3 * first:3 * (first + count)])), (first, count)
    out = torch.full((9 * T + 9,), -7.0, dtype=torch.float64, device='cuda:0')
    mesh.emit_device(out.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(bits(host[:-9]), bits(P.reshape(-1))) and (host[-9:] == -7.0).all()
    assert np.array_equal(bits(mesh.points()), bits(P))           # the source is what it was
    return P


PRODUCERS = {'a': 'b40', 'b': 'b33_dense_two_chunks', 'c': 'b322_regrown_soup', 'd': 'b32_two_pass', 'e': 'b32_shard_1_of_3',
             'f': 'b32_caller_buffer', 'g': 'b32_caller_buffer_not_waited_for', 'h': 'b40_records', 'i': 'b40_many_shells'}


@pytest.mark.parametrize('which', sorted(PRODUCERS), ids=[PRODUCERS[k] for k in sorted(PRODUCERS)])
def test_every_reader_on_every_producer(which, ns, oracle_lib, eng):
    with Produced(which, ns, oracle_lib, eng) as p:
        P = hold_every_reader(p.mesh, p.f, p.eps, eng)
        if which in 'fg':
            assert p.mesh.emitted if which == 'f' else p.mesh.wait()
            host = p.buf.cpu().numpy()                          # the soup that was read IS the caller's buffer
            assert np.array_equal(bits(host[:-9]), bits(P.reshape(-1))) and (host[-9:] == -7.0).all()
        if which == 'i':
            assert len(P) // 3 == 126232 and p.mesh.shell_summary()['count'] > 100


# ---- 5. the public entry points with batch_size > 32 ----
def test_generate_at_batch_size_64_is_the_reference_soup(ns, eng):
    d = np.load(os.path.join(GOLDEN, 'gen_example_s17_b64.npz'))
    f = fixtures.build('ex_example', ns)
    assert eval(str(d['kwargs'])) == {'samples': 2 ** 17, 'batch_size': 64}
    assert np.array_equal(np.array(core._estimate_bounds(f)), d['bounds'])      # the default bounds
    pts = f.generate(samples=2 ** 17, batch_size=64, verbose=False)
    assert np.array_equal(bits(pts), bits(d['points']))


def test_save_measure_and_shells_at_batch_sizes_above_32(tmp_path, ns, eng):
    f = fixtures.build('ex_example', ns)
    S = 2 ** 17
    soup = f.generate(samples=S, batch_size=48, verbose=False)
    assert len(soup) > 3000
    f.save(tmp_path / 'a.stl', samples=S, batch_size=48, verbose=False)
    stl.write_stl_records(str(tmp_path / 'want.stl'), stl.stl_records(soup).view(np.uint8).reshape(-1))
    assert open(tmp_path / 'a.stl', 'rb').read() == open(tmp_path / 'want.stl', 'rb').read()
    wp, wc = components_ref.weld(soup)
    bounds = core._estimate_bounds(f)
    lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
    eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
    wn = normals_ref.vertex_normals(lambda P: eng.eval_points(f, P), wp, eps)[0]
    f.save(str(tmp_path / 'a.ply'), writer='native', normals=True, samples=S, batch_size=48, verbose=False)
    p, nn, c, head = normals_ref.parse_ply(str(tmp_path / 'a.ply'))
    assert head == normals_ref.ply_header(len(wp), len(wc), True)
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32)) and np.array_equal(c, wc)
    assert np.array_equal(nn.view(np.int32), wn.astype(np.float32).view(np.int32))
    f.save(str(tmp_path / 'a.obj'), writer='native', normals=True, samples=S, batch_size=48, verbose=False)
    p, nn, c = normals_ref.parse_obj(str(tmp_path / 'a.obj'))
    assert np.array_equal(p.view(np.int32), wp.astype(np.float32).view(np.int32)) and np.array_equal(c, wc)
    assert np.array_equal(nn.view(np.int32), wn.astype(np.float32).view(np.int32))
    same_measurement(f.measure(samples=S, batch_size=48, verbose=False), measure_ref.measure(wp, wc))


@pytest.mark.parametrize('name', ('ex_example', 'many_shells'))
def test_shells_and_keep_at_batch_size_40(name, ns, eng):
    f = multi_shell(ns) if name == 'many_shells' else fixtures.build('ex_example', ns)
    kw = dict(bounds=((-1, -1, -1), (1, 1, 1)), samples=2 ** 18) if name == 'many_shells' else dict(samples=2 ** 17)
    soup = f.generate(batch_size=40, verbose=False, **kw).reshape(-1, 3, 3)
    wp, wc = components_ref.weld(soup)
    want = components_ref.components(wp, wc)
    sh = f.shells(batch_size=40, **kw)
    assert sh.count == want.count and np.array_equal(sh.triangle_shell, want.triangle_shell) and np.array_equal(sh.vertex_shell, want.vertex_shell)
    assert np.array_equal(sh.triangles, want.triangles) and np.array_equal(sh.vertices, want.vertices)
    assert np.array_equal(bits(sh.bounds), bits(want.bounds))
    order = shells.largest_first(want.triangles)
    largest = soup[want.triangle_shell == order[0]]
    pts, cells, n = f.generate_mesh(keep='largest', batch_size=40, verbose=False, **kw)
    lp, lc = components_ref.weld(largest)
    assert n is None and np.array_equal(bits(pts), bits(lp)) and np.array_equal(cells, lc)
    got = f.measure_shells(limit=3, batch_size=40, **kw)
    assert len(got) == min(3, want.count)
    for g, k in zip(got, order):
        same_measurement(g, measure_ref.measure(*components_ref.weld(soup[want.triangle_shell == k])))
    assert as_fields(f.measure(keep='largest', batch_size=40, verbose=False, **kw)) == as_fields(got[0])
    if name == 'many_shells':
        assert len(soup) == 126232 and want.count > 100
