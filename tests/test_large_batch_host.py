"""The cases of tests/test_large_batch_gpu.py (batch_size > 32: csrc/sdf_chunked.hip generate_big / march_chunk) and what each of
them is there to reach, held on the CPU checker alone: the models whose cells are ambiguous have such cells, every chunk length of
generate_big is taken by some batch size, the chunk counts, the per-item triangle counts and the growth of the soup are what the
table says.  The chunk length, the row slots and the growth rule are the library's own: csrc/sdf_chunk_plan.h, the host-only
arithmetic of sdf_chunked.hip, compiled here for the host -- and checked itself: a batch's box against NumPy slicing, the callback
path's plan, its `_skip` test against a restatement of the reference's.  No GPU: this file is what tells the next person that the
table needs new shapes when the chunk length or the growth rule change."""
import ctypes
import itertools
import os
import subprocess
import types

import numpy as np
import pytest

import fixtures
from conftest import GOLDEN, ROOT
from sdf_amd import core

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SRC = r'''
#include "sdf_chunk_plan.h"
extern "C" void consts(int *o) { o[0] = FIELD_CHUNK_MAX; o[1] = SDF_BATCH_SIZE_MAX; }
extern "C" void plan(int bs, int callback, int *o) { const ChunkPlan p = chunk_plan(bs, callback != 0); o[0] = p.ch; o[1] = p.slots; o[2] = (int)p.tile; }
extern "C" unsigned long long growth(unsigned long long cap, unsigned long long total, unsigned long long n) { return soup_growth(cap, total, n); }
extern "C" void box(int nx, int ny, int nz, int bs, int b, int *o) { const BatchBox x = batch_box(nx, ny, nz, bs, b); o[0] = x.ox; o[1] = x.oy; o[2] = x.oz; o[3] = x.lx; o[4] = x.ly; o[5] = x.lz; }
extern "C" void slice(long long n, long long i, long long k, int *o) { o[0] = shard_cut(n, i, k); o[1] = shard_cut(n, i + 1, k); }
extern "C" void skip_pts(const double *c, double *p) { skip_points(c[0], c[1], c[2], c[3], c[4], c[5], p); }
extern "C" int skip(const double *p, const double *v) { return skip_verdict(p, v); }
'''


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """csrc/sdf_chunk_plan.h built for the host: its constants, and its functions behind NumPy arguments"""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('chunk_plan')
    src, so = str(d / 'chunk_plan_host.hip'), str(d / 'libchunk_plan_host.so')
    open(src, 'w').write(SRC)
    subprocess.check_call([HIPCC, '--offload-host-only', '-O1', '-std=c++17', '-w', '-fPIC', '-shared', '-I', os.path.join(ROOT, 'sdf_amd', 'csrc'), '-o', so, src])
    L = ctypes.CDLL(so)
    vp, ll, ull, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int
    L.consts.argtypes = [vp]
    L.plan.argtypes = [i, i, vp]
    L.growth.argtypes = [ull, ull, ull]
    L.growth.restype = ull
    L.box.argtypes = [i, i, i, i, i, vp]
    L.slice.argtypes = [ll, ll, ll, vp]
    L.skip_pts.argtypes = [vp, vp]
    L.skip.argtypes = [vp, vp]

    def ints(n, fn, *args):
        o = np.zeros(n, np.int32)
        fn(*args, o.ctypes.data)
        return tuple(int(v) for v in o)

    def skip_points(x0, x1, y0, y1, z0, z1):
        c, p = np.array([x0, x1, y0, y1, z0, z1], np.float64), np.zeros((9, 3), np.float64)
        L.skip_pts(c.ctypes.data, p.ctypes.data)
        return p

    def skip_verdict(p, v):
        p, v = np.ascontiguousarray(p, np.float64), np.ascontiguousarray(v, np.float64)
        assert p.shape == (9, 3) and v.shape == (9,)
        return L.skip(p.ctypes.data, v.ctypes.data)

    def plan(bs, callback=False):
        ch, slots, tile = ints(3, L.plan, bs, int(callback))
        assert tile == (bs + 1) ** 3
        return ch, slots

    def chunk_plan(bs, item_triangles):
        """What csrc/sdf_chunked.hip does with a work list whose items have `item_triangles` triangles at batch size bs > 32: the
        tape path's plan, then per chunk with triangles the growth rule, both as compiled.  Returns a dict of `ch`, `slots`, `chunks`
        and `copied`: the triangles copied at each reallocation."""
        ch, slots = plan(bs)
        cap = total = 0
        copied = []
        n_chunks = -(-len(item_triangles) // ch)
        for k in range(n_chunks):
            n = int(sum(item_triangles[k * ch:(k + 1) * ch]))
            if n == 0:
                continue
            grown = L.growth(cap, total, n)
            if grown:
                cap = grown
                copied.append(total)
            total += n
        return dict(ch=ch, slots=slots, chunks=n_chunks, copied=copied)

    field_chunk_max, batch_size_max = ints(2, L.consts)
    return types.SimpleNamespace(FIELD_CHUNK_MAX=field_chunk_max, SDF_BATCH_SIZE_MAX=batch_size_max, plan=plan, chunk_plan=chunk_plan,
                                 box=lambda shape, bs, b: ints(6, L.box, *shape, bs, b), slice=lambda n, i, k: ints(2, L.slice, n, i, k),
                                 skip_points=skip_points, skip_verdict=skip_verdict)


def axis(n):
    return -0.9 + 1.8 * np.arange(n) / max(n - 1, 1)


def axes(shape):
    return tuple(axis(n) for n in shape)


# ---- section 1: model families through k_eval_tiles and the MC33 branch of k_field_* ----
# (model, samples, batch sizes, the checker's n_ambiguous > 0)
MODELS = (
    ('ex_knurling', 2 ** 19, (33, 50), True),
    ('ex_weave', 2 ** 19, (50,), True),
    ('ex_pawn', 2 ** 19, (50,), False),
    ('slots_plain_8_8_p8d8', 2 ** 18, (36,), True),
    ('slots_trig_8_8', 2 ** 18, (36,), True),
    ('slots_trig_2_4', 2 ** 18, (36,), True),
    ('grid_noise', 2 ** 17, (33, 48), True),
    ('image_blobs', 2 ** 15, (40,), False),
)
MODEL_CASES = [(name, samples, bs) for name, samples, sizes, _ in MODELS for bs in sizes]
AMBIGUOUS = {name for name, _, _, amb in MODELS if amb}


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), 'tools', name + '.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build_model(name, ns):
    if name == 'grid_noise':          # composed as in test_gpu.py::test_grid_leaf_on_device
        from sdf_amd import mesh
        X, Y, Z, A, bg, bb = _tool('make_golden_custom').grids()['noise']
        return mesh.grid_sdf((X, Y, Z), A, bg, bb).translate((0.05, -0.03, 0.02)) | ns['sphere'](0.2).translate((0, 0, 0.5))
    if name == 'image_blobs':         # as in test_gpu.py::test_image_leaf_on_device
        arr, kw = _tool('make_golden_texture').pictures()['blobs']
        return ns['image'](arr, **kw).extrude(0.4)
    return fixtures.build(name, ns)


_models = {}


def model_case(name, samples, ns, oracle):
    """(model, X, Y, Z, bounds) of a section 1 case: the axes of the checker's own bounds, built once"""
    if (name, samples) not in _models:
        f = build_model(name, ns)
        bounds = oracle.estimate_bounds(f)
        _models[name, samples] = (f,) + tuple(core.grid_axes(bounds, samples=samples)[:3]) + (bounds,)
    return _models[name, samples]


# ---- section 2: every chunk length, a full row-slot table, soup growth (ex_example) ----
# batch size, grid, sparse settings, chunk length, then what the checker must show: the least number of chunks, the triangles per
# work item, whether the soup is regrown while it holds triangles, the total, ambiguous cells
CHUNKS = (
    dict(bs=160, shape=(161, 161, 161), sparse=(True,), ch=16),
    dict(bs=255, shape=(600, 7, 6), sparse=(True, False), ch=4, ambiguous=True),
    dict(bs=256, shape=(600, 7, 6), sparse=(True, False), ch=3),
    dict(bs=300, shape=(700, 7, 6), sparse=(True,), ch=2),          # (not in the issue's table: the one chunk length it leaves out)
    dict(bs=322, shape=(660, 330, 7), sparse=(True,), ch=1, chunks=6, per_item=(353880, 0, 365160, 0, 0, 0), regrown=True),
    dict(bs=406, shape=(830, 20, 415), sparse=(True,), ch=1, chunks=6, per_item=(593424, 0, 610016, 0, 0, 0), regrown=True),
    dict(bs=512, shape=(1030, 4, 6), sparse=(True, False), ch=1, chunks=3),
    dict(bs=512, shape=(515, 515, 9), sparse=(True,), ch=1, triangles=873120),
)
CHUNK_CASES = [(c['bs'], c['shape'], sparse) for c in CHUNKS for sparse in c['sparse']]
CHUNK_IDS = ['b%d-%s-%s' % (bs, 'x'.join(map(str, shape)), 'sparse' if sparse else 'dense') for bs, shape, sparse in CHUNK_CASES]


def test_every_chunk_length_of_generate_big_is_taken(host):
    """CH as a function of the batch size: 32 down to 1, changing at 160, 255 / 256, 322 and 406 as the table says; the sizes the
    suite ran before this file (33 .. 128) all take 31 or 32"""
    assert (host.FIELD_CHUNK_MAX, host.SDF_BATCH_SIZE_MAX) == (32, 512)
    ch = {bs: host.chunk_plan(bs, [])['ch'] for bs in range(33, host.SDF_BATCH_SIZE_MAX + 1)}
    assert {ch[bs] for bs in (33, 40, 48, 64, 100, 128)} == {31, 32}
    assert (ch[159], ch[160]) == (16, 16) and (ch[254], ch[255], ch[256]) == (4, 4, 3) and (ch[321], ch[322]) == (2, 1)
    assert (ch[405], ch[406], ch[512]) == (1, 1, 1)
    assert [c['ch'] for c in CHUNKS] == [ch[c['bs']] for c in CHUNKS]
    assert {c['ch'] for c in CHUNKS} == {16, 4, 3, 2, 1}
    assert host.chunk_plan(512, [])['slots'] == 512 * 512          # no slack: every row slot of a tile is a row


def test_the_growth_rule_copies_only_a_soup_that_holds_triangles(host):
    assert host.chunk_plan(322, [10, 0, 0])['copied'] == [0]                        # the first allocation: nothing to copy
    assert host.chunk_plan(322, [30000, 0, 20000])['copied'] == [0]                 # 2 x 30000 triangles of room: the third item fits
    assert host.chunk_plan(322, [30000, 0, 40000])['copied'] == [0, 30000]
    assert host.chunk_plan(40, [30000, 0, 40000])['copied'] == [0]                  # one chunk


@pytest.mark.parametrize('case', CHUNKS, ids=['b%d-%s' % (c['bs'], 'x'.join(map(str, c['shape']))) for c in CHUNKS])
def test_section_2_cases_reach_what_the_table_says(case, ns, oracle_lib, host):
    f = fixtures.build('ex_example', ns)
    X, Y, Z = axes(case['shape'])
    bs = case['bs']
    for sparse in case['sparse']:
        o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
        work = np.flatnonzero(o.kinds != 0)
        counts = [len(oracle_lib.generate(f, X, Y, Z, bs, sparse, batch_range=(int(b), int(b) + 1)).points) // 3 for b in work]
        assert sum(counts) == len(o.points) // 3 and [c > 0 for c in counts] == (o.kinds[work] == 2).tolist()
        plan = host.chunk_plan(bs, counts)
        print(bs, case['shape'], sparse, plan, counts, o.n_ambiguous)
        assert plan['ch'] == case['ch'] and plan['chunks'] == -(-len(work) // case['ch'])
        if 'chunks' in case:
            assert plan['chunks'] == case['chunks'] >= 3
        if 'per_item' in case:
            assert tuple(counts) == case['per_item']
        if case.get('regrown'):
            assert plan['copied'] == [0, counts[0]] and counts[0] > 0           # the soup is regrown while it holds the first item
        if 'triangles' in case:
            assert len(o.points) // 3 == case['triangles']
        if case.get('ambiguous'):
            assert o.n_ambiguous > 0
    nb = [-(-n // bs) for n in case['shape']]
    if case['shape'] == (161, 161, 161):
        assert nb == [2, 2, 2] and o.kinds[0] == 2                               # one tile of 161^3 samples, slivers behind it
    if case['shape'] == (1030, 4, 6):
        assert case['shape'][0] - 2 * bs == 6                                     # the trailing batch: 6 samples
    if case['shape'] == (515, 515, 9):
        # the first tile has 512 x 512 rows of cells, one per row slot; 3-sample batches trail on two axes
        assert min(bs + 1, case['shape'][0]) - 1 == min(bs + 1, case['shape'][1]) - 1 == bs and plan['slots'] == bs * bs
        assert case['shape'][0] - bs == case['shape'][1] - bs == 3 and o.kinds[0] == 2


@pytest.mark.parametrize('name', [m[0] for m in MODELS])
def test_section_1_models_have_the_cells_they_are_there_for(name, ns, oracle_lib):
    """the MC33 branch of k_field_rows / k_field_emit is only exercised by a model with ambiguous cells"""
    _, samples, sizes, _ = [m for m in MODELS if m[0] == name][0]
    f, X, Y, Z, bounds = model_case(name, samples, ns, oracle_lib)
    for bs in sizes:
        o = oracle_lib.generate(f, X, Y, Z, bs, True)
        print(name, samples, bs, len(o.points) // 3, o.n_ambiguous, np.bincount(o.kinds, minlength=3))
        assert len(o.points) > 0 and (o.kinds == 2).sum() >= 1
        if name in AMBIGUOUS:
            assert o.n_ambiguous > 0


def test_the_many_shell_model_of_the_reader_tests(ns, oracle_lib):
    """sphere(0.055).repeat(0.17) & box(1.7) at 2^18 samples on [-1, 1]^3, batch size 40: 126232 triangles in many shells"""
    import components_ref
    f = ns['sphere'](0.055).repeat(0.17) & ns['box'](1.7)
    X, Y, Z, _ = core.grid_axes(((-1, -1, -1), (1, 1, 1)), samples=2 ** 18)
    o = oracle_lib.generate(f, X, Y, Z, 40, True)
    assert len(o.points) // 3 == 126232
    assert components_ref.components(*components_ref.weld(o.points.reshape(-1, 3, 3))).count > 100


# ---- csrc/sdf_chunk_plan.h itself ----
def test_batch_box_is_the_slicing_of_the_batch_loop(host):
    """every batch's box, in b = (ibx * nby + iby) * nbz + ibz order, is range(i * bs, min((i + 1) * bs + 1, n)) per axis: bs cells
    and the sample that closes the last of them, cut at the end of the axis"""
    from test_large_batch_gpu import edge_grids
    for bs, shape in [(33, s) for s in edge_grids(33)] + [(255, (600, 7, 6))]:
        nb = [-(-n // bs) for n in shape]
        b = 0
        for i in itertools.product(*map(range, nb)):
            want = [range(i[a] * bs, min((i[a] + 1) * bs + 1, shape[a])) for a in range(3)]
            assert [list(np.arange(shape[a])[i[a] * bs:(i[a] + 1) * bs + 1]) for a in range(3)] == [list(r) for r in want]
            assert host.box(shape, bs, b) == tuple(r.start for r in want) + tuple(len(r) for r in want), (bs, shape, b)
            b += 1
        assert b == nb[0] * nb[1] * nb[2]


def test_the_callback_path_has_the_same_chunks_and_pins_1024_slots(host):
    for bs in range(1, host.SDF_BATCH_SIZE_MAX + 1):
        ch, slots = host.plan(bs, callback=True)
        assert ch == host.plan(bs)[0] == max(1, min(host.FIELD_CHUNK_MAX, (64 << 20) // (bs + 1) ** 3))    # "<= 64 M points": the same rule
        assert slots == (1024 if bs <= 32 else (bs * bs + 255) & ~255)
        assert slots % 256 == 0 and slots >= bs * bs
        if bs > 32:
            assert slots == host.plan(bs)[1]


def test_a_shard_takes_its_slice_of_the_work_list(host):
    for n in (0, 1, 7, 40):
        for k in (1, 2, 3, 5):
            cuts = [host.slice(n, i, k) for i in range(k)]
            assert cuts == [(n * i // k, n * (i + 1) // k) for i in range(k)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))


def _ref_skip(P, V):
    """`_skip` of the reference (sdf/core.py:28-43) on the nine points P -- the centre, then the corners -- and the field's values V"""
    (x, y, z), (x0, y0, z0) = P[0], P[1]
    r = abs(V[0])
    d = np.linalg.norm(np.array((x - x0, y - y0, z - z0)))
    if r <= d:
        return False
    values = V[1:]
    same = np.all(values > 0) if values[0] > 0 else np.all(values < 0)
    return bool(same)


def test_skip_points_are_the_centre_and_the_product_of_the_ends(host):
    for box in ((0.0, 2.0, 0.0, 4.0, 0.0, 4.0), (-0.9, -0.3375, 0.1, 0.7, -1e-3, 3.25), (1.5, 1.5, -2.0, -2.0, 0.25, 0.5)):
        x0, x1, y0, y1, z0, z1 = box
        P = host.skip_points(*box)
        assert P[0].tolist() == [(x0 + x1) / 2, (y0 + y1) / 2, (z0 + z1) / 2]
        assert P[1:].tolist() == [list(c) for c in itertools.product((x0, x1), (y0, y1), (z0, z1))]


def test_skip_verdict_is_the_reference_skip(host):
    """the box (0, 2) x (0, 4) x (0, 4): its centre is exactly d = 3 from its corners"""
    P = host.skip_points(0.0, 2.0, 0.0, 4.0, 0.0, 4.0)
    assert np.linalg.norm(P[0] - P[1]) == 3.0
    nan = float('nan')

    def values(centre, corners, **at):
        v = np.full(9, float(corners))
        v[0] = centre
        for k, x in at.items():
            v[int(k[1:])] = x
        return v
    cases = [                                              # (values, skipped)
        (values(10.0, 10.0), True),                        # all positive and far
        (values(-10.0, -10.0), True),                      # all negative and far
        (values(10.0, 1.0, c6=-1.0), False),               # one corner of the other sign
        (values(-10.0, -1.0, c3=1.0), False),
        (values(10.0, 1.0, c1=-1.0), False),               # ... the FIRST corner, whose sign the others are held to
        (values(10.0, 1.0, c8=0.0), False),                # a corner exactly 0.0: neither > 0 nor < 0
        (values(-10.0, -1.0, c1=0.0), False),
        (values(10.0, 1.0, c1=0.0), False),
        (values(10.0, 1.0, c4=-0.0), False),
        (values(3.0, 1.0), False),                         # r == d: `r <= d`, not skipped
        (values(-3.0, -1.0), False),
        (values(np.nextafter(3.0, 4.0), 1.0), True),       # one ulp beyond
        (values(np.nextafter(3.0, 2.0), 1.0), False),
        (values(10.0, -1.0), True),                        # the centre's sign does not matter, its magnitude does
        (values(nan, 1.0), True),                          # a NaN centre: `r <= d` is False, so the corners decide
        (values(nan, 1.0, c5=-1.0), False),
        (values(10.0, 1.0, c2=nan), False),                # a NaN corner is on neither side
    ]
    for v, skipped in cases:
        assert _ref_skip(P, v) is skipped, v
        assert host.skip_verdict(P, v) == (0 if skipped else 255), v
    # a box whose d is not exact in float64: still the reference's verdict around it
    Q = host.skip_points(-0.9, -0.3375, 0.1, 0.7, -1e-3, 3.25)
    d = float(np.linalg.norm(Q[0] - Q[1]))
    for centre in (d * 0.999, d * 1.001, -d * 1.001, 5.0):
        v = values(centre, 2.0)
        assert host.skip_verdict(Q, v) == (0 if _ref_skip(Q, v) else 255), centre
