"""The cases of tests/test_large_batch_gpu.py (batch_size > 32: csrc/sdf_hip.hip generate_big / march_chunk) and what each of them
is there to reach, held on the CPU checker alone: the models whose cells are ambiguous have such cells, every chunk length of
generate_big is taken by some batch size, the chunk counts, the per-item triangle counts and the growth of the soup are what the
table says.  No GPU: this file is what tells the next person that the table needs new shapes when generate_big or march_chunk
change their chunk length or growth rule."""
import os

import numpy as np
import pytest

import fixtures
from conftest import GOLDEN
from sdf_amd import core

FIELD_CHUNK_MAX = 32            # csrc/sdf_hip.hip
SDF_BATCH_SIZE_MAX = 512        # csrc/sdf_internal.h


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


def chunk_plan(bs, item_triangles):
    """What csrc/sdf_hip.hip does with a work list whose items have `item_triangles` triangles at batch size bs > 32 -- MIRRORED from
    `generate_big` (the chunk length CH: as many (bs + 1)^3 float32 tiles as fit 256 MiB, between 1 and FIELD_CHUNK_MAX; the row
    slots per tile) and from `march_chunk` (the soup's capacity is set to max(2 * 72 * (total + n), 4 MiB) whenever a chunk of n
    triangles behind `total` kept ones needs more than it has, and what is there is copied).  Returns a dict of `ch`, `slots`,
    `chunks` and `copied`: the triangles copied at each reallocation.  If either function changes, change this with it and look
    at the shapes of CHUNKS again."""
    tile = (bs + 1) ** 3
    ch = max(1, min(FIELD_CHUNK_MAX, (256 << 20) // (tile * 4)))
    slots = (bs * bs + 255) & ~255
    cap = total = 0
    copied = []
    n_chunks = -(-len(item_triangles) // ch)
    for k in range(n_chunks):
        n = int(sum(item_triangles[k * ch:(k + 1) * ch]))
        if n == 0:
            continue
        if (total + n) * 72 > cap:
            cap = max(2 * 72 * (total + n), 4 << 20)
            copied.append(total)
        total += n
    return dict(ch=ch, slots=slots, chunks=n_chunks, copied=copied)


def test_every_chunk_length_of_generate_big_is_taken():
    """CH as a function of the batch size: 32 down to 1, changing at 160, 255 / 256, 322 and 406 as the table says; the sizes the
    suite ran before this file (33 .. 128) all take 31 or 32"""
    ch = {bs: chunk_plan(bs, [])['ch'] for bs in range(33, SDF_BATCH_SIZE_MAX + 1)}
    assert {ch[bs] for bs in (33, 40, 48, 64, 100, 128)} == {31, 32}
    assert (ch[159], ch[160]) == (16, 16) and (ch[254], ch[255], ch[256]) == (4, 4, 3) and (ch[321], ch[322]) == (2, 1)
    assert (ch[405], ch[406], ch[512]) == (1, 1, 1)
    assert [c['ch'] for c in CHUNKS] == [ch[c['bs']] for c in CHUNKS]
    assert {c['ch'] for c in CHUNKS} == {16, 4, 3, 2, 1}
    assert chunk_plan(512, [])['slots'] == 512 * 512          # no slack: every row slot of a tile is a row


def test_the_growth_rule_copies_only_a_soup_that_holds_triangles():
    assert chunk_plan(322, [10, 0, 0])['copied'] == [0]                        # the first allocation: nothing to copy
    assert chunk_plan(322, [30000, 0, 20000])['copied'] == [0]                 # 2 x 30000 triangles of room: the third item fits
    assert chunk_plan(322, [30000, 0, 40000])['copied'] == [0, 30000]
    assert chunk_plan(40, [30000, 0, 40000])['copied'] == [0]                  # one chunk


@pytest.mark.parametrize('case', CHUNKS, ids=['b%d-%s' % (c['bs'], 'x'.join(map(str, c['shape']))) for c in CHUNKS])
def test_section_2_cases_reach_what_the_table_says(case, ns, oracle_lib):
    f = fixtures.build('ex_example', ns)
    X, Y, Z = axes(case['shape'])
    bs = case['bs']
    for sparse in case['sparse']:
        o = oracle_lib.generate(f, X, Y, Z, bs, sparse)
        work = np.flatnonzero(o.kinds != 0)
        counts = [len(oracle_lib.generate(f, X, Y, Z, bs, sparse, batch_range=(int(b), int(b) + 1)).points) // 3 for b in work]
        assert sum(counts) == len(o.points) // 3 and [c > 0 for c in counts] == (o.kinds[work] == 2).tolist()
        plan = chunk_plan(bs, counts)
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
