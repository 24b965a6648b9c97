"""The definition of the connected shells (tests/components_ref.py) on hand-made meshes, `resolve_keep`, and the ABI's new names:
what can be checked without a device."""
import importlib
import os
import re

import numpy as np
import pytest

import components_ref as ref
from sdf_amd import engine

shells = importlib.import_module('sdf_amd.shells')            # (the package's `shells` attribute is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def of(soup):
    pts, cells = ref.weld(soup)
    return pts, cells, ref.components(pts, cells)


def test_two_tetrahedra_are_two_shells():
    pts, cells, c = of(np.concatenate([ref.tetrahedron(), ref.tetrahedron(shift=(3.0, 0.0, 0.0))]))
    assert c.count == 2 and c.triangles.tolist() == [4, 4] and c.vertices.tolist() == [4, 4]
    assert c.triangle_shell.tolist() == [0] * 4 + [1] * 4
    assert c.vertex_shell.dtype == np.int32 and c.triangle_shell.dtype == np.int32
    assert c.triangles.dtype == np.int64 and c.vertices.dtype == np.int64 and c.bounds.dtype == np.float64


def test_two_tetrahedra_sharing_one_vertex_are_one_shell():
    pts, cells, c = of(np.concatenate([ref.tetrahedron(), ref.tetrahedron(shift=(1.0, 0.0, 0.0))]))
    assert len(pts) == 7 and c.count == 1 and c.triangles.tolist() == [8] and c.vertices.tolist() == [7]
    assert not c.vertex_shell.any() and not c.triangle_shell.any()


def test_a_collapsed_cell_joins_what_it_names():
    soup = ref.collapsed_bridge()
    pts, cells, c = of(soup)
    assert (cells[2, 0] == cells[2, 1]) and c.count == 1 and c.triangles.tolist() == [3] and c.vertices.tolist() == [6]
    pts, cells, c = of(soup[:2])
    assert c.count == 2


def test_a_hollow_cube_is_two_shells():
    pts, cells, c = of(np.concatenate([ref.cube(-1.0, 1.0), ref.cube(-0.5, 0.5, inward=True)]))
    assert c.count == 2 and c.triangles.tolist() == [12, 12] and c.vertices.tolist() == [8, 8]
    # the outer cube holds the lexicographically smallest vertex: shell 0
    assert np.array_equal(c.bounds[0], [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    assert np.array_equal(c.bounds[1], [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]])


def test_numbering_follows_the_smallest_vertex():
    """three tetrahedra given in the order x = 5, -5, 0: the shells are numbered by where they lie, not by where they stand"""
    soup = np.concatenate([ref.tetrahedron(shift=(x, 0.0, 0.0)) for x in (5.0, -5.0, 0.0)])
    pts, cells, c = of(soup)
    assert c.count == 3 and c.triangle_shell.tolist() == [2] * 4 + [0] * 4 + [1] * 4
    assert c.labels.tolist() == [0] * 4 + [4] * 4 + [8] * 4 and c.vertex_shell.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert np.array_equal(c.bounds[:, 0, 0], [-5.0, 0.0, 5.0]) and np.array_equal(c.bounds[:, 1, 0], [-4.0, 1.0, 6.0])


def test_counts_and_bounds():
    rng = np.random.RandomState(5)
    parts = [ref.tetrahedron(shift=rng.uniform(-50, 50, 3), scale=0.25) for _ in range(70)] + [ref.cube(100.0, 101.0)]
    soup = np.concatenate(parts)[rng.permutation(70 * 4 + 12)]
    pts, cells, c = of(soup)
    assert c.count == 71 and c.triangles.sum() == len(soup) and c.vertices.sum() == len(pts)
    assert sorted(c.triangles.tolist()) == [4] * 70 + [12] and c.triangles[-1] == 12
    for k in range(c.count):
        mine = soup[c.triangle_shell == k].reshape(-1, 3)
        assert np.array_equal(c.bounds[k, 0], mine.min(axis=0)) and np.array_equal(c.bounds[k, 1], mine.max(axis=0))
        assert c.vertices[k] == len(np.unique(mine, axis=0))
    # a zero reads +0.0
    pts, cells, c = of(np.array([[[-0.0, 0.0, -0.0], [-1.0, -0.0, -2.0], [-3.0, -4.0, -0.0]]]))
    assert not np.signbit(c.bounds[0, 1]).any() and np.array_equal(c.bounds[0, 1], [0.0, 0.0, 0.0])


def test_an_empty_mesh_has_no_shells():
    c = ref.components(np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    assert c.count == 0 and len(c.vertex_shell) == 0 and len(c.triangle_shell) == 0 and c.bounds.shape == (0, 2, 3)


def test_the_rounds_bound():
    assert [ref.rounds_bound(v) for v in (1, 2, 3, 4, 5, 65537)] == [3, 3, 4, 4, 5, 19]


def test_resolve_keep():
    t = np.array([3, 9, 9, 1, 9])
    assert shells.resolve_keep('largest', t).tolist() == [False, True, False, False, False]          # a tie: the lowest number
    assert shells.resolve_keep(2, t).tolist() == [False, True, True, False, False]
    assert shells.resolve_keep(4, t).tolist() == [True, True, True, False, True]
    assert shells.resolve_keep(0, t).tolist() == [False] * 5
    assert shells.resolve_keep(17, t).all()                                                              # n larger than K
    assert shells.resolve_keep(np.int64(1), t).tolist() == shells.resolve_keep('largest', t).tolist()
    mask = [True, False, False, True, False]
    got = shells.resolve_keep(mask, t)
    assert got.dtype == np.bool_ and got.tolist() == mask
    assert shells.resolve_keep(np.array(mask), t).tolist() == mask
    s = shells.Shells(count=5, triangles=t, vertices=t + 2, bounds=np.zeros((5, 2, 3)), vertex_shell=np.zeros(0, np.int32),
                      triangle_shell=np.zeros(0, np.int32), rounds=2)
    seen = []

    def small(sh):
        seen.append(sh)
        return sh.triangles < 5
    assert shells.resolve_keep(small, s).tolist() == [True, False, False, True, False] and seen == [s]
    assert shells.resolve_keep('largest', s).tolist() == [False, True, False, False, False]
    assert shells.resolve_keep('largest', np.zeros(0, np.int64)).tolist() == [] and shells.resolve_keep([], np.zeros(0, np.int64)).tolist() == []
    for bad in ('smallest', 1.5, None, [1, 0, 1, 0, 1], [True, False], np.ones(6, bool), True, -1, {'a': 1}, lambda sh: [True],
                lambda sh: 'all', [[True] * 5]):
        with pytest.raises(ValueError, match='keep'):
            shells.resolve_keep(bad, t)


def test_largest_first_orders_ties_by_number():
    assert shells.largest_first([3, 9, 9, 1, 9]).tolist() == [1, 2, 4, 0, 3]


def test_the_shells_tuple_is_immutable():
    s = shells.Shells(1, 2, 3, 4, 5, 6, 7)
    assert s._fields == ('count', 'triangles', 'vertices', 'bounds', 'vertex_shell', 'triangle_shell', 'rounds')
    with pytest.raises(AttributeError):
        s.count = 2


def test_the_abi_names_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION and version >= 16
    for name in ('sdf_mesh_components', 'sdf_mesh_components_fetch', 'sdf_mesh_select_shells', 'sdf_mesh_components_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    lib = engine.load_library()
    assert lib.sdf_abi_version() == version and all(hasattr(lib, n) for n in engine.ABI)
    assert [k for k, _ in engine.SdfComponents._fields_] == ['n_shells', 'n_vertices', 'n_triangles', 'rounds', 'ms_label', 'ms_number']
    m = re.search(r'typedef struct sdf_components \{(.*?)\} sdf_components;', hdr, re.S).group(1)
    assert re.findall(r'\b(n_shells|n_vertices|n_triangles|rounds|ms_label|ms_number)\b', m) == [k for k, _ in engine.SdfComponents._fields_]


def test_the_public_names():
    import sdf_amd
    assert sdf_amd.shells is shells.shells and sdf_amd.measure_shells is shells.measure_shells and sdf_amd.Shells is shells.Shells
    f = sdf_amd.sphere(1)
    assert callable(f.shells) and callable(f.measure_shells) and callable(sdf_amd.Mesh.shells)
    import inspect
    from sdf_amd import core
    measure = importlib.import_module('sdf_amd.measure')
    for fn in (core.save, core.generate_mesh, measure.measure):
        assert inspect.signature(fn).parameters['keep'].default is None, fn


def test_keep_is_refused_before_anything_is_meshed():
    """a keep that no mesh could satisfy raises ValueError before the engine is asked for: this passes without a device"""
    import sdf_amd
    f = sdf_amd.sphere(1)
    for bad in ('smallest', 2.5, -3):
        with pytest.raises(ValueError, match='keep'):
            f.generate_mesh(keep=bad, samples=2 ** 10, verbose=False)
        with pytest.raises(ValueError, match='keep'):
            f.measure(keep=bad, samples=2 ** 10, verbose=False)
