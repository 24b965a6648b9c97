"""The device mesh-to-level-set voxelizer (csrc/sdf_level_set.hip, `Mesh.sdf(..., voxelizer='device')`): bit-exact
against the NumPy restatement (tests/level_set_ref.py), end to end through the fused meshing path, geometrically sane,
robust, and on a large mesh."""
import ctypes

import numpy as np
import pytest

import level_set_ref as ref
from sdf_amd import core, mesh
from test_level_set_host import box_mesh

pytestmark = pytest.mark.gpu


def icosphere(level=3, radius=1.0):
    t = (1 + 5 ** 0.5) / 2
    P = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    P = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in P]
    T = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = P[a] + P[b]
                P.append(q / np.linalg.norm(q))
                mid[k] = len(P) - 1
            return mid[k]
        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        T = nt
    return np.array(P) * radius, np.array(T)


def meshes(ns):
    P, T = box_mesh((-0.43, -0.31, -0.27), (0.52, 0.36, 0.33))
    Pt, Tt = box_mesh((-0.25, -0.375, -0.25), (0.5, 0.25, 0.375))          # vertices and edges on voxel centres (vs 0.125)
    F = Tt.copy()
    F[::2] = F[::2, ::-1]
    Pd = np.vstack([Pt, [[0.75, 0.0, 0.125], [1.0, 0.0, 0.125], [0.875, 0.0, 0.125]]])
    Td = np.vstack([Tt, [[8, 9, 10]]])
    pts, cells = core.generate_mesh(ns['torus'](0.6, 0.25), samples=2 ** 13, verbose=False)[:2]
    return {
        'box': (P, T, (0.1, 0.07)),
        'box_ties': (Pt, Tt, (0.125, 0.0625)),
        'icosphere': icosphere(3) + ((0.07, 0.05),),
        'torus': (pts, cells, (0.07, 0.05)),
        'half_flipped': (Pt, F, (0.125, 0.0625)),
        'degenerate': (Pd, Td, (0.125, 0.0625)),
    }


@pytest.fixture(scope='module')
def cases(ns):
    return meshes(ns)


@pytest.mark.parametrize('name', ['box', 'box_ties', 'icosphere', 'torus', 'half_flipped', 'degenerate'])
@pytest.mark.parametrize('half_width', [None, 0.3])
@pytest.mark.parametrize('which', [0, 1])
def test_grid_is_bit_identical_to_the_restatement(name, half_width, which, cases, eng):
    P, T, sizes = cases[name]
    vs = sizes[which]
    ijk0, A, bg, _ = ref.level_set(P, T, vs, half_width)
    hw = ref.half_width_voxels(vs, half_width)
    dijk0, dA = eng.mesh_level_set(P, T, vs, hw)
    assert np.array_equal(dijk0, ijk0) and dA.shape == A.shape, (dijk0, ijk0, dA.shape, A.shape)
    assert np.array_equal(dA.view(np.uint32), A.view(np.uint32)), np.count_nonzero(dA.view(np.uint32) != A.view(np.uint32))
    f = mesh.Mesh(P, T).sdf(vs, half_width, voxelizer='device')
    assert np.array_equal(f.array.view(np.uint32), A.view(np.uint32)) and np.array_equal(f.ijk0, ijk0) and f.background == bg
    for i in range(3):
        assert np.array_equal(f.xyz[i], np.linspace(ijk0[i] * vs, (ijk0[i] + A.shape[i] - 1) * vs, A.shape[i]))


def test_end_to_end_through_the_fused_path(ns, oracle_lib, eng):
    P, T = icosphere(3)
    vs = 0.07
    g = mesh.Mesh(P, T).sdf(vs, voxelizer='device') - ns['sphere'](0.3)
    ijk0, A, bg, _ = ref.level_set(P, T, vs)
    xyz = tuple(np.linspace(ijk0[i] * vs, (ijk0[i] + A.shape[i] - 1) * vs, A.shape[i]) for i in range(3))
    h = mesh.grid_sdf(xyz, A, bg, mesh.Mesh(P, T).bounding_box) - ns['sphere'](0.3)
    rng = np.random.default_rng(5)
    Q = rng.uniform(-1.4, 1.4, size=(20000, 3))
    assert np.array_equal(eng.eval_points(g, Q), oracle_lib.evaluate(h, Q))
    bounds = core._estimate_bounds(g)
    X, Y, Z, _ = core.grid_axes(bounds, samples=2 ** 17)
    pts = core.generate(g, bounds=bounds, samples=2 ** 17, verbose=False)
    o = oracle_lib.generate(h, X, Y, Z, 32, True)
    assert len(pts) > 0 and np.array_equal(pts, o.points)


def test_sphere_mesh_is_geometrically_sane(ns, eng):
    pts, cells = core.generate_mesh(ns['sphere'](1), samples=2 ** 18, verbose=False)[:2]
    # how far the mesh lies from the unit sphere: its vertices outward, its facets inward (the distance of the origin to each)
    zero = (np.zeros((1, 1)),) * 3
    V = pts[cells]
    a, b, c = (tuple(V[None, :, e, i] for i in range(3)) for e in range(3))
    inner = np.sqrt(ref.tri_d2(zero, a, b, c).min())
    r = np.linalg.norm(pts, axis=1)
    dev = max(r.max() - 1, 1 - inner, np.abs(r - 1).max())
    vs = 0.05
    f = mesh.Mesh(pts, cells).sdf(vs, voxelizer='device')
    I, J, K = np.meshgrid(*(np.arange(n) + o for n, o in zip(f.array.shape, f.ijk0)), indexing='ij')
    s = np.sqrt((I * vs) ** 2 + (J * vs) ** 2 + (K * vs) ** 2) - 1
    band = np.abs(f.array) < np.float32(f.background)
    assert band.sum() > 1000
    assert np.all(np.abs(f.array[band] - s[band]) <= dev + 1e-6), (np.abs(f.array[band] - s[band]).max(), dev)
    assert np.all(f.array[s < -dev - 1e-6] < 0) and np.all(f.array[s > dev + 1e-6] > 0)


def _lib_call(eng, P, T, vs, hw, out, cap):
    ijk0, dims = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    pts = np.ascontiguousarray(P, dtype=np.float64)
    tri = np.ascontiguousarray(T, dtype=np.int32)
    rc = eng.lib.sdf_mesh_level_set_host(eng.ctx, pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(pts),
                                         tri.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(tri), vs, hw, ijk0, dims,
                                         None if out is None else out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cap)
    return rc, list(dims)


def test_invalid_input_raises_and_nothing_is_held(eng):
    P, T = box_mesh((0, 0, 0), (1, 1, 1))
    for args in [(np.zeros((0, 3)), np.zeros((0, 3), int), 0.1), (P, np.zeros((0, 3), int), 0.1), (P, T + 1, 0.1), (P, T - 1, 0.1),
                 (np.where(P == 1, np.nan, P), T, 0.1), (np.where(P == 1, np.inf, P), T, 0.1), (P, T, 0.0), (P, T, -0.1),
                 (P, T, 1e-9), (P, T, 3e-4)]:
        with pytest.raises(ValueError):
            eng.mesh_level_set(*args, 3)
    with pytest.raises(ValueError):
        mesh.Mesh(P, T).sdf(3e-4, voxelizer='device')
    # the C entry point checks on its own, too
    assert _lib_call(eng, P, T + 5, 0.1, 3, None, 0)[0] == 2
    assert b'indexes point' in eng.lib.sdf_last_error()
    assert _lib_call(eng, np.where(P == 1, np.nan, P), T, 0.1, 3, None, 0)[0] == 2
    assert _lib_call(eng, P, T, -1.0, 3, None, 0)[0] == 2
    # a too small buffer: the dims come back and nothing is written
    out = np.full(4, 7.0, np.float32)
    rc, dims = _lib_call(eng, P, T, 0.1, 3, out, 4)
    assert rc == 0 and np.prod(dims) > 4 and np.all(out == 7.0)
    # device memory: equal before and after 20 calls
    Pi, Ti = icosphere(2)
    eng.mesh_level_set(Pi, Ti, 0.05, 3)

    def free():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert eng.lib.sdf_device_mem_info(0, ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    f0 = free()
    for i in range(20):
        eng.mesh_level_set(Pi, Ti, 0.05 + 0.001 * i, 3 + i % 3)
    assert free() == f0


def test_large_mesh_band_voxels(ns, eng):
    import fixtures
    f = fixtures.build('ex_example', ns)
    pts, cells = core.generate_mesh(f, samples=2 ** 24, verbose=False)[:2]
    assert len(cells) > 500000
    vs = float(np.ptp(pts, axis=0).max()) / 200
    g = mesh.Mesh(pts, cells).sdf(vs, voxelizer='device')
    A, ijk0 = g.array, g.ijk0
    band = np.argwhere(np.abs(A) < np.float32(g.background))
    assert len(band) > 10000 and (A < 0).any()
    pick = band[np.random.default_rng(11).choice(len(band), 300, replace=False)]
    want = ref.voxel_values(pts, cells, vs, None, ijk0 + pick)
    got = A[tuple(pick.T)]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.count_nonzero(got != want)
