"""The NumPy restatement of the device mesh-to-level-set voxelizer (tests/level_set_ref.py) against ground truth, and
the binary STL reader of `Mesh.from_stl`.  No GPU."""
import numpy as np
import pytest

import level_set_ref as ref
import level_set_truth as truth
from level_set_truth import CUBE_P, CUBE_T, box_mesh, torus_mesh                # noqa: F401 (other test modules take them from here)
from sdf_amd import mesh, stl


def box_distance(P, lo, hi):
    """exact signed distance to the box [lo, hi]"""
    c, h = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    q = np.abs(P - c) - h
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


def voxel_points(ijk0, shape, vs):
    I, J, K = np.meshgrid(*(np.arange(n) + o for n, o in zip(shape, ijk0)), indexing='ij')
    return np.stack([I.ravel() * vs, J.ravel() * vs, K.ravel() * vs], axis=1)


def expected_box(ijk0, shape, vs, bg, lo, hi):
    P = voxel_points(ijk0, shape, vs)
    s = box_distance(P, lo, hi)
    return np.clip(s, -bg, bg).astype(np.float32).reshape(shape), s.reshape(shape)


@pytest.mark.parametrize('vs,half_width', [(0.1, None), (0.07, 0.3)])
def test_box_matches_the_analytic_distance(vs, half_width):
    lo, hi = (-0.43, -0.31, -0.27), (0.52, 0.36, 0.33)
    P, T = box_mesh(lo, hi)
    ijk0, A, bg, (wlo, wn) = ref.level_set(P, T, vs, half_width)
    assert bg == float(np.float32(ref.half_width_voxels(vs, half_width) * vs))
    want, s = expected_box(ijk0, A.shape, vs, bg, lo, hi)
    assert np.allclose(A, want, rtol=0, atol=1e-6)
    assert np.all(np.abs(A) <= bg)
    assert np.all((A < 0) == (s < 0))                     # no voxel of this grid lies on the surface
    # the returned box is exactly the voxels with |v| < background: every face of it holds one
    act = np.abs(A) < np.float32(bg)
    for ax in range(3):
        assert act.take(0, axis=ax).any() and act.take(-1, axis=ax).any()
    assert np.all(ijk0 >= wlo) and np.all(ijk0 + A.shape <= wlo + wn)


def test_ties_on_column_centres_and_half_flipped_orientation():
    """every vertex and edge of the box lies on voxel centres: columns run through edges and vertices (the watertight
    crossing test counts each once); flipping every other triangle changes nothing"""
    vs = 0.125
    lo, hi = (-0.25, -0.375, -0.25), (0.5, 0.25, 0.375)
    P, T = box_mesh(lo, hi)
    ijk0, A, bg, _ = ref.level_set(P, T, vs)
    want, s = expected_box(ijk0, A.shape, vs, bg, lo, hi)
    # (a closest point on an edge is a + ab * t with t = 1/6, ...: not exact, so voxels ON the surface get |v| ~ 1e-17)
    assert np.allclose(A, want, rtol=0, atol=1e-6)
    assert np.all((A[s != 0] < 0) == (s[s != 0] < 0)) and np.all(np.abs(A[s == 0]) < 1e-12)
    assert np.count_nonzero(s == 0) > 100
    F = T.copy()
    F[::2] = F[::2, ::-1]
    ijk0f, Af, _, _ = ref.level_set(P, F, vs)
    # (the parity is the same; a distance may differ in its last bits: the vertices come in another order)
    assert np.array_equal(ijk0f, ijk0) and np.allclose(Af, A, rtol=0, atol=1e-6)
    off = np.abs(A) > 1e-12
    assert np.array_equal(Af[off] < 0, A[off] < 0)


def test_torus_columns_through_the_hole():
    R, r = 0.6, 0.25
    P, T = torus_mesh(R, r)
    vs = 0.05
    ijk0, A, bg, _ = ref.level_set(P, T, vs)
    Q = voxel_points(ijk0, A.shape, vs)
    s = (np.hypot(np.hypot(Q[:, 0], Q[:, 1]) - R, Q[:, 2]) - r).reshape(A.shape)
    dev = 0.03                                            # how far the facets stray from the torus (chords of 0.1 - 0.2)
    assert np.all(A[s < -dev] < 0) and np.all(A[s > dev] > 0)
    band = np.abs(s) < bg - dev
    assert np.all(np.abs(A[band] - s[band]) <= dev + 1e-6)
    centre = tuple(-ijk0)                                 # the voxel at the origin: in the hole, outside
    assert A[centre] == np.float32(bg)


def test_degenerate_triangle_contributes_its_edges():
    lo, hi = (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)
    P, T = box_mesh(lo, hi)
    # a zero-area triangle beside the box: three collinear points along x
    P = np.vstack([P, [[1.0, 0.25, 0.25], [1.3, 0.25, 0.25], [1.1, 0.25, 0.25]]])
    T = np.vstack([T, [[8, 9, 10]]])
    vs = 0.1
    ijk0, A, bg, _ = ref.level_set(P, T, vs)
    Q = voxel_points(ijk0, A.shape, vs)
    seg = np.hypot(np.clip(Q[:, 0], 1.0, 1.3) - Q[:, 0], np.hypot(Q[:, 1] - 0.25, Q[:, 2] - 0.25))
    d = np.minimum(np.abs(box_distance(Q, lo, hi)), seg)
    want = np.where(box_distance(Q, lo, hi) < 0, -1, 1) * np.minimum(d, bg)
    assert np.allclose(A.ravel(), want, rtol=0, atol=1e-6)
    # and the restated distance itself, point by point, against the segment
    p = tuple(Q[:, i][:, None] for i in range(3))
    a, b, c = (tuple(P[T[-1, e], i:i + 1][None, :] for i in range(3)) for e in range(3))
    assert np.allclose(ref.tri_d2(p, a, b, c)[:, 0], seg ** 2, rtol=0, atol=1e-12)


def test_voxel_values_agree_with_the_dense_restatement():
    P, T = torus_mesh(0.5, 0.2, 16, 8)
    vs = 0.06
    ijk0, A, _, _ = ref.level_set(P, T, vs, 0.2)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, A.shape, size=(40, 3))
    got = ref.voxel_values(P, T, vs, 0.2, ijk0 + idx)
    assert np.array_equal(got.view(np.uint32), A[tuple(idx.T)].view(np.uint32))


@pytest.mark.parametrize('name', truth.NAMES)
def test_restatement_holds_to_true_distance_and_winding_number(name):
    """The restatement against tests/level_set_truth.py, which shares none of its derivation: on every catalogue case the
    magnitude within one float32 ulp of the background of the true clamped distance, the sign that of the winding number,
    the distance to 1e-12 on the surface, and the returned box the index box of float32(want) < background (`truth.hold`).

    The open prefixes ('open1' ... 'open5': the first triangles of the octahedron) are held in magnitude and box only.  An
    open mesh has no inside; the sign it gets is the parity of the crossings below the voxel, which is this library's
    definition and stays so."""
    c = truth.get_case(name)
    ijk0, A, bg, work = ref.level_set(c.points, c.triangles, c.voxel_size, c.half_width)
    assert bg == truth.case_truth(name).bg
    f = truth.hold_case(name, ijk0, A, work)
    print('%s: grid %s, work grid %s, on the surface %d, largest | |v| - want | %.3f ulp of the background'
          % (name, f['shape'], f['work'], f['on_surface'], f['max_ulp']))


def test_truth_distance_and_winding_on_known_points():
    """the truth itself where the answer is known in closed form: the unit right triangle in the plane z = 0 (face, the three
    sides, the three corners, a point above), a triangle shrunk to a segment and to a point, and the winding number of the
    unit cube (1 inside, 0 outside, 2 for the cube listed twice, -1 turned inside out)"""
    V = np.array([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    Q = np.array([[0.25, 0.25, 0.5], [0.5, -2.0, 0.0], [-3.0, 0.5, 4.0], [1.0, 1.0, 1.0], [-1.0, -2.0, 2.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.0],
                  [0.25, 0.25, 0.0], [0.5, 0.5, 0.0]])
    want = [0.25, 4.0, 25.0, 1.5, 9.0, 5.0, 5.0, 0.0, 0.0]
    for turn in range(3):                                 # whichever corner is listed first
        assert np.allclose(truth.true_d2(Q, np.roll(V, turn, axis=1)).astype(np.float64), want, rtol=0, atol=1e-15)
    S = np.array([[[0.0, 0, 0], [2, 0, 0], [1, 0, 0]], [[5.0, 5, 5]] * 3])
    assert np.allclose(truth.true_d2(np.array([[3.0, 4.0, 0.0], [1.5, 0.0, 2.0]]), S[:1]).astype(np.float64), [17.0, 4.0], rtol=0, atol=1e-15)
    assert np.allclose(truth.true_d2(np.array([[5.0, 5.0, 7.0]]), S[1:]).astype(np.float64), [4.0], rtol=0, atol=1e-15)
    assert np.all(np.isinf(truth.true_d2(Q, V + 100.0, reach=1.0)))
    C = CUBE_P[CUBE_T]
    Q = np.array([[0.5, 0.5, 0.5], [0.1, 0.9, 0.3], [1.5, 0.5, 0.5], [-0.2, -0.2, -0.2], [0.5, 0.5, 7.0]])
    assert np.allclose(truth.winding(Q, C), [1, 1, 0, 0, 0], rtol=0, atol=1e-12)
    assert np.allclose(truth.winding(Q, np.concatenate([C, C])), [2, 2, 0, 0, 0], rtol=0, atol=1e-12)
    assert np.allclose(truth.winding(Q, C[:, ::-1]), [-1, -1, 0, 0, 0], rtol=0, atol=1e-12)


def test_from_stl_round_trip_and_truncated_file(tmp_path):
    P, T = torus_mesh(0.6, 0.25, 12, 6)
    soup = P[T].reshape(-1, 3) * 1.37 + 0.1
    path = str(tmp_path / 'a.stl')
    stl.write_binary_stl(path, soup)
    m = mesh.Mesh.from_stl(path)
    want_p, want_c = np.unique(soup.astype(np.float32).astype(np.float64), axis=0, return_inverse=True)
    assert m.points.dtype == np.float64 and np.array_equal(m.points, want_p)
    assert np.array_equal(m.triangles, np.asarray(want_c).reshape(-1, 3))
    assert len(m.points) == len(P)                        # the shared vertices are welded
    data = open(path, 'rb').read()
    for cut in (data[:-1], data[:-50], data[:60], data + b'\0'):
        bad = str(tmp_path / 'bad.stl')
        open(bad, 'wb').write(cut)
        with pytest.raises(ValueError):
            mesh.Mesh.from_stl(bad)


def test_mesh_sdf_keeps_openvdb_as_default_and_checks_the_keyword():
    m = mesh.Mesh(*box_mesh((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ImportError):
        m.sdf(0.1)
    with pytest.raises(ValueError):
        m.sdf(0.1, voxelizer='cpu')
    assert mesh.half_width_voxels(0.1) == 3 and mesh.half_width_voxels(0.1, 0.55) == 6 and mesh.half_width_voxels(0.1, 0.1) == 3
