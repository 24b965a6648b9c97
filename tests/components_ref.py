"""The definition of the connected shells of a welded mesh, in plain NumPy: what csrc/sdf_components.hip
reproduces exactly.

Vertices are the welded vertices (`Mesh.weld()`: points in lexicographic order, cells (T, 3) int64).  Every cell joins its three
indices -- a collapsed cell (a, a, b) joins a and b, no special case; every welded vertex belongs to at least one cell, so there are
no isolated vertices.  The LABEL of a vertex is the smallest welded index in its connected component; shells are numbered 0 .. K - 1
by ascending label, that is by their lexicographically smallest vertex.  vertex_shell[v] is int32, triangle_shell[t] =
vertex_shell[cells[t, 0]]; per shell: triangles[k], vertices[k] (int64) and bounds[k] (2, 3) float64 over its vertices, a zero
reading +0.0.  (Points that are not finite are outside the definition: the weld does not order them.)  Everything is a function of
the cells, and for the bounds of the points, alone."""
import collections

import numpy as np

Components = collections.namedtuple('Components', ('count', 'vertex_shell', 'triangle_shell', 'triangles', 'vertices', 'bounds', 'labels'))


def labels(cells, n_vertices):
    """(n_vertices,) int64: the smallest index of every vertex's component.  Repeated min-label sweeps over the cells with pointer
    jumping: lab[v] <= v always names a vertex of v's component, and between sweeps lab[lab] == lab (every vertex names its root).
    A sweep hooks the roots of a cell's three vertices under the smallest of them; jumping replaces lab by lab[lab] until that
    changes nothing.  The fixed point is constant on components and maps the smallest vertex of a component to itself."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    lab = np.arange(n_vertices, dtype=np.int64)
    while True:
        roots = lab[cells]
        new = lab.copy()
        np.minimum.at(new, roots.reshape(-1), np.repeat(roots.min(axis=1), 3))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            return lab
        lab = new


def components(points, cells):
    """the Components of the welded mesh (points (U, 3) float64, cells (T, 3) int64)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    lab = labels(cells, len(points))
    roots = np.unique(lab)                                        # ascending: the numbering
    k = len(roots)
    vertex_shell = np.searchsorted(roots, lab).astype(np.int32)
    triangle_shell = vertex_shell[cells[:, 0]] if len(cells) else np.zeros(0, np.int32)
    bounds = np.empty((k, 2, 3), np.float64)
    if k:                                                         # minimum and maximum over each shell's run of the sorted vertices
        order = np.argsort(vertex_shell, kind='stable')
        starts = np.searchsorted(vertex_shell[order], np.arange(k))
        bounds[:, 0] = np.minimum.reduceat(points[order], starts, axis=0)
        bounds[:, 1] = np.maximum.reduceat(points[order], starts, axis=0)
    bounds = bounds + 0.0                                         # -0.0 reads +0.0
    return Components(count=k, vertex_shell=vertex_shell, triangle_shell=triangle_shell.astype(np.int32),
                      triangles=np.bincount(triangle_shell, minlength=k).astype(np.int64),
                      vertices=np.bincount(vertex_shell, minlength=k).astype(np.int64), bounds=bounds, labels=lab)


def weld(soup):
    """(points, cells) of a host soup (T, 3, 3): np.unique over the rows, as `Mesh.weld()` orders them"""
    pts, inv = np.unique(np.asarray(soup, dtype=np.float64).reshape(-1, 3), axis=0, return_inverse=True)
    return pts, np.asarray(inv, dtype=np.int64).reshape(-1, 3)


def rounds_bound(n_vertices):
    """what root hooking with full compression is bounded by: ceil(log2(max(V, 2))) + 2 hook passes, the verifying one included"""
    return int(np.ceil(np.log2(max(int(n_vertices), 2)))) + 2


# ---- hand-made soups (T, 3, 3) ----
TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
TET_FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def tetrahedron(shift=(0.0, 0.0, 0.0), scale=1.0):
    return (TET * scale + np.asarray(shift, dtype=np.float64))[TET_FACES]


def cube(lo, hi, inward=False):
    """the 12 triangles of the box [lo, hi]^3, outward (or reversed)"""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return c[f[:, ::-1] if inward else f]


def collapsed_bridge():
    """two triangles far apart, joined only by a third cell that is collapsed: (a, a, b) with a in the first and b in the second"""
    t0 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    t1 = t0 + np.array([5.0, 5.0, 5.0])
    return np.stack([t0, t1, np.stack([t0[1], t0[1], t1[2]])])
