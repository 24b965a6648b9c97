"""The definition of mesh simplification to a tolerance, in plain NumPy on top of tests/simplify_ref.py: octree
vertex clustering (Schaefer and Warren) with the quadric of section 4j as the error measure; what csrc/sdf_simplify.hip reproduces
bit for bit under sdf_mesh_simplify_adaptive.

Input: the weld (points (U, 3) float64, cells (T, 3) int64), `origin`, `cell`, `reg` as for `simplify_ref.simplify`, `tolerance` >= 0
(+inf is allowed, NaN is refused) and `levels`, an integer from 0 to 10.  Every float64 operation is one IEEE operation, in the order
written; nothing is fused.

Level L (0 .. levels) is exactly `simplify_ref` on the grid (origin, cell * 2^L) -- its `clusters`, `means`, `quadrics` and `solve`
with that cell: per cluster the representative v = centre + x, the weight w = (A00 + A11) + A22 of its quadric and the flags `flat`
and `mean_fallback`.  The refusals of `clusters` apply per level (level 0 has the widest key range: it decides); a cell * 2^levels
that is not finite is refused like a cell that is not.

Error of a level-L cluster.  With n and d of every item as `quadrics` computes them, about the centre of the item's cluster, and x
the representative actually used (after the fallbacks): r = ((nx * x0 + ny * x1) + nz * x2) - d, and err is the sum of r * r over
the cluster's items in ascending item index, from 0.0.  The cluster is ACCEPTED iff err <= (tolerance * tolerance) * w -- no
division: a flat cluster has 0 <= 0 and is accepted -- or tolerance * tolerance is +inf (every cluster then: inf * 0 and an err that
overflowed would otherwise be NaNs that compare false).  Level 0 is always accepted.  That is the squared-area-weighted mean squared
distance of the representative from the planes of the triangles that touch the cluster, compared with tolerance^2.  It is not a
Hausdorff bound.

Choice.  Every welded vertex takes the COARSEST level whose cluster (the one it falls into) is accepted; its id is (level, cluster
number on that level) and its position is that cluster's representative.  Intermediate levels need not accept.

Triangles.  A triangle survives if its three ids differ; survivors keep their order and their winding; the output is the soup of the
survivors.

Stats: triangles_in, triangles_out, collapsed, levels; per level (lists of levels + 1 integers) clusters_used -- the clusters that
at least one vertex chose -- and vertices -- the vertices that chose the level; mean_fallback and flat summed over the used clusters.

Two identities: levels = 0 is `simplify_ref.simplify(points, cells, origin, cell)` bit for bit, and tolerance = inf is
`simplify_ref.simplify(points, cells, origin, cell * 2^levels)` bit for bit."""
import collections
import numbers

import numpy as np

import simplify_ref

Adaptive = collections.namedtuple('Adaptive', ('soup', 'stats', 'vertex_level', 'vertex_cluster', 'positions', 'accepted', 'err', 'weight'))
Adaptive.__doc__ = """soup (T', 3, 3) float64 and stats: what the device reproduces.  For the tests: vertex_level (U,) and
vertex_cluster (U,) int64 the chosen id, positions (U, 3) the chosen representative of every welded vertex; accepted, err, weight:
per level the (K_L,) arrays of the clusters (accepted[0] is all True)."""

STAT_KEYS = ('triangles_in', 'triangles_out', 'collapsed', 'levels', 'clusters_used', 'vertices', 'mean_fallback', 'flat')
MAX_LEVELS = 10


def check_args(tolerance, levels):
    """(tolerance as a float, levels as an int), or ValueError"""
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (numbers.Real, np.floating, np.integer)):
        raise ValueError('simplify_adaptive: tolerance must be a real number >= 0 (inf is allowed), got %r' % (tolerance,))
    t = float(tolerance)
    if not t >= 0:                                                # (NaN fails this too)
        raise ValueError('simplify_adaptive: tolerance must be a real number >= 0 (inf is allowed), got %r' % (tolerance,))
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (numbers.Integral, np.integer)) or not 0 <= int(levels) <= MAX_LEVELS:
        raise ValueError('simplify_adaptive: levels must be an integer from 0 to %d, got %r' % (MAX_LEVELS, levels))
    return t, int(levels)


def errors(points, cells, vertex_cluster, centres, x):
    """err (K,): per cluster the sum over its items, in ascending item index from 0.0, of the squared residual of the representative
    (x (K, 3), about the centre) in the item's plane -- n and d as `simplify_ref.quadrics` computes them"""
    item_cluster = vertex_cluster[cells].reshape(-1)              # item 3t + c
    c = centres[item_cluster]
    tri = np.repeat(np.arange(len(cells)), 3)
    a = points[cells[tri, 0]] - c
    b = points[cells[tri, 1]] - c
    cc = points[cells[tri, 2]] - c
    e1, e2 = b - a, cc - a
    xi = x[item_cluster]
    with np.errstate(all='ignore'):
        nx = (e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1])
        ny = (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2])
        nz = (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])
        d = (nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2]
        r = ((nx * xi[:, 0] + ny * xi[:, 1]) + nz * xi[:, 2]) - d
        return simplify_ref.segment_sums(item_cluster, (r * r)[:, None], len(centres))[0][:, 0]


Level = collections.namedtuple('Level', ('vertex_cluster', 'vertices', 'flat', 'fallback', 'err', 'weight'))


def level(points, cells, origin, cell, reg):
    """the Level of the grid (origin, cell): `simplify_ref` on it, and the error and the weight of every cluster"""
    vertex_cluster, qk, centres = simplify_ref.clusters(points, origin, cell)
    mean = simplify_ref.means(points, vertex_cluster, centres)
    quadric = simplify_ref.quadrics(points, cells, vertex_cluster, centres)
    x, flat, fallback = simplify_ref.solve(quadric, mean, cell, reg)
    err = errors(points, cells, vertex_cluster, centres, x)
    with np.errstate(all='ignore'):
        w = (quadric[:, 0] + quadric[:, 3]) + quadric[:, 5]
    return Level(vertex_cluster, centres + x, flat, fallback, err, w)


def accepted(lv, t2, always):
    """(K,) bool: err <= t2 * w, or every cluster at level 0 and under an infinite t2"""
    if always or np.isinf(t2):
        return np.ones(len(lv.err), bool)
    with np.errstate(all='ignore'):
        return lv.err <= t2 * lv.weight


def check_mesh(points, cells, origin, cell, reg, levels):
    """the arguments that do not depend on the tolerance, as float64 / int64 arrays, or ValueError"""
    origin, cell, reg = simplify_ref.check_args(origin, cell, reg)
    with np.errstate(over='ignore'):
        coarsest = cell * 2.0 ** levels
    if not np.isfinite(coarsest).all():
        raise ValueError('simplify_adaptive: cell * 2^levels must be finite, got %r and %d' % (cell.tolist(), levels))
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    if len(points) >= 2 ** 31 or 3 * len(cells) >= 2 ** 31:
        raise ValueError('simplify_adaptive: 2^31 or more vertices or corners (3 x triangles)')
    return points, cells, origin, cell, reg


def pyramid(points, cells, origin, cell, levels=5, reg=1e-3):
    """the Levels 0 .. levels of a welded mesh: everything that does not depend on the tolerance (a test that tries several
    tolerances on one mesh computes it once and hands it to `simplify_adaptive`)"""
    levels = check_args(0.0, levels)[1]
    points, cells, origin, cell, reg = check_mesh(points, cells, origin, cell, reg, levels)
    if len(points) == 0:
        return [None] * (levels + 1)
    return [level(points, cells, origin, cell * 2.0 ** lv, reg) for lv in range(levels + 1)]


def simplify_adaptive(points, cells, origin, cell, tolerance, levels=5, reg=1e-3, pyramid_of_it=None):
    """the Adaptive of the welded mesh (points (U, 3) float64, cells (T, 3) int64) on the grids (origin, cell * 2^L), L = 0 .. levels;
    pyramid_of_it: `pyramid` of the same arguments, where it has been computed already"""
    tolerance, levels = check_args(tolerance, levels)
    points, cells, origin, cell, reg = check_mesh(points, cells, origin, cell, reg, levels)
    pyr = pyramid(points, cells, origin, cell, levels, reg) if pyramid_of_it is None else pyramid_of_it
    u = len(points)
    t2 = tolerance * tolerance
    vertex_level = np.full(u, -1, np.int64)
    chosen = np.full(u, -1, np.int64)
    positions = np.zeros((u, 3), np.float64)
    stats = {'triangles_in': len(cells), 'triangles_out': 0, 'collapsed': 0, 'levels': levels, 'clusters_used': [0] * (levels + 1),
             'vertices': [0] * (levels + 1), 'mean_fallback': 0, 'flat': 0}
    acc, err, weight = [np.zeros(0, bool)] * (levels + 1), [np.zeros(0)] * (levels + 1), [np.zeros(0)] * (levels + 1)
    for lv in range(levels, -1, -1):                              # from the coarsest down: the first level that accepts is the coarsest
        r = pyr[lv]
        if r is None:
            continue
        acc[lv], err[lv], weight[lv] = accepted(r, t2, lv == 0), r.err, r.weight
        take = (vertex_level < 0) & acc[lv][r.vertex_cluster]
        vertex_level[take] = lv
        chosen[take] = r.vertex_cluster[take]
        positions[take] = r.vertices[r.vertex_cluster[take]]
        used = np.zeros(len(r.vertices), bool)
        used[r.vertex_cluster[take]] = True
        stats['clusters_used'][lv] = int(used.sum())
        stats['vertices'][lv] = int(take.sum())
        stats['mean_fallback'] += int((used & r.fallback).sum())
        stats['flat'] += int((used & r.flat).sum())
    tl, tc = vertex_level[cells], chosen[cells]
    same = lambda i, j: (tl[:, i] == tl[:, j]) & (tc[:, i] == tc[:, j])
    live = ~(same(0, 1) | same(1, 2) | same(0, 2))
    soup = positions[cells[live]].reshape(-1, 3, 3)
    stats['triangles_out'] = int(live.sum())
    stats['collapsed'] = int(len(cells) - live.sum())
    return Adaptive(soup, stats, vertex_level, chosen, positions, acc, err, weight)
