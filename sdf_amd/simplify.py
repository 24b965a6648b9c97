"""A mesh simplified on the device (not in the reference): a model has to be sampled finely to catch thin walls
and small features, and almost nobody wants that many triangles in the file.  `save`, `generate_mesh`, `measure`, `shells` and
`measure_shells` take `simplify=` -- a real number k > 0: the welded vertices are clustered in blocks of k x k x k grid cells
(Rossignac-Borrel), every cluster gets one representative placed by its quadric error function (Lindstrom), and the triangles whose
three clusters differ survive (`engine.Mesh.simplify`, sdf_mesh_simplify, csrc/sdf_simplify.hip).  About k^2 times fewer triangles
reach the link and the file.  Duplicate triangles and oppositely wound pairs, where two sheets of the surface fall into the same
clusters, are not removed unless `mend=True` follows (`sdf_amd/mend.py`): `measure` reports them.  tests/simplify_ref.py is the
definition.

To a tolerance (tests/adaptive_ref.py is the definition).  One uniform grid keeps about 1 / k^2 of the triangles
of a flat face however flat it is, and a fillet loses its shape as soon as k is large enough to matter for the flat ones.  The same
places take `simplify_tolerance=` -- a real number >= 0 in MODEL UNITS -- and `simplify_levels=` (0 .. 10, default 5): the clustering
above is run on the grids of simplify x 2^L grid cells, L = 0 .. simplify_levels (`simplify=` is then the finest cluster, 1 when only
the tolerance is given), and every welded vertex takes the COARSEST cluster it falls into whose representative lies within the
tolerance of the planes of the triangles that touch the cluster: the squared-area-weighted mean squared distance from those planes
-- the value of the cluster's quadric at the representative over its trace -- is compared with tolerance^2 (octree vertex clustering,
Schaefer and Warren; `engine.Mesh.simplify_adaptive`, sdf_mesh_simplify_adaptive).  Flat faces collapse to a few triangles, creases
and fillets stay as fine as the tolerance asks.  It is not a Hausdorff bound, topology is not preserved (coplanar faces of different
parts closer than the coarsest cell can be joined), and a handful of inverted faces can appear at creases, as with `simplify=`.  A
mostly curved model gains little over `simplify=`."""
import numbers

import numpy as np


def check_simplify(simplify):
    """None (off) or the block size as a float; ValueError for anything that is not a real number > 0 (what can be told before
    anything is meshed)"""
    if simplify is None:
        return None
    if isinstance(simplify, (bool, np.bool_)) or not isinstance(simplify, (numbers.Real, np.floating, np.integer)):
        raise ValueError('simplify: None or a real number > 0 (the edge of a cluster in grid cells), got %r' % (simplify,))
    k = float(simplify)
    if not (np.isfinite(k) and k > 0):
        raise ValueError('simplify: None or a real number > 0 (the edge of a cluster in grid cells), got %r' % (simplify,))
    return k


def resolve_cell(simplify, X, Y, Z, step):
    """(origin (3,), cell (3,)) float64 of the clustering grid of a sampled model: the origin is the first sample (X[0], Y[0], Z[0]),
    the cell simplify x (dx, dy, dz) -- the clusters are blocks of simplify^3 grid cells"""
    k = check_simplify(simplify)
    if k is None:
        raise ValueError('simplify: None has no cell')
    origin = np.array([X[0], Y[0], Z[0]], dtype=np.float64)
    cell = k * np.array([float(s) for s in step], dtype=np.float64)
    return origin, cell


def check_tolerance(tolerance, name='simplify_tolerance'):
    """None (off) or the tolerance as a float; ValueError naming `name` for anything that is not a real number >= 0 (+inf is
    allowed: every cluster of the coarsest level is then accepted; NaN is not)"""
    if tolerance is None:
        return None
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (numbers.Real, np.floating, np.integer)):
        raise ValueError('%s: None or a real number >= 0 in model units, got %r' % (name, tolerance))
    t = float(tolerance)
    if not t >= 0:
        raise ValueError('%s: None or a real number >= 0 in model units, got %r' % (name, tolerance))
    return t


def check_levels(levels, name='simplify_levels'):
    """the number of levels above the finest as an int; ValueError naming `name` for anything that is not an integer from 0 to 10"""
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (numbers.Integral, np.integer)) or not 0 <= int(levels) <= 10:
        raise ValueError('%s: an integer from 0 to 10 (the levels above the finest cluster), got %r' % (name, levels))
    return int(levels)


DEFAULT_LEVELS = 5


def check_adaptive(simplify, simplify_tolerance, simplify_levels):
    """(simplify, tolerance, levels) of a call that takes the three keywords, checked before anything is meshed: without a
    tolerance (simplify as `check_simplify` gives it, None, None) -- and a simplify_levels other than the default is refused, it
    would do nothing --; with one, simplify defaults to 1: the finest cluster is a grid cell"""
    k = check_simplify(simplify)
    t = check_tolerance(simplify_tolerance)
    if t is None:
        if simplify_levels is not None and not (isinstance(simplify_levels, (numbers.Integral, np.integer)) and not isinstance(simplify_levels, (bool, np.bool_))
                                                and int(simplify_levels) == DEFAULT_LEVELS):
            raise ValueError('simplify_levels: given without simplify_tolerance (the levels belong to simplifying to a tolerance), got %r' % (simplify_levels,))
        return k, None, None
    return (1.0 if k is None else k), t, check_levels(DEFAULT_LEVELS if simplify_levels is None else simplify_levels)
