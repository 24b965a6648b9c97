"""A mesh simplified on the device (not in the reference): a model has to be sampled finely to catch thin walls
and small features, and almost nobody wants that many triangles in the file.  `save`, `generate_mesh`, `measure`, `shells` and
`measure_shells` take `simplify=` -- a real number k > 0: the welded vertices are clustered in blocks of k x k x k grid cells
(Rossignac-Borrel), every cluster gets one representative placed by its quadric error function (Lindstrom), and the triangles whose
three clusters differ survive (`engine.Mesh.simplify`, sdf_mesh_simplify, csrc/sdf_simplify.hip).  About k^2 times fewer triangles
reach the link and the file.  Duplicate triangles and oppositely wound pairs, where two sheets of the surface fall into the same
clusters, are not removed unless `mend=True` follows (`sdf_amd/mend.py`): `measure` reports them.  tests/simplify_ref.py is the
definition."""
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
