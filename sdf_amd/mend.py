"""A mesh mended on the device (not in the reference): where a wall is thinner than a cluster, `simplify=`
folds its two sheets onto the same vertices -- every triangle of the wall then exists twice, once in each winding, every edge of it
has four uses, a slicer's manifold check fails and `measure().area` counts the sheet twice.  `save`, `generate_mesh`, `measure`,
`shells` and `measure_shells` take `mend=True`: after keep= and simplify=, the cells of the weld with two equal indices are dropped,
and of the cells over one face (the same three vertices) as many in either winding cancel; if one winding has the majority, its
first triangle in soup order survives alone (`engine.Mesh.mend`, sdf_mesh_mend, csrc/sdf_mend.hip).  A cancelled pair encloses
nothing, so the volume is what it was; the triangles of the two sheets around the hole pair up with each other.  What mending does
not do: a wall that collapsed only in part keeps a non-manifold rim around the collapsed region, and a misoriented mesh is not
re-oriented -- `measure` goes on reporting both.  tests/mend_ref.py is the definition."""
import numpy as np


def check_mend(mend):
    """False or True as a bool; ValueError for anything that is not a boolean (what can be told before anything is meshed)"""
    if not isinstance(mend, (bool, np.bool_)):
        raise ValueError('mend: False or True, got %r' % (mend,))
    return bool(mend)
