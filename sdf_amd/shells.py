"""The connected shells of a mesh, found and kept or dropped on the device (not in the reference): a model
sampled on a grid routinely meshes into more pieces than were asked for -- crumbs of a wall thinner than the step, a part that a
`-` has cut loose, sealed inner cavities (shells of negative volume), knurls clipped by the bounds.  `shells(f)` labels the welded
mesh (`Mesh.components`, sdf_mesh_components), `measure_shells(f)` measures every shell on its own, and `save`, `generate_mesh` and
`measure` take `keep=` (`resolve_keep`) to write or return a selection (`Mesh.select`, sdf_mesh_select_shells).
tests/components_ref.py is the definition."""
import collections
import numbers

import numpy as np

from .meshfile import frozen as _frozen

Shells = collections.namedtuple('Shells', ('count', 'triangles', 'vertices', 'bounds', 'vertex_shell', 'triangle_shell', 'rounds'))
Shells.__doc__ = """what `shells` returns (immutable).  count: K; per shell k, numbered by its lexicographically smallest vertex:
triangles[k], vertices[k] (int64) and bounds[k] (2, 3) float64; vertex_shell (U,) int32 over the welded vertices, triangle_shell
(T,) int32 over the triangles in soup order; rounds: the passes the labelling took."""


def shells_of_mesh(mesh):
    """the Shells of a device mesh (`engine.Mesh`): welds and labels it there if that has not happened"""
    c = mesh.components()
    return Shells(count=c['count'], triangles=_frozen(c['triangles']), vertices=_frozen(c['vertices']), bounds=_frozen(c['bounds']),
                  vertex_shell=_frozen(c['vertex_shell']), triangle_shell=_frozen(c['triangle_shell']), rounds=c['rounds'])


def shells_of_soup(soup):
    """the Shells of a float64 soup (T, 3, 3) on the host: uploaded (torch), adopted and labelled on the device"""
    from . import core
    with core.adopted(soup) as mesh:
        return shells_of_mesh(mesh)


def _meshed(sdf, generate_kwargs, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5):
    """`core.meshed` for `shells` and `measure_shells`: the arguments of `generate`, nothing printed, one process; simplify: the
    shells are those of the simplified mesh (`sdf_amd/simplify.py`; simplify_tolerance, simplify_levels: simplified to a tolerance), mend: ... of the mended mesh (`sdf_amd/mend.py`)"""
    from . import core, dist
    from .mend import check_mend
    mend = check_mend(mend)      # (before anything else is looked at: a bad value is refused without a device)
    if dist.world_size() > 1:
        raise NotImplementedError('shells: a multi-process run gathers its soup per step; label it in one process, or adopt the '
                                  'gathered soup (Engine.adopt_soup) and use shells_of_mesh')
    return core.meshed(sdf, keep=None, simplify=simplify, mend=mend, to_host=False,
                       **core.pipeline_kwargs(dict(generate_kwargs, verbose=False), simplify_tolerance=simplify_tolerance, simplify_levels=simplify_levels))


def shells(sdf, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`) and label the connected shells of the welded mesh there: only the
    Shells cross the link, not the soup.  simplify: label the mesh simplified in clusters of simplify^3 grid cells (simplify_tolerance,
    simplify_levels: ... simplified to that tolerance); mend: True -- ... and mended (duplicate triangles dropped, oppositely wound pairs cancelled)"""
    with _meshed(sdf, generate_kwargs, simplify, mend, simplify_tolerance, simplify_levels) as m:
        return shells_of_mesh(m.mesh)


def largest_first(triangles):
    """shell numbers by descending triangle count; ties go to the lower number"""
    t = np.asarray(triangles, dtype=np.int64)
    return np.lexsort((np.arange(len(t)), -t))


def measure_shells(sdf, limit=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, **generate_kwargs):
    """a list of `Measurement` (sdf_amd/measure.py), one per shell, largest first by triangle count (ties: the lower shell number);
    `limit` bounds how many.  The model is meshed ONCE; then every shell costs one selection (a compaction of the soup) plus one
    measure (moments, weld, census) on the device, so ask for `limit` shells when the crumbs are many.  A sealed cavity is
    recognisable by its negative `volume`.  simplify: the shells of the mesh simplified in clusters of simplify^3 grid cells;
    simplify_tolerance, simplify_levels: ... simplified to that tolerance; mend: True -- ... and mended."""
    with _meshed(sdf, generate_kwargs, simplify, mend, simplify_tolerance, simplify_levels) as m:
        return measure_shells_of_mesh(m.mesh, limit)


def measure_shells_of_mesh(mesh, limit=None):
    """`measure_shells` of a device mesh"""
    from .measure import measure_mesh
    summary = mesh.shell_summary()
    order = largest_first(summary['triangles'])
    if limit is not None:
        order = order[:max(int(limit), 0)]
    out = []
    for k in order:
        mask = np.zeros(summary['count'], dtype=bool)
        mask[k] = True
        sel = mesh.select(mask)
        try:
            out.append(measure_mesh(sel))
        finally:
            sel.close()
    return out


def check_keep(keep):
    """ValueError for a `keep` that no shell count could make valid (what can be told before anything is meshed)"""
    if isinstance(keep, str):
        if keep != 'largest':
            raise ValueError("keep: the only name is 'largest', got %r" % (keep,))
    elif isinstance(keep, (bool, np.bool_)):
        raise ValueError('keep: a single boolean selects nothing; give a mask with one entry per shell')
    elif isinstance(keep, numbers.Integral):
        if keep < 0:
            raise ValueError('keep: the number of shells to keep cannot be negative, got %d' % keep)
    elif callable(keep):
        pass
    else:
        try:
            a = np.asarray(keep)
        except Exception:
            raise ValueError('keep: %r is neither \'largest\', a count, a boolean mask nor a callable' % (keep,))
        if a.ndim != 1 or (a.dtype != np.bool_ and a.size):      # (an empty mask, for a mesh of no shells, has no type to speak of)
            raise ValueError("keep: %r is neither 'largest', a count, a boolean mask (one entry per shell) nor a callable" % (keep,))


def resolve_keep(keep, triangles):
    """the boolean mask (K,) of the shells to keep.  triangles: the per-shell triangle counts, or the `Shells` they come from (which
    is what a callable is handed).  keep = 'largest': the shell with the most triangles, ties to the lowest shell number; an int n:
    the n largest by the same rule (n >= K: all); a boolean sequence of length K: taken as it is; a callable keep(Shells) -> mask.
    Anything else, or a mask of another length, raises ValueError.  Pure host code: nothing here touches the device."""
    given = triangles
    counts = np.asarray(triangles.triangles if isinstance(triangles, Shells) else triangles, dtype=np.int64).reshape(-1)
    k = len(counts)
    check_keep(keep)
    if callable(keep) and not isinstance(keep, str):
        got = keep(given)
        if callable(got):
            raise ValueError('keep: the callable returned another callable')
        try:
            return resolve_keep(got, counts)
        except ValueError as e:
            raise ValueError('keep: what the callable returned is not usable: %s' % e)
    mask = np.zeros(k, dtype=bool)
    if isinstance(keep, str):
        mask[largest_first(counts)[:1]] = True
    elif isinstance(keep, numbers.Integral):
        mask[largest_first(counts)[:int(keep)]] = True
    else:
        a = np.asarray(keep)
        if len(a) != k:
            raise ValueError('keep: the mask has %d entries, the mesh has %d shells' % (len(a), k))
        mask[:] = a
    return mask
