"""Build directions rated on the device (not in the reference): which way up should a part be printed, and what
does each choice cost in supports?  `overhangs(f, directions)` meshes a model, keeps the soup on the GPU and rates every direction
there (`engine.Mesh.overhangs`, sdf_mesh_overhangs: a dense triangles x directions pass with a lane per direction and a fixed
summation tree): the area of the faces that overhang more steeply than the printer's angle, the volume of support under them, the
area that lies on the bed, and the height.  Nothing crosses the link but a few numbers per direction.  tests/overhang_ref.py is the
definition; `normalise`, `sin_limit_of` and `derive` restate its few lines of host arithmetic.

support_volume is a PROXY: the prism from every overhanging face straight down to the bed plane.  It does not subtract the part's
own material under an overhang, and in a soup of overlapping solids it counts the faces hidden inside the union.  `supports`
(sdf_amd/supports.py, section 4o) traces rays from the overhanging faces down to the part for the directions this rating puts first.

To use a result: `f.rotate_to(o.directions[o.best()], Z)` -- or `o.rotation(o.best())` for a mesh."""
import collections
import math

import numpy as np

from .meshfile import frozen as _frozen

UP = (0.0, 0.0, 1.0)
NEITHER, OVERHANG, CONTACT, NONFINITE = 0, 1, 2, 3      # the classes of `Overhangs.classes`
MAX_DIRECTIONS = 1 << 20

_FIELDS = ('directions', 'lo', 'hi', 'height', 'overhang_area', 'support_volume', 'contact_area', 'overhang_triangles',
           'contact_triangles', 'angle', 'bed_tolerance', 'sums', 'classes')


class Overhangs(collections.namedtuple('Overhangs', _FIELDS)):
    """what `overhangs` returns (immutable; the arrays are read-only).  directions (K, 3): the unit build directions, "up"; lo, hi,
    height (K,): the extent of the part along each; overhang_area, support_volume, contact_area (K,): the area of the faces with
    n.d < -sin(angle) that do not lie on the bed, the volume of the prisms from those faces down to the bed plane (a proxy: the
    part's own material is not subtracted, hidden faces of overlapping solids count), the area of the downward faces within
    bed_tolerance of the bed; overhang_triangles, contact_triangles (K,) int64; angle (degrees), bed_tolerance: float; sums (K, 3):
    the raw totals the values come from; classes: (T,) uint8 -- 0 neither, 1 overhang, 2 bed contact, 3 non-finite -- or None."""
    __slots__ = ()

    def best(self, key='support_volume'):
        """the index of the direction with the smallest `key`, the first one on ties.  key: a field name, or a callable that takes
        this record and returns (K,) values"""
        v = np.asarray(key(self) if callable(key) else getattr(self, key), dtype=np.float64).reshape(-1)
        if v.shape != (len(self.directions),):
            raise ValueError('best: the key gives %d values for %d directions' % (len(v), len(self.directions)))
        return int(np.argmin(v))

    def rotation(self, k):
        """the 3 x 3 rotation that takes directions[k] to +z"""
        return rotation_to_z(self.directions[k])


def sin_limit_of(angle):
    """sin of the overhang angle in degrees (tests/overhang_ref.py::sin_limit_of)"""
    return math.sin(math.radians(float(angle)))


def normalise(directions):
    """(K, 3) unit directions, d / sqrt((dx*dx + dy*dy) + dz*dz) as tests/overhang_ref.py::normalise; ValueError for a zero or
    non-finite direction"""
    d = np.array(directions, dtype=np.float64)
    if d.ndim == 1:
        d = d.reshape(1, -1)
    if d.ndim != 2 or d.shape[1] != 3 or len(d) < 1:
        raise ValueError('directions must be one vector of 3 components or an array (K, 3) with K >= 1, got shape %r' % (d.shape,))
    if not np.isfinite(d).all():
        raise ValueError('a direction is not finite')
    with np.errstate(all='ignore'):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if not (np.isfinite(length).all() and (length > 0).all()):
        raise ValueError('a direction is zero (or its length is not a finite float64)')
    return d / length[:, None]


def sphere_directions(n):
    """(n + 6, 3) unit directions on the host: the six axis directions +x, -x, +y, -y, +z, -z, then n points of a Fibonacci spiral
    (tests/overhang_ref.py::sphere_directions)"""
    n = int(n)
    if n < 0:
        raise ValueError('sphere_directions: n must be >= 0, got %d' % n)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / max(n, 1)
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = (i + 0.5) * (math.pi * (3.0 - math.sqrt(5.0)))          # (half a turn of the golden angle in: no point on an axis)
    return normalise(np.concatenate([axes, np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)]))


def rotation_to_z(d):
    """the rotation R with R d = (0, 0, 1) for a unit d: the turn about d x z, written out so that no term is divided by less than 1
    (a d in the lower half-space is first taken to -z, then turned over about x)"""
    x, y, z = (float(v) for v in d)
    flip = z < 0
    if flip:
        x, y, z = -x, -y, -z
    q = 1.0 + z
    R = np.array([[1.0 - x * x / q, -x * y / q, -x],
                  [-x * y / q, 1.0 - y * y / q, -y],
                  [x, y, z]])
    if flip:                                            # R takes -d to +z, so d to -z; diag(1, -1, -1) takes -z to +z
        R[1:] = -R[1:]
    return R


def derive(r):
    """overhang_area = s0 / 2, support_volume = s1 / 6, contact_area = s2 / 2, height = hi - lo, each (K,), from the raw rating of
    `engine.Mesh.overhangs`, in the order of tests/overhang_ref.py::derive"""
    s = np.asarray(r['sums'], dtype=np.float64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        return {'overhang_area': s[:, 0] / 2.0, 'support_volume': s[:, 1] / 6.0, 'contact_area': s[:, 2] / 2.0,
                'height': np.asarray(r['hi'], dtype=np.float64) - np.asarray(r['lo'], dtype=np.float64)}


def check_params(directions, angle, bed_tolerance, classes):
    """(unit directions (K, 3), sin_limit, angle, bed_tolerance or None): ValueError for what cannot be rated, before any device work"""
    if isinstance(directions, (int, np.integer)) and not isinstance(directions, bool):
        d = sphere_directions(directions)
    else:
        d = normalise(directions)
    if len(d) > MAX_DIRECTIONS:
        raise ValueError('at most 2^20 directions in one call, got %d' % len(d))
    angle = float(angle)
    if not (0.0 <= angle < 90.0):
        raise ValueError('angle must lie in [0, 90) degrees, got %r' % angle)
    if bed_tolerance is not None:
        bed_tolerance = float(bed_tolerance)
        if not (bed_tolerance >= 0.0):
            raise ValueError('bed_tolerance must not be negative, got %r' % bed_tolerance)
    if classes and len(d) != 1:
        raise ValueError('classes=True needs exactly one direction, got %d' % len(d))
    return d, sin_limit_of(angle), angle, bed_tolerance


def _rated(mesh, d, sin_limit, angle, tol, classes, max_scratch_bytes=0):
    r = mesh.overhangs(d, sin_limit, tol, max_scratch_bytes)
    v = derive(r)
    cls = _frozen(mesh.overhang_classes(d[0], sin_limit, tol), np.uint8) if classes else None
    return Overhangs(
        directions=_frozen(d, np.float64), lo=_frozen(r['lo'], np.float64), hi=_frozen(r['hi'], np.float64), height=_frozen(v['height'], np.float64),
        overhang_area=_frozen(v['overhang_area'], np.float64), support_volume=_frozen(v['support_volume'], np.float64), contact_area=_frozen(v['contact_area'], np.float64),
        overhang_triangles=_frozen(r['overhang_triangles'], np.int64), contact_triangles=_frozen(r['contact_triangles'], np.int64),
        angle=angle, bed_tolerance=tol, sums=_frozen(r['sums'], np.float64), classes=cls)


def overhangs_of_mesh(mesh, directions=UP, angle=45.0, bed_tolerance=None, classes=False, max_scratch_bytes=0):
    """the Overhangs of a device mesh (`engine.Mesh`).  directions: one vector, an array (K, 3) (any length, normalised here) or an
    int n for `sphere_directions(n)`; bed_tolerance=None: 0.0"""
    d, sin_limit, angle, tol = check_params(directions, angle, bed_tolerance, classes)
    return _rated(mesh, d, sin_limit, angle, 0.0 if tol is None else tol, classes, max_scratch_bytes)


def overhangs_soup(soup, directions=UP, angle=45.0, bed_tolerance=None, classes=False):
    """the Overhangs of a float64 soup (T, 3, 3) on the host: uploaded (torch), adopted and rated on the device"""
    from . import core
    d, sin_limit, angle, tol = check_params(directions, angle, bed_tolerance, classes)       # (before the engine is asked for)
    with core.adopted(soup) as mesh:
        return _rated(mesh, d, sin_limit, angle, 0.0 if tol is None else tol, classes)


def overhangs(sdf, directions=UP, angle=45.0, bed_tolerance=None, classes=False, keep=None, simplify=None, mend=False,
              simplify_tolerance=None, simplify_levels=5, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and rate build
    directions there: an `Overhangs`.  directions: one vector, an array (K, 3) or an int n -- the six axis directions and n points
    of a Fibonacci spiral (`sphere_directions`); "up" is the build direction, the bed lies below the part.  angle: degrees in
    [0, 90), the steepest overhang from the vertical that prints without support -- a face is an overhang when n.d < -sin(angle).
    bed_tolerance: faces that look down and lie within it of the lowest point are bed contact, not overhang; None: the largest of
    the grid's three steps, so that the facets by which marching cubes rounds the bottom edges count as contact.  classes: True --
    also the class of every triangle (one direction only).  keep, simplify, simplify_tolerance, simplify_levels, mend: as for
    `measure`.  A multi-process run whose gathered soup is on the host raises NotImplementedError."""
    from . import core
    d, sin_limit, angle, tol = check_params(directions, angle, bed_tolerance, classes)       # (before anything is meshed)
    kw = core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend)
    with core.meshed(sdf, keep=keep, **kw) as m:
        core.need_device_mesh(m.mesh, 'overhangs', 'build directions are rated')
        if tol is None:
            tol = float(max(core.grid_steps(m, kw)))
        return _rated(m.mesh, d, sin_limit, angle, tol, classes)
