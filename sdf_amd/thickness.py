"""How thick is a wall?  (not in the reference.)  `thickness(f)` meshes a model on the device and, from every
welded vertex, sphere-traces a ray INWARD -- along the negated field normal -- through the solid until the field turns positive
again (`engine.Mesh.vertex_thickness`, sdf_mesh_vertex_thickness, csrc/sdf_thickness.hip).  The field's sign says where the solid
ends and its magnitude is a safe step, so the probe needs no triangle intersection tests.  The length of the ray is the wall's ray
thickness at the vertex.  tests/thickness_ref.py is the definition; `vertex_thickness` restates it on the host for what the kernel
does not reach: a model with user closures, a soup that a multi-process run gathered on the host.

What it is not: it measures along the field normal, not the largest inscribed sphere; an outside gap narrower than `min_step` can
be stepped over; the vertices of a simplified mesh lie off the surface, so measure before `simplify=`, raise `start` or put them back
with `snap=True`; a field
that is only a bound, not a distance, costs steps and not correctness."""
import numpy as np

from .meshfile import central_difference, frozen as _frozen

OPEN, THICK, THIN, FLAT, NAN = 0, 1, 2, 3, 4
STATUS_NAMES = ('OPEN', 'THICK', 'THIN', 'FLAT', 'NAN')
_MARCH = 5


def check_params(normal_eps, start, min_step, t_far, step_scale, max_steps, refine):
    """the refusals of sdf_mesh_vertex_thickness, as ValueError: (normal_eps, start, min_step, t_far, step_scale, max_steps, refine)"""
    p = [float(normal_eps), float(start), float(min_step), float(t_far), float(step_scale)]
    if not np.isfinite(p).all():
        raise ValueError('vertex_thickness: the parameters are not finite: %r' % (p,))
    for name, v in zip(('normal_eps', 'start', 'min_step'), p):
        if not v > 0:
            raise ValueError('vertex_thickness: %s must be positive, got %r' % (name, v))
    if not 0 < p[4] <= 1:
        raise ValueError('vertex_thickness: step_scale must lie in (0, 1], got %r' % p[4])
    if p[3] < p[1]:
        raise ValueError('vertex_thickness: t_far %r lies before start %r' % (p[3], p[1]))
    if int(max_steps) < 1:
        raise ValueError('vertex_thickness: max_steps must be at least 1, got %r' % (max_steps,))
    if int(refine) < 0:
        raise ValueError('vertex_thickness: refine must not be negative, got %r' % (refine,))
    return p + [int(max_steps), int(refine)]


def vertex_thickness(ev, points, normal_eps, start, min_step, t_far, step_scale=1.0, max_steps=256, refine=16):
    """the probe's definition on the host over an evaluator ev(P) -> (N,) float64: (thickness (U,) float64, status (U,) uint8, steps
    (U,) int32).  float64, one rounding per operation.  The direction is d = -(g / len) with g the central difference of
    `meshfile.vertex_normals` at step normal_eps; len 0 or NaN: FLAT, thickness NaN.  The march starts at t = start with the bracket
    (0, start): v = ev(p + t d); NaN: NAN; v >= 0: the ray is outside again, hi = t -- THIN on the first pass (the thickness is
    `start`, an upper bound), THICK later; else lo = t and t grows by max((-v) * step_scale, min_step), beyond t_far: OPEN (+inf), as
    after max_steps passes.  A THICK bracket is bisected `refine` times; the thickness is hi."""
    normal_eps, start, min_step, t_far, step_scale, max_steps, refine = check_params(normal_eps, start, min_step, t_far, step_scale, max_steps, refine)
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    U = len(P)
    if U == 0:
        return np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.int32)

    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), dtype=np.float64).reshape(-1)

    g = central_difference(f, P, normal_eps)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        flat = (ln == 0) | np.isnan(ln)
        D = -(g / ln[:, None])
    D[flat] = 0.0
    t, lo, hi = np.full(U, start), np.zeros(U), np.full(U, start)
    status = np.where(flat, FLAT, _MARCH).astype(np.uint8)
    steps = np.zeros(U, np.int32)
    for k in range(max_steps):
        m = np.flatnonzero(status == _MARCH)
        if len(m) == 0:
            break
        v = f(P[m] + t[m, None] * D[m])
        steps[m] += 1
        nan = np.isnan(v)
        left = ~nan & (v >= 0)
        status[m[nan]] = NAN
        status[m[left]] = THIN if k == 0 else THICK
        hi[m[left]] = t[m[left]]
        inside = ~nan & ~left
        i = m[inside]
        lo[i] = t[i]
        adv = (-v[inside]) * step_scale
        t[i] = t[i] + np.where(adv > min_step, adv, min_step)
        status[i[t[i] > t_far]] = OPEN
    status[status == _MARCH] = OPEN
    r = np.flatnonzero(status == THICK)
    for _ in range(refine if len(r) else 0):
        mid = 0.5 * (lo[r] + hi[r])
        neg = f(P[r] + mid[:, None] * D[r]) < 0
        lo[r[neg]] = mid[neg]
        hi[r[~neg]] = mid[~neg]
    th = np.where((status == THICK) | (status == THIN), hi, np.where(status == OPEN, np.inf, np.nan))
    return th, status, steps


class Thickness:
    """what `thickness` returns.  points (U, 3) float64 and cells (T, 3) int64: the welded mesh; per vertex thickness (U,) float64
    (+inf where OPEN, NaN where FLAT or NAN, `start` where THIN), status (U,) uint8 (OPEN 0, THICK 1, THIN 2, FLAT 3, NAN 4) and
    steps (U,) int32 (evaluations of the march); params: the dict of normal_eps, start, min_step, t_far, step_scale, max_steps, refine
    the probe ran with."""

    def __init__(self, points, cells, thickness, status, steps, params):
        self.points, self.cells = _frozen(points), _frozen(cells)
        self.thickness, self.status, self.steps = _frozen(thickness), _frozen(status), _frozen(steps)
        self.params = dict(params)
        if not (len(self.points) == len(self.thickness) == len(self.status) == len(self.steps)):
            raise ValueError('Thickness: %d points, %d thicknesses, %d statuses, %d step counts'
                             % (len(self.points), len(self.thickness), len(self.status), len(self.steps)))

    @property
    def measured(self):
        """the vertex mask of THICK and THIN: where a thickness (or, for THIN, an upper bound of it) was found"""
        return (self.status == THICK) | (self.status == THIN)

    @property
    def argmin(self):
        """the vertex of the smallest thickness over THICK and THIN, or None when there is none"""
        idx = np.flatnonzero(self.measured)
        return int(idx[np.argmin(self.thickness[idx])]) if len(idx) else None

    @property
    def min(self):
        """the smallest thickness over THICK and THIN (NaN when there is none)"""
        i = self.argmin
        return float(self.thickness[i]) if i is not None else float('nan')

    @property
    def thinnest_point(self):
        i = self.argmin
        return self.points[i] if i is not None else None

    def percentile(self, q):
        """np.percentile of the thickness over THICK and THIN"""
        idx = self.measured
        return float(np.percentile(self.thickness[idx], q)) if idx.any() else float('nan')

    def thinner_than(self, x):
        """the vertex mask of THICK and THIN vertices whose thickness is below x"""
        with np.errstate(invalid='ignore'):
            return self.measured & (self.thickness < x)

    @property
    def counts(self):
        return {name: int((self.status == code).sum()) for code, name in enumerate(STATUS_NAMES)}

    def save(self, path):
        """a binary PLY file of the mesh whose vertices carry `property float quality` (MeshLab's name for a scalar per vertex):
        the float32 cast of the thickness, inf and nan as they are"""
        from . import meshfile
        if not str(path).lower().endswith('.ply'):
            raise ValueError('Thickness.save writes .ply, not %r' % (path,))
        vb, fb = meshfile.ply_records(self.points, self.cells, quality=self.thickness)
        meshfile.write_ply(path, vb, fb, len(self.points), len(self.cells), False, quality=True)

    def __repr__(self):
        return 'Thickness(%d vertices, min %g, %s)' % (len(self.points), self.min, ', '.join('%s %d' % kv for kv in self.counts.items() if kv[1]))


def default_params(bounds, steps3, start=None, min_step=None, t_far=None, normal_eps=None):
    """the defaults of `thickness`: start = min_step = a quarter of the smallest grid step, t_far = the diagonal of the bounds,
    normal_eps = the preview's value (`core.default_normal_eps`)"""
    from . import core
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    diagonal = float(np.sqrt(np.dot(hi - lo, hi - lo)))
    quarter = float(min(steps3)) / 4 if steps3 is not None else None
    if quarter is None and (start is None or min_step is None):
        raise ValueError('thickness: give step, or start and min_step')
    return {'normal_eps': core.default_normal_eps(bounds) if normal_eps is None else float(normal_eps),
            'start': quarter if start is None else float(start), 'min_step': quarter if min_step is None else float(min_step),
            't_far': diagonal if t_far is None else float(t_far)}


def read_thickness(m, params, with_mesh=True):
    """the probe on a `core.Meshed`: on the device, or -- a soup gathered on the host -- by the definition over eval_points.
    Returns (points, cells, thickness, status, steps); points and cells are None unless with_mesh."""
    from . import core, engine
    if m.mesh is None:
        pts, cells = core.read_weld(m)
        return (pts, cells) + vertex_thickness(engine.evaluator(m.engine, m.tape), pts, **params)
    got = m.mesh.vertex_thickness(m.tape, **params)
    pts, cells = m.mesh.weld() if with_mesh else (None, None)
    return (pts, cells) + got


def thickness(sdf, start=None, min_step=None, t_far=None, max_steps=256, refine=16, normal_eps=None, step_scale=1.0,
              keep=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, snap=False, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and probe the wall
    thickness at every welded vertex of the final mesh -- after keep, simplify and mend -- there: a `Thickness`.  start: how far
    inside the vertex the ray begins (a wall thinner than that is THIN); min_step: the least advance of a step (it lets a ray leave
    the surface it starts on; a gap narrower than it can be stepped over); both default to a quarter of the smallest grid step.
    t_far: where a ray gives up (OPEN), default the diagonal of the bounds.  normal_eps: the step of the central difference that
    gives the direction, default the preview's.  step_scale in (0, 1]: shorten the steps for a field that overestimates distances.
    simplify_tolerance, simplify_levels: the final mesh is the one simplified to that tolerance.  snap: True or
    a dict -- the vertices of the final mesh are put back on the zero set first (`sdf_amd/deviation.py`), so a
    simplified mesh can be probed with the default `start`."""
    from . import core
    kw = core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap)
    check_params(1.0 if normal_eps is None else normal_eps, 1.0 if start is None else start, 1.0 if min_step is None else min_step,
                 np.finfo(np.float64).max if t_far is None else t_far, step_scale, max_steps, refine)      # (what can be refused before meshing)
    with core.meshed(sdf, keep=keep, **kw) as m:
        params = dict(default_params(m.bounds, core.grid_steps(m, kw), start, min_step, t_far, normal_eps), step_scale=float(step_scale),
                      max_steps=int(max_steps), refine=int(refine))
        pts, cells, th, status, steps = read_thickness(m, params)
        return Thickness(pts, cells, th, status, steps, params)


def thickness_of_soup(soup, sdf, normal_eps, start, min_step, t_far, step_scale=1.0, max_steps=256, refine=16):
    """the Thickness of a float64 soup (T, 3, 3) on the host in the field `sdf`: uploaded (torch), adopted, welded and probed on the device"""
    from . import core
    params = dict(normal_eps=float(normal_eps), start=float(start), min_step=float(min_step), t_far=float(t_far),
                  step_scale=float(step_scale), max_steps=int(max_steps), refine=int(refine))
    with core.adopted(soup) as mesh:
        th, status, steps = mesh.vertex_thickness(sdf, **params)
        pts, cells = mesh.weld()
        return Thickness(pts, cells, th, status, steps, params)
