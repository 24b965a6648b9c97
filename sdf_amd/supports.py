"""How much support does a build direction really need?  (not in the reference.)  `overhangs` (section 4n)
rates hundreds of directions by a proxy: the prism from every overhanging face down to the bed plane.  `supports(f, directions)`
meshes a model, keeps the soup on the GPU and, per direction, sphere-traces a ray DOWNWARD from the centroid of every overhanging
face through the air until it meets the part or the bed (`engine.Mesh.support_rays`, sdf_mesh_support_rays, csrc/sdf_supports.hip):
the field's sign says where the part is and its magnitude is a safe step, so no ray-triangle test and no BVH is needed.  The volume
of the support columns is then split into what stands on the bed and what rests on the part itself, and the faces hidden inside a
union of solids (BURIED) drop out.  tests/supports_ref.py is the definition; `support_rays_host` restates it on the host for what
the kernel does not reach: a model with user closures, a soup that a multi-process run gathered on the host.

What it is not: one ray per face from its centroid -- first-order quadrature, a face that is partly over the part is all or nothing;
a gap narrower than `min_step` can be stepped over; the columns are vertical (no tree supports, no draft angle); with `angle` near 0
many near-vertical faces are BURIED, which is why `buried_area` is reported; a field that overestimates distance wants
step_scale < 1."""
import numpy as np

from .meshfile import frozen as _frozen
from .overhang import UP, normalise, overhangs_of_mesh, rotation_to_z, sin_limit_of, sphere_directions

BED, PART, BURIED, UNRESOLVED, NAN = 0, 1, 2, 3, 4
STATUS_NAMES = ('BED', 'PART', 'BURIED', 'UNRESOLVED', 'NAN')
_MARCH = 5
MAX_DIRECTIONS = 1024
N_SUMS = 5
_C, _LANES = 1024, 256


def check_params(directions, sin_limit, bed_tol, start, min_step, step_scale, max_steps, refine):
    """the refusals of sdf_mesh_support_rays, as ValueError: (unit directions (K, 3) AS GIVEN, [sin_limit, bed_tol, start, min_step,
    step_scale, max_steps, refine])"""
    d = np.ascontiguousarray(directions, dtype=np.float64)
    if d.ndim == 1:
        d = d.reshape(1, -1)
    if d.ndim != 2 or d.shape[1] != 3 or len(d) < 1:
        raise ValueError('support_rays: directions must have the shape (K, 3) with K >= 1, got %r' % (d.shape,))
    if len(d) > MAX_DIRECTIONS:
        raise ValueError('support_rays: at most 1024 directions in one call, got %d' % len(d))
    with np.errstate(all='ignore'):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if not (np.abs(length - 1.0) <= 1e-12).all():
            raise ValueError('support_rays: a direction is zero, not finite or not of unit length to 1e-12')
    p = [float(sin_limit), float(bed_tol), float(start), float(min_step), float(step_scale)]
    if not np.isfinite(p).all():
        raise ValueError('support_rays: the parameters are not finite: %r' % (p,))
    if not 0.0 <= p[0] < 1.0:
        raise ValueError('support_rays: sin_limit must lie in [0, 1), got %r' % p[0])
    if not p[1] >= 0.0:
        raise ValueError('support_rays: bed_tol must not be negative, got %r' % p[1])
    for name, v in zip(('start', 'min_step'), p[2:4]):
        if not v > 0:
            raise ValueError('support_rays: %s must be positive, got %r' % (name, v))
    if not 0 < p[4] <= 1:
        raise ValueError('support_rays: step_scale must lie in (0, 1], got %r' % p[4])
    if int(max_steps) < 1:
        raise ValueError('support_rays: max_steps must be at least 1, got %r' % (max_steps,))
    if int(refine) < 0:
        raise ValueError('support_rays: refine must not be negative, got %r' % (refine,))
    return d, p + [int(max_steps), int(refine)]


def _halve(x):
    """(groups, 256, cols) -> (groups, cols): x[:h] + x[h:] for h = 128 ... 1 (tests/measure_ref.py::_halve)"""
    h = x.shape[1] // 2
    while h >= 1:
        x = x[:, :h] + x[:, h:2 * h]
        h //= 2
    return x[:, 0]


def chunk_tree_sum(terms):
    """the fixed tree of tests/overhang_ref.py::chunk_tree_sum over terms (M, cols) in ray order: one sequential accumulator per
    chunk of 1024 from +0.0, the chunk partials in groups of 256 through the halving tree until one is left"""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    M, cols = terms.shape
    if M == 0:
        return np.zeros(cols)
    n_chunks = -(-M // _C)
    padded = np.zeros((n_chunks * _C, cols))
    padded[:M] = terms
    x = padded.reshape(n_chunks, _C, cols)
    part = np.zeros((n_chunks, cols))
    for s in range(_C):
        part = part + x[:, s]
    while True:
        n_groups = -(-len(part) // _LANES)
        padded = np.zeros((n_groups * _LANES, cols))
        padded[:len(part)] = part
        part = _halve(padded.reshape(n_groups, _LANES, cols))
        if len(part) == 1:
            return part[0]


def overhanging_faces(soup, d, sin_limit, bed_tol):
    """(triangle (M,) int32, lo, hi) of a soup (T, 3, 3) for ONE unit direction d: the faces of class OVERHANG of
    tests/overhang_ref.py::rate in triangle order, and the extremes of the finite triangles along d (none: +inf, -inf)"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    finite = np.isfinite(tri).all(axis=(1, 2))
    if not finite.any():
        return np.zeros(0, np.int32), np.inf, -np.inf
    with np.errstate(all='ignore'):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ux, uy, uz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
        wx, wy, wz = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
        nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        dbl = np.sqrt((nx * nx + ny * ny) + nz * nz)
        h = [(tri[:, v, 0] * d[0] + tri[:, v, 1] * d[1]) + tri[:, v, 2] * d[2] for v in range(3)]
        hf = np.concatenate([x[finite] for x in h])
        lo, hi = hf.min() + 0.0, hf.max() + 0.0
        top = np.maximum(np.maximum(h[0] - lo, h[1] - lo), h[2] - lo)
        dn = (nx * d[0] + ny * d[1]) + nz * d[2]
        over = finite & ~(top <= bed_tol) & (dn < -(sin_limit * dbl))
    return np.flatnonzero(over).astype(np.int32), float(lo), float(hi)


def support_rays_host(ev, soup, d, sin_limit, bed_tol, start, min_step, step_scale=1.0, max_steps=256, refine=16):
    """the definition on the host over an evaluator ev(P) -> (N,) float64 for ONE unit direction d (used as given): a dict of
    triangle (M,) int32, height (M,) float64, status (M,) uint8, steps (M,) int32, origin (M, 3) float64, sums (5,), counts (5,)
    int64, lo, hi.  float64, one rounding per operation.  The rays start at the centroids ((a + b) + c) / 3.0 of the overhanging
    faces and run along -d from t = start; tb = max(h(c) - lo, 0) is the distance to the bed.  start >= tb: BED, no evaluation.  Else
    v = ev(c + t (-d)): NaN: NAN; v < 0: hi = t -- BURIED on the first pass (height +0), PART later; else lo = t and t grows by
    max(v * step_scale, min_step), t >= tb: BED (height tb), as is UNRESOLVED after max_steps passes.  A PART bracket is bisected
    `refine` times; the height is hi.  The five terms are summed over the rays in their order through `chunk_tree_sum`."""
    d, (sin_limit, bed_tol, start, min_step, step_scale, max_steps, refine) = check_params(d, sin_limit, bed_tol, start, min_step, step_scale,
                                                                                           max_steps, refine)
    d = d[0]
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    idx, lo, hi = overhanging_faces(tri, d, sin_limit, bed_tol)
    M = len(idx)

    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), dtype=np.float64).reshape(-1)

    a, b, c = tri[idx, 0], tri[idx, 1], tri[idx, 2]
    ux, uy, uz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
    wx, wy, wz = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
    nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
    proj = -((nx * d[0] + ny * d[1]) + nz * d[2])
    origin = ((a + b) + c) / 3.0
    h = ((origin[:, 0] * d[0] + origin[:, 1] * d[1]) + origin[:, 2] * d[2]) - lo
    tb = np.where(h > 0.0, h, 0.0)
    nd = -d
    t, lo_t, hi_t = np.full(M, start), np.zeros(M), np.full(M, start)
    status = np.where(start >= tb, BED, _MARCH).astype(np.uint8)
    height = np.where(status == BED, tb, 0.0)
    steps = np.zeros(M, np.int32)
    for k in range(max_steps):
        m = np.flatnonzero(status == _MARCH)
        if len(m) == 0:
            break
        v = f(origin[m] + t[m, None] * nd)
        steps[m] += 1
        nan = np.isnan(v)
        inside = ~nan & (v < 0)
        status[m[nan]] = NAN
        height[m[nan]] = np.nan
        status[m[inside]] = BURIED if k == 0 else PART
        hi_t[m[inside]] = t[m[inside]]
        i = m[~nan & ~inside]
        lo_t[i] = t[i]
        adv = v[~nan & ~inside] * step_scale
        t[i] = t[i] + np.where(adv > min_step, adv, min_step)
        down = i[t[i] >= tb[i]]
        status[down] = BED
        height[down] = tb[down]
    left = status == _MARCH
    status[left] = UNRESOLVED
    height[left] = tb[left]
    r = np.flatnonzero(status == PART)
    for _ in range(refine if len(r) else 0):
        mid = 0.5 * (lo_t[r] + hi_t[r])
        neg = f(origin[r] + mid[:, None] * nd) < 0
        hi_t[r[neg]] = mid[neg]
        lo_t[r[~neg]] = mid[~neg]
    height[r] = hi_t[r]
    with np.errstate(invalid='ignore'):
        ph = proj * height
    zero = np.zeros(M)
    part = status == PART
    terms = np.stack([np.where((status == BED) | (status == UNRESOLVED), ph, zero), np.where(part, ph, zero), np.where(part, proj, zero),
                      proj, np.where(status == BURIED, proj, zero)], axis=1) if M else np.zeros((0, N_SUMS))
    return {'triangle': idx, 'height': height, 'status': status, 'steps': steps, 'origin': origin, 'sums': chunk_tree_sum(terms),
            'counts': np.bincount(status, minlength=5)[:5].astype(np.int64), 'lo': lo, 'hi': hi}


def derive(r):
    """on_bed_volume = s0 / 2, on_part_volume = s1 / 2, support_volume = (s0 + s1) / 2, touch_area = s2 / 2, projected_area = s3 / 2,
    buried_area = s4 / 2, height = hi - lo, each (K,), from the raw result of `engine.Mesh.support_rays`, in the order of
    tests/supports_ref.py::derive"""
    s = np.asarray(r['sums'], dtype=np.float64).reshape(-1, N_SUMS)
    with np.errstate(all='ignore'):
        return {'on_bed_volume': s[:, 0] / 2.0, 'on_part_volume': s[:, 1] / 2.0, 'support_volume': (s[:, 0] + s[:, 1]) / 2.0,
                'touch_area': s[:, 2] / 2.0, 'projected_area': s[:, 3] / 2.0, 'buried_area': s[:, 4] / 2.0,
                'height': np.asarray(r['hi'], dtype=np.float64) - np.asarray(r['lo'], dtype=np.float64)}


class Supports:
    """what `supports` returns (the arrays are read-only).  Per traced direction, each (K,): directions (K, 3) -- unit, "up" --,
    support_volume = on_bed_volume + on_part_volume (the columns that stand on the bed, and those that rest on the part itself),
    touch_area (the projected area where supports scar the part), projected_area (of all overhanging faces), buried_area (of the
    faces with material `start` below them: hidden inside a union, or near-vertical), height, lo, hi; counts (K, 5) int64 -- rays
    that ended BED, PART, BURIED, UNRESOLVED, NAN --, sums (K, 5): the raw totals.  angle (degrees), bed_tolerance, params: what the
    rays ran with.  proxy: the `Overhangs` of the directions that were rated first when `directions` was an int, else None, and
    traced: the indices of the traced directions in it."""

    def __init__(self, directions, raw, angle, bed_tolerance, params, proxy=None, traced=None):
        v = derive(raw)
        self.directions = _frozen(directions, np.float64)
        for k in ('support_volume', 'on_bed_volume', 'on_part_volume', 'touch_area', 'projected_area', 'buried_area', 'height'):
            setattr(self, k, _frozen(v[k], np.float64))
        self.lo, self.hi, self.sums = _frozen(raw['lo'], np.float64), _frozen(raw['hi'], np.float64), _frozen(raw['sums'], np.float64)
        self.counts = _frozen(raw['counts'], np.int64)
        self._rays = [tuple(_frozen(a, a.dtype) for a in ray) for ray in raw['rays']]
        self.angle, self.bed_tolerance, self.params = angle, bed_tolerance, dict(params)
        self.proxy = proxy
        self.traced = None if traced is None else _frozen(traced, np.int64)

    def rays(self, k):
        """(triangle (M,) int32, height (M,) float64, status (M,) uint8, steps (M,) int32, origin (M, 3) float64) of direction k"""
        return self._rays[k]

    def columns(self, k):
        """(M', 2, 3) float64: the support columns of direction k as segments from a face's centroid straight down, origin and
        origin + height * (-d); the rays whose height is NaN are dropped"""
        _, height, _, _, origin = self._rays[k]
        ok = ~np.isnan(height)
        o, hgt = origin[ok], height[ok]
        return np.stack([o, o + hgt[:, None] * (-self.directions[k])], axis=1) if len(o) else np.zeros((0, 2, 3))

    def best(self, key='support_volume'):
        """the index of the traced direction with the smallest `key`, the first one on ties.  key: a field name, or a callable that
        takes this record and returns (K,) values"""
        v = np.asarray(key(self) if callable(key) else getattr(self, key), dtype=np.float64).reshape(-1)
        if v.shape != (len(self.directions),):
            raise ValueError('best: the key gives %d values for %d directions' % (len(v), len(self.directions)))
        return int(np.argmin(v))

    def rotation(self, k):
        """the 3 x 3 rotation that takes directions[k] to +z"""
        return rotation_to_z(self.directions[k])

    def __repr__(self):
        k = self.best()
        return 'Supports(%d directions, best %d: volume %g, %g of it on the part)' % (len(self.directions), k, self.support_volume[k],
                                                                                   self.on_part_volume[k])


def check_call(directions, angle, bed_tolerance, start, min_step, step_scale, max_steps, refine, top):
    """what `supports` can refuse before anything is meshed: (unit directions (K, 3) or the int n, sin_limit, angle, bed_tolerance or
    None, top)"""
    n = None
    if isinstance(directions, (int, np.integer)) and not isinstance(directions, bool):
        n = int(directions)
        d = sphere_directions(n)                        # (refuses n < 0)
        top = int(top)
        if top < 1:
            raise ValueError('supports: top must be at least 1, got %r' % (top,))
    else:
        d = normalise(directions)
    angle = float(angle)
    if not (0.0 <= angle < 90.0):
        raise ValueError('angle must lie in [0, 90) degrees, got %r' % angle)
    if bed_tolerance is not None:
        bed_tolerance = float(bed_tolerance)
        if not (bed_tolerance >= 0.0):
            raise ValueError('bed_tolerance must not be negative, got %r' % bed_tolerance)
    check_params(d if n is None else d[:1], sin_limit_of(angle),
                 0.0 if bed_tolerance is None else bed_tolerance, 1.0 if start is None else start, 1.0 if min_step is None else min_step,
                 step_scale, max_steps, refine)
    return (d if n is None else n), sin_limit_of(angle), angle, bed_tolerance, top


def supports_of_mesh(mesh, sdf, directions, angle, bed_tolerance, start, min_step, step_scale=1.0, max_steps=256, refine=16, top=8):
    """the Supports of a device mesh (`engine.Mesh`) in the field `sdf`.  directions: one vector, an array (K, 3) (any length,
    normalised here), or an int n: the mesh is first rated by `overhangs_of_mesh` over `sphere_directions(n)` and the `top` directions
    with the smallest proxy volume are traced, ties by index"""
    d, sin_limit, angle, tol, top = check_call(directions, angle, bed_tolerance, start, min_step, step_scale, max_steps, refine, top)
    proxy = traced = None
    if isinstance(d, int):
        proxy = overhangs_of_mesh(mesh, d, angle, tol)
        traced = np.argsort(proxy.support_volume, kind='stable')[:top]
        d = proxy.directions[traced]
    params = dict(start=float(start), min_step=float(min_step), step_scale=float(step_scale), max_steps=int(max_steps), refine=int(refine))
    raw = mesh.support_rays(sdf, d, sin_limit, tol, **params)
    return Supports(d, raw, angle, tol, params, proxy, traced)


def supports_soup(soup, sdf, directions=UP, angle=45.0, bed_tolerance=0.0, start=None, min_step=None, step_scale=1.0, max_steps=256,
                  refine=16, top=8):
    """the Supports of a float64 soup (T, 3, 3) on the host in the field `sdf`: uploaded (torch), adopted and traced on the device"""
    from . import core
    check_call(directions, angle, bed_tolerance, start, min_step, step_scale, max_steps, refine, top)      # (before the engine is asked for)
    if start is None or min_step is None:
        raise ValueError('supports: give step, or start and min_step')
    with core.adopted(soup) as mesh:
        return supports_of_mesh(mesh, sdf, directions, angle, bed_tolerance, start, min_step, step_scale, max_steps, refine, top)


def supports(sdf, directions=UP, angle=45.0, bed_tolerance=None, start=None, min_step=None, step_scale=1.0, max_steps=256, refine=16,
             top=8, keep=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and trace the
    support rays of build directions there: a `Supports`.  directions: one vector or an array (K, 3) -- each is traced --, or an int
    n: the mesh is rated by `overhangs` over the six axis directions and n spiral points first, and the `top` directions with the
    smallest proxy volume are traced (`Supports.proxy` keeps the rating).  angle, bed_tolerance: as for `overhangs`
    (bed_tolerance=None: the largest grid step).  start: how far below the face's centroid a ray begins (a face with material that
    close is BURIED); min_step: the least advance of a step (a gap narrower than it can be stepped over); both default to a quarter
    of the smallest grid step.  step_scale in (0, 1]: shorten the steps for a field that overestimates distances.  keep, simplify,
    simplify_tolerance, simplify_levels, mend: as for `measure`.  A model with user closures, and a multi-process run whose gathered soup is on the host, take the same
    definition on the host over `Engine.eval_points`."""
    from . import core, engine
    d, sin_limit, angle, tol, top = check_call(directions, angle, bed_tolerance, start, min_step, step_scale, max_steps, refine, top)
    kw = core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend)
    with core.meshed(sdf, keep=keep, **kw) as m:
        steps3 = core.grid_steps(m, kw)
        if tol is None:
            tol = float(max(steps3))
        quarter = float(min(steps3)) / 4
        start = quarter if start is None else float(start)
        min_step = quarter if min_step is None else float(min_step)
        if m.mesh is not None:
            return supports_of_mesh(m.mesh, m.tape, directions, angle, tol, start, min_step, step_scale, max_steps, refine, top)
        if isinstance(d, int):
            raise NotImplementedError('supports: the soup of this multi-process run was gathered on the host; directions are rated on '
                                      'the device only -- give the directions to trace')
        params = dict(start=start, min_step=min_step, step_scale=float(step_scale), max_steps=int(max_steps), refine=int(refine))
        soup, ev = m.points.reshape(-1, 3, 3), engine.evaluator(m.engine, m.tape)
        got = [support_rays_host(ev, soup, d[i], sin_limit, tol, **params) for i in range(len(d))]
        raw = {'lo': [g['lo'] for g in got], 'hi': [g['hi'] for g in got], 'sums': np.array([g['sums'] for g in got]).reshape(-1, N_SUMS),
               'counts': np.array([g['counts'] for g in got]).reshape(-1, 5),
               'rays': [(g['triangle'], g['height'], g['status'], g['steps'], g['origin']) for g in got]}
        return Supports(d, raw, angle, tol, params)
