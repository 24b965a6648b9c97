"""How far is a mesh from its model, and can its vertices be put back?  (not in the reference.)  `deviation(f)`
meshes a model on the device and samples the FIELD on every triangle of the final mesh -- after keep, simplify, snap and mend -- on a
barycentric lattice (`engine.Mesh.triangle_deviation`, sdf_mesh_triangle_deviation, csrc/sdf_deviation.hip): the library has the
field, so "how far off is this mesh" costs one interpreter evaluation per sample point and needs no second mesh.  `snap=` puts the
welded vertices back on the zero set by a few Newton steps on the same interpreter (`engine.Mesh.snap`, sdf_mesh_snap).
tests/deviation_ref.py is the definition; `triangle_deviation` and `vertex_snap` restate it on the host for what the kernels do not
reach: a model with user closures.

What it is not: it is one-sided, mesh to surface -- a part of the model that the mesh lost is not seen; |f| is a distance only where
the field is one -- `ellipsoid`, smooth unions and scaled models report a bound; snapping does not restore the creases that
clustering rounded, and it does not preserve topology (vertices that land on one point collapse their triangles; `mend` drops
those)."""
import numpy as np

from .meshfile import central_difference, frozen as _frozen

LEFT, SNAPPED, HELD, FLAT, NAN = 0, 1, 2, 3, 4
STATUS_NAMES = ('LEFT', 'SNAPPED', 'HELD', 'FLAT', 'NAN')
_ITER = 5
SNAP_KEYS = ('eps', 'tol', 'max_move', 'iters')


def check_order(order):
    """the order of the sample lattice, an integer from 1 to 8, as ValueError otherwise"""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= 8:
        raise ValueError('deviation: order must be an integer from 1 to 8, got %r' % (order,))
    return int(order)


def check_snap(eps, tol, max_move, iters):
    """the refusals of sdf_mesh_snap, as ValueError: (eps, tol, max_move, iters)"""
    p = [float(eps), float(tol), float(max_move)]
    if not np.isfinite(p).all():
        raise ValueError('snap: the parameters are not finite: %r' % (p,))
    if not p[0] > 0:
        raise ValueError('snap: eps must be positive, got %r' % p[0])
    if p[1] < 0:
        raise ValueError('snap: tol must not be negative, got %r' % p[1])
    if p[2] < 0:
        raise ValueError('snap: max_move must not be negative, got %r' % p[2])
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or int(iters) < 1:
        raise ValueError('snap: iters must be an integer of at least 1, got %r' % (iters,))
    return p + [int(iters)]


def check_snap_option(snap):
    """the `snap=` of the mesh pipeline: None for False / None (the call without it), else the dict of overrides (True: {}).  A dict
    may hold eps, tol, max_move, iters; whatever it holds is checked here, before anything is meshed"""
    if snap is None or snap is False:
        return None
    if snap is True:
        return {}
    if not isinstance(snap, dict):
        raise ValueError('snap: True, False or a dict of %s, got %r' % (', '.join(SNAP_KEYS), snap))
    unknown = set(snap) - set(SNAP_KEYS)
    if unknown:
        raise ValueError('snap: unknown arguments %s' % sorted(unknown))
    check_snap(snap.get('eps', 1.0), snap.get('tol', 0.0), snap.get('max_move', 0.0), snap.get('iters', 4))
    return dict(snap)


def snap_params(over, bounds, steps3, cluster=None):
    """the arguments of `engine.Mesh.snap` for a mesh on the grid steps3 within bounds: eps = the preview's normal_eps
    (`core.default_normal_eps`), tol = 1e-3 x the smallest grid step, max_move = the diagonal of one cluster cell (cluster x the
    grid step; one grid cell without simplify), iters = 4 -- each overridden by the dict `over`"""
    from . import core
    cell = np.asarray(steps3, dtype=np.float64) * (1.0 if cluster is None else float(cluster))
    par = {'eps': core.default_normal_eps(bounds), 'tol': 1e-3 * float(min(steps3)),
           'max_move': float(np.sqrt(np.dot(cell, cell))), 'iters': 4}
    par.update(over)
    eps, tol, max_move, iters = check_snap(par['eps'], par['tol'], par['max_move'], par['iters'])
    return {'eps': eps, 'tol': tol, 'max_move': max_move, 'iters': iters}


def lattice(order):
    """(S, 3) float64: the weights wa, wb, wc of the S = (n+1)(n+2)/2 samples, in the order for i in 0..n: for j in 0..n-i"""
    n = check_order(order)
    dn = np.float64(n)
    return np.array([[np.float64(n - i - j) / dn, np.float64(i) / dn, np.float64(j) / dn] for i in range(n + 1) for j in range(n + 1 - i)], np.float64)


def sample_points(soup, order):
    """(T, S, 3) float64: the sample points (A*wa + B*wb) + C*wc of a soup (T, 3, 3)"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    W = lattice(order)
    return (tri[:, None, 0, :] * W[None, :, 0, None] + tri[:, None, 1, :] * W[None, :, 1, None]) + tri[:, None, 2, :] * W[None, :, 2, None]


def triangle_deviation(ev, soup, order=2):
    """the deviation's definition on the host over an evaluator ev(P) -> (N,) float64: (dev (T,) float64, at (T,) int32, sumsq (T,)
    float64).  float64, one rounding per operation.  dev: the sampled value of largest magnitude -- a later sample replaces it only
    where |v| is strictly greater, the first NaN replaces it for good; at: that sample's index; sumsq: the sum of v*v in order."""
    Q = sample_points(soup, order)
    T, S = Q.shape[:2]
    dev, at, sumsq = np.zeros(T), np.zeros(T, np.int32), np.zeros(T)
    if T == 0:
        return dev, at, sumsq
    V = np.asarray(ev(np.ascontiguousarray(Q.reshape(-1, 3))), dtype=np.float64).reshape(T, S)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(S):
            v = V[:, s]
            take = np.ones(T, bool) if s == 0 else ~np.isnan(dev) & (np.isnan(v) | (np.abs(v) > np.abs(dev)))
            dev = np.where(take, v, dev)
            at[take] = s
            sumsq = sumsq + v * v
    return dev, at, sumsq


def vertex_snap(ev, points, eps, tol, max_move, iters=4):
    """the snap's definition on the host over an evaluator ev(P) -> (N,) float64: (q (U, 3) float64, status (U,) uint8, residual (U,)
    float64, evals (U,) int32).  Every vertex starts at q = P as ITER; per pass a vertex still ITER takes v = ev(q): NaN -> NAN, q
    back to P; |v| <= tol -> SNAPPED; else g = the central difference of `meshfile.vertex_normals` at q with step eps, len2 =
    (g0*g0 + g1*g1) + g2*g2, zero or NaN -> FLAT; else s = (v * (2 eps)) / len2, qn = q - s g, and |qn - P| > max_move -> HELD, else
    q = qn.  After the passes residual = ev(q) (NaN for NAN); a vertex still ITER is SNAPPED if |residual| <= tol, else LEFT."""
    eps, tol, max_move, iters = check_snap(eps, tol, max_move, iters)
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    U = len(P)

    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), dtype=np.float64).reshape(-1) if len(Q) else np.zeros(0)

    q = P.copy()
    status = np.full(U, _ITER, np.uint8)
    evals = np.zeros(U, np.int32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for _ in range(iters):
            m = np.flatnonzero(status == _ITER)
            if len(m) == 0:
                break
            v = f(q[m])
            evals[m] += 1
            nan = np.isnan(v)
            ok = ~nan & (np.abs(v) <= tol)
            status[m[nan]] = NAN
            q[m[nan]] = P[m[nan]]
            status[m[ok]] = SNAPPED
            m, v = m[~nan & ~ok], v[~nan & ~ok]
            if len(m) == 0:
                continue
            g = central_difference(f, q[m], eps)
            evals[m] += 6
            len2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            flat = (len2 == 0) | np.isnan(len2)
            s = (v * (2 * eps)) / len2
            qn = q[m] - s[:, None] * g
            d = qn - P[m]
            far = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > max_move
            status[m[flat]] = FLAT
            status[m[~flat & far]] = HELD
            q[m[~flat & ~far]] = qn[~flat & ~far]
        residual = f(q)
        residual[status == NAN] = np.nan
        it = status == _ITER
        evals[it] += 1
        status[it & (np.abs(residual) <= tol)] = SNAPPED
        status[status == _ITER] = LEFT
    return q, status, residual, evals


class Deviation:
    """what `deviation` returns.  points (U, 3) float64 and cells (T, 3) int64: the welded mesh; per triangle dev (T,) float64 (the
    sampled field value of largest magnitude; NaN where a sample was NaN), at (T,) int32 (the index of that sample on the lattice
    of `order`) and sumsq (T,) float64 (the sum of the squared samples); order: the lattice's; snap_stats: the statistics of
    `snap=`, or None."""

    def __init__(self, points, cells, dev, at, sumsq, order, snap_stats=None):
        self.points, self.cells = _frozen(points), _frozen(cells)
        self.dev, self.at, self.sumsq = _frozen(dev), _frozen(at), _frozen(sumsq)
        self.order = check_order(order)
        self.snap_stats = snap_stats
        if not (len(self.cells) == len(self.dev) == len(self.at) == len(self.sumsq)):
            raise ValueError('Deviation: %d cells, %d deviations, %d indices, %d sums' % (len(self.cells), len(self.dev), len(self.at), len(self.sumsq)))

    @property
    def finite(self):
        """the triangle mask of finite deviations"""
        return np.isfinite(self.dev)

    @property
    def argmax(self):
        """the triangle of the largest |dev| over the finite ones, or None when there is none"""
        idx = np.flatnonzero(self.finite)
        return int(idx[np.argmax(np.abs(self.dev[idx]))]) if len(idx) else None

    @property
    def max(self):
        """the largest |dev| over the finite triangles (NaN when there is none)"""
        i = self.argmax
        return float(abs(self.dev[i])) if i is not None else float('nan')

    @property
    def worst_point(self):
        """the sample point of the largest |dev|, recomputed from `at`"""
        i = self.argmax
        if i is None:
            return None
        return sample_points(self.points[self.cells[i]][None], self.order)[0, int(self.at[i])]

    @property
    def outside_max(self):
        """the largest positive dev (the mesh lies outside the model there), 0.0 when none is positive"""
        d = self.dev[self.finite]
        return float(d.max()) if len(d) and d.max() > 0 else 0.0

    @property
    def inside_max(self):
        """the most negative dev (the mesh lies inside the model there), 0.0 when none is negative"""
        d = self.dev[self.finite]
        return float(d.min()) if len(d) and d.min() < 0 else 0.0

    @property
    def rms(self):
        """the area-weighted root mean square of the samples: sqrt(sum(area * sumsq / S) / sum(area)) over the finite triangles"""
        k = self.finite & np.isfinite(self.sumsq)
        tri = self.points[self.cells[k]]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        area = 0.5 * np.sqrt((n * n).sum(axis=1))
        s = (self.order + 1) * (self.order + 2) // 2
        return float(np.sqrt((area * self.sumsq[k] / s).sum() / area.sum())) if area.sum() > 0 else float('nan')

    def percentile(self, q):
        """np.percentile of |dev| over the finite triangles"""
        k = self.finite
        return float(np.percentile(np.abs(self.dev[k]), q)) if k.any() else float('nan')

    def farther_than(self, x):
        """the triangle mask of finite deviations whose magnitude is above x"""
        with np.errstate(invalid='ignore'):
            return self.finite & (np.abs(self.dev) > x)

    @property
    def counts(self):
        return {'finite': int(self.finite.sum()), 'nan': int(np.isnan(self.dev).sum())}

    def __repr__(self):
        return 'Deviation(%d triangles, order %d, max %g, rms %g)' % (len(self.cells), self.order, self.max, self.rms)


def read_deviation(m, order):
    """the deviation of a `core.Meshed`: on the device, or -- a soup gathered on the host -- by the definition over eval_points.
    Returns (points, cells, dev, at, sumsq)."""
    from . import core, engine
    pts, cells = core.read_weld(m)
    if m.mesh is None:
        return (pts, cells) + triangle_deviation(engine.evaluator(m.engine, m.tape), np.asarray(m.points).reshape(-1, 3, 3), order)
    return (pts, cells) + m.mesh.triangle_deviation(m.tape, order)


def deviation(sdf, order=2, keep=None, simplify=None, simplify_tolerance=None, simplify_levels=5, snap=False, mend=False, **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and sample the field
    on every triangle of the final mesh -- after keep, simplify, snap and mend -- there: a `Deviation`.  order: the lattice has
    (order+1)(order+2)/2 sample points per triangle, the corners among them (1 .. 8).  snap: True, or a dict of eps, tol, max_move,
    iters -- the welded vertices are put back on the zero set first (`core.meshed`)."""
    from . import core
    order = check_order(order)
    with core.meshed(sdf, keep=keep, **core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap)) as m:
        pts, cells, dev, at, sumsq = read_deviation(m, order)
        return Deviation(pts, cells, dev, at, sumsq, order, getattr(m.mesh, 'snap_stats', None))


def deviation_of_soup(soup, sdf, order=2):
    """the Deviation of a float64 soup (T, 3, 3) on the host in the field `sdf`: uploaded (torch), adopted and sampled on the device"""
    from . import core
    order = check_order(order)
    with core.adopted(soup) as mesh:
        dev, at, sumsq = mesh.triangle_deviation(sdf, order)
        pts, cells = mesh.weld()
        return Deviation(pts, cells, dev, at, sumsq, order)


def snap_of_soup(soup, sdf, eps, tol, max_move, iters=4):
    """a float64 soup (T, 3, 3) on the host with its welded vertices snapped onto the zero set of `sdf` on the device: (points (U, 3),
    cells (T, 3), status (U,), residual (U,), statistics) -- the points are the moved ones, in the weld order of the source"""
    from . import core
    with core.adopted(soup) as mesh:
        cells = mesh.weld()[1]
        moved = mesh.snap(sdf, eps, tol, max_move, iters)
        try:
            q, status, residual = moved.snap_result
            return q, cells, status, residual, moved.snap_stats
        finally:
            moved.close()
