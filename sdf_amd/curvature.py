"""How tightly does the surface bend?  (not in the reference.)  `curvature(f)` meshes a model on the device and,
at every welded vertex, takes the mean, the Gaussian and the two principal curvatures of the FIELD's level set through the vertex
(`engine.Mesh.vertex_curvature`, sdf_mesh_vertex_curvature, csrc/sdf_curvature.hip): closed forms in the gradient and the Hessian of
the field, both from second differences of the interpreter's float64 values at step eps -- 19 evaluations per vertex.  The triangles
are not asked: marching cubes chamfers a crease and `simplify=` rounds it, the field still knows it.  tests/curvature_ref.py is the
definition; `vertex_curvature` restates it on the host for what the kernel does not reach: a model with user closures, a soup that a
multi-process run gathered on the host.

The field is negative inside, so convex is positive: `sphere(R)` has k1 = k2 = 1 / R, a cavity or an inside fillet is negative.

What it is not: eps is the scale it looks at.  The default is the smallest grid step of the meshing call -- curvature at the scale
the mesh can show -- so a vertex within eps of a crease reads about 1 / eps, and a feature smaller than eps is averaged over.  The
second differences lose about eps^2 / R^2 to truncation and about 1e-16 |f| / eps^2 to rounding; a field that is only a bound, not a
distance, still has the level set's curvature (the forms are invariant under a rescaling of the field).  A vertex of a simplified
mesh lies off the surface and reads the curvature of the level set it lies on: `snap=True` puts it back first."""
import numpy as np

from .meshfile import frozen as _frozen

CURVED, FLAT, NAN = 0, 1, 2
STATUS_NAMES = ('CURVED', 'FLAT', 'NAN')
FIELDS = ('mean', 'gauss', 'k1', 'k2')
QUALITIES = FIELDS + ('max',)
_PAIRS = ((0, 1), (0, 2), (1, 2))
_CORNERS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
_NAN_BITS = 0x7ff8000000000000


def check_params(eps):
    """the refusal of sdf_mesh_vertex_curvature, as ValueError: eps as a float"""
    eps = float(eps)
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError('vertex_curvature: eps must be finite and positive, got %r' % eps)
    return eps


def _stencil(P, k, eps):
    Q = P.copy()
    if 1 <= k <= 6:
        a = (k - 1) // 2
        Q[:, a] = P[:, a] + (eps if (k - 1) % 2 == 0 else -eps)
    elif k >= 7:
        a, b = _PAIRS[(k - 7) // 4]
        sa, sb = _CORNERS[(k - 7) % 4]
        Q[:, a] = P[:, a] + (eps if sa > 0 else -eps)
        Q[:, b] = P[:, b] + (eps if sb > 0 else -eps)
    return Q


def vertex_curvature(ev, points, eps):
    """the probe's definition on the host over an evaluator ev(P) -> (N,) float64: (curv (U, 4) float64 -- mean, gauss, k1, k2 --,
    status (U,) uint8).  float64, one rounding per operation.  19 values: v0 at the point; for axis a the values at x_a + eps and
    x_a + (-eps); for the pairs (x, y), (x, z), (y, z) the corners ++, +-, -+, --.  G_a = (va+ - va-) / (2 eps), H_aa = ((va+ - v0) +
    (va- - v0)) / (eps eps), H_ab = ((v++ - v+-) - (v-+ - v--)) / ((4 eps) eps); mean = (L2 tr - gHg) / ((2 L2) L), gauss = gAg /
    (L2 L2) over the cofactors A of H; k1, k2 = mean +- sqrt(max(mean mean - gauss, 0)).  NAN: a value or a result is not finite;
    FLAT: no gradient; both hold np.nan's bits in all four."""
    eps = np.float64(check_params(eps))
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    U = len(P)
    if U == 0:
        return np.zeros((0, 4)), np.zeros(0, np.uint8)

    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), dtype=np.float64).reshape(-1)

    with np.errstate(all='ignore'):
        v = [f(_stencil(P, k, eps)) for k in range(19)]
        v0 = v[0]
        two_eps, eps2, four_eps2 = 2 * eps, eps * eps, (4 * eps) * eps
        Gx, Gy, Gz = [(v[1 + 2 * a] - v[2 + 2 * a]) / two_eps for a in range(3)]
        Hxx, Hyy, Hzz = [((v[1 + 2 * a] - v0) + (v[2 + 2 * a] - v0)) / eps2 for a in range(3)]
        Hxy, Hxz, Hyz = [((v[7 + 4 * p] - v[8 + 4 * p]) - (v[9 + 4 * p] - v[10 + 4 * p])) / four_eps2 for p in range(3)]
        L2 = (Gx * Gx + Gy * Gy) + Gz * Gz
        L = np.sqrt(L2)
        tr = (Hxx + Hyy) + Hzz
        gHg = ((Gx * Gx * Hxx + Gy * Gy * Hyy) + Gz * Gz * Hzz) + 2 * ((Gx * Gy * Hxy + Gx * Gz * Hxz) + Gy * Gz * Hyz)
        mean = (L2 * tr - gHg) / ((2 * L2) * L)
        Axx = Hyy * Hzz - Hyz * Hyz
        Ayy = Hxx * Hzz - Hxz * Hxz
        Azz = Hxx * Hyy - Hxy * Hxy
        Axy = Hxz * Hyz - Hxy * Hzz
        Axz = Hxy * Hyz - Hxz * Hyy
        Ayz = Hxy * Hxz - Hxx * Hyz
        gAg = ((Gx * Gx * Axx + Gy * Gy * Ayy) + Gz * Gz * Azz) + 2 * ((Gx * Gy * Axy + Gx * Gz * Axz) + Gy * Gz * Ayz)
        gauss = gAg / (L2 * L2)
        disc = mean * mean - gauss
        s = np.sqrt(np.where(disc > 0, disc, 0.0))
        k1 = mean + s
        k2 = mean - s
    bad = np.zeros(U, bool)
    for k in range(19):
        bad |= ~np.isfinite(v[k])
    flat = (L2 == 0) | ~np.isfinite(L)
    broken = ~(np.isfinite(mean) & np.isfinite(gauss) & np.isfinite(k1) & np.isfinite(k2))
    status = np.where(bad, NAN, np.where(flat, FLAT, np.where(broken, NAN, CURVED))).astype(np.uint8)
    curv = np.ascontiguousarray(np.stack([mean, gauss, k1, k2], axis=1), dtype=np.float64)
    curv.view(np.uint64)[status != CURVED] = _NAN_BITS
    return curv, status


class Curvature:
    """what `curvature` returns.  points (U, 3) float64 and cells (T, 3) int64: the welded mesh; per vertex mean, gauss, k1 >= k2
    (U,) float64 (NaN where the status is not CURVED) and status (U,) uint8 (CURVED 0, FLAT 1: no gradient, NAN 2: the field or a
    result was not finite); params: the dict of eps the probe ran with."""

    def __init__(self, points, cells, curv, status, params):
        curv = np.asarray(curv, dtype=np.float64).reshape(-1, 4)
        self.points, self.cells = _frozen(points), _frozen(cells)
        self.mean, self.gauss, self.k1, self.k2 = (_frozen(curv[:, c]) for c in range(4))
        self.status = _frozen(status)
        self.params = dict(params)
        if not (len(self.points) == len(self.mean) == len(self.status)):
            raise ValueError('Curvature: %d points, %d curvatures, %d statuses' % (len(self.points), len(self.mean), len(self.status)))

    @property
    def measured(self):
        """the vertex mask of CURVED: where the four curvatures are numbers"""
        return self.status == CURVED

    @property
    def counts(self):
        return {name: int((self.status == code).sum()) for code, name in enumerate(STATUS_NAMES)}

    @property
    def max_abs(self):
        """max(|k1|, |k2|) per vertex, NaN where nothing was measured: 1 / the tightest radius of the surface there"""
        with np.errstate(invalid='ignore'):
            return np.where(self.measured, np.maximum(np.abs(self.k1), np.abs(self.k2)), np.nan)

    @property
    def min_convex_radius(self):
        """1 / the largest k1 over the vertices with k1 > 0 (the fillet check), inf when no vertex is convex"""
        with np.errstate(invalid='ignore'):
            k = self.k1[self.measured & (self.k1 > 0)]
        return float(1.0 / k.max()) if len(k) else float('inf')

    @property
    def min_concave_radius(self):
        """-1 / the smallest k2 over the vertices with k2 < 0 (the largest ball-end cutter that reaches every inside corner), inf
        when no vertex is concave"""
        with np.errstate(invalid='ignore'):
            k = self.k2[self.measured & (self.k2 < 0)]
        return float(-1.0 / k.min()) if len(k) else float('inf')

    @property
    def argsharpest(self):
        """the vertex of the largest max(|k1|, |k2|), or None when nothing was measured"""
        idx = np.flatnonzero(self.measured)
        return int(idx[np.argmax(self.max_abs[idx])]) if len(idx) else None

    @property
    def sharpest_point(self):
        i = self.argsharpest
        return self.points[i] if i is not None else None

    def tighter_than(self, r):
        """the vertex mask of CURVED vertices that bend tighter than the radius r either way: max(|k1|, |k2|) > 1 / r"""
        with np.errstate(invalid='ignore'):
            return self.measured & (self.max_abs > 1.0 / float(r))

    def percentile(self, q, of='k1'):
        """np.percentile of one of mean, gauss, k1, k2 over the CURVED vertices"""
        if of not in FIELDS:
            raise ValueError('percentile: of must be one of %s, got %r' % (', '.join(FIELDS), of))
        idx = self.measured
        return float(np.percentile(getattr(self, of)[idx], q)) if idx.any() else float('nan')

    def quality(self, which='mean'):
        """the scalar per vertex that a .ply file carries: one of mean, gauss, k1, k2, or 'max' -- of k1 and k2 the one of larger
        magnitude, with its sign"""
        return quality_of(np.stack([self.mean, self.gauss, self.k1, self.k2], axis=1), which)

    def save(self, path, which='mean'):
        """a binary PLY file of the mesh whose vertices carry `property float quality`: the float32 cast of `quality(which)`"""
        from . import meshfile
        if not str(path).lower().endswith('.ply'):
            raise ValueError('Curvature.save writes .ply, not %r' % (path,))
        vb, fb = meshfile.ply_records(self.points, self.cells, quality=self.quality(which))
        meshfile.write_ply(path, vb, fb, len(self.points), len(self.cells), False, quality=True)

    def __repr__(self):
        return 'Curvature(%d vertices, min convex radius %g, min concave radius %g, %s)' % (
            len(self.points), self.min_convex_radius, self.min_concave_radius, ', '.join('%s %d' % kv for kv in self.counts.items() if kv[1]))


def check_quality(which):
    if which not in QUALITIES:
        raise ValueError('curvature: the quality must be one of %s, got %r' % (', '.join(QUALITIES), which))
    return which


def quality_of(curv, which):
    """one column of curv (U, 4), or 'max': k1 where |k1| >= |k2|, else k2"""
    check_quality(which)
    curv = np.asarray(curv, dtype=np.float64).reshape(-1, 4)
    if which != 'max':
        return curv[:, FIELDS.index(which)].copy()
    with np.errstate(invalid='ignore'):
        return np.where(np.abs(curv[:, 2]) >= np.abs(curv[:, 3]), curv[:, 2], curv[:, 3])


def save_option(option):
    """`save(..., curvature=option)`: a quality name, or a dict of `quality` (default 'mean') and `eps` -- (name, eps or None),
    refused as ValueError before anything is meshed"""
    probe = dict(option) if isinstance(option, dict) else {'quality': 'mean' if option is True else option}
    unknown = set(probe) - {'quality', 'eps'}
    if unknown:
        raise ValueError('curvature: unknown probe arguments %s' % sorted(unknown))
    eps = probe.get('eps')
    return check_quality(probe.get('quality', 'mean')), None if eps is None else check_params(eps)


def default_eps(steps3, eps=None):
    """the default of `curvature`: the smallest of the three grid steps -- curvature at the scale the mesh can show"""
    if eps is not None:
        return check_params(eps)
    if steps3 is None:
        raise ValueError('curvature: give step, or eps')
    return check_params(min(float(s) for s in steps3))


def read_curvature(m, eps, with_mesh=True):
    """the probe on a `core.Meshed`: on the device, or -- a soup gathered on the host -- by the definition over eval_points.
    Returns (points, cells, curv, status); points and cells are None unless with_mesh."""
    from . import core, engine
    if m.mesh is None:
        pts, cells = core.read_weld(m)
        return (pts, cells) + vertex_curvature(engine.evaluator(m.engine, m.tape), pts, eps)
    curv, status, _ = m.mesh.vertex_curvature(m.tape, eps)
    pts, cells = m.mesh.weld() if with_mesh else (None, None)
    return pts, cells, curv, status


def curvature(sdf, step=None, eps=None, keep=None, simplify=None, mend=False, simplify_tolerance=None, simplify_levels=5, snap=False,
              **generate_kwargs):
    """mesh `sdf` on the device (the arguments of `generate`: step, bounds, samples, batch_size, sparse, verbose) and probe the
    curvature of the field at every welded vertex of the final mesh -- after keep, simplify, snap and mend -- there: a `Curvature`.
    eps: the step of the second differences, default the smallest of the three grid steps of this meshing call: curvature at the
    scale the mesh can show, so a vertex within eps of a crease reads about 1 / eps.  Give a smaller eps (1e-3 x the size of the
    part is safe in float64) for the curvature of the exact surface.  simplify_tolerance, simplify_levels, snap: as for `thickness`."""
    from . import core
    if step is not None:
        generate_kwargs['step'] = step
    kw = core.pipeline_kwargs(generate_kwargs, simplify, simplify_tolerance, simplify_levels, mend, snap)
    if eps is not None:
        check_params(eps)                                           # (what can be refused before meshing)
    with core.meshed(sdf, keep=keep, **kw) as m:
        eps = default_eps(core.grid_steps(m, kw), eps)
        pts, cells, curv, status = read_curvature(m, eps)
        return Curvature(pts, cells, curv, status, {'eps': eps})


def curvature_of_soup(soup, sdf, eps):
    """the Curvature of a float64 soup (T, 3, 3) on the host in the field `sdf`: uploaded (torch), adopted, welded and probed on the device"""
    from . import core
    eps = check_params(eps)
    with core.adopted(soup) as mesh:
        curv, status, _ = mesh.vertex_curvature(sdf, eps)
        pts, cells = mesh.weld()
        return Curvature(pts, cells, curv, status, {'eps': eps})
