"""The contours of a 2-D model, and the slices of a 3-D one (not in the reference, whose 2-D models can only be
sampled or extruded): closed, oriented polylines -- outer boundaries counter-clockwise with positive area, holes clockwise with
negative area -- linked and ordered on the device (csrc/sdf_contour.hip), and written as SVG for a laser or a plotter and as DXF
for a CAM program.  tests/contour_ref.py is the definition; the device reproduces it bit for bit.

    f = rounded_x(1, 0.2)
    c = f.contours(step=0.01)                 # a Contours object
    f.save('x.svg', step=0.01)                # or 'x.dxf'
    layers = g.slices(np.arange(0.1, 2, 0.2), samples=2 ** 20)     # a 3-D model cut at those heights
    for points, closed, area in layers.loops(layer=3): ...

The grid: the axes are np.arange(lo, hi, step), extended by one sample past `hi` when the last sample falls short of it, so that a
model that fits its bounds yields closed loops.  `step` is a number or (dx, dy); without it, step = sqrt(area of the bounds /
samples).  `bounds` is ((x0, y0), (x1, y1)) (a 3-D model also takes its 3-D bounds, of which x and y are used); without them a 2-D
model is probed by the reference's shrinking 16-per-axis grid, on two axes, and a 3-D model by its own estimate.

Models of the library's own nodes are sampled on the device, in float64, and contoured there (sdf_contour_host).  A model with user
closures and an engine set to float32 are sampled through Engine.eval_points and contoured from those samples
(sdf_contour_grid_host).

The writers are plain text and need no other package.  Every number is written as '%.17g', which reads back to the same float64."""
import ctypes

import numpy as np


class Contours:
    """points (N, 2) float64; offsets (L + 1) int64: contour i is points[offsets[i]:offsets[i + 1]]; closed (L) bool; layer (L) int32;
    area (L) float64, signed, 0 for an open chain; z: the heights of the layers (None for a 2-D model); counts: n_points, n_contours,
    n_segments, nonfinite_cells, rounds; bounds: ((x0, y0), (x1, y1)) of the grid; X, Y: its axes"""

    def __init__(self, points, offsets, closed, layer, area, z, counts, X, Y):
        self.points, self.offsets, self.closed, self.layer, self.area = points, offsets, closed, layer, area
        self.z, self.counts, self.X, self.Y = z, counts, X, Y
        self.bounds = ((float(X[0]), float(Y[0])), (float(X[-1]), float(Y[-1])))

    def __len__(self):
        return len(self.closed)

    @property
    def n_layers(self):
        return 1 if self.z is None else len(self.z)

    def loops(self, layer=None):
        """(points view (n, 2), closed, area) of every contour, or of those of one layer, in order"""
        for i in range(len(self.closed)):
            if layer is None or self.layer[i] == layer:
                yield self.points[self.offsets[i]:self.offsets[i + 1]], bool(self.closed[i]), float(self.area[i])

    def save(self, path):
        """.svg or .dxf, by the extension"""
        ext = str(path).rsplit('.', 1)[-1].lower()
        if ext == 'svg':
            text = svg_text(self)
        elif ext == 'dxf':
            text = dxf_text(self)
        else:
            raise ValueError('contours are saved as .svg or .dxf, got %r' % (path,))
        with open(path, 'w', newline='\n') as fp:
            fp.write(text)


def _num(v):
    return '%.17g' % float(v)


def svg_text(c):
    """one <path> per layer, fill-rule evenodd, M / L / Z per closed contour and no Z for an open one; the viewBox is the bounds; y is
    flipped by the group's transform, so the file holds the model's own coordinates and up is up"""
    (x0, y0), (x1, y1) = c.bounds
    out = ['<?xml version="1.0" encoding="UTF-8"?>\n',
           '<svg xmlns="http://www.w3.org/2000/svg" viewBox="%s %s %s %s">\n' % (_num(x0), _num(-y1), _num(x1 - x0), _num(y1 - y0)),
           '<g transform="scale(1,-1)" fill="black" stroke="none" fill-rule="evenodd">\n']
    for k in range(c.n_layers):
        d = []
        for pts, closed, _ in c.loops(k):
            d.append(' '.join(('M' if i == 0 else 'L') + _num(p[0]) + ',' + _num(p[1]) for i, p in enumerate(pts.tolist()))
                     + (' Z' if closed else ''))
        z = '' if c.z is None else ' data-z="%s"' % _num(c.z[k])
        out.append('<path id="L%d"%s fill-rule="evenodd" d="%s"/>\n' % (k, z, ' '.join(d)))
    out.append('</g>\n</svg>\n')
    return ''.join(out)


def dxf_text(c):
    """ASCII DXF R12: one POLYLINE / VERTEX ... / SEQEND entity per contour, flag 70 = 1 for a closed one, on layer L<k>, at the
    elevation of the layer's z"""
    out = ['0\nSECTION\n2\nHEADER\n9\n$ACADVER\n1\nAC1009\n0\nENDSEC\n0\nSECTION\n2\nENTITIES\n']
    for i in range(len(c)):
        k = int(c.layer[i])
        z = _num(0.0 if c.z is None else c.z[k])
        out.append('0\nPOLYLINE\n8\nL%d\n66\n1\n10\n0\n20\n0\n30\n%s\n70\n%d\n' % (k, z, 1 if c.closed[i] else 0))
        for p in c.points[c.offsets[i]:c.offsets[i + 1]].tolist():
            out.append('0\nVERTEX\n8\nL%d\n10\n%s\n20\n%s\n30\n%s\n' % (k, _num(p[0]), _num(p[1]), z))
        out.append('0\nSEQEND\n8\nL%d\n' % k)
    out.append('0\nENDSEC\n0\nEOF\n')
    return ''.join(out)


def axis(lo, hi, step):
    """np.arange(lo, hi, step), extended by one sample when the last one falls short of hi"""
    a = np.arange(lo, hi, step)
    if len(a) == 0 or a[-1] < hi:
        a = np.append(a, lo + len(a) * step)
    return np.ascontiguousarray(a, dtype=np.float64)


def estimate_bounds_2d(sdf, eng):
    """the reference's shrink loop (reference sdf/core.py:62-82) on two axes: up to 32 rounds of a 16 x 16 probe grid from +-1e9,
    evaluated by Engine.eval_points"""
    s = 16
    x0 = y0 = -1e9
    x1 = y1 = 1e9
    prev = None
    for _ in range(32):
        X = np.linspace(x0, x1, s)
        Y = np.linspace(y0, y1, s)
        d = np.array([X[1] - X[0], Y[1] - Y[0]])
        threshold = np.linalg.norm(d) / 2
        if threshold == prev:
            break
        prev = threshold
        P = np.stack(np.meshgrid(X, Y, indexing='ij'), axis=-1).reshape(-1, 2)
        values = eng.eval_points(sdf, P).reshape(s, s)
        where = np.argwhere(np.abs(values) <= threshold)
        x1, y1 = (x0, y0) + where.max(axis=0) * d + d / 2
        x0, y0 = (x0, y0) + where.min(axis=0) * d - d / 2
    return ((x0, y0), (x1, y1))


def contour_grid(values, X, Y, level=0.0, z=None, eng=None):
    """the contours of samples V[nw, nx, ny] (or [nx, ny]) on the device: sdf_contour_grid_host"""
    from . import engine
    eng = eng or engine.get_engine()
    V = np.ascontiguousarray(values, dtype=np.float64)
    if V.ndim == 2:
        V = V[None]
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if V.ndim != 3 or X.ndim != 1 or Y.ndim != 1 or V.shape[1:] != (len(X), len(Y)):
        raise ValueError('samples (nw, nx, ny) with axes X (nx), Y (ny) expected, got %r, %r, %r' % (V.shape, X.shape, Y.shape))
    lib = eng.lib
    h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
    f64p = engine._f64p
    engine._check(lib, lib.sdf_contour_grid_host(eng.ctx, V.ctypes.data_as(f64p), V.shape[0], len(X), len(Y), X.ctypes.data_as(f64p),
                                                 Y.ctypes.data_as(f64p), float(level), ctypes.byref(h), ctypes.byref(cnt)))
    return _fetch(eng, h, cnt, z, X, Y)


def contour_tape(sdf, X, Y, W=None, level=0.0, eng=None, return_values=False):
    """the contours of a model sampled on the device over X x Y (a 2-D model) or over X x Y at every height of W (a 3-D one):
    sdf_contour_host.  With return_values, (Contours, the samples (nw, nx, ny))"""
    from . import engine
    eng = eng or engine.get_engine()
    dt = eng.tape_for(sdf)
    dim = 2 if W is None else 3
    if dt.tape.dim != dim:
        raise ValueError('a %d-D model cannot be contoured as a %d-D one' % (dt.tape.dim, dim))
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Wa = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
    if X.ndim != 1 or Y.ndim != 1 or (Wa is not None and Wa.ndim != 1):
        raise ValueError('one-dimensional axes expected')
    nw = 1 if Wa is None else len(Wa)
    lib = eng.lib
    f64p = engine._f64p
    values = np.empty((nw, len(X), len(Y)), np.float64) if return_values else None
    h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
    engine._check(lib, lib.sdf_contour_host(dt.handle, dim, X.ctypes.data_as(f64p), len(X), Y.ctypes.data_as(f64p), len(Y),
                                            None if Wa is None else Wa.ctypes.data_as(f64p), nw, float(level),
                                            None if values is None else values.ctypes.data_as(f64p), ctypes.byref(h), ctypes.byref(cnt)))
    c = _fetch(eng, h, cnt, Wa, X, Y)
    return (c, values) if return_values else c


def _fetch(eng, h, cnt, z, X, Y):
    from . import engine
    lib = eng.lib
    try:
        n, m = int(cnt.n_points), int(cnt.n_contours)
        points = np.empty((n, 2), np.float64)
        offsets = np.zeros(m + 1, np.int64)
        closed = np.empty(m, np.uint8)
        layer = np.empty(m, np.int32)
        area = np.empty(m, np.float64)
        engine._check(lib, lib.sdf_contours_fetch(h, points.ctypes.data_as(engine._f64p), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                  closed.ctypes.data_as(engine._u8p), layer.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  area.ctypes.data_as(engine._f64p)))
    finally:
        lib.sdf_contours_destroy(h)
    counts = {k: int(getattr(cnt, k)) for k in engine.CONTOUR_COUNTS}
    return Contours(points, offsets, closed.astype(bool), layer, area, None if z is None else np.array(z, np.float64), counts, X, Y)


def _steps(step):
    try:
        dx, dy = step
    except TypeError:
        dx = dy = step
    dx, dy = float(dx), float(dy)
    if not (np.isfinite(dx) and np.isfinite(dy) and dx > 0 and dy > 0):
        raise ValueError('step must be positive and finite, got %r' % (step,))
    return dx, dy


def contours(f, step=None, bounds=None, samples=2 ** 20, level=0.0, z=None):
    """the contours of the 2-D model f at `level`, or -- z given: a height or a sequence of heights -- the slices of the 3-D model f"""
    from . import core, engine
    from .d2 import SDF2
    from .d3 import SDF3
    if not isinstance(f, (SDF2, SDF3)):
        raise ValueError('contours: a 2-D or a 3-D model expected, got %r' % (type(f),))
    three = isinstance(f, SDF3)
    if three and z is None:
        raise ValueError('contours: a 3-D model is cut at heights: give z (SDF3.slices)')
    if not three and z is not None:
        raise ValueError('contours: a 2-D model has no heights: z must be None')
    level = float(level)
    if not np.isfinite(level):
        raise ValueError('contours: the level must be finite, got %r' % (level,))
    W = None
    if three:
        W = np.atleast_1d(np.asarray(z, dtype=np.float64))
        if W.ndim != 1 or len(W) < 1 or not np.all(np.isfinite(W)):
            raise ValueError('contours: z must be a finite height or a sequence of them, got %r' % (z,))
    eng = engine.get_engine()
    if bounds is None:
        bounds = core._estimate_bounds(f) if three else estimate_bounds_2d(f, eng)
    (x0, y0), (x1, y1) = (tuple(bounds[0])[:2], tuple(bounds[1])[:2])
    x0, y0, x1, y1 = float(x0), float(y0), float(x1), float(y1)
    if not (np.isfinite([x0, y0, x1, y1]).all() and x1 > x0 and y1 > y0):
        raise ValueError('contours: bounds ((x0, y0), (x1, y1)) with x1 > x0 and y1 > y0 expected, got %r' % (bounds,))
    if step is None:
        step = np.sqrt((x1 - x0) * (y1 - y0) / samples)
    dx, dy = _steps(step)
    X, Y = axis(x0, x1, dx), axis(y0, y1, dy)
    dt = eng.tape_for(f)
    if dt.tape.externs or eng.precision != engine.PRECISION_F64:
        G = np.stack(np.meshgrid(X, Y, indexing='ij'), axis=-1).reshape(-1, 2)
        if three:
            V = np.stack([eng.eval_points(dt, np.ascontiguousarray(np.column_stack([G, np.full(len(G), h)]))) for h in W])
        else:
            V = eng.eval_points(dt, np.ascontiguousarray(G))[None]
        return contour_grid(V.reshape(-1, len(X), len(Y)), X, Y, level, W, eng)
    return contour_tape(dt, X, Y, W, level, eng)
