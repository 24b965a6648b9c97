"""Constructed sample grids for the contour tests (tests/test_contour_host.py drives the definition with them,
tests/test_contour_gpu.py the device): name -> (V[nw, nx, ny], X, Y, level)."""
import numpy as np

H = 0.05


def axes(lo=-1.2, hi=1.2, h=H):
    n = int(round((hi - lo) / h))
    a = lo + h * np.arange(n + 1)
    return a, a.copy()


def field(fn, X, Y):
    gx, gy = np.meshgrid(X, Y, indexing='ij')
    return fn(gx, gy)


def two_by_two():
    """the 16 cases on a 2 x 2 grid, the saddles with either centre: (name, V, inside corners (c0 .. c3), centre inside or None)"""
    out = []
    for case in range(16):
        ins = [bool(case >> k & 1) for k in range(4)]
        variants = [(None, -1.0, 1.0)]
        if case in (5, 10):
            variants = [(True, -3.0, 1.0), (False, -1.0, 3.0)]          # centre = (2 in + 2 out) / 4
        for centre, vin, vout in variants:
            c = [vin if i else vout for i in ins]
            V = np.array([[[c[0], c[3]], [c[1], c[2]]]])                # V[ix, iy]: c0 = [0, 0], c1 = [1, 0], c2 = [1, 1], c3 = [0, 1]
            out.append(('case%d%s' % (case, '' if centre is None else ('in' if centre else 'out')), V, ins, centre))
    return out


def ties():
    """3 x 3, the centre sample equal to the level -- so outside -- and the eight others inside: the hole around it is four segments
    of length zero, all at the centre sample"""
    V = np.full((1, 3, 3), -1.0)
    V[0, 1, 1] = 0.0
    return V, np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.5, 3.0]), 0.0


def circle(r=1.0):
    X, Y = axes()
    return field(lambda x, y: np.hypot(x, y) - r, X, Y)[None], X, Y, 0.0


def annulus():
    X, Y = axes()
    return field(lambda x, y: np.abs(np.hypot(x, y) - 0.75) - 0.25, X, Y)[None], X, Y, 0.0


def two_layers():
    X, Y = axes()
    return np.stack([field(lambda x, y: np.hypot(x, y) - r, X, Y) for r in (1.0, 0.6)]), X, Y, 0.0


def clipped():
    X, Y = axes(-0.8, 0.8)
    return field(lambda x, y: np.hypot(x, y) - 0.95, X, Y)[None], X, Y, 0.0      # (0.95: no grid point of the border lies on it)


def with_nan():
    V, X, Y, level = circle()
    V = V.copy()
    V[0, int(np.argmin(np.abs(X - 1.0))), int(np.argmin(np.abs(Y)))] = np.nan      # a sample on the circle, in the interior of the grid
    return V, X, Y, level


def shifted_level():
    V, X, Y, _ = circle()
    return V + 0.25, X, Y, 0.25


def random_field(nx=67, ny=131, nw=1, seed=7):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((nw, nx, ny)), np.cumsum(rng.uniform(0.5, 1.5, nx)), np.cumsum(rng.uniform(0.5, 1.5, ny)), 0.1


def comb(n=257):
    """ONE closed loop of tens of thousands of segments: a bar along iy = 2 with a tooth one sample wide on every fourth ix"""
    i = np.arange(n)
    ix, iy = np.meshgrid(i, i, indexing='ij')
    box = (ix >= 2) & (ix <= n - 3) & (iy >= 2) & (iy <= n - 3)
    inside = box & ((iy == 2) | (ix % 4 == 2))
    return np.where(inside, -1.0, 1.0)[None], i * 0.5, i * 0.25, 0.0


GRIDS = {
    'ties': ties, 'circle': circle, 'annulus': annulus, 'two_layers': two_layers, 'clipped': clipped, 'with_nan': with_nan,
    'shifted_level': shifted_level,
}
