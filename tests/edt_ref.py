"""NumPy restatement of the device distance texture (csrc/sdf_edt.hip), with integer arithmetic and
without scipy.  For a boolean mask `a` that holds both classes:

    D(p)       = min over the pixels q with a[q] != a[p] of (p.row - q.row)^2 + (p.col - q.col)^2     (an integer)
    texture[p] = -sqrt(float64(D(p))) where a[p], +sqrt(float64(D(p))) elsewhere

`squared` is the definition itself, brute force over the pixels of the other class; `squared_separable` is the two-pass
form (a scan along the rows, then a bounded minimum along the columns) for masks that brute force cannot reach.  The CPU
tests hold the two to each other, and both to scipy where it is installed.  `cases()` are the masks every test uses."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edt.npz')


def _check(mask):
    a = np.asarray(mask)
    if a.ndim != 2 or a.size == 0:
        raise ValueError('the mask must be 2-D and not empty, got shape %s' % (a.shape,))
    a = a != 0
    if a.all() or not a.any():
        raise ValueError('every pixel of the mask is of one class')
    return a


def squared(mask, chunk=1 << 22):
    """D of the definition, int64: brute force, `chunk` pixel pairs at a time"""
    a = _check(mask)
    D = np.zeros(a.shape, np.int64)
    for cls in (True, False):
        P = np.argwhere(a == cls).astype(np.int64)          # the pixels of this class ...
        Q = np.argwhere(a != cls).astype(np.int64)          # ... and of the other one
        step = max(1, chunk // len(Q))
        for s in range(0, len(P), step):
            p = P[s:s + step]
            d = (p[:, None, 0] - Q[None, :, 0]) ** 2 + (p[:, None, 1] - Q[None, :, 1]) ** 2
            D[p[:, 0], p[:, 1]] = d.min(axis=1)
    return D


def _row_distance(t):
    """per pixel, the distance along its row to the nearest True pixel of t (0 on one); -1 where the row has none"""
    R, C = t.shape
    far = 4 * (R + C)
    idx = np.arange(C, dtype=np.int64)[None, :]
    last = np.maximum.accumulate(np.where(t, idx, -far), axis=1)
    nxt = np.minimum.accumulate(np.where(t, idx, far)[:, ::-1], axis=1)[:, ::-1]
    d = np.minimum(idx - last, nxt - idx)
    return np.where(d >= C, -1, d)


def _column_minimum(g, want):
    """min over j of g[j, c]^2 + (i - j)^2, exact at the pixels `want` (g < 0: no candidate in that row); offsets are tried
    outwards and the walk stops once the offset squared reaches the largest value still standing at a wanted pixel"""
    R = g.shape[0]
    none = np.int64(1) << 40
    g2 = np.where(g < 0, none, g * g)
    best = g2.copy()
    k = 1
    while k < R and k * k < best[want].max():
        best[k:] = np.minimum(best[k:], g2[:-k] + k * k)
        best[:-k] = np.minimum(best[:-k], g2[k:] + k * k)
        k += 1
    return best


def squared_separable(mask):
    """D by the two-pass form, int64: equal to `squared` (tests/test_edt_host.py), usable on large masks"""
    a = _check(mask)
    to_false = _column_minimum(_row_distance(~a), a)       # what a True pixel takes
    to_true = _column_minimum(_row_distance(a), ~a)        # what a False pixel takes
    return np.where(a, to_false, to_true)


def texture_of(D, mask):
    r = np.sqrt(D.astype(np.float64))
    return np.where(np.asarray(mask) != 0, -r, r)


def distance_texture(mask):
    return texture_of(squared(mask), mask)


def distance_texture_separable(mask):
    return texture_of(squared_separable(mask), mask)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def dejavu():
    """matplotlib's bundled DejaVuSans.ttf, or None where matplotlib is not installed"""
    try:
        import matplotlib
    except ImportError:
        return None
    return os.path.join(os.path.dirname(matplotlib.__file__), 'mpl-data/fonts/ttf/DejaVuSans.ttf')


def rendered_mask(font, string, points, pixels=None):
    """the mask `text(font, string, points=points, pixels=pixels)` hands to `distance_texture`"""
    import importlib
    T = importlib.import_module('sdf_amd.text')
    canvas, pad = T._canvas(font, string, points)
    return np.array(T._mask(T.PIXELS if pixels is None else pixels, pad[0], pad[1], canvas)[0], dtype=bool)


def cases():
    """name -> mask: random masks at several densities and shapes (1 x n, n x 1, non-square, sizes off every multiple of 64
    and of the kernels' tiles), a single True pixel, a single False pixel, a checkerboard, a frame.  Seeded; brute force
    reaches all of them.  (The rendered 'Hello' mask is a golden: its raster depends on the FreeType build.)"""
    rng = np.random.RandomState(20240)
    out = {}
    for name, shape, p in [('r_37x53_50', (37, 53), 0.5), ('r_53x37_10', (53, 37), 0.1), ('r_64x64_90', (64, 64), 0.9),
                           ('r_1x200_50', (1, 200), 0.5), ('r_200x1_30', (200, 1), 0.3), ('r_1x2', (1, 2), 0.5),
                           ('r_17x130_02', (17, 130), 0.02), ('r_131x19_98', (131, 19), 0.98), ('r_65x129_50', (65, 129), 0.5),
                           ('r_100x100_001', (100, 100), 0.001)]:
        m = rng.uniform(size=shape) < p
        m.flat[0] = True                                    # both classes, whatever the draw
        m.flat[-1] = False
        out[name] = m
    one = np.zeros((41, 67), bool)
    one[29, 5] = True
    out['single_true'] = one
    out['single_false'] = ~one
    yy, xx = np.mgrid[0:33, 0:47]
    out['checkerboard'] = (yy + xx) % 2 == 0
    out['blocks'] = ((yy // 5) + (xx // 7)) % 2 == 0
    fr = np.zeros((40, 60), bool)
    fr[10:30, 15:45] = True
    fr[18:22, 25:35] = False
    out['frame'] = fr
    return out


def golden():
    """{name: (mask, scipy's texture)} recorded by tools/make_golden_edt.py"""
    z = np.load(GOLDEN)
    return {k[5:]: (np.unpackbits(z[k])[:int(np.prod(z['shape_' + k[5:]]))].reshape(z['shape_' + k[5:]]).astype(bool), z['tex_' + k[5:]])
            for k in z.files if k.startswith('mask_')}
