"""Constructed triangle soups for the readers of a finished mesh (k_stl and k_ply_* of csrc/sdf_plain.hip, csrc/sdf_weld.hip): named,
seeded builders of (3T, 3) float64 arrays, plain NumPy.  tests/test_mesh_readers_host.py and tests/test_mesh_readers_gpu.py read
them; tools/make_golden_stl.py runs the reference's STL writer over them (so this module stays importable under Python 3.9, like
tests/fixtures.py) and records a sha256 of every soup, by which the tests notice a builder that drifts.

Class A (`CLASS_A`): every coordinate is finite and at most 2^60 in magnitude after the float32 cast, so every component of a
cross product is finite and the only NaN of an STL record is the 0/0 of the final division.  Class B (`CLASS_B`): a coordinate is
NaN, +-inf, overflows float32 or is so large that the cross product overflows; `generate` never emits these.  `WELD` are row sets
for the weld: ties, neighbours one ulp apart, both zeros, the ends of the float64 range."""
import itertools
import zlib

import numpy as np

CLASS_A = ('duplicate', 'collinear', 'f32_collapse', 'tiny', 'denormal', 'wide_exponent', 'signed_zero', 'ordinary')
CLASS_B = ('nan', 'inf', 'overflow', 'huge')
COUNTS = (1, 255, 256, 257)              # k_stl's 256-thread boundary; the 50-byte records are 2-byte aligned
WIDE_COUNT = 513
B_COUNT = 64
PLY_COUNTS = (1, 2, 3, 4, 255, 256, 257, 259, 515)     # 13 T mod 4 = 1, 2, 3, 0 alone, then 3, 0, 1, 3, 3 behind full workgroups
WELD = ('all_equal', 'all_distinct', 'z_neighbours', 'mixed_signs', 'signed_zeros', 'extremes')
WELD_COUNTS = (1, 85, 86, 171, 257)      # 3, 255, 258, 513, 771 rows: around the weld's 256-thread blocks

TINY = 5e-324                            # the smallest float64 denormal
MIN_NORMAL = 2.2250738585072014e-308


def _rng(name, T):
    return np.random.RandomState((zlib.crc32(name.encode('ascii')) + 7919 * T) % (2 ** 32))


def _well_shaped(rng, T):
    """T triangles around random centres in [-1, 1]^3, vertices on three distinct axes' sides of the centre"""
    c = rng.uniform(-1, 1, (T, 1, 3))
    d = rng.uniform(0.05, 0.3, (T, 3, 3)) * np.where(rng.uniform(size=(T, 3, 3)) < 0.5, -1.0, 1.0)
    return c + d * (0.25 + 0.75 * np.eye(3))


def ordinary(T):
    return _well_shaped(_rng('ordinary', T), T)


def duplicate(T):
    """two or three equal vertices, in every position: triangle i has v1 = v0, v2 = v0, v2 = v1, v0 = v1 = v2 for i mod 4 = 0 .. 3"""
    t = _well_shaped(_rng('duplicate', T), T)
    k = np.arange(T) % 4
    t[k == 0, 1] = t[k == 0, 0]
    t[k == 1, 2] = t[k == 1, 0]
    t[k == 2, 2] = t[k == 2, 1]
    t[k == 3, 1] = t[k == 3, 0]
    t[k == 3, 2] = t[k == 3, 0]
    return t


def collinear(T):
    """exactly collinear in float32: a, a + p d, a + q d on a lattice of eighths; (p, q) cycles through both orientations --
    the third vertex beyond the second, between the first two, behind the first"""
    rng = _rng('collinear', T)
    a = rng.randint(-64, 65, (T, 3)) / 8.0
    d = rng.randint(-8, 9, (T, 3)) / 8.0
    d[~d.any(axis=1)] = (0.125, -0.25, 0.5)
    pq = np.array([(1, 2), (2, 1), (1, -1), (-1, 1), (3, -2), (-2, -3)], dtype=np.float64)[np.arange(T) % 6]
    return np.stack([a, a + pq[:, :1] * d, a + pq[:, 1:] * d], axis=1)


def f32_collapse(T):
    """vertices distinct in float64 and equal after the float32 cast: s (1 + k 1e-9), s a power of two with a sign, |k| <= 27
    (half a float32 ulp below 1 is 2.98e-8)"""
    rng = _rng('f32_collapse', T)
    k = np.arange(1, 10, dtype=np.float64).reshape(1, 3, 3) * rng.randint(1, 4, (T, 1, 1)) * rng.choice([-1.0, 1.0], (T, 1, 1))
    s = rng.choice([-1.0, 1.0], (T, 1, 3)) * 2.0 ** rng.randint(-3, 4, (T, 1, 3))
    t = s * (1.0 + k * 1e-9)
    f = t.astype(np.float32)
    assert (f[:, 0] == f[:, 1]).all() and (f[:, 0] == f[:, 2]).all()
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    return t


def tiny(T):
    """edges of 1e-30: every product of the cross product underflows to zero in float32, the normal is 0/0"""
    return _well_shaped(_rng('tiny', T), T) * 1e-30


def denormal(T):
    """edges of 1e-20: the cross product's components are float32 denormals, their squares are zero, the normal is +-inf"""
    return _well_shaped(_rng('denormal', T), T) * 1e-20


def wide_exponent(T):
    """coordinates +-m 2^e, m uniform in [1, 2), e an integer uniform in [-60, 59]: drawn once per triangle for the even triangles
    -- their cross products are of the order 2^2e, normal numbers all, and the squares under the root, 2^4e, underflow to zero,
    are denormal, normal or overflow -- and per coordinate for the odd ones, where the largest coordinate absorbs the others"""
    rng = _rng('wide_exponent', T)
    m = rng.uniform(1.0, 2.0, (T, 3, 3))
    e = rng.randint(-60, 60, (T, 3, 3))
    e[::2] = e[::2, :1, :1]
    return np.where(rng.uniform(size=(T, 3, 3)) < 0.5, -1.0, 1.0) * m * 2.0 ** e


def signed_zero(T):
    """triangles in the coordinate planes: the plane's coordinate is -0.0 or +0.0 per vertex, the other two lie on a lattice of
    quarters whose zeros are negative half of the time -- the edges, the products and the normal hold zeros of both signs"""
    rng = _rng('signed_zero', T)
    t = rng.randint(-4, 5, (T, 3, 3)) / 4.0
    t[np.arange(T), :, np.arange(T) % 3] = 0.0
    return np.where((t == 0) & (rng.uniform(size=t.shape) < 0.5), -0.0, t)


def _class_b(name, values):
    """well-shaped triangles with one, two or three coordinates replaced by `values`, at every position in turn"""
    rng = _rng('b_' + name, B_COUNT)
    t = _well_shaped(rng, B_COUNT).reshape(B_COUNT, 9)
    for i in range(B_COUNT):
        for j in range(1 + i % 3):
            t[i, (i + 4 * j) % 9] = values[(i + j) % len(values)]
    return t.reshape(B_COUNT, 3, 3)


def class_b(name):
    if name == 'nan':
        t = _class_b(name, [np.nan])
    elif name == 'inf':
        t = _class_b(name, [np.inf, -np.inf])
    elif name == 'overflow':
        t = _class_b(name, [1e39, -1e39, 3.5e38])
    elif name == 'huge':
        t = _class_b(name, [1e19, -1e30, 3e38, -2e25])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(t.reshape(-1, 3))


_BUILDERS = {'duplicate': duplicate, 'collinear': collinear, 'f32_collapse': f32_collapse, 'tiny': tiny, 'denormal': denormal,
             'wide_exponent': wide_exponent, 'signed_zero': signed_zero, 'ordinary': ordinary}


def class_a(name, T):
    """the (3T, 3) float64 soup of a class-A case"""
    t = np.ascontiguousarray(_BUILDERS[name](T).reshape(-1, 3), dtype=np.float64)
    assert t.shape == (3 * T, 3) and np.isfinite(t).all() and np.abs(t).max() <= 2.0 ** 60
    return t


def stl_cases():
    """[(key, class 'A' or 'B', soup)] of everything the STL golden records, in a fixed order"""
    out = [('%s_%d' % (n, T), 'A', class_a(n, T)) for n in CLASS_A for T in COUNTS]
    out.append(('wide_exponent_%d' % WIDE_COUNT, 'A', class_a('wide_exponent', WIDE_COUNT)))
    out += [('b_%s_%d' % (n, B_COUNT), 'B', class_b(n)) for n in CLASS_B]
    return out


def cast_edges(T):
    """(3T, 3) rows drawn from the edges of the float64 -> float32 cast: results that are float32 denormals, ties at the smallest
    denormal, at the denormal/normal border, at 1 and at the largest float32 (to even: down to zero, up to 2^-126, to infinity),
    underflow to +-0 and overflow to +-inf"""
    f32_max = float(np.finfo(np.float32).max)
    v = [1e-40, 3e-39, 2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 3 * 2.0 ** -150, 1e-46, 2.0 ** -126,
         (1 - 2.0 ** -25) * 2.0 ** -126, (1 - 2.0 ** -24) * 2.0 ** -126, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, np.nextafter(1 + 2.0 ** -24, 2.0),
         f32_max, f32_max + 2.0 ** 102, np.nextafter(f32_max + 2.0 ** 102, 0.0), 3.5e38, 1e39, 0.0, 0.5]
    v = np.array(v + [-x for x in v])
    rows = v[_rng('cast_edges', T).randint(0, len(v), (3 * T, 3))]
    rows[:len(v), 0] = v[:3 * T]                      # every value at least once
    return np.ascontiguousarray(rows, dtype=np.float64)


def ulp_chain(x, below, above):
    """x with `below` predecessors and `above` successors, ascending"""
    lo, hi = [x], [x]
    for _ in range(below):
        lo.append(np.nextafter(lo[-1], -np.inf))
    for _ in range(above):
        hi.append(np.nextafter(hi[-1], np.inf))
    return lo[:0:-1] + hi


def weld_rows(name, T):
    """the (3T, 3) float64 rows of a weld case (no NaN: np.unique leaves the order of NaN rows open)"""
    n = 3 * T
    rng = _rng('weld_' + name, T)
    if name == 'all_equal':
        r = np.tile(np.array([[0.375, -2.5, 1e-3]]), (n, 1))
    elif name == 'all_distinct':
        r = rng.permutation(3 * n).reshape(n, 3) * 0.5 - 0.75 * n
    elif name == 'z_neighbours':
        # equal x and y; z runs one ulp at a time across zero (both zeros among them), the denormal/normal border on both sides
        # and 1.0; every value occurs, then the rest is drawn with repeats
        z = np.array(ulp_chain(0.0, 3, 3) + [-0.0] + ulp_chain(MIN_NORMAL, 3, 3) + ulp_chain(-MIN_NORMAL, 3, 3)
                     + ulp_chain(1.0, 2, 2) + ulp_chain(-1.0, 2, 2))
        z = np.concatenate([z, z[rng.randint(0, len(z), max(n - len(z), 0))]])[rng.permutation(max(n, len(z)))][:n]
        r = np.stack([np.full(n, -0.625), np.full(n, 3.0), z], axis=1)
    elif name == 'mixed_signs':
        r = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (n, 3))
    elif name == 'signed_zeros':
        # +-0.0 in every column and order, alone and next to a non-zero column: classes whose members differ in the signs of zero
        v = [np.array(p) for p in itertools.product([0.0, -0.0], repeat=3)]
        v += [np.array(p) for p in itertools.product([0.0, -0.0, 1.0], repeat=3)]
        v = np.array(v)
        r = v[rng.randint(0, len(v), n)]
    elif name == 'extremes':
        v = np.array([TINY, -TINY, 1e308, -1e308, np.inf, -np.inf, 0.0, -0.0])
        r = v[rng.randint(0, len(v), (n, 3))]
    else:
        raise KeyError(name)
    r = np.ascontiguousarray(r, dtype=np.float64)
    assert r.shape == (n, 3) and not np.isnan(r).any()
    return r
