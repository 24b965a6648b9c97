"""Volumes and sampling grids aimed at the places where the marching-cubes vertex arithmetic is fragile: float32 ties of the
vertex coordinate, grid indices at which a float64 ulp outgrows the fast vertex path's safety window, non-finite and denormal
samples, row counts at the kernels' block boundaries, models sampled exactly on their surface.  Named, seeded builders, plain
NumPy (tests/soups_ref.py is the pattern).  tools/make_golden_mc_edges.py runs the reference over them -- so this module stays
importable under Python 3.9 and imports nothing of the package -- and records a sha256 of every volume, by which
tests/test_mc_edges_host.py notices a builder that drifts; tests/test_mc_edges_gpu.py holds the device to the same golden.

  ties         pairs v_lo = k s, v_hi = -(2^m - k) s on the edge i .. i + 1: i + k / 2^m is a float32 tie (2^-m half the float32
               spacing at i) up to the roundings of t; the fast path has to fall back to the three divisions
  large_index  the same layout at indices 511 .. 4094, with the pairs tools/find_mc_near_ties.py found (NEAR_TIES) and random ones
  special      NaN, infinities, zeros of both signs, denormals, +-3e38, values that overflow the float32 cast
  shapes       (n0 - 1)(n1 - 1) rows around the 256 threads of k_mc_rows / k_mc_emit and the 1024 of k_scan_rows; long thin volumes
  on_surface   models whose zero set holds whole planes of grid samples (GRIDS are dyadic), through `generate`
"""
import hashlib
import zlib

import numpy as np

ROWS = 257                                   # one full 256-thread workgroup of k_mc_rows plus one row
TIE_INDICES = (1, 16, 31, 32)
LARGE_INDICES = (511, 512, 513, 1023, 1024, 2048, 2049, 3001, 4094)
RANDOM_PAIRS = 200                           # at least: the rest of the ROWS rows of a large_index volume

# The output of tools/find_mc_near_ties.py: (v_lo, v_hi, mask) per binade 2^e <= index < 2^(e + 1) -- the search's result depends
# on the index through its binade alone.  mask: bit 1 / 2 / 4 = skimage's float32 differs from the one-division path's with the
# quotient correctly rounded / one ulp up / one ulp down; 0 (binade 8, where the window works): the 32 pairs nearest a tie.
_NEAR_TIES = {
    8: [
        (8454015.0, -129.0, 0), (8519550.0, -130.0, 0), (8585085.0, -131.0, 0),
        (8650620.0, -132.0, 0), (8716155.0, -133.0, 0), (8781690.0, -134.0, 0),
        (8847225.0, -135.0, 0), (8912760.0, -136.0, 0), (8978295.0, -137.0, 0),
        (9043830.0, -138.0, 0), (9109365.0, -139.0, 0), (9174900.0, -140.0, 0),
        (9240435.0, -141.0, 0), (9305970.0, -142.0, 0), (9371505.0, -143.0, 0),
        (9437040.0, -144.0, 0), (9502575.0, -145.0, 0), (9568110.0, -146.0, 0),
        (9633645.0, -147.0, 0), (9699180.0, -148.0, 0), (9764715.0, -149.0, 0),
        (9830250.0, -150.0, 0), (9895785.0, -151.0, 0), (9961320.0, -152.0, 0),
        (10026855.0, -153.0, 0), (10092390.0, -154.0, 0), (10157925.0, -155.0, 0),
        (10223460.0, -156.0, 0), (10288995.0, -157.0, 0), (10354530.0, -158.0, 0),
        (10420065.0, -159.0, 0), (10485600.0, -160.0, 0),
    ],
    9: [
        (8420604.0, -256.9842834472656, 2), (8420605.0, -256.98431396484375, 3), (8431584.0, -772.0052490234375, 4),
        (8453369.0, -257.9842224121094, 2), (8453370.0, -257.9842529296875, 3), (8482552.0, -776.6719360351562, 5),
        (8486134.0, -258.9841613769531, 2), (8500755.0, -778.338623046875, 4), (8518899.0, -259.9841003417969, 2),
        (8551664.0, -260.9840393066406, 2), (8551723.0, -783.0053100585938, 5), (8569926.0, -784.6719970703125, 4),
        (8584429.0, -261.9839782714844, 2), (8617194.0, -262.9839172363281, 2), (8639097.0, -791.00537109375, 4),
        (8649959.0, -263.9838562011719, 2), (8682724.0, -264.9837951660156, 2), (8715489.0, -265.9837341308594, 2),
        (8726471.0, -799.0054321289062, 4), (8748254.0, -266.9836730957031, 2), (8777439.0, -803.672119140625, 5),
        (8781019.0, -267.9836120605469, 2), (8781020.0, -267.983642578125, 3), (8795642.0, -805.3388061523438, 4),
        (8813784.0, -268.9835510253906, 2), (8864813.0, -811.6721801757812, 4), (8933984.0, -818.0055541992188, 4),
        (8952187.0, -819.6722412109375, 4), (9003155.0, -824.3389282226562, 5), (9021358.0, -826.005615234375, 4),
        (9090529.0, -832.3389892578125, 4), (9159700.0, -838.67236328125, 4), (9298042.0, -851.339111328125, 5),
        (9367213.0, -857.6724853515625, 5), (9370790.0, -285.9825439453125, 3), (9600145.0, -292.98211669921875, 3),
        (9662100.0, -884.6726684570312, 5), (9731271.0, -891.0060424804688, 5), (9960560.0, -303.9814453125, 3),
        (10124385.0, -308.98114013671875, 3), (10182703.0, -932.3396606445312, 5),
    ],
    10: [
        (8420605.0, -513.9843139648438, 4), (8453370.0, -515.9842529296875, 4), (8486135.0, -517.9841918945312, 4),
        (8518900.0, -519.984130859375, 4), (8551665.0, -521.9840698242188, 4), (8584430.0, -523.9840087890625, 4),
        (8617195.0, -525.9839477539062, 4), (8649960.0, -527.98388671875, 4), (8682725.0, -529.9838256835938, 4),
        (8715490.0, -531.9837646484375, 4), (8748255.0, -533.9837036132812, 4), (8781020.0, -535.983642578125, 4),
        (8813785.0, -537.9835815429688, 4), (8846550.0, -539.9835205078125, 4), (8879315.0, -541.9834594726562, 4),
        (8912080.0, -543.9833984375, 4), (9698440.0, -591.98193359375, 3), (9763970.0, -595.9818115234375, 3),
        (9862265.0, -601.9816284179688, 3), (9895030.0, -603.9815673828125, 3), (10452035.0, -637.9805297851562, 3),
        (10484800.0, -639.98046875, 3), (10517565.0, -641.9804077148438, 3), (10615860.0, -647.980224609375, 3),
        (10943510.0, -667.9796142578125, 3), (11009040.0, -671.9794921875, 3), (11140100.0, -679.979248046875, 3),
        (11451367.0, -698.9786376953125, 2), (11484132.0, -700.9785766601562, 2), (11516897.0, -702.978515625, 2),
        (11549662.0, -704.9784545898438, 2), (11566045.0, -705.9784545898438, 3), (11664340.0, -711.978271484375, 3),
        (12417935.0, -757.9768676757812, 3), (12450700.0, -759.976806640625, 3), (12483465.0, -761.9767456054688, 3),
    ],
    11: [
        (8452983.0, -1031.9842529296875, 4), (8518510.0, -1039.984130859375, 4), (8584037.0, -1047.9840087890625, 3),
        (8649564.0, -1055.98388671875, 4), (8715091.0, -1063.9837646484375, 4), (8780618.0, -1071.983642578125, 4),
        (8846145.0, -1079.9835205078125, 4), (8911672.0, -1087.9833984375, 4), (8977199.0, -1095.9832763671875, 4),
        (9042726.0, -1103.983154296875, 4), (9108253.0, -1111.9830322265625, 4), (9173780.0, -1119.98291015625, 4),
        (9239307.0, -1127.9827880859375, 4), (9304834.0, -1135.982666015625, 3), (9370361.0, -1143.9825439453125, 4),
        (9435888.0, -1151.982421875, 4), (9501415.0, -1159.9822998046875, 4), (9566942.0, -1167.982177734375, 4),
        (10287739.0, -1255.9808349609375, 3), (10549847.0, -1287.9803466796875, 3), (10680901.0, -1303.9801025390625, 3),
        (10746428.0, -1311.97998046875, 3), (11459034.0, -1398.9786376953125, 2), (11524561.0, -1406.978515625, 2),
        (11590088.0, -1414.9783935546875, 2), (11655615.0, -1422.978271484375, 2), (11721142.0, -1430.9781494140625, 2),
        (11786669.0, -1438.97802734375, 2), (11852196.0, -1446.9779052734375, 2), (11860387.0, -1447.9779052734375, 3),
        (11917723.0, -1454.977783203125, 2), (11983250.0, -1462.9776611328125, 2), (12122495.0, -1479.9774169921875, 3),
        (12515657.0, -1527.9766845703125, 3), (12581184.0, -1535.9765625, 3), (12777765.0, -1559.9761962890625, 3),
        (13105400.0, -1599.9755859375, 3), (13170927.0, -1607.9754638671875, 3), (13433035.0, -1639.9749755859375, 3),
        (13498562.0, -1647.974853515625, 3), (13564089.0, -1655.9747314453125, 3),
    ],
}
NEAR_TIES = {i: _NEAR_TIES[int(np.floor(np.log2(i)))] for i in LARGE_INDICES}
# skimage and the checker on the edge 2048 .. 2049; a correctly rounded a / (a + b) ends on the tie and in 2049.0
QUOTED_PAIR = (2048, 8584037.0, -1047.9840087890625, 2048.999755859375)

EPS = 2.220446049250313e-16


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode('ascii')) % (2 ** 32))


def sha256(volume):
    v = np.ascontiguousarray(volume)
    return hashlib.sha256(repr((v.shape, v.dtype.str)).encode('ascii') + v.tobytes()).hexdigest()


def edge_positions(i, v_lo, v_hi):
    """skimage's vertex coordinate along the edge i .. i + 1: three float64 divisions, stored as float32"""
    w_lo, w_hi = 1.0 / (EPS + np.abs(np.asarray(v_lo, np.float64))), 1.0 / (EPS + np.abs(np.asarray(v_hi, np.float64)))
    return (np.float64(i) + w_hi / (w_lo + w_hi)).astype(np.float32)


# ---- ties and large_index: one pair per row -----------------------------------------------------------------------------
def tie_pairs(i):
    """(ROWS, 2) float64: v_lo = k s, v_hi = -(2^m - k) s, k odd below 2^m, s a power of two"""
    rng = _rng('ties_%d' % i)
    m = 24 - int(np.floor(np.log2(i)))
    k = 2 * rng.randint(0, 2 ** (m - 1), ROWS) + 1
    k[:4] = (1, 2 ** m - 1, 2 ** (m - 1) - 1, 2 ** (m - 1) + 1)[:4]
    s = 2.0 ** rng.randint(-30, 61, ROWS)
    return np.stack([k * s, -(2 ** m - k) * s], axis=1)


def large_index_pairs(i):
    """(ROWS, 2) float64: the recorded near-tie pairs of the index, then random ones (v_lo > 0 > v_hi, five decades)"""
    rng = _rng('large_index_%d' % i)
    rec = np.array([(a, b) for a, b, _ in NEAR_TIES[i]], np.float64)
    n = ROWS - len(rec)
    assert n >= RANDOM_PAIRS
    rnd = np.abs(rng.standard_normal((n, 2))) * 10.0 ** rng.uniform(-2, 3, (n, 2)) * (1, -1)
    return np.concatenate([rec, rnd.astype(np.float32).astype(np.float64)])


def pair_volume(i, pairs, axis):
    """(ROWS, 2, i + 2) float32, 1.0 up to index i - 1 and the row's pair at i, i + 1: every row changes sign on the same edge,
    the surface is one flat sheet of 2 (ROWS - 1) triangles.  axis 2 as it stands; for axis 0 / 1 the edge's axis is moved there"""
    vol = np.ones((len(pairs), 2, i + 2), np.float32)
    vol[:, :, i] = pairs[:, :1]
    vol[:, :, i + 1] = pairs[:, 1:]
    return np.ascontiguousarray(vol.transpose({0: (2, 1, 0), 1: (1, 2, 0), 2: (0, 1, 2)}[axis]))


# ---- special -------------------------------------------------------------------------------------------------------------
DENORMAL = float(np.float32(2.0 ** -149))
SPECIAL = {
    'nan': (np.nan,), 'pinf': (np.inf,), 'ninf': (-np.inf,), 'zero': (0.0,), 'negzero': (-0.0,), 'denormal': (DENORMAL, -DENORMAL),
    'huge': (3e38, -3e38), 'overflow': (1e39, -1e39),
}
SPECIAL['mixed'] = tuple(v for k in ('nan', 'pinf', 'ninf', 'zero', 'negzero', 'denormal', 'huge', 'overflow') for v in SPECIAL[k])


def special_volume(kind):
    """9 x 10 x 11 float64 standard normal with about a tenth of the samples replaced by the kind's values"""
    rng = _rng('special_' + kind)
    vol = rng.standard_normal((9, 10, 11))
    where = rng.uniform(size=vol.shape) < 0.1
    vals = np.array(SPECIAL[kind])
    vol[where] = vals[rng.randint(0, len(vals), int(where.sum()))]
    return vol


def special_corner(kind):
    """2 x 2 x 2 float64 standard normal with the kind's first value at one corner (the corner moves with the kind)"""
    rng = _rng('corner_' + kind)
    vol = rng.standard_normal((2, 2, 2))
    vol.reshape(-1)[sorted(SPECIAL).index(kind) % 8] = SPECIAL[kind][0]
    return vol


# ---- shapes --------------------------------------------------------------------------------------------------------------
# (n0 - 1)(n1 - 1) = 1, 255, 256, 257, 1023, 1024, 1025, 2049 rows of two cells; then one row and 4999 rows
SHAPES = ((2, 2, 3), (16, 18, 3), (17, 17, 3), (258, 2, 3), (32, 34, 3), (33, 33, 3), (26, 42, 3), (4, 684, 3), (2, 2, 5000), (5000, 2, 2))
assert [(s[0] - 1) * (s[1] - 1) for s in SHAPES[:8]] == [1, 255, 256, 257, 1023, 1024, 1025, 2049]


def shape_volume(shape):
    return _rng('shape_%dx%dx%d' % shape).standard_normal(shape)


# ---- the table of volume cases -------------------------------------------------------------------------------------------
def _volume_table():
    t = {}
    for i in TIE_INDICES:
        for ax in range(3):
            t['ties_i%d_ax%d' % (i, ax)] = ('ties', lambda i=i, ax=ax: pair_volume(i, tie_pairs(i), ax))
    for i in LARGE_INDICES:
        for ax in range(3):
            t['large_i%d_ax%d' % (i, ax)] = ('large_index', lambda i=i, ax=ax: pair_volume(i, large_index_pairs(i), ax))
    for kind in SPECIAL:
        t['special_' + kind] = ('special', lambda kind=kind: special_volume(kind))
    for kind in SPECIAL:
        if kind != 'mixed':
            t['corner_' + kind] = ('special', lambda kind=kind: special_corner(kind))
    t['all_nan'] = ('special', lambda: np.full((3, 4, 5), np.nan))
    for s in SHAPES:
        t['shape_%dx%dx%d' % s] = ('shapes', lambda s=s: shape_volume(s))
    return t


VOLUMES = _volume_table()
FAMILIES = ('ties', 'large_index', 'special', 'shapes', 'on_surface')


def volume_keys(family=None):
    return [k for k, (f, _) in VOLUMES.items() if family is None or f == family]


def volume(key):
    """the case's volume as the reference is given it: float32 for the pair layouts, float64 otherwise"""
    return VOLUMES[key][1]()


def pair_case(key):
    """(index, axis, pairs) of a ties / large_index case"""
    fam, rest = key.split('_i')
    i, ax = (int(s) for s in rest.split('_ax'))
    return i, ax, (tie_pairs(i) if fam == 'ties' else large_index_pairs(i))


# ---- on_surface: models through generate ---------------------------------------------------------------------------------
# programs over the `from sdf import *` namespace (tests/param_cases.py); the zero set of each holds grid samples of both grids
MODELS = {
    'box': "f = box(1)",                                   # faces at +-1/2: whole planes of samples are 0.0
    'sphere': "f = sphere(0.5)",                           # the six axis points
    'slab': "f = slab(z0=0)",
    'plane': "f = plane((1, 0, 0), (0.25, 0, 0))",
    # positive everywhere but NaN on the plane z = 0 (tests/param_cases.py DEGENERATE): a partially-NaN field for k_mesh
    'nan_plane': "f = rectangle(2).extrude_to(circle(1), 0)",
}
GRIDS = {'g8': np.arange(-8, 9) / 8.0, 'g32': np.arange(-40, 41) / 32.0}
BATCH = 32


def surface_keys():
    return ['%s_%s' % (m, g) for m in MODELS for g in GRIDS]


def surface_case(key):
    """(program, axis) -- the same axis in x, y and z"""
    m, g = key.rsplit('_', 1)
    return MODELS[m], GRIDS[g]


def reference_grid(axis):
    """(bounds, step) from which the reference's np.arange gives exactly `axis`"""
    step = float(axis[1] - axis[0])
    lo, hi = float(axis[0]), float(axis[-1]) + step / 2
    assert np.array_equal(np.arange(lo, hi, step), axis)
    return ((lo, lo, lo), (hi, hi, hi)), step


def build_model(program, namespace):
    ns = dict(namespace)
    exec(program, ns)
    return ns['f']


CASE_COUNTS = {f: len(volume_keys(f)) for f in FAMILIES[:4]}
CASE_COUNTS['on_surface'] = 2 * len(surface_keys())          # sparse and dense


# ---- soups in the golden, and how two soups are compared ------------------------------------------------------------------
def pack_soup(soup):
    """(rows, code) from which unpack_soup gives the soup back bit for bit (NaN payloads and zero signs too).  rows (3, V): the
    soup's distinct rows in the order of their first appearance, one coordinate per line.  code, per soup row: 0 for a row seen
    for the first time, else 1 + how many distinct rows were first seen since it was.  (A mesh refers to recent vertices: the codes
    are small and deflate well, which is what keeps a few hundred thousand vertices of noise under the size limit.)"""
    a = np.ascontiguousarray(soup)
    bits = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).reshape(-1, 3)
    u, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(len(u), np.int64)
    rank[order] = np.arange(len(u))
    index = rank[inv.reshape(-1)]
    new = np.zeros(len(index), bool)
    new[first] = True
    code = np.where(new, 0, np.cumsum(new) - index)
    return np.ascontiguousarray(u[order].view(a.dtype).T), code.astype(np.uint16 if len(u) < 65536 else np.uint32)


def unpack_soup(rows, code):
    code = code.astype(np.int64)
    seen = np.cumsum(code == 0)
    return np.ascontiguousarray(rows.T)[np.where(code == 0, seen - 1, seen - code)]


def assert_same_soup(got, want, what=''):
    """NaN coordinates in the same places, every other coordinate bit-identical (the sign of a zero included).  Which NaN --
    skimage's comes out of its float64 arithmetic with whatever sign and payload the operations leave -- is not part of the
    contract, nor is it stable between CPUs."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    n_got, n_want = np.isnan(got), np.isnan(want)
    assert np.array_equal(n_got, n_want), '%s: %d NaN coordinates, expected %d' % (what, int(n_got.sum()), int(n_want.sum()))
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = got[~n_got].view(bits), want[~n_want].view(bits)
    assert np.array_equal(a, b), '%s: %d of %d coordinates differ' % (what, int((a != b).sum()), a.size)
