"""The definition of mesh mending, in plain NumPy and in integers only: what csrc/sdf_mend.hip reproduces
exactly.  Duplicate triangles are dropped and oppositely wound pairs cancel -- what vertex clustering (`simplify=`) leaves behind
where two sheets of a surface fall into the same clusters.

Input: the cells (T, 3) int64 of a weld (`Mesh.weld()`), in soup order.  Which triangles survive is a function of the cells alone.

1.  A cell with two equal indices is COLLAPSED: it is dropped and counted in `collapsed`.
2.  Every other cell is rotated so that its smallest index comes first: (a, b, c) with a < b and a < c.  Its FACE is
    (a, min(b, c), max(b, c)), its SIDE 0 when b < c and 1 when b > c.  The rotations of one cell have the same face and the same
    side; the flipped winding has the same face and the other side.
3.  The cells are grouped by face; n0 and n1 are how many cells of a face lie on each side.  n0 == n1: all of them are dropped and
    counted in `cancelled` -- each pair encloses nothing.  Otherwise exactly one survives, the first in soup order among the cells of
    the majority side, and the other n0 + n1 - 1 are counted in `duplicates`.
4.  The result is the surviving triangles in soup order with unchanged winding; the nine doubles of each are those of the SOURCE
    soup, bit for bit (not the welded points: -0.0 stays -0.0).

`faces` is the number of distinct faces among the cells that are not collapsed.  triangles_in == triangles_out + collapsed +
duplicates + cancelled always, and mending a mended mesh removes nothing.

Mending does not re-orient a misoriented mesh and does not close what stays open: where a thin wall collapses only in part, the rim
of the collapsed region keeps its non-manifold edges, and the edge census goes on reporting them."""
import collections

import numpy as np

import measure_ref

Mended = collections.namedtuple('Mended', ('keep', 'stats', 'soup', 'face', 'side'))
Mended.__doc__ = """keep (T,) bool in soup order and stats (dict of the integers of STAT_KEYS): what the device reproduces; soup
(T', 3, 3) float64 = the source soup's kept triangles (None when mend() was given no soup).  For the tests: face (T, 3) int64 and
side (T,) int64 of every cell (-1 for a collapsed one)."""

STAT_KEYS = ('triangles_in', 'triangles_out', 'collapsed', 'duplicates', 'cancelled', 'faces')


def faces_and_sides(cells):
    """(face (T, 3) int64, side (T,) int64, collapsed (T,) bool): step 1 and 2; a collapsed cell has face and side -1"""
    c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 3)
    collapsed = (c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 2] == c[:, 0])
    k = np.argmin(c, axis=1)
    rows = np.arange(len(c))
    a, b, cc = c[rows, k], c[rows, (k + 1) % 3], c[rows, (k + 2) % 3]
    face = np.stack([a, np.minimum(b, cc), np.maximum(b, cc)], axis=1)
    side = (b > cc).astype(np.int64)
    face[collapsed] = -1
    side[collapsed] = -1
    return face, side, collapsed


def mend(cells, soup=None):
    """the Mended of the cells (T, 3) int64 of a weld; soup: the (T, 3, 3) float64 source soup the survivors are copied from"""
    if 3 * len(cells) >= 2 ** 31:                                 # (before anything is copied)
        raise ValueError('mend: 2^31 or more corners (3 x triangles) or vertices')
    c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 3)
    n = len(c)
    if n and c.max() >= 2 ** 31:
        raise ValueError('mend: 2^31 or more corners (3 x triangles) or vertices')
    if n and c.min() < 0:
        raise ValueError('mend: a negative index')
    face, side, collapsed = faces_and_sides(c)
    live = np.flatnonzero(~collapsed)
    # face, then side, then soup order (lexsort: the last key is the primary one; `live` ascends and the sort is stable)
    order = live[np.lexsort((live, side[live], face[live, 2], face[live, 1], face[live, 0]))]
    f = face[order]
    head = np.r_[True, (f[1:] != f[:-1]).any(axis=1)] if len(order) else np.zeros(0, bool)
    start = np.flatnonzero(head)
    run = np.cumsum(head) - 1
    n1 = np.bincount(run, weights=side[order], minlength=len(start)).astype(np.int64)
    n0 = np.diff(np.r_[start, len(order)]).astype(np.int64) - n1
    wins = n0 != n1
    survivor = order[(start + np.where(n0 > n1, 0, n0))[wins]]
    keep = np.zeros(n, bool)
    keep[survivor] = True
    stats = {'triangles_in': n, 'triangles_out': int(keep.sum()), 'collapsed': int(collapsed.sum()),
             'duplicates': int((n0 + n1 - 1)[wins].sum()), 'cancelled': int((n0 + n1)[~wins].sum()), 'faces': int(len(start))}
    out = None
    if soup is not None:
        s = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
        if len(s) != n:
            raise ValueError('mend: %d cells, but a soup of %d triangles' % (n, len(s)))
        out = s[keep]
    return Mended(keep, stats, out, face, side)


def mend_soup(soup):
    """the Mended of a host soup (T, 3, 3) over its own weld (np.unique, as `Mesh.weld()` orders it)"""
    s = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    return mend(weld(s)[1], s)


weld = measure_ref.weld


# ---- the constructed cases the host and the device tests share ----
ROTATIONS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))                    # the same winding
FLIPS = ((0, 2, 1), (2, 1, 0), (1, 0, 2))                        # the other one


def unrelated(n, seed=3):
    """n triangles that share no vertex with each other or with anything in [-1, 4]^3"""
    rng = np.random.RandomState(seed + n)
    return rng.uniform(-9.0, -5.0, size=(n, 3, 3))


def repeated_face(n0, n1, n_other=7, seed=11):
    """one triangle n0 times in its winding and n1 times flipped, every copy in another rotation where there are that many, shuffled
    among n_other unrelated triangles: (soup, the soup index of the expected survivor or None)"""
    rng = np.random.RandomState(seed + 10 * n0 + n1)
    tri = np.array([[0.25, 0.5, 0.75], [0.5, 1.75, 0.25], [1.5, 0.25, 0.5]])
    # (the welded indices of tri's rows ascend, so rotation 0 has b < c: side 0)
    copies = [tri[list(ROTATIONS[j % 3])] for j in range(n0)] + [tri[list(FLIPS[j % 3])] for j in range(n1)]
    sides = np.array([0] * n0 + [1] * n1 + [-1] * n_other)
    soup = np.concatenate([np.array(copies).reshape(-1, 3, 3), unrelated(n_other)])
    perm = rng.permutation(len(soup))
    soup, sides = soup[perm], sides[perm]
    if n0 == n1:
        return soup, None
    return soup, int(np.flatnonzero(sides == (0 if n0 > n1 else 1))[0])


REPEATS = ((2, 0), (0, 2), (2, 1), (1, 2), (3, 3), (3, 1))


def near_faces():
    """four triangles over six points whose faces are (1, 2, 4), (1, 2, 5), (1, 3, 4) and (0, 2, 4): the first agrees with each of the
    others in two of its three indices -- the smallest two, the smallest and the largest, the largest two -- and two of them are wound
    the other way, so that a merge would cancel.  Nothing merges."""
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 1.0, 0.0], [3.0, 0.0, 1.0], [4.0, 1.0, 1.0], [5.0, 0.5, 0.5]])
    return p[np.array([[1, 2, 4], [5, 2, 1], [4, 3, 1], [2, 4, 0]])]


def long_run(k, n_pad, flipped=0):
    """n_pad unrelated triangles whose vertices all sort before the face's, then one face k times (rotated in turn), the last
    `flipped` of them in the other winding: in the sorted order the run is [n_pad, n_pad + k)"""
    tri = np.array([[0.25, 0.5, 0.75], [0.5, 1.75, 0.25], [1.5, 0.25, 0.5]])
    copies = [tri[list((ROTATIONS if j < k - flipped else FLIPS)[j % 3])] for j in range(k)]
    return np.concatenate([unrelated(n_pad, seed=k), np.array(copies).reshape(k, 3, 3)])


def cube_and_its_flip(seed=2):
    """the cube's 12 triangles and their flipped copies, interleaved and shuffled, every copy in a rotation of its own: (24, 3, 3)"""
    rng = np.random.RandomState(seed)
    cube = measure_ref.cube_soup()
    both = np.concatenate([cube[:, list(ROTATIONS[1])], cube[:, list(FLIPS[2])]])
    return both[rng.permutation(24)]


def mend_cases():
    """name -> (soup (T, 3, 3), expected statistics): the constructed cases"""
    cube = measure_ref.cube_soup()
    sliver = np.array([[cube[0, 0], cube[0, 0], cube[0, 1]], [cube[3, 1], cube[3, 2], cube[3, 1]]])
    out = {
        'empty': (np.zeros((0, 3, 3)), dict(triangles_in=0, triangles_out=0, collapsed=0, duplicates=0, cancelled=0, faces=0)),
        'one': (cube[:1], dict(triangles_in=1, triangles_out=1, collapsed=0, duplicates=0, cancelled=0, faces=1)),
        'all_collapsed': (sliver, dict(triangles_in=2, triangles_out=0, collapsed=2, duplicates=0, cancelled=0, faces=0)),
        'cube': (cube, dict(triangles_in=12, triangles_out=12, collapsed=0, duplicates=0, cancelled=0, faces=12)),
        'cube_and_its_flip': (cube_and_its_flip(), dict(triangles_in=24, triangles_out=0, collapsed=0, duplicates=0, cancelled=24, faces=12)),
        'cube_twice': (np.concatenate([cube, cube[:, [2, 0, 1]]]), dict(triangles_in=24, triangles_out=12, collapsed=0, duplicates=12,
                                                                        cancelled=0, faces=12)),
        'cube_with_slivers': (np.concatenate([sliver[:1], cube, sliver[1:]]), dict(triangles_in=14, triangles_out=12, collapsed=2,
                                                                                  duplicates=0, cancelled=0, faces=12)),
        'near_faces': (near_faces(), dict(triangles_in=4, triangles_out=4, collapsed=0, duplicates=0, cancelled=0, faces=4)),
    }
    for n0, n1 in REPEATS:
        soup, _ = repeated_face(n0, n1)
        out['repeat_%d_%d' % (n0, n1)] = (soup, dict(triangles_in=n0 + n1 + 7, triangles_out=7 + (n0 != n1), collapsed=0,
                                                    duplicates=(n0 + n1 - 1) if n0 != n1 else 0, cancelled=(n0 + n1) if n0 == n1 else 0,
                                                    faces=8))
    return out
