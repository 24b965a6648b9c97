"""The definition of the support rays, in NumPy over an evaluator `ev(P) -> (N,) float64` that the caller passes:
the CPU checker (`oracle.evaluate`) or the device interpreter (`Engine.eval_points`).  For a triangle soup in the field of a model
and ONE build direction d ("up": the bed lies below the part), from the centroid of every overhanging face a ray is sphere-traced
DOWNWARD, along -d, through the air until it meets the part or the bed plane; the ray's length is the height of the support column
under that face.  csrc/sdf_supports.hip (k_support_rays) and the sums of csrc/sdf_overhang.hip reproduce `supports` bit for bit;
sdf_amd/supports.py (`support_rays_host`) restates it for the host path.

All arithmetic is float64 with one rounding per written operation: a product and a sum are two operations, a dot product is
(x*x' + y*y') + z*z', a point on a ray is c + t * nd.  No np.dot and no np.sum over the triangles (measure_ref.py says why).

WHICH FACES: exactly overhang_ref.rate(soup, d[None], sin_limit, bed_tol, classes=True).  The rays are the triangles of class
OVERHANG in ascending triangle index, M of them; `triangle` (M,) int32 holds their indices; lo, hi are that rating's; n and dn are
as there and proj = -dn > 0 is the doubled area of the face projected on the bed.
ORIGIN: the centroid, per coordinate ((a + b) + c) / 3.0.  nd = -d.  tb = max(((cx dx + cy dy) + cz dz) - lo, 0.0) -- written
h > 0 ? h : +0.0 -- is the distance to the bed plane.
MARCH: t = start, the bracket lo_t = 0, hi_t unset, steps = 0.  start >= tb: BED (0), height = tb, no evaluation.  Otherwise at most
max_steps passes, each with v = ev(c + t nd) and steps += 1:  v NaN: NAN (4), height NaN.  v < 0 (inside, strictly): hi_t = t -- on
the first pass BURIED (2), height = +0.0: the face has material `start` below it (a face inside a union, the chord error at a concave
corner, a near-vertical face); on a later pass PART (1).  Otherwise lo_t = t and t += max(v * step_scale, min_step); if now
t >= tb: BED, height = tb.  A ray still marching after max_steps passes is UNRESOLVED (3), height = tb: an upper bound, and counted.
REFINE: the bracket of a PART ray is bisected `refine` times: mid = 0.5 * (lo_t + hi_t); ev(c + mid nd) < 0 moves hi_t, anything
else (NaN included) moves lo_t; height = hi_t: inside, and within bracket * 2^-refine of the crossing.  By construction
height <= tb for every ray that is not NAN.
TERMS, five columns per ray, all >= +0.0:  proj*height if BED or UNRESOLVED else +0.0;  proj*height if PART;  proj if PART;  proj;
proj if BURIED.  (A NAN ray adds +0.0 to the first two.)  THE SUMS are overhang_ref.chunk_tree_sum over THE M RAYS IN THEIR ORDER --
chunks of 1024 consecutive RAYS with one sequential accumulator each, then the 256-wide halving tree: the order is over the rays,
not over all the triangles of the soup.  `derive`: on_bed_volume = s0 / 2, on_part_volume = s1 / 2, support_volume = (s0 + s1) / 2,
touch_area = s2 / 2 (the projected area where supports scar the part), projected_area = s3 / 2, buried_area = s4 / 2,
height = hi - lo.  counts (5,) int64 per status.  M = 0 gives zeros and no evaluation (T = 0 and a soup with no finite triangle,
where lo, hi = +inf, -inf, among them).

WHAT THE FIGURE IS NOT.  One ray per face, from its centroid: first-order quadrature, and a face that is partly over the part is
all or nothing.  A gap narrower than min_step can be stepped over.  The support columns are vertical: no tree supports, no draft
angle.  With `angle` near 0 many near-vertical faces are BURIED (knurling at angle 0: 40 % of its rays on the checker), which is why
buried_area is reported.  A field that overestimates distance wants step_scale < 1."""
import numpy as np

import overhang_ref

BED, PART, BURIED, UNRESOLVED, NAN = 0, 1, 2, 3, 4
_MARCH = 5                                   # (inside the march only)
NAMES = ('BED', 'PART', 'BURIED', 'UNRESOLVED', 'NAN')
N_SUMS = 5


def bits(a):
    """the bit patterns of an array (float64 -> int64): what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def rays_of(soup, d, sin_limit, bed_tol):
    """(triangle (M,) int32, origin (M, 3), proj (M,), tb (M,), lo, hi) for one unit direction d, used as given"""
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(3)
    r = overhang_ref.rate(soup, d[None], sin_limit, bed_tol, classes=True)
    lo, hi = float(r['lo'][0]), float(r['hi'][0])
    tri, n, _, _ = overhang_ref.triangle_parts(soup)
    idx = np.flatnonzero(r['classes'][0] == overhang_ref.OVERHANG).astype(np.int32)
    a, b, c = tri[idx, 0], tri[idx, 1], tri[idx, 2]
    n = n[idx]
    dn = (n[:, 0] * d[0] + n[:, 1] * d[1]) + n[:, 2] * d[2]
    proj = -dn
    origin = ((a + b) + c) / 3.0
    h = ((origin[:, 0] * d[0] + origin[:, 1] * d[1]) + origin[:, 2] * d[2]) - lo
    tb = np.where(h > 0.0, h, 0.0)
    return idx, origin, proj, tb, lo, hi


def supports(ev, soup, d, sin_limit, bed_tol, start, min_step, step_scale=1.0, max_steps=256, refine=16):
    """dict of triangle (M,) int32, height (M,) float64, status (M,) uint8, steps (M,) int32, origin (M, 3) float64, tb (M,),
    proj (M,), terms (M, 5), sums (5,), counts (5,) int64, lo, hi for ONE unit direction d"""
    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), np.float64).reshape(-1)

    d = np.ascontiguousarray(d, dtype=np.float64).reshape(3)
    start, min_step, step_scale = np.float64(start), np.float64(min_step), np.float64(step_scale)
    idx, origin, proj, tb, lo, hi = rays_of(soup, d, sin_limit, bed_tol)
    M = len(idx)
    nd = -d
    t = np.full(M, start)
    lo_t, hi_t = np.zeros(M), np.full(M, start)
    height = np.zeros(M)
    steps = np.zeros(M, np.int32)
    status = np.full(M, _MARCH, np.int32)
    bed = start >= tb
    status[bed] = BED
    height[bed] = tb[bed]
    for k in range(int(max_steps)):
        m = np.flatnonzero(status == _MARCH)
        if not len(m):
            break
        v = f(origin[m] + t[m][:, None] * nd)
        steps[m] += 1
        nan = v != v
        inside = ~nan & (v < 0)
        go = ~nan & ~inside
        status[m[nan]] = NAN
        height[m[nan]] = np.nan
        status[m[inside]] = BURIED if k == 0 else PART
        hi_t[m[inside]] = t[m[inside]]
        g = m[go]
        lo_t[g] = t[g]
        adv = v[go] * step_scale
        t[g] = t[g] + np.where(adv > min_step, adv, min_step)
        down = g[t[g] >= tb[g]]
        status[down] = BED
        height[down] = tb[down]
    left = status == _MARCH
    status[left] = UNRESOLVED
    height[left] = tb[left]
    r = np.flatnonzero(status == PART)
    for _ in range(int(refine)):
        if not len(r):
            break
        mid = 0.5 * (lo_t[r] + hi_t[r])
        inside = f(origin[r] + mid[:, None] * nd) < 0
        hi_t[r[inside]] = mid[inside]
        lo_t[r[~inside]] = mid[~inside]                 # (NaN included)
    height[r] = hi_t[r]
    with np.errstate(invalid='ignore'):
        ph = proj * height
    zero = np.zeros(M)
    part, buried = status == PART, status == BURIED
    terms = np.stack([np.where((status == BED) | (status == UNRESOLVED), ph, zero), np.where(part, ph, zero), np.where(part, proj, zero),
                      proj, np.where(buried, proj, zero)], axis=1) if M else np.zeros((0, N_SUMS))
    return {'triangle': idx, 'height': height, 'status': status.astype(np.uint8), 'steps': steps, 'origin': origin, 'tb': tb, 'proj': proj,
            'terms': terms, 'sums': overhang_ref.chunk_tree_sum(terms), 'counts': np.bincount(status, minlength=5)[:5].astype(np.int64),
            'lo': lo, 'hi': hi}


def derive(r):
    """the volumes and areas from the raw sums of one direction: the factor 1/2 meets the totals here, once"""
    s = np.asarray(r['sums'], dtype=np.float64).reshape(N_SUMS)
    with np.errstate(all='ignore'):
        return {'on_bed_volume': s[0] / 2.0, 'on_part_volume': s[1] / 2.0, 'support_volume': (s[0] + s[1]) / 2.0, 'touch_area': s[2] / 2.0,
                'projected_area': s[3] / 2.0, 'buried_area': s[4] / 2.0, 'height': np.float64(r['hi']) - np.float64(r['lo'])}


def lockstep_share(steps, wave=64):
    """sum(steps) / (wave * sum over runs of `wave` rays, in ray order, of the run's largest step count): the share of a wave's march
    evaluations that a ray still needed"""
    steps = np.asarray(steps)
    total = sum(int(steps[i:i + wave].max()) for i in range(0, len(steps), wave))
    return float(steps.sum()) / (wave * total) if total else 1.0
