#!/usr/bin/env python3
"""Search for float32 sample pairs on which a one-division marching-cubes vertex lands in another float32 than skimage's
three-division one (tests/mc_cases.py `NEAR_TIES` records the output as literals; NumPy only, minutes on a CPU).

skimage places the vertex of the edge between grid indices i and i + 1 at float32(i + t), t = w_hi / (w_lo + w_hi) with
w = 1 / (eps + |v|): three float64 divisions.  The device's fast path (csrc/sdf_device.h `mc_edge_pos`) takes ONE quotient
t' = a / (a + b), a = eps + |v_lo|, b = eps + |v_hi|, and keeps float32(i + t') wherever float32(q - D) == float32(q + D)
for q = i + t'.  t and t' differ by an ulp of t or two; that decides the float32 only where the float64 sum i + t falls
within half a float64 ulp U / 2 of a float32 tie i + k / 2^m (k odd, 2^-m half the float32 spacing at i): on one side the
sum rounds ONTO the tie, which the float32 cast then rounds to even, on the other it rounds to the tie's float64
neighbour and the cast follows it.  From i = 512 on, D = 2^-44 is at most half an ulp of q and the window sees nothing.

The search: targets t* = k / 2^m -+ U / 2 for the odd k nearest 2^m (there |v_hi| << |v_lo|, and the float32 pairs whose
quotient comes within an ulp of a given t* are dense: an error of 2^-24 in v_hi moves t by 2^-24 (1 - t)).  For every
24-bit a = 2^23 .. 2^24 - 1, b = the float32 nearest rho a, rho = (1 - t*) / t* in np.longdouble.  A pair is kept when
skimage's float32 and the modelled fast path's differ, the quotient modelled three ways: correctly rounded (bit 1 of the
recorded mask), one ulp up (bit 2), one ulp down (bit 4).  Which of the three the hardware's reciprocal, two Newton
steps and final correction deliver is what the GPU test finds out.

For an index below 512 the window does its work and nothing differs; the 32 pairs whose sum comes nearest to a tie are
recorded instead (mask 0): the fast path has to fall back on them.

    python3 tools/find_mc_near_ties.py [index ...]      prints the NEAR_TIES literal
"""
import sys

import numpy as np

EPS = 2.220446049250313e-16
INDICES = (511, 512, 513, 1023, 1024, 2048, 2049, 3001, 4094)
PER_VARIANT = 16        # pairs recorded per (index, variant), ascending in v_lo
MAX_K = 12              # odd k tried per index: 2^m - 1, 2^m - 3, ...
CHUNK = 1 << 21


def skimage_pos(vlo, vhi, i):
    """float32(i + t) by the three divisions, float64 on float32 samples"""
    a, b = EPS + np.abs(vlo), EPS + np.abs(vhi)
    wlo, whi = 1.0 / a, 1.0 / b
    return (i + whi / (wlo + whi)).astype(np.float32)


def fast_pos(vlo, vhi, i, ulps):
    """the modelled fast path: the correctly rounded float64 quotient a / (a + b) moved by `ulps`, the 2^-44 window, the
    fall-back to the three divisions where the window straddles a float32 boundary"""
    a, b = EPS + np.abs(vlo), EPS + np.abs(vhi)
    tq = a / (a + b)
    if ulps:
        tq = np.nextafter(tq, np.inf if ulps > 0 else -np.inf)
    q = i + tq
    f_lo, f_hi = (q - 2.0 ** -44).astype(np.float32), (q + 2.0 ** -44).astype(np.float32)
    return np.where(f_lo == f_hi, f_lo, skimage_pos(vlo, vhi, i))


def candidates(i, k, sign):
    """for every 24-bit a: (a, b) with b the float32 nearest rho a for the target t* = k / 2^m + sign U / 2"""
    e = int(np.floor(np.log2(i)))
    m, U = 24 - e, np.longdouble(2.0) ** (e - 52)
    tstar = np.longdouble(k) / np.longdouble(2 ** m) + sign * U / 2
    rho = (1 - tstar) / tstar
    for start in range(1 << 23, 1 << 24, CHUNK):
        a = np.arange(start, start + CHUNK, dtype=np.float64)
        x = rho * a.astype(np.longdouble)
        _, ex = np.frexp(x)
        b = np.ldexp(np.rint(np.ldexp(x, 24 - ex)), ex - 24).astype(np.float64)
        yield a, b


def search(i):
    e = int(np.floor(np.log2(i)))
    m = 24 - e
    found = {}            # (a, b) -> mask
    near = []
    per_variant = [0, 0, 0]
    for k in range(2 ** m - 1, 2 ** m - 1 - 2 * MAX_K, -2):
        for sign in (-1, 1):
            for a, b in candidates(i, k, sign):
                assert np.array_equal(b.astype(np.float32).astype(np.float64), b)
                ref = skimage_pos(a, b, i)
                mask = np.zeros(len(a), np.int64)
                for bit, ulps in enumerate((0, 1, -1)):
                    mask |= (fast_pos(a, b, i, ulps) != ref).astype(np.int64) << bit
                for j in np.nonzero(mask)[0]:
                    found[(float(a[j]), float(b[j]))] = int(mask[j])
                if i < 512 and k == 2 ** m - 1:
                    t = a.astype(np.longdouble) / (a.astype(np.longdouble) + b.astype(np.longdouble))
                    d = np.abs(t - np.longdouble(k) / np.longdouble(2 ** m)).astype(np.float64)
                    j = np.argsort(d)[:32]
                    near += [(float(d[q]), float(a[q]), float(b[q])) for q in j]
        per_variant = [sum(1 for v in found.values() if v >> bit & 1) for bit in range(3)]
        if i < 512 or min(per_variant) >= PER_VARIANT:
            break
    if i < 512:
        assert not found, 'the window fails below 512: %r' % sorted(found)[:4]
        return [(a, -b, 0) for _, a, b in sorted(set(near))[:32]]
    keep = set()
    for bit in range(3):
        keep |= set(sorted(p for p, v in found.items() if v >> bit & 1)[:PER_VARIANT])
    print('# index %d: %d pairs differ (per variant %r), %d kept' % (i, len(found), per_variant, len(keep)), file=sys.stderr)
    return [(a, -b, found[(a, b)]) for a, b in sorted(keep)]


def main():
    indices = [int(s) for s in sys.argv[1:]] or INDICES
    print('NEAR_TIES = {')
    for i in indices:
        print('    %d: [' % i)
        for vlo, vhi, mask in search(i):
            print('        (%r, %r, %d),' % (vlo, vhi, mask))
        print('    ],')
        sys.stdout.flush()
    print('}')


if __name__ == '__main__':
    main()
