#!/usr/bin/env python3
"""Time the rating of build directions (sdf_mesh_overhangs, sdf_mesh_overhang_classes; csrc/sdf_overhang.hip) in one run:

    python tools/overhang_time.py [--calls 8] [--warmup 2] [--model ex_example] [--samples 134217728] [--directions 1,6,262,2054]
                                   [--numpy-directions 6] [--no-numpy]

Per direction count K, one JSON line: the triangles of the mesh at --samples; the median, minimum and maximum over --calls calls
after --warmup of the kernels of sdf_mesh_overhangs by HIP events (sdf_overhang_last_kernel_ms: k_overhang_init +
k_overhang_extents + k_overhang_terms + k_overhang_partials, all slabs) and the slabs it took; triangle-direction pairs per second;
that rate as float64 operations per second over the operations the definition writes per pair (OPS_PER_PAIR) and as a share of the
float64 vector peak (F64_VECTOR_PEAK_TFLOPS); and the whole call.  K = 1 is the single direction (0, 0, 1); K = 6 the axes; larger
K the axes and K - 6 spiral points (`sphere_directions`).  Then one line for the classes of one direction, and -- unless --no-numpy
-- one for the NumPy definition (tests/overhang_ref.py) on the same soup with --numpy-directions directions, once, with a check
that the device gave the same bits.  Needs an MI355X."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
# the MI355X's float64 vector peak as AMD publishes it, half of the 157.3 TFLOPS float32 vector peak; it counts a fused multiply-add as
# two operations, and this kernel may not fuse (one rounding per written operation), so half of it is the most it can reach
F64_VECTOR_PEAK_TFLOPS = 78.6
# what tests/overhang_ref.py writes per triangle and direction: three h (3 mul + 2 add + 1 sub each), dn (3 mul + 2 add), the sum of
# the three heights (2), (-dn) * sum (1), three accumulations (3) -- 29 -- without the comparisons, the maxima and the selects
OPS_PER_PAIR = 29


def timed(fn, kernel_ms, calls, warmup):
    wall, kern = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(kernel_ms())
    return float(np.median(wall)), float(np.median(kern)), min(kern), max(kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--model', default='ex_example')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--directions', default='1,6,262,2054')
    ap.add_argument('--numpy-directions', type=int, default=6)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition')
    args = ap.parse_args()

    import fixtures
    import overhang_ref
    import sdf_amd
    from sdf_amd import core, engine, overhang
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    f = fixtures.build(args.model, ns)
    bounds = eng.estimate_bounds(f)
    X, Y, Z, steps = core.grid_axes(bounds, samples=args.samples)
    sin_limit, tol = overhang.sin_limit_of(45.0), float(max(steps))
    mesh = eng.generate(eng.tape_for(f), X, Y, Z, 32, True)
    try:
        t = mesh.n_triangles
        for k in (int(v) for v in args.directions.split(',')):
            d = overhang.normalise(overhang.UP) if k == 1 else overhang.sphere_directions(k - 6)
            slabs = ctypes.c_int64(0)
            wall, k_ms, k_min, k_max = timed(lambda: mesh.overhangs(d, sin_limit, tol), lambda: lib.sdf_overhang_last_kernel_ms(ctypes.byref(slabs)),
                                             args.calls, args.warmup)
            pairs = float(t) * len(d)
            r = mesh.overhangs(d, sin_limit, tol)
            v = overhang.derive(r)
            best = int(np.argmin(v['support_volume']))
            print(json.dumps({
                'metric': 'build directions rated: median ms of the kernels (HIP events) and of the whole call', 'model': args.model,
                'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'directions': len(d), 'slabs': int(slabs.value),
                'pairs': pairs, 'kernels_ms_median': round(k_ms, 4), 'kernels_ms_min': round(k_min, 4), 'kernels_ms_max': round(k_max, 4),
                'call_ms_median': round(wall, 4), 'pairs_per_s': round(pairs / (k_ms * 1e-3)),
                'f64_tflops_over_%d_ops_per_pair' % OPS_PER_PAIR: round(pairs * OPS_PER_PAIR / (k_ms * 1e-3) / 1e12, 3),
                'share_of_f64_vector_peak': round(pairs * OPS_PER_PAIR / (k_ms * 1e-3) / 1e12 / F64_VECTOR_PEAK_TFLOPS, 4),
                'bed_tolerance': tol, 'best_direction': d[best].tolist(), 'best_support_volume': float(v['support_volume'][best]),
                'up_support_volume': float(v['support_volume'][0 if k == 1 else 4])}), flush=True)
        c_wall, c_ms, c_min, c_max = timed(lambda: mesh.overhang_classes(overhang.UP, sin_limit, tol), lambda: lib.sdf_overhang_last_kernel_ms(None),
                                           args.calls, args.warmup)
        print(json.dumps({'metric': 'overhang classes of one direction: median ms of the kernels (k_overhang_extents + k_overhang_classes) '
                                    'and of the whole call, which brings one byte per triangle to the host', 'triangles': t,
                          'kernels_ms_median': round(c_ms, 4), 'kernels_ms_min': round(c_min, 4), 'kernels_ms_max': round(c_max, 4),
                          'call_ms_median': round(c_wall, 4)}), flush=True)
        if not args.no_numpy:
            d = overhang.sphere_directions(args.numpy_directions - 6) if args.numpy_directions >= 6 else overhang.normalise(overhang.UP)
            got = mesh.overhangs(d, sin_limit, tol)
            soup = mesh.points().reshape(-1, 3, 3)
            t0 = time.perf_counter()
            want = overhang_ref.rate(soup, d, sin_limit, tol)
            ms = (time.perf_counter() - t0) * 1e3
            same = all(np.array_equal(np.ascontiguousarray(got[key]).view(np.int64), np.ascontiguousarray(want[key]).view(np.int64))
                       for key in ('lo', 'hi', 'sums', 'overhang_triangles', 'contact_triangles'))
            print(json.dumps({'metric': 'the NumPy definition (tests/overhang_ref.py::rate) on the same soup, once', 'triangles': t,
                              'directions': len(d), 'numpy_ms': round(ms, 1), 'numpy_ms_per_direction': round(ms / len(d), 1),
                              'bit_identical_to_numpy': bool(same)}), flush=True)
    finally:
        mesh.close()


if __name__ == '__main__':
    main()
