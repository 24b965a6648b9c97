#!/usr/bin/env python3
"""Time the measurements of a mesh (sdf_mesh_moments, sdf_mesh_edge_census; csrc/sdf_measure.hip) in one run:

    python tools/measure_time.py [--calls 12] [--warmup 2] [--models ex_example,ex_gearlike,ex_knurling] [--samples 134217728]
                                  [--no-numpy]
    python tools/measure_time.py --summarize <rocprofv3 kernel_stats.csv>        # the kernel table of a profiled run, as markdown

Per model, one JSON line: triangles and welded vertices of the mesh at --samples; the median over --calls calls after --warmup of
the kernels of sdf_mesh_moments by HIP events (sdf_mesh_measure_last_kernel_ms: k_soup_box + k_soup_moments + k_moment_partials, two
passes over the soup) and that time as a fraction of the HBM roof bench.py --full uses (8000 GB/s) over 2 x 72 B per triangle; the
same with an explicit origin; the kernels of sdf_mesh_edge_census (k_edge_keys + the radix sort + k_edge_classes); the weld's first
call; both whole calls; the whole `f.measure(...)`; and the NumPy definition (tests/measure_ref.py) on the same soup, once.  The
split between k_soup_box and k_soup_moments comes from a profiled run (`rocprofv3 --kernel-trace --stats -- python
tools/measure_time.py --no-numpy`, then --summarize).  Needs an MI355X."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
HBM_PEAK_GBS = 8000.0          # bench.py's roof


def summarize(path):
    keep = ('k_soup_box', 'k_soup_moments', 'k_moment_partials', 'k_edge_keys', 'k_edge_classes', 'k_weld', 'rocprim', 'k_mesh')
    rows = [r for r in csv.DictReader(open(path)) if any(k in r['Name'] for k in keep)]
    print('| kernel | calls | total ms | avg us | min us | max us |')
    print('|---|---|---|---|---|---|')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        print('| `%s` | %d | %.3f | %.1f | %.1f | %.1f |' % (r['Name'].split('(')[0][:90], int(r['Calls']), float(r['TotalDurationNs']) / 1e6,
                                                         float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))


def timed(fn, kernel_ms, calls, warmup):
    """(median wall ms of the call, median / min / max of the kernels' ms)"""
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
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_gearlike,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition (a profiled run)')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    import fixtures
    import measure_ref
    import sdf_amd
    from sdf_amd import core, engine
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, _ = core.grid_axes(bounds, samples=args.samples)
        mesh = eng.generate(eng.tape_for(f), X, Y, Z, 32, True)
        try:
            t = mesh.n_triangles
            t0 = time.perf_counter()
            nu = mesh._welded()
            weld_ms = (time.perf_counter() - t0) * 1e3
            m_wall, m_k, m_min, m_max = timed(mesh.moments, lib.sdf_mesh_measure_last_kernel_ms, args.calls, args.warmup)
            o_wall, o_k, _, _ = timed(lambda: mesh.moments(origin=(0.0, 0.0, 0.0)), lib.sdf_mesh_measure_last_kernel_ms, args.calls, args.warmup)
            c_wall, c_k, c_min, c_max = timed(mesh.edge_census, lib.sdf_mesh_measure_last_kernel_ms, args.calls, args.warmup)
            got, census = mesh.moments(), mesh.edge_census()
            line = {'metric': 'mesh measurements: median ms of the kernels (HIP events) and of the whole calls', 'model': name,
                    'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'vertices': nu,
                    'soup_bytes': 72 * t, 'weld_ms_first_call': round(weld_ms, 3),
                    'moments_kernels_ms_median': round(m_k, 4), 'moments_kernels_ms_min': round(m_min, 4), 'moments_kernels_ms_max': round(m_max, 4),
                    'moments_kernels_GBps_over_144B': round(144e-6 * t / m_k, 1), 'moments_frac_of_hbm_roof_over_144B': round(144e-6 * t / m_k / HBM_PEAK_GBS, 4),
                    'moments_call_ms_median': round(m_wall, 4), 'moments_origin_kernels_ms_median': round(o_k, 4), 'moments_origin_call_ms_median': round(o_wall, 4),
                    'census_kernels_ms_median': round(c_k, 4), 'census_kernels_ms_min': round(c_min, 4), 'census_kernels_ms_max': round(c_max, 4),
                    'census_call_ms_median': round(c_wall, 4), 'census_keys_per_s': round(3 * t / (c_k * 1e-3)),
                    'census': census, 'volume': float(measure_ref.derive(got)['volume']), 'area': float(measure_ref.derive(got)['area'])}
            if not args.no_numpy:
                soup = mesh.points().reshape(-1, 3, 3)
                pts, cells = mesh.weld()
                t0 = time.perf_counter()
                want = measure_ref.moments(soup)
                line['numpy_moments_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                t0 = time.perf_counter()
                want_census = measure_ref.edge_census(cells, len(pts))
                line['numpy_census_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                line['bit_identical_to_numpy'] = bool(np.array_equal(want['sums'].view(np.int64), got['sums'].view(np.int64)) and
                                                      np.array_equal(want['box'], got['box']) and want_census == census)
                del soup, pts, cells
        finally:
            mesh.close()
        ms = []
        for i in range(1 + max(args.calls // 4, 3)):
            t0 = time.perf_counter()
            f.measure(bounds=bounds, samples=args.samples, verbose=False)
            ms.append((time.perf_counter() - t0) * 1e3)
        line['measure_call_ms_median'] = round(float(np.median(ms[1:])), 3)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
