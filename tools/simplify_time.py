#!/usr/bin/env python3
"""Time the simplification of a mesh on the device (sdf_mesh_simplify; csrc/sdf_simplify.hip) in one run:

    python tools/simplify_time.py [--calls 12] [--warmup 2] [--models ex_example,ex_gearlike,ex_knurling] [--samples 134217728]
                                   [--saves 3] [--no-numpy]

Per model and per simplify in (2, 4), one JSON line: triangles and welded vertices of the mesh at --samples, clusters and surviving
triangles, the two counters; the median over --calls calls after --warmup, on one mesh welded beforehand, of the kernels by HIP events
split into keys + numbering (k_cluster_box, the host's look at the box, k_cluster_keys, the sort over U, flags, scan, k_cluster_number),
the item sort (k_cluster_items, the sort over 3T, k_item_starts), k_cluster_vertex, and live + emit (k_cluster_live, the scan,
k_cluster_emit), and of the whole `Mesh.simplify` call; the NumPy definition (tests/simplify_ref.py) on the same weld, once, with
whether the device agrees bit for bit.  Then one line per model for `save('x.ply')` and `save('x.stl')` with and without simplify=4:
median seconds of --saves calls after one, and the file sizes.  Needs an MI355X."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_gearlike,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--saves', type=int, default=3)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition (a profiled run)')
    args = ap.parse_args()

    import fixtures
    import simplify_ref
    import sdf_amd
    from sdf_amd import core, engine, simplify
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        tape = eng.tape_for(f)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        mesh = eng.generate(tape, X, Y, Z, 32, True)
        try:
            t0 = time.perf_counter()
            nu = mesh._welded()
            weld_ms = (time.perf_counter() - t0) * 1e3
            for k in (2, 4):
                origin, cell = simplify.resolve_cell(k, X, Y, Z, step)
                parts, wall, stats = [], [], None
                for i in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    small = mesh.simplify(origin, cell)
                    dt = (time.perf_counter() - t0) * 1e3
                    p = (ctypes.c_double * 4)()
                    lib.sdf_mesh_simplify_last_kernel_ms(p)
                    stats = small.simplify_stats
                    if i == args.warmup + args.calls - 1 and not args.no_numpy and k == 4:
                        got = small.points().copy()
                    small.close()
                    if i >= args.warmup:
                        parts.append(list(p)); wall.append(dt)
                parts = np.array(parts)
                line = {'metric': 'mesh simplification: median ms of the kernels (HIP events) and of the whole call', 'model': name,
                        'samples': args.samples, 'simplify': k, 'calls': args.calls, 'warmup': args.warmup, 'triangles': mesh.n_triangles,
                        'vertices': nu, 'weld_ms_first_call': round(weld_ms, 3),
                        'keys_numbering_ms_median': med(parts[:, 0]), 'item_sort_ms_median': med(parts[:, 1]),
                        'cluster_vertex_ms_median': med(parts[:, 2]), 'live_emit_ms_median': med(parts[:, 3]),
                        'kernels_ms_median': med(parts.sum(axis=1)), 'kernels_ms_min': round(float(parts.sum(axis=1).min()), 4),
                        'kernels_ms_max': round(float(parts.sum(axis=1).max()), 4), 'simplify_call_ms_median': med(wall)}
                line.update({key: stats[key] for key in simplify_ref.STAT_KEYS})
                if not args.no_numpy and k == 4:
                    pts, cells = mesh.weld()
                    t0 = time.perf_counter()
                    want = simplify_ref.simplify(pts, cells, origin, cell)
                    line['numpy_simplify_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                    line['identical_to_numpy'] = bool(got.shape == (3 * len(want.soup), 3) and np.array_equal(
                        got.view(np.int64), want.soup.reshape(-1, 3).view(np.int64)) and
                        all(stats[key] == want.stats[key] for key in simplify_ref.STAT_KEYS))
                    del pts, cells, want, got
                print(json.dumps(line), flush=True)
        finally:
            mesh.close()
        line = {'metric': 'save with and without simplify=4: median seconds and file sizes', 'model': name, 'samples': args.samples,
                'saves': args.saves}
        with tempfile.TemporaryDirectory() as d:
            for ext in ('ply', 'stl'):
                for k in (None, 4):
                    path = os.path.join(d, 'x.' + ext)
                    s = []
                    for i in range(1 + args.saves):
                        t0 = time.perf_counter()
                        f.save(path, bounds=bounds, samples=args.samples, simplify=k, verbose=False, **({'writer': 'native'} if ext == 'ply' else {}))
                        s.append(time.perf_counter() - t0)
                    tag = ext + ('_simplify4' if k else '')
                    line['save_%s_s_median' % tag] = round(float(np.median(s[1:])), 4)
                    line['size_%s_bytes' % tag] = os.path.getsize(path)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
