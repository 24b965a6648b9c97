#!/usr/bin/env python3
"""Time the indexed export (sdf_mesh_vertex_normals, sdf_mesh_emit_ply_host; csrc/sdf_normals.hip, k_ply_* of csrc/sdf_plain.hip) against
the interpreter's own throughput and against STL, in one run:

    python tools/export_time.py [--calls 12] [--warmup 2] [--models ex_example,ex_gearlike,ex_knurling] [--samples 134217728]
                                 [--no-yardstick] [--no-saves]
    python tools/export_time.py --summarize <rocprofv3 kernel_stats.csv>        # the kernel table of a profiled run, as markdown

Per model, one JSON line: triangles and welded vertices of the mesh at --samples; the median over --calls calls after --warmup of
k_vertex_normals alone by HIP events (sdf_mesh_normals_last_kernel_ms; the calls alternate between two values of eps, so none is
served from the mesh's cache) and vertices/s; the yardstick: ONE `sdf_eval_points` launch of the same tape on 6 U points (uniform in
the bounds, already on the device), wall time around launch + synchronise; `useful_fraction` = (6 U evaluations / kernel time) / (the
yardstick's points / its time); the whole `Mesh.ply_records` call with and without normals (the two packing kernels, one device
allocation, two copies to pinned memory) and the bytes it delivers; and the whole calls `f.save('x.ply')`, `f.save('x.ply',
normals=True)` and `f.save('x.stl')` (native writers, into a temporary directory) with the files' sizes.  The packing kernels' own
times come from a profiled run (`rocprofv3 --kernel-trace --stats -- python tools/export_time.py --no-yardstick --no-saves`, then
--summarize).  Needs an MI355X and torch (for the yardstick's device buffer)."""
import argparse
import csv
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def summarize(path):
    keep = ('k_vertex_normals', 'k_ply_vertices', 'k_ply_faces', 'k_stl', 'k_eval_points', 'k_weld')
    rows = [r for r in csv.DictReader(open(path)) if any(k in r['Name'] for k in keep)]
    print('| kernel | calls | total ms | avg us | min us | max us |')
    print('|---|---|---|---|---|---|')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        print('| `%s` | %d | %.3f | %.1f | %.1f | %.1f |' % (r['Name'].split('(')[0], int(r['Calls']), float(r['TotalDurationNs']) / 1e6,
                                                         float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))


def median_ms(fn, calls, warmup):
    ms = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn(i)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_gearlike,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--no-yardstick', action='store_true', help='the export alone (a profiled run)')
    ap.add_argument('--no-saves', action='store_true', help='without the whole save calls')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    import torch
    torch.cuda.is_available()                      # torch's HIP runtime initialises first
    import fixtures
    import sdf_amd
    from sdf_amd import core, engine
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
        eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
        X, Y, Z, _ = core.grid_axes(bounds, samples=args.samples)
        dt_ = eng.tape_for(f)
        mesh = eng.generate(dt_, X, Y, Z, 32, True)
        try:
            t0 = time.perf_counter()
            nu = mesh._welded()
            weld_ms = (time.perf_counter() - t0) * 1e3
            t = mesh.n_triangles
            flat = ctypes.c_int64(0)
            kern = []

            def normals(i):
                rc = lib.sdf_mesh_vertex_normals(mesh.handle, dt_.handle, eps * (1.0 + 0.001 * (i & 1)), None, ctypes.byref(flat))
                if rc:
                    raise RuntimeError(lib.sdf_last_error().decode())
                if i >= args.warmup:
                    kern.append(lib.sdf_mesh_normals_last_kernel_ms())
            call_ms = median_ms(normals, args.calls, args.warmup)
            k_ms = float(np.median(kern))
            line = {'metric': 'indexed export: median ms of k_vertex_normals alone (HIP events) and of the whole calls', 'model': name,
                    'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'vertices': nu, 'n_flat': int(flat.value),
                    'weld_ms_first_call': round(weld_ms, 3), 'normals_call_ms_median': round(call_ms, 3), 'kernel_ms_median': round(k_ms, 4),
                    'kernel_ms_min': round(min(kern), 4), 'kernel_ms_max': round(max(kern), 4), 'vertices_per_s': round(nu / (k_ms * 1e-3)),
                    'evals_per_s': round(6 * nu / (k_ms * 1e-3))}
            for wn in (False, True):
                ms = median_ms(lambda i: mesh.ply_records(normals=wn), args.calls, args.warmup)
                nbytes = nu * (24 if wn else 12) + 13 * t
                line['ply_records%s_call_ms_median' % ('_normals' if wn else '')] = round(ms, 3)
                line['ply_records%s_bytes' % ('_normals' if wn else '')] = nbytes
                line['ply_records%s_call_GBps' % ('_normals' if wn else '')] = round(nbytes / (ms * 1e-3) / 1e9, 2)
            ms = median_ms(lambda i: mesh.stl_records(), args.calls, args.warmup)
            line.update({'stl_records_call_ms_median': round(ms, 3), 'stl_records_bytes': 50 * t})
        finally:
            mesh.close()
        if not args.no_yardstick:
            n = 6 * nu
            tlo, thi = (torch.tensor(b, dtype=torch.float64, device='cuda') for b in bounds)
            pts = tlo + torch.rand((n, 3), dtype=torch.float64, device='cuda') * (thi - tlo)
            out = torch.empty(n, dtype=torch.float64, device='cuda')
            torch.cuda.synchronize()

            def yard(i):
                rc = lib.sdf_eval_points(dt_.handle, ctypes.c_void_p(pts.data_ptr()), n, 3, ctypes.c_void_p(out.data_ptr()), eng.precision)
                eng.synchronize()
                if rc:
                    raise RuntimeError(lib.sdf_last_error().decode())
            y_ms = median_ms(yard, args.calls, args.warmup)
            line.update({'yardstick': 'sdf_eval_points on 6 U uniform points in the bounds, wall ms around launch + synchronise',
                         'yardstick_ms_median': round(y_ms, 4), 'yardstick_points_per_s': round(n / (y_ms * 1e-3)),
                         'useful_fraction': round(y_ms / k_ms, 3)})
            del pts, out
        if not args.no_saves:
            with tempfile.TemporaryDirectory() as d:
                for key, fname, kw in (('save_ply', 'x.ply', dict(writer='native')), ('save_ply_normals', 'x.ply', dict(writer='native', normals=True)),
                                       ('save_stl', 'x.stl', {})):
                    path = os.path.join(d, fname)
                    ms = median_ms(lambda i: f.save(path, bounds=bounds, samples=args.samples, verbose=False, **kw), max(args.calls // 4, 3), 1)
                    line[key + '_ms_median'] = round(ms, 2)
                    line[key + '_file_bytes'] = os.path.getsize(path)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
