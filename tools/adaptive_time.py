#!/usr/bin/env python3
"""Time the simplification of a mesh to a tolerance on the device (sdf_mesh_simplify_adaptive; csrc/sdf_simplify.hip) in one run:

    python tools/adaptive_time.py [--calls 8] [--warmup 2] [--models ex_example] [--samples 134217728] [--levels 5]
                                  [--tolerances 0.05,0.1] [--simplify 1] [--uniform 4]

Per model, one JSON line for the unsimplified mesh (triangles, welded vertices, volume), one per tolerance (given in grid steps) and
one for the uniform `simplify=--uniform` on the same welded mesh: surviving triangles, the volume of the result, the statistics, and
the median over --calls calls after --warmup of the kernels by HIP events -- per level for the tolerance (a level is box, keys, sort,
numbering, items, item sort, k_cluster_vertex with the error walk, k_adaptive_choose and k_adaptive_count) plus live + emit -- and of
the whole call.  Needs an MI355X."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--tolerances', default='0.05,0.1', help='in grid steps')
    ap.add_argument('--simplify', type=float, default=1.0, help='the finest cluster, in grid cells')
    ap.add_argument('--uniform', type=float, default=4.0, help='the uniform simplify= to compare with')
    args = ap.parse_args()

    import fixtures
    import sdf_amd
    from sdf_amd import core, engine, simplify
    from sdf_amd.measure import measure_mesh
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
            nu = mesh._welded()
            head = {'model': name, 'samples': args.samples, 'step': step[0], 'calls': args.calls, 'warmup': args.warmup}
            print(json.dumps(dict(head, metric='the unsimplified mesh', triangles=mesh.n_triangles, vertices=nu,
                                  volume=measure_mesh(mesh).volume)), flush=True)
            origin, cell = simplify.resolve_cell(args.simplify, X, Y, Z, step)
            for tol in [float(t) for t in args.tolerances.split(',')]:
                levels, emit, wall, stats, volume = [], [], [], None, None
                for i in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    small = mesh.simplify_adaptive(origin, cell, tol * step[0], args.levels)
                    dt = (time.perf_counter() - t0) * 1e3
                    p = (ctypes.c_double * (args.levels + 1))()
                    total = lib.sdf_mesh_simplify_adaptive_last_kernel_ms(p)
                    stats = small.simplify_stats
                    if i == 0:
                        volume = measure_mesh(small).volume
                    small.close()
                    if i >= args.warmup:
                        levels.append(list(p)); emit.append(total - sum(p)); wall.append(dt)
                levels = np.array(levels)
                line = dict(head, metric='to a tolerance: median ms of the kernels per level (HIP events) and of the whole call', simplify=args.simplify,
                            levels=args.levels, tolerance_steps=tol, level_ms_median=[med(levels[:, k]) for k in range(args.levels + 1)],
                            live_emit_ms_median=med(emit), kernels_ms_median=med(levels.sum(axis=1) + np.array(emit)),
                            call_ms_median=med(wall), volume=volume)
                line.update({k: v for k, v in stats.items() if k != 'kernel_ms'})
                print(json.dumps(line), flush=True)
            origin, cell = simplify.resolve_cell(args.uniform, X, Y, Z, step)
            parts, wall, stats, volume = [], [], None, None
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                small = mesh.simplify(origin, cell)
                dt = (time.perf_counter() - t0) * 1e3
                p = (ctypes.c_double * 4)()
                lib.sdf_mesh_simplify_last_kernel_ms(p)
                stats = small.simplify_stats
                if i == 0:
                    volume = measure_mesh(small).volume
                small.close()
                if i >= args.warmup:
                    parts.append(sum(p)); wall.append(dt)
            line = dict(head, metric='uniform: median ms of the kernels (HIP events) and of the whole call', simplify=args.uniform,
                        kernels_ms_median=med(parts), call_ms_median=med(wall), volume=volume)
            line.update({k: v for k, v in stats.items() if k != 'kernel_ms'})
            print(json.dumps(line), flush=True)
        finally:
            mesh.close()


if __name__ == '__main__':
    main()
