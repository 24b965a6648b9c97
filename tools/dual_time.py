#!/usr/bin/env python3
"""Time dual contouring (sdf_generate_dual; csrc/sdf_dual.hip) next to the marching-cubes path on the same grid, in one run:

    python tools/dual_time.py [--calls 5] [--warmup 2] [--model ex_example] [--half 0.85] [--samples 262144,16777216,134217728]
                              [--no-mc] [--table]

Per sample count, one JSON line: the grid; the median over --calls calls after --warmup of the five phases of one
`Engine.generate_dual` call by HIP events (sdf_generate_dual_last_kernel_ms: sampling through sdf_eval_points; classify + scan +
crossing points + scan; k_vertex_normals at the crossings; cell flags + scan + k_dual_vertex; emission), their sum and the whole
call by the host clock (it ends in a device synchronise); the eight counters; and, unless --no-mc, the marching-cubes path
(`Engine.generate`, batch_size 32, sparse) on the same grid: its `ms_total` by HIP events and the whole call.  The per-KERNEL times
of the same calls come from running this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own.

--table: the comparison of DESIGN.md section 4u on the device -- per model and grid, triangles, the largest and the rms |f| over
corners, edge midpoints and centroids, the volume, the edge census (`Mesh.edge_census`) and the faces against the gradient, for
marching cubes and for dual contouring; the field through `Engine.eval_points`.  Needs an MI355X."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def cube_bounds(half, shift=0.0):
    return ((-half + shift,) * 3, (half + shift,) * 3)


def table(eng, ns):
    import dual_ref as ref
    import fixtures
    from sdf_amd import core
    rows = (('box(1)', ns['box'](1), cube_bounds(0.6, 0.013), 2 ** 15),
            ('ex_example', fixtures.build('ex_example', ns), cube_bounds(0.85), 2 ** 18),
            ('box(1).rotate(0.5, (1, 1, 0) / sqrt 2)', ns['box'](1).rotate(0.5, np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)), cube_bounds(0.95), 2 ** 16))
    for name, f, bounds, samples in rows:
        X, Y, Z, _ = core.grid_axes(bounds, None, samples)
        ev = lambda P: eng.eval_points(f, P)
        for how in ('marching cubes', 'dual'):
            mesh = eng.generate(f, X, Y, Z, 32, True) if how == 'marching cubes' else eng.generate_dual(f, X, Y, Z, core.default_normal_eps(bounds))
            try:
                soup = mesh.points().reshape(-1, 3, 3).copy()
                mesh._welded()
                census = mesh.edge_census()
            finally:
                mesh.close()
            dev = ref.deviation(ev, soup)
            against, faces = ref.against_gradient(ev, soup, min_area=1e-12)
            print(json.dumps({'model': name, 'samples': samples, 'mesher': how, 'triangles': len(soup), 'vertices': int(census['vertices']),
                              'max_deviation': dev[0], 'rms_deviation': dev[1], 'volume': ref.volume(soup), 'closed': bool(census['closed']),
                              'oriented': bool(census['oriented']), 'boundary': int(census['boundary']), 'nonmanifold': int(census['nonmanifold']),
                              'against_gradient': against, 'faces_over_1e-12': faces, 'dual_stats': getattr(mesh, 'dual_stats', None)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--model', default='ex_example')
    ap.add_argument('--half', type=float, default=0.85, help='the bounds are the cube of this half side')
    ap.add_argument('--samples', default='262144,16777216,134217728')
    ap.add_argument('--no-mc', action='store_true', help='without the marching-cubes path')
    ap.add_argument('--table', action='store_true', help='the comparison with marching cubes instead of the timing')
    args = ap.parse_args()

    try:
        import torch
        torch.cuda.is_available()                  # torch's HIP runtime initialises first
    except ImportError:
        pass
    import fixtures
    import sdf_amd
    from sdf_amd import core, engine
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    if args.table:
        return table(eng, ns)
    f = fixtures.build(args.model, ns)
    bounds = cube_bounds(args.half)
    eps = core.default_normal_eps(bounds)
    dt = eng.tape_for(f)
    names = ('sample', 'crossings', 'normals', 'vertices', 'emit')
    for samples in (int(s) for s in args.samples.split(',')):
        X, Y, Z, step = core.grid_axes(bounds, None, samples)
        parts, call_ms = [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            mesh = eng.generate_dual(dt, X, Y, Z, eps)
            wall = (time.perf_counter() - t0) * 1e3
            stats, tris = mesh.dual_stats, mesh.n_triangles
            mesh.close()
            if i >= args.warmup:
                p5 = np.zeros(5)
                lib.sdf_generate_dual_last_kernel_ms(p5.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
                parts.append(p5)
                call_ms.append(wall)
        med = np.median(np.array(parts), axis=0)
        line = {'metric': 'dual contouring: median ms of the phases of one generate_dual call (HIP events) and of the whole call',
                'model': args.model, 'bounds_half': args.half, 'samples': samples, 'grid': [len(X), len(Y), len(Z)], 'calls': args.calls,
                'warmup': args.warmup, 'phase_ms_median': {k: round(float(v), 4) for k, v in zip(names, med)},
                'phases_ms_median': round(float(med.sum()), 4), 'call_ms_median': round(float(np.median(call_ms)), 3),
                'call_ms_min': round(min(call_ms), 3), 'call_ms_max': round(max(call_ms), 3), 'triangles': tris, 'stats': stats}
        if not args.no_mc:
            mc_ms, mc_call = [], []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                mesh = eng.generate(dt, X, Y, Z, 32, True)
                wall = (time.perf_counter() - t0) * 1e3
                st, mc_tris = mesh.stats(), mesh.n_triangles
                mesh.close()
                if i >= args.warmup:
                    mc_ms.append(float(st['ms_total']))
                    mc_call.append(wall)
            line.update(marching_cubes_ms_total_median=round(float(np.median(mc_ms)), 4), marching_cubes_call_ms_median=round(float(np.median(mc_call)), 3),
                        marching_cubes_triangles=mc_tris)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
