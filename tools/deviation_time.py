#!/usr/bin/env python3
"""Time the deviation of a mesh from its field and the snap of its vertices (sdf_mesh_triangle_deviation, sdf_mesh_snap;
csrc/sdf_deviation.hip) next to k_vertex_normals on the same mesh, in one run:

    python tools/deviation_time.py [--calls 8] [--warmup 2] [--models ex_example] [--samples 134217728] [--simplify 4] [--order 2]

Per model and per mesh -- plain, and after simplify= --, one JSON line: triangles and welded vertices; the median over --calls calls
after --warmup of k_vertex_normals alone by HIP events (sdf_mesh_normals_last_kernel_ms; the calls alternate between two values of
eps, so none is served from the mesh's cache) -- the yardstick: 6 evaluations per vertex in lockstep --; of k_triangle_deviation alone
(sdf_mesh_deviation_last_kernel_ms) at --order, S evaluations per triangle, with its evaluations per second and their ratio to the
yardstick's; of k_vertex_snap alone (the statistics' kernel_ms) with the defaults of `snap=True`, with the status counts, the
evaluations the vertices needed, those the waves issued (64 x the largest count of each run of 64 vertices in weld order), the share
needed / issued and both rates; the largest |dev| and the rms before and after the snap; the whole `deviation()` call.  Needs an
MI355X."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--simplify', type=float, default=4.0)
    ap.add_argument('--order', type=int, default=2)
    args = ap.parse_args()

    try:
        import torch
        torch.cuda.is_available()                  # torch's HIP runtime initialises first
    except ImportError:
        pass
    import fixtures
    import sdf_amd
    from sdf_amd import core, engine
    from sdf_amd.deviation import STATUS_NAMES, Deviation, snap_params
    from sdf_amd.simplify import resolve_cell
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    n_samples = (args.order + 1) * (args.order + 2) // 2
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        dt_ = eng.tape_for(f)
        full = eng.generate(dt_, X, Y, Z, 32, True)
        small = full.simplify(*resolve_cell(args.simplify, X, Y, Z, step))
        try:
            for label, mesh, cluster in (('plain', full, None), ('simplify=%g' % args.simplify, small, args.simplify)):
                par = snap_params({}, bounds, step, cluster)
                nu, t = mesh._welded(), mesh.n_triangles
                flat = ctypes.c_int64(0)
                k_nrm, k_dev, k_snap = [], [], []
                for i in range(args.warmup + args.calls):
                    rc = lib.sdf_mesh_vertex_normals(mesh.handle, dt_.handle, par['eps'] * (1.0 + 0.001 * (i & 1)), None, ctypes.byref(flat))
                    if rc:
                        raise RuntimeError(lib.sdf_last_error().decode())
                    if i >= args.warmup:
                        k_nrm.append(lib.sdf_mesh_normals_last_kernel_ms())
                for i in range(args.warmup + args.calls):
                    dev, at, sumsq = mesh.triangle_deviation(dt_, args.order)
                    if i >= args.warmup:
                        k_dev.append(lib.sdf_mesh_deviation_last_kernel_ms())
                for i in range(args.warmup + args.calls):
                    moved = mesh.snap(dt_, **par)
                    if i >= args.warmup:
                        k_snap.append(moved.snap_stats['kernel_ms'])
                    if i + 1 < args.warmup + args.calls:
                        moved.close()
                try:
                    status, evals = moved.snap_result[1], moved.snap_evals.astype(np.int64)
                    before = Deviation(*mesh.weld(), dev, at, sumsq, args.order)
                    after = Deviation(*moved.weld(), *moved.triangle_deviation(dt_, args.order), args.order)
                finally:
                    moved.close()
                n_ms, d_ms, s_ms = float(np.median(k_nrm)), float(np.median(k_dev)), float(np.median(k_snap))
                pad = (-nu) % 64
                issued = 64 * int(np.concatenate([evals, np.zeros(pad, np.int64)]).reshape(-1, 64).max(axis=1).sum())
                nrm_rate = 6.0 * nu / (n_ms * 1e-3)
                dev_rate = float(n_samples) * t / (d_ms * 1e-3)
                line = {'metric': 'deviation and snap: median ms of k_triangle_deviation, k_vertex_snap and k_vertex_normals alone (HIP events), same mesh',
                        'model': name, 'mesh': label, 'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'vertices': nu,
                        'order': args.order, 'samples_per_triangle': n_samples,
                        'normals_kernel_ms_median': round(n_ms, 4), 'normals_evals_per_s': round(nrm_rate),
                        'deviation_kernel_ms_median': round(d_ms, 4), 'deviation_kernel_ms_min': round(min(k_dev), 4), 'deviation_kernel_ms_max': round(max(k_dev), 4),
                        'deviation_evals_per_s': round(dev_rate), 'deviation_rate_fraction': round(dev_rate / nrm_rate, 4),
                        'snap_params': {k: (round(v, 9) if isinstance(v, float) else v) for k, v in par.items()},
                        'snap_kernel_ms_median': round(s_ms, 4), 'snap_kernel_ms_min': round(min(k_snap), 4), 'snap_kernel_ms_max': round(max(k_snap), 4),
                        'snap_status': dict(zip(STATUS_NAMES, np.bincount(status, minlength=5).tolist())),
                        'snap_evals_needed': int(evals.sum()), 'snap_evals_issued': issued, 'snap_needed_share': round(float(evals.sum()) / issued, 4),
                        'snap_evals_mean': round(float(evals.mean()), 3), 'snap_evals_max': int(evals.max()),
                        'snap_needed_evals_per_s': round(float(evals.sum()) / (s_ms * 1e-3)), 'snap_issued_evals_per_s': round(issued / (s_ms * 1e-3)),
                        'snap_issued_rate_fraction': round(issued / (s_ms * 1e-3) / nrm_rate, 4),
                        'max_dev_before': before.max, 'rms_before': before.rms, 'inside_max_before': before.inside_max, 'outside_max_before': before.outside_max,
                        'max_dev_after': after.max, 'rms_after': after.rms, 'inside_max_after': after.inside_max, 'outside_max_after': after.outside_max}
                print(json.dumps(line), flush=True)
        finally:
            small.close()
            full.close()
        whole = {}
        for label, kw in (('plain', {}), ('simplify', {'simplify': args.simplify}), ('simplify_snap', {'simplify': args.simplify, 'snap': True})):
            ms = []
            for i in range(3):
                t0 = time.perf_counter()
                got = f.deviation(order=args.order, bounds=bounds, samples=args.samples, verbose=False, **kw)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            whole[label] = {'call_ms': ms, 'max': got.max, 'rms': got.rms}
        print(json.dumps({'metric': 'the whole deviation() call, three times each', 'model': name, 'samples': args.samples, 'order': args.order, 'calls': whole}), flush=True)


if __name__ == '__main__':
    main()
