#!/usr/bin/env python3
"""Time the curvature probe (sdf_mesh_vertex_curvature; csrc/sdf_curvature.hip) next to k_vertex_normals on the same mesh, in one run:

    python tools/curvature_time.py [--calls 8] [--warmup 2] [--models ex_example,ex_knurling] [--samples 134217728] [--no-definition]

Per model, one JSON line: triangles and welded vertices of the mesh at --samples; the median over --calls calls after --warmup of
k_vertex_normals alone by HIP events (sdf_mesh_normals_last_kernel_ms; the calls alternate between two values of eps, so none is
served from the mesh's cache) -- the yardstick: 6 evaluations per vertex in lockstep -- and of k_vertex_curvature alone
(sdf_mesh_curvature_last_kernel_ms) at the default eps of `curvature()`, the smallest grid step: 19 evaluations per vertex in
lockstep, no data-dependent trip count; both kernels' evaluations per second and `rate_fraction`, the curvature kernel's rate over
the normals kernel's (1.0: the kernel costs 19 / 6 of the normals'); the whole `Mesh.vertex_curvature` call; the status counts and
the radii; the whole `f.curvature()` call; and, unless --no-definition, the NumPy definition (tests/curvature_ref.py) over
`Engine.eval_points` on the same vertices, once, with whether the device result is bit-identical to it.  Needs an MI355X."""
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
    ap.add_argument('--models', default='ex_example,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--no-definition', action='store_true', help='without the NumPy definition over eval_points')
    args = ap.parse_args()

    try:
        import torch
        torch.cuda.is_available()                  # torch's HIP runtime initialises first
    except ImportError:
        pass
    import curvature_ref as ref
    import fixtures
    import sdf_amd
    from sdf_amd import core, engine
    from sdf_amd.curvature import Curvature
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        eps = float(min(step))
        lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
        normal_eps = 1e-4 * float(np.sqrt(np.dot(hi - lo, hi - lo)) / 2)
        dt_ = eng.tape_for(f)
        mesh = eng.generate(dt_, X, Y, Z, 32, True)
        try:
            nu, t = mesh._welded(), mesh.n_triangles
            flat = ctypes.c_int64(0)
            k_nrm, k_curv, call_ms = [], [], []
            for i in range(args.warmup + args.calls):
                rc = lib.sdf_mesh_vertex_normals(mesh.handle, dt_.handle, normal_eps * (1.0 + 0.001 * (i & 1)), None, ctypes.byref(flat))
                if rc:
                    raise RuntimeError(lib.sdf_last_error().decode())
                if i >= args.warmup:
                    k_nrm.append(lib.sdf_mesh_normals_last_kernel_ms())
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                curv, status, counts = mesh.vertex_curvature(dt_, eps)
                if i >= args.warmup:
                    call_ms.append((time.perf_counter() - t0) * 1e3)
                    k_curv.append(lib.sdf_mesh_curvature_last_kernel_ms())
            pts, cells = mesh.weld()
            pts = pts.copy()
        finally:
            mesh.close()
        n_ms, c_ms = float(np.median(k_nrm)), float(np.median(k_curv))
        nrm_rate, curv_rate = 6.0 * nu / (n_ms * 1e-3), 19.0 * nu / (c_ms * 1e-3)
        c = Curvature(pts, cells, curv, status, {'eps': eps})
        line = {'metric': 'curvature probe: median ms of k_vertex_curvature and k_vertex_normals alone (HIP events), same mesh',
                'model': name, 'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'vertices': nu,
                'eps': round(eps, 9), 'normals_kernel_ms_median': round(n_ms, 4), 'normals_evals_per_s': round(nrm_rate),
                'curvature_kernel_ms_median': round(c_ms, 4), 'curvature_kernel_ms_min': round(min(k_curv), 4),
                'curvature_kernel_ms_max': round(max(k_curv), 4), 'curvature_evals_per_s': round(curv_rate),
                'rate_fraction': round(curv_rate / nrm_rate, 4), 'kernel_ms_over_normals': round(c_ms / n_ms, 3),
                'vertex_curvature_call_ms_median': round(float(np.median(call_ms)), 3),
                'status': dict(zip(ref.NAMES, counts.tolist())),
                'min_convex_radius': c.min_convex_radius, 'min_concave_radius': c.min_concave_radius}
        whole = []
        for i in range(3):
            t0 = time.perf_counter()
            got = f.curvature(bounds=bounds, samples=args.samples, verbose=False)
            whole.append((time.perf_counter() - t0) * 1e3)
        line['curvature_call_ms'] = [round(x, 2) for x in whole]
        line['curvature_call_eps'] = got.params['eps']
        if not args.no_definition:
            t0 = time.perf_counter()
            with np.errstate(all='ignore'):
                want = ref.curvature(lambda P: eng.eval_points(dt_, P), pts, eps)
            line['definition_over_eval_points_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            line['bit_identical_to_definition'] = bool(np.array_equal(ref.bits(curv), ref.bits(want[0])) and np.array_equal(status, want[1])
                                                       and counts.tolist() == ref.counts(want[1]).tolist())
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
