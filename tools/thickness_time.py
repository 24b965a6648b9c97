#!/usr/bin/env python3
"""Time the wall-thickness probe (sdf_mesh_vertex_thickness; csrc/sdf_thickness.hip) next to k_vertex_normals on the same mesh, in one run:

    python tools/thickness_time.py [--calls 8] [--warmup 2] [--models ex_example,ex_knurling] [--samples 134217728] [--no-definition]

Per model, one JSON line: triangles and welded vertices of the mesh at --samples; the median over --calls calls after --warmup of
k_vertex_normals alone by HIP events (sdf_mesh_normals_last_kernel_ms; the calls alternate between two values of eps, so none is
served from the mesh's cache) -- the yardstick: 6 evaluations per vertex in lockstep -- and of k_vertex_thickness alone
(sdf_mesh_thickness_last_kernel_ms) with the defaults of `thickness()`; the status counts; `evals_per_vertex` = 6 + mean steps + refine x
the THICK share: what the vertices needed; `lockstep_share` = sum(steps) / (64 x the sum over runs of 64 vertices in weld order of the
run's largest step count); `issued_per_vertex`: what the waves evaluated per lane (6 + the run's largest step count + refine where
the run has a THICK vertex); `rate_fraction` = (needed evaluations / thickness kernel time) / (6 U / normals kernel time), and
`issued_rate_fraction` the same with the issued evaluations; the whole `f.thickness()` call; and, unless --no-definition, the NumPy
definition (tests/thickness_ref.py) over `Engine.eval_points` on the same vertices, once, with whether the device result is
bit-identical to it.  Needs an MI355X."""
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
    import fixtures
    import sdf_amd
    import thickness_ref as ref
    from sdf_amd import core, engine
    from sdf_amd.thickness import default_params
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        par = dict(default_params(bounds, step), step_scale=1.0, max_steps=256, refine=16)
        dt_ = eng.tape_for(f)
        mesh = eng.generate(dt_, X, Y, Z, 32, True)
        try:
            nu, t = mesh._welded(), mesh.n_triangles
            flat = ctypes.c_int64(0)
            k_nrm, k_thick = [], []
            for i in range(args.warmup + args.calls):
                rc = lib.sdf_mesh_vertex_normals(mesh.handle, dt_.handle, par['normal_eps'] * (1.0 + 0.001 * (i & 1)), None, ctypes.byref(flat))
                if rc:
                    raise RuntimeError(lib.sdf_last_error().decode())
                if i >= args.warmup:
                    k_nrm.append(lib.sdf_mesh_normals_last_kernel_ms())
            call_ms = []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                th, status, steps = mesh.vertex_thickness(dt_, **par)
                if i >= args.warmup:
                    call_ms.append((time.perf_counter() - t0) * 1e3)
                    k_thick.append(lib.sdf_mesh_thickness_last_kernel_ms())
            pts = mesh.weld()[0].copy() if not args.no_definition else None
        finally:
            mesh.close()
        n_ms, t_ms = float(np.median(k_nrm)), float(np.median(k_thick))
        thick = status == ref.THICK
        pad = (-nu) % 64
        s64 = np.concatenate([steps, np.zeros(pad, steps.dtype)]).reshape(-1, 64)
        k64 = np.concatenate([thick, np.zeros(pad, bool)]).reshape(-1, 64)
        wave_steps = s64.max(axis=1).astype(np.int64)
        needed = 6.0 + float(steps.mean()) + par['refine'] * float(thick.mean())
        issued = 6.0 + 64.0 * float((wave_steps + par['refine'] * k64.any(axis=1)).sum()) / nu
        nrm_rate = 6.0 * nu / (n_ms * 1e-3)
        line = {'metric': 'wall-thickness probe: median ms of k_vertex_thickness and k_vertex_normals alone (HIP events), same mesh',
                'model': name, 'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': t, 'vertices': nu,
                'params': {k: (round(v, 9) if isinstance(v, float) else v) for k, v in par.items()},
                'normals_kernel_ms_median': round(n_ms, 4), 'normals_evals_per_s': round(nrm_rate),
                'thickness_kernel_ms_median': round(t_ms, 4), 'thickness_kernel_ms_min': round(min(k_thick), 4), 'thickness_kernel_ms_max': round(max(k_thick), 4),
                'vertex_thickness_call_ms_median': round(float(np.median(call_ms)), 3),
                'status': dict(zip(ref.NAMES, np.bincount(status, minlength=5).tolist())),
                'steps_mean': round(float(steps.mean()), 3), 'steps_max': int(steps.max()),
                'min_thickness': float(th[thick | (status == ref.THIN)].min()) if (thick | (status == ref.THIN)).any() else None,
                'evals_per_vertex': round(needed, 3), 'lockstep_share': round(float(steps.sum()) / (64.0 * wave_steps.sum()), 4),
                'issued_per_vertex': round(issued, 3),
                'rate_fraction': round(needed * nu / (t_ms * 1e-3) / nrm_rate, 4),
                'issued_rate_fraction': round(issued * nu / (t_ms * 1e-3) / nrm_rate, 4)}
        whole = []
        for i in range(3):
            t0 = time.perf_counter()
            got = f.thickness(bounds=bounds, samples=args.samples, verbose=False)
            whole.append((time.perf_counter() - t0) * 1e3)
        line['thickness_call_ms'] = [round(x, 2) for x in whole]
        line['thickness_call_min'] = got.min
        if not args.no_definition:
            t0 = time.perf_counter()
            want = ref.thickness(lambda P: eng.eval_points(dt_, P), pts, **par)
            line['definition_over_eval_points_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            line['bit_identical_to_definition'] = bool(np.array_equal(ref.bits(th), ref.bits(want[0])) and np.array_equal(status, want[1])
                                                       and np.array_equal(steps, want[2]))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
