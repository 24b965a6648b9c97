#!/usr/bin/env python3
"""Time the support rays (sdf_mesh_support_rays; csrc/sdf_supports.hip, the driver in csrc/sdf_overhang.hip) next to k_vertex_thickness
on the same mesh, in one run:

    python tools/supports_time.py [--calls 8] [--warmup 2] [--models ex_example,ex_knurling] [--samples 134217728] [--rate 200] [--no-definition]

Per model and direction -- +z, and the best of --rate spiral directions (+ the six axes) by the proxy of `overhangs` -- one JSON line:
triangles of the mesh at --samples and M, the overhanging faces = rays; the median over --calls calls after --warmup of the kernels of
one sdf_mesh_support_rays call by HIP events (sdf_mesh_supports_last_kernel_ms) and of its four parts: classes + extents, numbering,
rays, sums; the whole `Mesh.support_rays` call with its fetch; the status counts; `steps_mean`, the march evaluations a ray needed;
`evals_per_ray` = mean steps + refine x the PART share; `lockstep_share` = sum(steps) / (64 x the sum over runs of 64 rays of the run's
largest step count); `issued_per_ray`: what the waves evaluated per lane (the run's largest step count + refine where the run has a
PART ray); the yardstick -- k_vertex_thickness alone on the same mesh with the defaults of `thickness()`, as evaluations per second
needed and issued -- and `rate_fraction` / `issued_rate_fraction`: the rays' evaluations per second over the yardstick's; the volumes;
and, unless --no-definition, the NumPy definition (tests/supports_ref.py) over `Engine.eval_points` on the same soup, once, with whether
every device output is bit-identical to it.  A last line per model times the whole `f.supports()` call.  Needs an MI355X."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def waves(steps, flag):
    """(lockstep share, evaluations issued per lane) of rays in their order: runs of 64"""
    n = len(steps)
    pad = (-n) % 64
    s64 = np.concatenate([steps, np.zeros(pad, steps.dtype)]).reshape(-1, 64).max(axis=1).astype(np.int64)
    k64 = np.concatenate([flag, np.zeros(pad, bool)]).reshape(-1, 64).any(axis=1)
    return s64, k64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--rate', type=int, default=200, help='spiral directions rated by the proxy for the second direction')
    ap.add_argument('--no-definition', action='store_true', help='without the NumPy definition over eval_points')
    args = ap.parse_args()

    try:
        import torch
        torch.cuda.is_available()                  # torch's HIP runtime initialises first
    except ImportError:
        pass
    import fixtures
    import sdf_amd
    import supports_ref as ref
    import thickness_ref
    from sdf_amd import core, engine
    from sdf_amd.overhang import overhangs_of_mesh, sin_limit_of
    from sdf_amd.thickness import default_params
    derive = importlib.import_module('sdf_amd.supports').derive      # (the package's attribute `supports` is the function)
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    parts = np.zeros(4)
    parts_p = parts.ctypes.data_as(engine._f64p)
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        tol, quarter, refine = float(max(step)), float(min(step)) / 4, 16
        p = dict(sin_limit=sin_limit_of(45.0), bed_tol=tol, start=quarter, min_step=quarter, step_scale=1.0, max_steps=256, refine=refine)
        dt_ = eng.tape_for(f)
        mesh = eng.generate(dt_, X, Y, Z, 32, True)
        try:
            t = mesh.n_triangles
            # the yardstick: k_vertex_thickness on the same mesh
            nu = mesh._welded()
            tpar = dict(default_params(bounds, step), step_scale=1.0, max_steps=256, refine=refine)
            k_thick = []
            for i in range(args.warmup + args.calls):
                th, tstatus, tsteps = mesh.vertex_thickness(dt_, **tpar)
                if i >= args.warmup:
                    k_thick.append(lib.sdf_mesh_thickness_last_kernel_ms())
            th_ms = float(np.median(k_thick))
            thick = tstatus == thickness_ref.THICK
            ts64, tk64 = waves(tsteps, thick)
            th_needed = (6.0 + float(tsteps.mean()) + refine * float(thick.mean())) * nu / (th_ms * 1e-3)
            th_issued = (6.0 * nu + 64.0 * float((ts64 + refine * tk64).sum())) / (th_ms * 1e-3)
            t0 = time.perf_counter()
            proxy = overhangs_of_mesh(mesh, args.rate, 45.0, tol)
            proxy_ms = (time.perf_counter() - t0) * 1e3
            best = proxy.best()
            soup = mesh.points().copy().reshape(-1, 3, 3) if not args.no_definition else None
            for label, d in (('+z', np.array([[0.0, 0.0, 1.0]])), ('best of %d by proxy' % len(proxy.directions), proxy.directions[best:best + 1].copy())):
                k_ms, k_parts, call_ms = [], [], []
                for i in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    raw = mesh.support_rays(dt_, d, **p)
                    if i >= args.warmup:
                        call_ms.append((time.perf_counter() - t0) * 1e3)
                        k_ms.append(lib.sdf_mesh_supports_last_kernel_ms(parts_p))
                        k_parts.append(parts.copy())
                tri, height, status, steps, origin = raw['rays'][0]
                m = len(tri)
                part = status == ref.PART
                s64, k64 = waves(steps, part)
                ms = float(np.median(k_ms))
                pm = np.median(np.array(k_parts), axis=0)
                needed = float(steps.mean()) + refine * float(part.mean()) if m else 0.0
                issued = 64.0 * float((s64 + refine * k64).sum()) / m if m else 0.0
                v = derive(raw)
                line = {'metric': 'support rays: median ms of the kernels of sdf_mesh_support_rays (HIP events) and of k_vertex_thickness alone, same mesh',
                        'model': name, 'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'direction': label,
                        'd': [round(float(x), 6) for x in d[0]], 'triangles': t, 'rays': m,
                        'params': {k: (round(x, 9) if isinstance(x, float) else x) for k, x in p.items()},
                        'kernels_ms_median': round(ms, 4), 'kernels_ms_min': round(min(k_ms), 4), 'kernels_ms_max': round(max(k_ms), 4),
                        'parts_ms_median': dict(zip(('classes', 'numbering', 'rays', 'sums'), [round(float(x), 4) for x in pm])),
                        'support_rays_call_ms_median': round(float(np.median(call_ms)), 3),
                        'status': dict(zip(ref.NAMES, raw['counts'][0].tolist())),
                        'steps_mean': round(float(steps.mean()), 3) if m else 0.0, 'steps_max': int(steps.max()) if m else 0,
                        'evals_per_ray': round(needed, 3), 'lockstep_share': round(float(steps.sum()) / (64.0 * s64.sum()), 4) if m and s64.sum() else 1.0,
                        'issued_per_ray': round(issued, 3),
                        'thickness_vertices': nu, 'thickness_kernel_ms_median': round(th_ms, 4),
                        'thickness_evals_per_s': round(th_needed), 'thickness_issued_evals_per_s': round(th_issued),
                        'rate_fraction': round(needed * m / (pm[2] * 1e-3) / th_needed, 4) if m else None,
                        'issued_rate_fraction': round(issued * m / (pm[2] * 1e-3) / th_issued, 4) if m else None,
                        'proxy_support_volume': float(proxy.support_volume[4 if label == '+z' else best]),
                        'support_volume': float(v['support_volume'][0]), 'on_part_volume': float(v['on_part_volume'][0]),
                        'buried_area': float(v['buried_area'][0]), 'projected_area': float(v['projected_area'][0])}
                if not args.no_definition:
                    t0 = time.perf_counter()
                    want = ref.supports(lambda P: eng.eval_points(dt_, P), soup, d[0], **p)
                    line['definition_over_eval_points_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                    line['bit_identical_to_definition'] = bool(
                        np.array_equal(tri, want['triangle']) and np.array_equal(ref.bits(height), ref.bits(want['height']))
                        and np.array_equal(status, want['status']) and np.array_equal(steps, want['steps'])
                        and np.array_equal(ref.bits(origin), ref.bits(want['origin'])) and np.array_equal(ref.bits(raw['sums'][0]), ref.bits(want['sums']))
                        and np.array_equal(raw['counts'][0], want['counts']) and raw['lo'][0] == want['lo'] and raw['hi'][0] == want['hi'])
                print(json.dumps(line), flush=True)
        finally:
            mesh.close()
        whole = []
        for i in range(3):
            t0 = time.perf_counter()
            got = f.supports(args.rate, top=8, bounds=bounds, samples=args.samples, verbose=False)
            whole.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({'metric': 'f.supports(%d, top=8): mesh, rate, trace 8 directions; ms per call' % args.rate, 'model': name,
                          'samples': args.samples, 'supports_call_ms': [round(x, 2) for x in whole], 'rate_directions_ms_once': round(proxy_ms, 2),
                          'best': int(got.best()), 'best_support_volume': float(got.support_volume[got.best()]),
                          'best_proxy_volume': float(got.proxy.support_volume[got.traced[got.best()]])}), flush=True)


if __name__ == '__main__':
    main()
