#!/usr/bin/env python3
"""Time the sphere tracer (sdf_render_host, csrc/sdf_render.hip) against the interpreter's own throughput, in one run:

    python tools/render_time.py [--calls 12] [--warmup 2] [--models ex_example,ex_gearlike,ex_knurling] [--sizes 1024x768,1920x1080]
                                 [--max-steps 256] [--refine 8] [--no-yardstick]
    python tools/render_time.py --summarize <rocprofv3 kernel_stats.csv>        # the kernel table of a profiled run, as markdown

Per model and size, one JSON line: the median wall time of `Engine.render_buffers` -- the whole call: the allocation, the kernel,
four pageable copies, the free -- over --calls calls after --warmup, and of the kernel alone by HIP events
(sdf_render_last_kernel_ms); rays/s; the mean and the largest step count; the lockstep share sum(steps) / (64 * sum over 8 x 8
tiles of the tile's largest step count), from the returned buffer; and the yardstick: ONE `sdf_eval_points` launch of the same
tape on as many points (uniform in the bounds, already on the device) as the frame's steps sum, wall time around launch +
synchronise.  `useful_fraction` = (march evaluations a ray needed / kernel time) / (the yardstick's points / its time): 1.0 would
be a tracer that evaluates only what is needed at the interpreter's full rate.  The kernel also evaluates the normal (6 per ray
of a tile with a hit) and the refinement (up to --refine per ray of a tile that needs it); `wave_evals` counts all of them, in
lane evaluations.  Needs an MI355X and torch (for the yardstick's device buffer)."""
import argparse
import csv
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def tile_max(steps, th=8, tw=8):
    h, w = steps.shape
    p = np.zeros(((h + th - 1) // th * th, (w + tw - 1) // tw * tw), steps.dtype)
    p[:h, :w] = steps
    return p.reshape(p.shape[0] // th, th, p.shape[1] // tw, tw).max(axis=(1, 3))


def summarize(path):
    rows = [r for r in csv.DictReader(open(path)) if 'k_render' in r['Name'] or 'k_eval_points' in r['Name']]
    print('| kernel | calls | total ms | avg us | min us | max us |')
    print('|---|---|---|---|---|---|')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        print('| `%s` | %d | %.3f | %.1f | %.1f | %.1f |' % (r['Name'].split('(')[0], int(r['Calls']), float(r['TotalDurationNs']) / 1e6,
                                                         float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_gearlike,ex_knurling')
    ap.add_argument('--sizes', default='1024x768,1920x1080')
    ap.add_argument('--refine', type=int, default=8)
    ap.add_argument('--max-steps', type=int, default=256)
    ap.add_argument('--no-yardstick', action='store_true', help='the tracer alone (a profiled run)')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    import torch
    torch.cuda.is_available()                      # torch's HIP runtime initialises first
    import fixtures
    import sdf_amd
    from sdf_amd import engine
    R = importlib.import_module('sdf_amd.render')
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        bounds = eng.estimate_bounds(f)
        for size in args.sizes.split(','):
            w, h = (int(v) for v in size.split('x'))
            frame, t_near, t_far, radius = R.camera(bounds, w, h)
            p = dict(t_near=t_near, t_far=t_far, hit_eps=1e-4 * radius, step_scale=1.0, normal_eps=1e-4 * radius, max_steps=args.max_steps, refine=args.refine)
            wall, kern = [], []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                buf = eng.render_buffers(f, frame, w, h, **p)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    wall.append(dt)
                    kern.append(eng.lib.sdf_render_last_kernel_ms())
            steps, status = buf['steps'], buf['status']
            tmax, thit = tile_max(steps), tile_max(status)
            total = int(steps.sum())
            k_ms = float(np.median(kern))
            line = {'metric': 'render_buffers: median ms of the whole call and of k_render alone (HIP events)', 'model': name, 'width': w, 'height': h,
                    'max_steps': args.max_steps, 'refine': args.refine, 'calls': args.calls, 'warmup': args.warmup, 'call_ms_median': round(float(np.median(wall)), 3), 'call_ms_min': round(min(wall), 3),
                    'kernel_ms_median': round(k_ms, 3), 'kernel_ms_min': round(min(kern), 3), 'kernel_ms_max': round(max(kern), 3),
                    'rays_per_s': round(w * h / (k_ms * 1e-3)), 'hits': int(status.sum()), 'steps_sum': total, 'steps_mean': round(total / (w * h), 2),
                    'steps_max': int(steps.max()), 'lockstep_share': round(total / (64.0 * int(tmax.sum())), 3),
                    'wave_evals': int(64 * (int(tmax.sum()) + int((thit > 0).sum()) * 6)), 'wave_evals_note': 'march + normal; the refinement adds up to 64 * refine per tile that needs it',
                    'march_evals_per_s': round(total / (k_ms * 1e-3))}
            if not args.no_yardstick:
                lib, dt_ = eng.lib, eng.tape_for(f)
                lo, hi = (torch.tensor(b, dtype=torch.float64, device='cuda') for b in bounds)
                pts = lo + torch.rand((total, 3), dtype=torch.float64, device='cuda') * (hi - lo)
                out = torch.empty(total, dtype=torch.float64, device='cuda')
                torch.cuda.synchronize()
                ms = []
                for i in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    rc = lib.sdf_eval_points(dt_.handle, ctypes.c_void_p(pts.data_ptr()), total, 3, ctypes.c_void_p(out.data_ptr()), eng.precision)
                    eng.synchronize()
                    if rc:
                        raise RuntimeError(lib.sdf_last_error().decode())
                    if i >= args.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                y_ms = float(np.median(ms))
                line.update({'yardstick': 'sdf_eval_points on steps_sum uniform points in the bounds, wall ms around launch + synchronise',
                             'yardstick_ms_median': round(y_ms, 3), 'yardstick_points_per_s': round(total / (y_ms * 1e-3)),
                             'useful_fraction': round(y_ms / k_ms, 3)})
                del pts, out
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
