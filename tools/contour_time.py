#!/usr/bin/env python3
"""Time the contouring of models on the device (sdf_contour_host / sdf_contour_grid_host; csrc/sdf_contour.hip) in one run:

    python tools/contour_time.py [--calls 12] [--warmup 2] [--side 4096] [--layers 256] [--layer-side 1024] [--no-numpy]

Three cases, one JSON line each:
  rounded_x   `rounded_x(1, 0.2)` on --side x --side samples over [-0.9, 0.9]^2 (the tape entry, dim 2);
  example     the canonical example cut at --layers heights in [-0.7, 0.7], --layer-side x --layer-side samples each over
              [-0.85, 0.85]^2 (the tape entry, dim 3);
  comb        tests/contour_cases.py's comb on 1449 x 1449 samples through the grid entry: ONE closed loop of about 10^6 points, which
              k_contour_area walks with one lane.
Per case: the counts, the linking rounds, and the median over --calls calls after --warmup of the parts by HIP events -- sampling
(k_contour_points + the interpreter, in slabs), count + scan + emit, the linking (both pointer-jumping phases, the scans, lengths and
scatter), the areas -- of the whole call and of the fetch (wall clock).  Beside them: ONE sdf_eval_points launch on the same points
(wall ms around launch + synchronise; the points made by torch), and the NumPy definition (tests/contour_ref.py) on the same samples,
once -- for the layered case on the first --numpy-layers layers only, the figure scaled to all of them -- with whether the device
agrees bit for bit on what was compared.  Needs an MI355X."""
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


def identical(c, want):
    import contour_ref
    return bool(all(getattr(c, k).shape == want[k].shape and np.array_equal(getattr(c, k).view(np.uint8), want[k].view(np.uint8))
                    for k in contour_ref.ARRAYS))


def run(eng, args, line, call, fetch_of):
    """`call()` -> (handle, counts): timed; the handle fetched (timed) and destroyed"""
    from sdf_amd import contour
    lib = eng.lib
    parts, wall, fetch, c = [], [], [], None
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        h, cnt = call()
        t1 = time.perf_counter()
        p = (ctypes.c_double * 4)()
        lib.sdf_contour_last_kernel_ms(p)
        c = fetch_of(h, cnt)
        t2 = time.perf_counter()
        if i >= args.warmup:
            parts.append(list(p)); wall.append((t1 - t0) * 1e3); fetch.append((t2 - t1) * 1e3)
    parts = np.array(parts)
    line.update(dict(c.counts))
    line.update({'sampling_ms_median': med(parts[:, 0]), 'count_emit_ms_median': med(parts[:, 1]), 'linking_ms_median': med(parts[:, 2]),
                 'area_ms_median': med(parts[:, 3]), 'kernels_ms_median': med(parts.sum(axis=1)),
                 'kernels_ms_min': round(float(parts.sum(axis=1).min()), 4), 'kernels_ms_max': round(float(parts.sum(axis=1).max()), 4),
                 'call_ms_median': med(wall), 'fetch_ms_median': med(fetch), 'longest_contour_points': int(np.diff(c.offsets).max()) if len(c) else 0})
    return c


def tape_case(eng, args, name, f, X, Y, W):
    import torch
    import contour_ref
    from sdf_amd import contour, engine
    lib = eng.lib
    dt = eng.tape_for(f)
    dim = 2 if W is None else 3
    nw = 1 if W is None else len(W)
    f64p = engine._f64p
    line = {'metric': 'contours: median ms of the parts (HIP events), of the whole call and of the fetch', 'case': name, 'dim': dim, 'nw': nw,
            'nx': len(X), 'ny': len(Y), 'calls': args.calls, 'warmup': args.warmup}

    def call():
        h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
        engine._check(lib, lib.sdf_contour_host(dt.handle, dim, X.ctypes.data_as(f64p), len(X), Y.ctypes.data_as(f64p), len(Y),
                                                None if W is None else W.ctypes.data_as(f64p), nw, 0.0, None, ctypes.byref(h), ctypes.byref(cnt)))
        return h, cnt
    c = run(eng, args, line, call, lambda h, cnt: contour._fetch(eng, h, cnt, W, X, Y))
    # the yardstick: one launch of the interpreter on the same points
    tx, ty = torch.from_numpy(X).to('cuda:0'), torch.from_numpy(Y).to('cuda:0')
    axes = [tx, ty] if W is None else [torch.from_numpy(W).to('cuda:0'), tx, ty]
    grids = torch.meshgrid(*axes, indexing='ij')
    pts = torch.stack(grids if W is None else (grids[1], grids[2], grids[0]), dim=-1).reshape(-1, dim).contiguous()
    out = torch.empty(len(pts), dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    ev = []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        engine._check(lib, lib.sdf_eval_points(dt.handle, ctypes.c_void_p(pts.data_ptr()), len(pts), dim, ctypes.c_void_p(out.data_ptr()), eng.precision))
        eng.synchronize()
        if i >= args.warmup:
            ev.append((time.perf_counter() - t0) * 1e3)
    line['eval_points_alone_ms_median'] = med(ev)
    if not args.no_numpy:
        k = nw if W is None else min(nw, args.numpy_layers)
        V = out.reshape(nw, len(X), len(Y))[:k].cpu().numpy()
        t0 = time.perf_counter()
        want = contour_ref.contours(V, X, Y, 0.0)
        ms = (time.perf_counter() - t0) * 1e3
        line.update({'numpy_layers': k, 'numpy_ms': round(ms, 1), 'numpy_ms_scaled_to_all_layers': round(ms * nw / k, 1)})
        part = c if k == nw else contour.contour_tape(dt, X, Y, W[:k], 0.0, eng)
        line['identical_to_numpy'] = identical(part, want)
    del pts, out
    print(json.dumps(line), flush=True)


def grid_case(eng, args, name, V, X, Y, level):
    import contour_ref
    from sdf_amd import contour, engine
    lib = eng.lib
    f64p = engine._f64p
    V = np.ascontiguousarray(V, dtype=np.float64)
    line = {'metric': 'contours: median ms of the parts (HIP events), of the whole call and of the fetch', 'case': name, 'dim': 0, 'nw': V.shape[0],
            'nx': len(X), 'ny': len(Y), 'calls': args.calls, 'warmup': args.warmup}

    def call():
        h, cnt = ctypes.c_void_p(), engine.SdfContourCounts()
        engine._check(lib, lib.sdf_contour_grid_host(eng.ctx, V.ctypes.data_as(f64p), V.shape[0], len(X), len(Y), X.ctypes.data_as(f64p),
                                                     Y.ctypes.data_as(f64p), level, ctypes.byref(h), ctypes.byref(cnt)))
        return h, cnt
    c = run(eng, args, line, call, lambda h, cnt: contour._fetch(eng, h, cnt, None, X, Y))
    if not args.no_numpy:
        t0 = time.perf_counter()
        want = contour_ref.contours(V, X, Y, level)
        line['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        line['identical_to_numpy'] = identical(c, want)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--side', type=int, default=4096)
    ap.add_argument('--layers', type=int, default=256)
    ap.add_argument('--layer-side', type=int, default=1024)
    ap.add_argument('--comb', type=int, default=1449)
    ap.add_argument('--numpy-layers', type=int, default=4)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition (a profiled run)')
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()                       # (torch's HIP runtime initialises first)
    import contour_cases
    import sdf_amd
    from sdf_amd import engine
    eng = engine.get_engine(0)
    X = np.linspace(-0.9, 0.9, args.side)
    tape_case(eng, args, 'rounded_x', sdf_amd.rounded_x(1, 0.2), X, X.copy(), None)
    cyl = sdf_amd.cylinder(0.5)
    example = (sdf_amd.sphere(1) & sdf_amd.box(1.5)) - (cyl.orient(sdf_amd.X) | cyl.orient(sdf_amd.Y) | cyl.orient(sdf_amd.Z))
    X = np.linspace(-0.85, 0.85, args.layer_side)
    tape_case(eng, args, 'example', example, X, X.copy(), np.linspace(-0.7, 0.7, args.layers))
    grid_case(eng, args, 'comb', *contour_cases.comb(args.comb))


if __name__ == '__main__':
    main()
