#!/usr/bin/env python3
"""Time the connected shells of a mesh (sdf_mesh_components, sdf_mesh_select_shells; csrc/sdf_components.hip) in one run:

    python tools/shells_time.py [--calls 12] [--warmup 2] [--models ex_example,ex_gearlike,ex_knurling] [--samples 134217728]
                                 [--no-numpy]

Per model, one JSON line: triangles and welded vertices of the mesh at --samples and the shells found; the weld's first call; the
median over --calls labellings after --warmup -- every one on a FRESH mesh of the same grid, welded beforehand, because a mesh keeps
its shells -- of the kernels by HIP events, split into labelling (k_shell_init, the rounds of k_shell_hook + k_shell_compress, with
the host's look at the counter between them) and numbering + counts (k_shell_roots, the scan, k_shell_of_vertex, k_shell_of_cell,
k_shell_clear, k_shell_tally x 2), the rounds taken, and the whole call; the same for the selection of the largest shell (k_keep_flags,
the scan, k_select_copy; the selection's soup comes from the pool after the first call); the whole `f.shells(...)`; and the NumPy
definition (tests/components_ref.py) on the same welded mesh, once, with whether the device agrees exactly.  Needs an MI355X."""
import argparse
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
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default='ex_example,ex_gearlike,ex_knurling')
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition (a profiled run)')
    args = ap.parse_args()

    import ctypes
    import components_ref
    import fixtures
    import sdf_amd
    from sdf_amd import core, engine
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    eng = engine.get_engine(0)
    lib = eng.lib
    for name in args.models.split(','):
        f = fixtures.build(name, ns)
        tape = eng.tape_for(f)
        bounds = eng.estimate_bounds(f)
        X, Y, Z, _ = core.grid_axes(bounds, samples=args.samples)
        label, number, wall, rounds, weld_ms = [], [], [], [], []
        sel_k, sel_wall = [], []
        mesh = None
        for i in range(args.warmup + args.calls):
            if mesh is not None:
                mesh.close()
            mesh = eng.generate(tape, X, Y, Z, 32, True)
            t0 = time.perf_counter()
            nu = mesh._welded()
            weld_ms.append((time.perf_counter() - t0) * 1e3)
            out = engine.SdfComponents()
            t0 = time.perf_counter()
            rc = lib.sdf_mesh_components(mesh.handle, ctypes.byref(out))
            dt = (time.perf_counter() - t0) * 1e3
            if rc:
                raise SystemExit('sdf_mesh_components: %s' % lib.sdf_last_error().decode())
            k = int(out.n_shells)
            mask = np.zeros(k, np.uint8)
            t0 = time.perf_counter()
            tri = mesh.shell_summary()['triangles']
            mask[int(np.lexsort((np.arange(k), -tri))[0])] = 1
            sel = mesh.select(mask)
            dts = (time.perf_counter() - t0) * 1e3
            kept = sel.n_triangles
            sel.close()
            if i >= args.warmup:
                label.append(out.ms_label); number.append(out.ms_number); wall.append(dt); rounds.append(int(out.rounds))
                sel_k.append(lib.sdf_mesh_components_last_kernel_ms()); sel_wall.append(dts)
        try:
            got = mesh.components()
            line = {'metric': 'connected shells: median ms of the kernels (HIP events) and of the whole calls', 'model': name,
                    'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup, 'triangles': mesh.n_triangles, 'vertices': nu,
                    'shells': got['count'], 'largest_shell_triangles': int(got['triangles'].max()), 'kept_triangles': int(kept),
                    'rounds': sorted(set(rounds)), 'weld_ms_first_call_median': med(weld_ms),
                    'label_kernels_ms_median': med(label), 'label_kernels_ms_min': round(min(label), 4), 'label_kernels_ms_max': round(max(label), 4),
                    'number_counts_kernels_ms_median': med(number), 'number_counts_kernels_ms_min': round(min(number), 4),
                    'number_counts_kernels_ms_max': round(max(number), 4), 'components_call_ms_median': med(wall),
                    'select_kernels_ms_median': med(sel_k), 'select_kernels_ms_min': round(min(sel_k), 4), 'select_kernels_ms_max': round(max(sel_k), 4),
                    'summary_and_select_call_ms_median': med(sel_wall)}
            if not args.no_numpy:
                pts, cells = mesh.weld()
                t0 = time.perf_counter()
                want = components_ref.components(pts, cells)
                line['numpy_components_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                line['identical_to_numpy'] = bool(want.count == got['count'] and all(
                    np.array_equal(got[key], getattr(want, key)) for key in ('vertex_shell', 'triangle_shell', 'triangles', 'vertices')) and
                    np.array_equal(got['bounds'].view(np.int64), want.bounds.view(np.int64)))
                del pts, cells
        finally:
            mesh.close()
        ms = []
        for i in range(1 + max(args.calls // 4, 3)):
            t0 = time.perf_counter()
            f.shells(bounds=bounds, samples=args.samples)
            ms.append((time.perf_counter() - t0) * 1e3)
        line['shells_call_ms_median'] = round(float(np.median(ms[1:])), 3)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
