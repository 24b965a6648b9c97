#!/usr/bin/env python3
"""Time the mending of a mesh on the device (sdf_mesh_mend; csrc/sdf_mend.hip) in one run:

    python tools/mend_time.py [--calls 12] [--warmup 2] [--samples 134217728] [--no-numpy]

Two models: the thin plates mending was made for -- `box((2, 2, w)) | box((2, 2, w)).translate((0, 0, 2.5 w))` with the wall w = 2.4
grid steps at --samples, which is 0.12 at step 0.05: thinner than a cluster of simplify=4, so its two sheets fold together -- and the
example, which has nothing to mend.
Per model, for the mesh at --samples as it is (nothing to mend: what the passes cost per triangle) and for the mesh simplified with
simplify=4 (where the pairs are), one JSON line: triangles and welded vertices, the statistics, the median over --calls calls after
--warmup, on one mesh welded beforehand, of the kernels by HIP events split into the keys (k_mend_keys), the two sorts (over T 32-bit
and T 64-bit keys, with k_mend_gather between them) and runs + emission (k_mend_runs, the scan, the copy), and of the whole
`Mesh.mend` call; for comparison the edge census of the same mesh (one sort over 3T 64-bit keys; kernels by HIP events) and the NumPy
definition (tests/mend_ref.py) on the same cells, once, with whether the device agrees bit for bit.  Needs an MI355X."""
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


def time_mend(lib, mesh, args, line):
    """adds the timings of `mesh.mend()`, of the mesh's census and of the NumPy definition to `line` and prints it"""
    import mend_ref
    nu = mesh._welded()
    parts, wall, census, stats, got = [], [], [], None, None
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        mended = mesh.mend()
        dt = (time.perf_counter() - t0) * 1e3
        p = (ctypes.c_double * 3)()
        lib.sdf_mesh_mend_last_kernel_ms(p)
        stats = mended.mend_stats
        if i == args.warmup + args.calls - 1 and not args.no_numpy:
            got = mended.points().copy()
        mended.close()
        mesh.edge_census()
        if i >= args.warmup:
            parts.append(list(p)); wall.append(dt); census.append(lib.sdf_mesh_measure_last_kernel_ms())
    parts = np.array(parts)
    line.update({'triangles': mesh.n_triangles, 'vertices': nu, 'keys_ms_median': med(parts[:, 0]), 'sorts_ms_median': med(parts[:, 1]),
                 'runs_emit_ms_median': med(parts[:, 2]), 'kernels_ms_median': med(parts.sum(axis=1)),
                 'kernels_ms_min': round(float(parts.sum(axis=1).min()), 4), 'kernels_ms_max': round(float(parts.sum(axis=1).max()), 4),
                 'mend_call_ms_median': med(wall), 'edge_census_kernels_ms_median': med(census)})
    line.update({key: stats[key] for key in mend_ref.STAT_KEYS})
    if not args.no_numpy:
        cells = np.array(mesh.weld()[1])
        soup = np.array(mesh.points()).reshape(-1, 3, 3)
        t0 = time.perf_counter()
        want = mend_ref.mend(cells, soup)
        line['numpy_mend_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        line['identical_to_numpy'] = bool(got.shape == (3 * len(want.soup), 3) and np.array_equal(
            got.view(np.int64), want.soup.reshape(-1, 3).view(np.int64)) and all(stats[key] == want.stats[key] for key in mend_ref.STAT_KEYS))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--samples', type=int, default=2 ** 27)
    ap.add_argument('--no-numpy', action='store_true', help='without the NumPy definition (a profiled run)')
    args = ap.parse_args()

    import sdf_amd
    from sdf_amd import core, engine, simplify
    eng = engine.get_engine(0)
    lib = eng.lib
    wall = 2.4 * core.grid_axes(((-1.3,) * 3, (1.3,) * 3), samples=args.samples)[3][2]
    plate = sdf_amd.box((2, 2, wall))
    cyl = sdf_amd.cylinder(0.5)
    models = (('thin_plates', plate | plate.translate((0, 0, 2.5 * wall)), ((-1.3,) * 3, (1.3,) * 3)),
              ('example', (sdf_amd.sphere(1) & sdf_amd.box(1.5)) - (cyl.orient(sdf_amd.X) | cyl.orient(sdf_amd.Y) | cyl.orient(sdf_amd.Z)),
               ((-0.85,) * 3, (0.85,) * 3)))
    for name, f, bounds in models:
        X, Y, Z, step = core.grid_axes(bounds, samples=args.samples)
        mesh = eng.generate(eng.tape_for(f), X, Y, Z, 32, True)
        try:
            head = {'metric': 'mesh mending: median ms of the kernels (HIP events) and of the whole call', 'model': name,
                    'samples': args.samples, 'calls': args.calls, 'warmup': args.warmup}
            time_mend(lib, mesh, args, dict(head, simplify=None))
            small = mesh.simplify(*simplify.resolve_cell(4, X, Y, Z, step))
            try:
                time_mend(lib, small, args, dict(head, simplify=4))
            finally:
                small.close()
        finally:
            mesh.close()


if __name__ == '__main__':
    main()
