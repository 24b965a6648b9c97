#!/usr/bin/env python3
"""Time the device mesh-to-level-set voxelizer (sdf_mesh_level_set_host, csrc/sdf_level_set.hip) on a large mesh:

    python tools/level_set_time.py [--samples-log2 24] [--voxels 200] [--calls 10] [--warmup 2]

The mesh is the canonical CSG example (bench.py's model) welded on the device at 2^samples_log2 samples; the voxel size
is its extent / --voxels.  Prints one JSON line: triangle count, work grid and active dims, the median wall time of the
C call (host clock around the synchronous call: upload, all kernels, the copy of the cropped grid) and whether the grid
stays under the tape-constant limit below which `generate` still prunes a model holding it (0xFFFFF0 constants,
csrc/sdf_generate.hip: `t->n_consts < 0xFFFFF0u`).  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sdf_amd  # noqa: E402
from sdf_amd import core, engine, mesh, tape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples-log2', type=int, default=24)
    ap.add_argument('--voxels', type=int, default=200)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()

    f = sdf_amd.sphere(1) & sdf_amd.box(1.5)
    c = sdf_amd.cylinder(0.5)
    f -= c.orient(sdf_amd.X) | c.orient(sdf_amd.Y) | c.orient(sdf_amd.Z)
    pts, cells = core.generate_mesh(f, samples=2 ** args.samples_log2, verbose=False)[:2]
    vs = float(np.ptp(pts, axis=0).max()) / args.voxels
    hw = mesh.half_width_voxels(vs)
    eng = engine.get_engine(0)
    lo = np.floor(pts.min(axis=0) / vs) - hw - 1
    hi = np.ceil(pts.max(axis=0) / vs) + hw + 1
    for _ in range(args.warmup):
        eng.mesh_level_set(pts, cells, vs, hw)
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ijk0, A = eng.mesh_level_set(pts, cells, vs, hw)
        ms.append((time.perf_counter() - t0) * 1e3)
    g = mesh.level_set(pts, cells, vs)
    n_consts = len(tape.lower(g).consts)
    print(json.dumps({
        'metric': 'mesh level set (device voxelizer), median wall ms of sdf_mesh_level_set_host',
        'triangles': int(len(cells)), 'points': int(len(pts)), 'voxel_size': vs, 'half_width_voxels': hw,
        'work_dims': [int(x) for x in hi - lo + 1], 'active_dims': list(A.shape), 'active_voxels': int(A.size),
        'ms_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3),
        'tape_consts': n_consts, 'generate_prunes': n_consts < 0xFFFFF0,
    }))


if __name__ == '__main__':
    main()
