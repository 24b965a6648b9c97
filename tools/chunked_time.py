#!/usr/bin/env python3
"""Fingerprint and time the meshing paths through device memory (csrc/sdf_chunked.hip: batch_size > 32, and models with user
closures at any batch size):

    python tools/chunked_time.py [--calls 10] [--warmup 2]

Five calls of the canonical CSG example (bench.py's model): the tape path at batch_size 64 on a 2^21-sample grid, at 322 on
660 x 330 x 7 (the soup is regrown while it holds triangles) and at 512 on 515 x 515 x 9 (a tile fills every row slot); the same
model with the README's sphere as a user closure -- the callback path -- at 32 and at 255 on 600 x 7 x 6.  Prints one JSON line per
call: the sha256 of the soup, of the kinds and of the batch offsets (or the refusal, for a closure model), the statistics without
their ms_* fields, and the median / min / max wall time of the whole synchronous call.  SDF_HIP_LIB selects another build of the
library, so two builds can be compared line by line.  Needs an MI355X."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sdf_amd  # noqa: E402
from sdf_amd import core, engine  # noqa: E402


@sdf_amd.sdf3
def my_sphere(radius=1, center=sdf_amd.ORIGIN):
    def f(p):
        return np.linalg.norm(p - center, axis=1) - radius
    return f


def example(sphere):
    f = sphere(1) & sdf_amd.box(1.5)
    c = sdf_amd.cylinder(0.5)
    return f - (c.orient(sdf_amd.X) | c.orient(sdf_amd.Y) | c.orient(sdf_amd.Z))


def axes(shape):
    return tuple(-0.9 + 1.8 * np.arange(n) / max(n - 1, 1) for n in shape)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    tape_model, closure_model = example(sdf_amd.sphere), example(my_sphere)
    cases = [
        ('tape b64 2^21', tape_model, core.grid_axes(((-0.85, -0.85, -0.85), (0.85, 0.85, 0.85)), samples=2 ** 21)[:3], 64),
        ('tape b322 660x330x7', tape_model, axes((660, 330, 7)), 322),
        ('tape b512 515x515x9', tape_model, axes((515, 515, 9)), 512),
        ('closure b32 600x7x6', closure_model, axes((600, 7, 6)), 32),
        ('closure b255 600x7x6', closure_model, axes((600, 7, 6)), 255),
    ]
    eng = engine.get_engine(0)
    for name, f, (X, Y, Z), bs in cases:
        ms = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            m = eng.generate(f, X, Y, Z, bs, True)
            if k >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            if k + 1 < args.warmup + args.calls:
                m.close()
        try:
            offsets = sha(m.batch_offsets())
        except engine.SdfHipError as e:
            offsets = 'refused: %s' % e
        stats = {k: v for k, v in m.stats().items() if not k.startswith('ms_')}
        print(json.dumps({'case': name, 'lib': engine.LIB_PATH, 'points': sha(m.points()), 'kinds': sha(m.kinds()), 'batch_offsets': offsets,
                          'stats': stats, 'ms_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3)}, default=str))
        m.close()


if __name__ == '__main__':
    main()
