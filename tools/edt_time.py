#!/usr/bin/env python3
"""Time `distance_texture` on the host (scipy) and on the device (sdf_distance_texture_host, csrc/sdf_edt.hip) on the same
masks, in one run:

    python tools/edt_time.py [--calls 10] [--warmup 2] [--font path/to/font.ttf] [--device-only]
    python tools/edt_time.py --summarize <rocprofv3 kernel_stats.csv>        # the kernel table of a profiled run, as markdown

The masks are the ones `text()` makes of 'Hello, World!' in DejaVuSans (matplotlib's bundled copy unless --font says
otherwise): the default call (points=512, pixels=2**22: 627 x 4615) and one at points=1536, pixels=2**24 (the canvas is
resized down to 2**24 pixels).  Per mask, one JSON line: the median wall time of `distance_texture(mask, 'host')` and of
`distance_texture(mask, 'device')` -- the whole call: mask to bytes, the allocation, both pageable copies, the kernels, the
free -- over --calls calls after --warmup, their ratio, and whether the two textures are bit-identical.  The kernels alone
come from a run of their own, `rocprofv3 --kernel-trace --stats ... -- python tools/edt_time.py --device-only`, whose
kernel_stats.csv `--summarize` turns into the table kept in profiles/.  Needs an MI355X, scipy, Pillow and a font."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def default_font():
    import matplotlib
    return os.path.join(os.path.dirname(matplotlib.__file__), 'mpl-data/fonts/ttf/DejaVuSans.ttf')


def text_mask(T, font, string, points, pixels):
    canvas, pad = T._canvas(font, string, points)
    return np.array(T._mask(pixels, pad[0], pad[1], canvas)[0], dtype=bool)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def summarize(path):
    rows = [r for r in csv.DictReader(open(path)) if 'k_edt' in r['Name']]
    print('| kernel | calls | total ms | avg us | min us | max us |')
    print('|---|---|---|---|---|---|')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        print('| `%s` | %d | %.3f | %.1f | %.1f | %.1f |' % (r['Name'].split('(')[0], int(r['Calls']), float(r['TotalDurationNs']) / 1e6,
                                                         float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--font', default=None)
    ap.add_argument('--device-only', action='store_true', help='skip the host path (a profiled run)')
    ap.add_argument('--summarize', default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    from sdf_amd import engine
    T = importlib.import_module('sdf_amd.text')
    font = args.font or default_font()
    eng = engine.get_engine(0)
    for label, points, pixels in (('default: points=512, pixels=2**22', 512, 2 ** 22), ('points=1536, pixels=2**24', 1536, 2 ** 24)):
        mask = text_mask(T, font, 'Hello, World!', points, pixels)
        dev, dms = timed(lambda: T.distance_texture(mask, 'device'), args.calls, args.warmup)
        line = {'metric': "distance_texture, median wall ms of the whole call, 'host' (scipy) against 'device'", 'mask': label,
                'rows': int(mask.shape[0]), 'cols': int(mask.shape[1]), 'true_pixels': int(mask.sum()),
                'max_squared_distance': int(np.rint(np.abs(dev).max() ** 2)), 'calls': args.calls, 'warmup': args.warmup,
                'device_ms_median': round(float(np.median(dms)), 3), 'device_ms_min': round(min(dms), 3), 'device_ms_max': round(max(dms), 3),
                'bytes_up': int(mask.size), 'bytes_down': int(mask.size) * 8}
        if not args.device_only:
            host, hms = timed(lambda: T.distance_texture(mask, 'host'), args.calls, args.warmup)
            line.update({'host_ms_median': round(float(np.median(hms)), 3), 'host_ms_min': round(min(hms), 3), 'host_ms_max': round(max(hms), 3),
                         'host_over_device': round(float(np.median(hms) / np.median(dms)), 2),
                         'bit_identical': bool(np.array_equal(host.view(np.int64), dev.view(np.int64)))})
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
