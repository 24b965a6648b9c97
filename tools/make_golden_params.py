#!/opt/conda/bin/python3.9
"""Generate tests/golden/values_params.npz by RUNNING the unmodified reference on the parameter sweep of
tests/param_cases.py (the sibling of tools/make_golden.py, same interpreter, same container):

    env -u PYTHONPATH /opt/conda/bin/python3.9 -W ignore tools/make_golden_params.py

Nothing here is imported by the product or by the tests; the tests read the .npz file.  What is recorded, per case, on
the shared point set P of values.npz (which is read, not regenerated):

  v_<name>   reference SDF values f(P), float64[600]
  e_<name>   the class name of the exception the reference raises while it builds or evaluates the model

and, for the one case whose samples are positive except for a plane of NaN (GENERATED), what the reference's `generate`
makes of it on a small grid -- a volume with a NaN in it passes skimage's range check and is marched, a NaN sample
counts as inside and the vertices next to it are NaN:

  g_<name>_bounds, g_<name>_step   the call's arguments
  g_<name>_kinds                   0 skipped / 1 empty / 2 nonempty per batch (as tools/make_golden.py records it)
  g_<name>_points                  the triangle soup, float64[3 T, 3]

Machine dependence: as for values.npz -- the cases that go through BLAS or libm change by a few ulp on another CPU, the
tests hold them to `value_tolerance`.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import sdf  # the reference  # noqa: E402
from sdf import core  # noqa: E402

import param_cases  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
NS = {k: getattr(sdf, k) for k in dir(sdf) if not k.startswith('_')}


GENERATED = {'extrude_to_zero': dict(bounds=((-1, -1, -1), (1, 1, 1)), step=0.25)}


def run_generate(name, bounds, step):
    grid_step = step
    kinds = []
    orig = core._worker

    def worker(sdf_, job, step, sparse):          # (the reference passes step and sparse by keyword)
        r = orig(sdf_, job, step, sparse)
        kinds.append(0 if r is None else (1 if len(r) == 0 else 2))
        return r
    core._worker = worker
    try:
        with np.errstate(all='ignore'):
            pts = core.generate(param_cases.build(name, NS), step=grid_step, bounds=bounds, workers=1, verbose=False)
    finally:
        core._worker = orig
    pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
    print('  generate %-25s %d triangles, %d coordinates NaN' % (name, len(pts) // 3, int(np.isnan(pts).sum())))
    return {'g_%s_bounds' % name: np.array(bounds, np.float64), 'g_%s_step' % name: np.array(grid_step, np.float64),
            'g_%s_kinds' % name: np.array(kinds, np.uint8), 'g_%s_points' % name: pts}


def gen_params(fname='values_params.npz'):
    P = np.load(os.path.join(OUT, 'values.npz'))['P']
    out = {}
    for name in param_cases.CASES:
        try:
            with np.errstate(all='ignore'):
                v = param_cases.build(name, NS)(P.copy()).reshape(-1)
        except Exception as e:
            out['e_' + name] = np.array(type(e).__name__)
            print('  %-34s raises %s: %s' % (name, type(e).__name__, e))
            continue
        assert v.dtype == np.float64 and v.shape == (len(P),)
        out['v_' + name] = v
        print('  %-34s NaN at %3d of %d points' % (name, int(np.isnan(v).sum()), len(P)))
    for name, kw in GENERATED.items():
        out.update(run_generate(name, **kw))
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **out)
    print(fname, len(param_cases.CASES), 'cases x', len(P), 'points,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen_params()
