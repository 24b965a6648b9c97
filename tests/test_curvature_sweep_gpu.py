"""Every swept case of tests/probe_cases.py through k_vertex_curvature (csrc/sdf_curvature.hip), the seventh kernel that inlines its own
copy of the tape interpreter, in a translation unit of its own built with the structurizer option of the interpreters
(csrc/build.units): what tests/test_probe_sweep_gpu.py does for the other six, with the same models and inputs (`pc.model`,
`pc.inputs`).  Both outputs are compared BIT FOR BIT with the definition (tests/curvature_ref.py) run over `Engine.eval_points` -- the
same interpreter arithmetic, so no tolerance, and a vertex without a curvature holds np.nan's bits by a select on both sides -- and,
for the tapes without libm calls (test_register_slots.is_trig), with the definition over the CPU checker: the status exactly, floats
equal with NaN == NaN.  Two steps: eps = pc.NORMAL_EPS, where the second differences of many fixtures are rounding noise (the
arithmetic is compared, not its meaning), and eps = pc.START, a quarter of the grid step.

The kernel's only data-independent trip count is 19: one `#pragma unroll 1` loop of 19 wave-uniform passes around the one
run_tape1, whatever the field's values -- a NaN or an infinite value changes a lane's status by a select, never a trip count.  It has no
data-dependent one.  Inside the interpreter the loops are those the head of test_probe_sweep_gpu.py lists (L_POLYGON, L_CIRC_PREP,
the bisection of grid3d_lookup).  The kernel stores through `i < n` guards on indices that come from the launch, not from the field.
So no case is host-only."""
import numpy as np
import pytest

import curvature_ref as ref
import probe_cases as pc
from sdf_amd import engine
from test_probe_sweep_gpu import adopted, differences
from test_register_slots import is_trig

pytestmark = pytest.mark.gpu


def _namespace():
    import sdf_amd
    return {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}


_NS = _namespace()
CASES = [n for n in pc.CASES if pc.swept(n, _NS)]               # (a tape with closures takes the definition on the host: nothing to sweep)
STEPS = (pc.NORMAL_EPS, pc.START)


@pytest.fixture(scope='module')
def soups(eng):
    """case -> the adopted soup of its input, uploaded once and closed when the module is done"""
    held = {}
    yield held
    for s in held.values():
        s.close()


def define(ev, pts, eps):
    curv, status = ref.curvature(ev, pts, eps)
    return {'curv': curv, 'status': status, 'counts': ref.counts(status)}


@pytest.mark.parametrize('name', CASES)
def test_curvature(name, ns, eng, oracle_lib, soups):
    f, t = pc.model(name, ns)
    soup, pts = pc.inputs(name, ns)
    mesh = adopted(soups, eng, name, ns)
    assert mesh.n_triangles == len(soup)
    bad = []
    for eps in STEPS:
        try:
            curv, status, counts = mesh.vertex_curvature(f, eps)
            dt = eng.tape_for(f)
            with np.errstate(all='ignore'):
                want = define(lambda P: eng.eval_points(dt, P), pts, eps)
        except engine.SdfHipError as e:                     # a HIP error: this session starts nothing more on the device
            pytest.exit('curvature %s: %s' % (name, e), returncode=3)
        got = {'curv': curv, 'status': status, 'counts': counts}
        bad += ['eps %g over eval_points: %s' % (eps, d) for d in differences(got, want, exact_nan=True)]
        if not is_trig(t):
            with np.errstate(all='ignore'):
                want = define(lambda P: oracle_lib.evaluate(f, P), pts, eps)
            bad += ['eps %g over the checker: %s' % (eps, d) for d in differences(got, want, exact_nan=False)]
    assert not bad, 'curvature %s against the definition: %s' % (name, '; '.join(bad))
