"""Every swept case of tests/probe_cases.py through dual contouring on the device (csrc/sdf_dual.hip, `Engine.generate_dual`): what
tests/test_curvature_sweep_gpu.py does for the curvature probe, with the same models (`pc.model`), on the case's own 24^3 grid
(`pc.axes`) with eps = pc.NORMAL_EPS, once with the default regularisation and once without one (reg = 0: the mean fallback).  Every
output -- the crossing points and normals, the vertices, the cells, the soup, the eight counters, the blocks of the closing line -- is
compared BIT FOR BIT (`test_dual_gpu.same`) with the definition (tests/dual_ref.py) run over `Engine.eval_points`, the same
interpreter arithmetic, and, for the tapes without libm calls (test_register_slots.is_trig), with the definition over the CPU
checker.  tests/test_dual_sweep_host.py shows without a device what the table reaches: every counter, 229 cases with crossings and 61
that leave by the early return.

Read in csrc/sdf_dual.hip and csrc/sdf_dual.h before any case went to a device:
  * No trip count comes from data.  The seven kernels loop over the 3 axes, the 4 edges of a cell along an axis (12 in all) or the 4
    samples round one, the 6 corners of a quad, all `#pragma unroll` over constants; quadric_solve is straight-line code.  A NaN, an
    infinite value or a zero changes a flag or a select (differ && both, the clamp, is_flat / fell_back), never a count.  The unit
    holds no tape interpreter: it samples through sdf_eval_points and takes its normals through the launcher of k_vertex_normals,
    whose loops the head of test_probe_sweep_gpu.py lists, and which that sweep runs on every one of these tapes.
  * Every index that comes from a scan is checked before it addresses anything: k_dual_cross leaves at `e < 0 || e >= n_cross`,
    k_dual_cell_list stores only for `k >= 0 && k < n_active`, k_dual_vertex takes its sample from csample only for `k < n_active`,
    checks `s >= 0 && s < n` and that s is a cell's low corner before it gathers, and skips an edge with `e < 0 || e >= n_cross`;
    k_dual_emit leaves at `r < 0 || r >= n_quads`, at `a > 2`, at a sample whose four cells would lie below the grid and at a cell
    number outside [0, n_active).  The neighbours k_dual_classify and k_dual_cells read lie inside the grid by `idx[a] + 1 < n[a]`;
    the block a vertex marks is idx / bs < the block counts by the same bound.  What is left is indexed by the launch (`s < n`).
  * A crossing point is finite: its edge has two finite ends of which exactly one is negative, so v0 - v1 is not zero (it may
    overflow: t = 0), t = v0 / (v0 - v1) lies in [0, 1] -- 0 / (0 - v1) = 0 and v0 / v0 = 1 at a sample that is exactly 0 -- and
    lo + t * (hi - lo) lies on the edge of a finite grid.  So the normals launcher meets finite points only, which the probe sweep
    sends it for every tape; where the field is NaN beside a crossing the normal is the zero vector by that kernel's definition,
    and a cell whose system is not finite takes its crossings' mean, so the vertices are finite as well.  Only a normal could hold
    a NaN (an infinite difference: inf / inf), whose sign is the device's or glibc's; on this table none does
    (test_dual_sweep_host.py asserts it), so the comparison over the checker is by bits too.
  * A case without a crossing returns after the first scan, before anything sized by the crossings is allocated; a case whose
    crossings all lie on the border allocates no soup (n_quads == 0) and launches no k_dual_emit.
So no case is host-only.  A HIP error ends the session: nothing is started on the device after one."""
import numpy as np
import pytest

import dual_ref as ref
import probe_cases as pc
from sdf_amd import engine
from test_dual_gpu import same
from test_register_slots import is_trig

pytestmark = pytest.mark.gpu


def _namespace():
    import sdf_amd
    return {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}


_NS = _namespace()
HOST_ONLY = {}          # case -> why it is not sent to a device (see the head comment: none)
CASES = [n for n in pc.CASES if pc.swept(n, _NS) and n not in HOST_ONLY]      # (a tape with closures is refused before any launch)
REGS = (1e-3, 0.0)


@pytest.mark.parametrize('name', CASES)
def test_dual(name, ns, eng, oracle_lib):
    f, t = pc.model(name, ns)
    X, Y, Z = pc.axes(name, ns)
    n = (len(X), len(Y), len(Z))
    for reg in REGS:
        mesh = None
        try:
            dt = eng.tape_for(f)
            with np.errstate(all='ignore'):
                want = ref.dual(lambda P: eng.eval_points(dt, P), X, Y, Z, pc.NORMAL_EPS, reg)
            mesh = eng.generate_dual(f, X, Y, Z, pc.NORMAL_EPS, reg, parts=True)
        except engine.SdfHipError as e:                     # a HIP error: this session starts nothing more on the device
            pytest.exit('dual %s, reg = %g: %s' % (name, reg, e), returncode=3)
        try:
            same(mesh, want, '%s, reg = %g, over eval_points' % (name, reg), n)
            if not is_trig(t):
                with np.errstate(all='ignore'):
                    cpu = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, pc.NORMAL_EPS, reg)
                same(mesh, cpu, '%s, reg = %g, over the checker' % (name, reg), n)
        except engine.SdfHipError as e:                     # (the soup and the closing line are fetched by the comparison)
            pytest.exit('dual %s, reg = %g: %s' % (name, reg, e), returncode=3)
        finally:
            mesh.close()
