"""Every case of tests/probe_cases.py through the six kernels that inline their own copy of the tape interpreter: k_vertex_normals
(csrc/sdf_normals.hip), k_vertex_thickness (sdf_thickness.hip), k_support_rays (sdf_supports.hip), k_triangle_deviation and
k_vertex_snap (sdf_deviation.hip), k_render (sdf_render.hip).  Each is a translation unit of its own, built with the structurizer
option of the interpreters (csrc/build.units): the jump table, the register-file tricks and the outlined libm bodies of
`run_tape1` are generated once per unit, around other live state, so a wrong label or a clobbered register would belong to ONE
kernel and ONE opcode.  The unit tests of these kernels run a handful of models (14 opcodes); `sdf_eval_points` is held to the
checker on every tape (test_gpu.py, test_params_gpu.py).  Here every output array of every kernel is compared BIT FOR BIT with
the kernel's NumPy definition run over `Engine.eval_points` -- the same interpreter arithmetic, so no tolerance -- and, for the
tapes without libm calls (test_register_slots.is_trig), with the definition over the CPU checker: integers exactly, floats
equal with NaN == NaN (the sign of a NaN is the device's or glibc's).  tests/test_probe_sweep_host.py shows without a device
that the sweep holds every opcode, post code and easing id and reaches every status.

Loops of the six kernels whose trip count comes from data, read before any case went to a device (as the head of
test_params_gpu.py does for the interpreter itself):
  * k_vertex_normals: six passes, a constant.
  * k_vertex_thickness: six passes, then the march -- left when no lane of the wave marches or after `max_steps` passes --,
    then `refine` passes, entered only for refine > 0.  k_support_rays: the same without the six.  k_render: the march
    (`max_steps`), `refine` passes (entered only for refine > 0), six passes.  max_steps >= 1 and refine >= 0 are checked on
    the host by every entry (thickness.check_params, supports.check_params, sdf_render_host), again in the C entry.
  * k_triangle_deviation: (order + 1)(order + 2) / 2 samples, order in 1 .. 8 checked on the host.
  * k_vertex_snap: `iters` rounds of one value pass and six gradient passes, then the final value pass (`pass == iters`);
    iters >= 1 checked on the host.
  Every one of these counters is wave-uniform and none depends on a value of the field: a NaN or an infinite value changes a
  lane's status by a select, never a trip count.  An infinite step makes t infinite, which ends the ray (beyond t_far / at the
  bed); a NaN ends it with its NaN status.
  * inside the interpreter: L_POLYGON's vertex count and L_CIRC_PREP's rotation count, both written by the lowering (see
    test_params_gpu.py), and the bisection of grid3d_lookup over an axis of n grid lines: `while (lo < hi)` on integers with
    hi - lo halved every pass, at most floor(log2 n) + 1 passes whatever the coordinate (a NaN coordinate compares as behind
    everything); its trip count differs from lane to lane when n is no power of two, inside a unit built with the structurizer
    option, which is what the three grid cases are here for.  Its indices are clamped to [0, n - 2] before any load, those of
    L_TEXTURE2D to the texture.
The kernels store through `i < n` guards on indices that come from the launch, not from the field.  So no case is host-only."""
import numpy as np
import pytest

import probe_cases as pc
from deviation_ref import bits
from sdf_amd import engine
from test_register_slots import is_trig
from test_thickness_gpu import Soup

pytestmark = pytest.mark.gpu

HOST_ONLY = {}          # case -> why it is not sent to a device (see the head comment: none)
CASES = [n for n in pc.CASES if n not in HOST_ONLY]


@pytest.fixture(scope='module')
def soups(eng):
    """case -> the adopted soup of its input, uploaded once and closed when the module is done"""
    held = {}
    yield held
    for s in held.values():
        s.close()


def adopted(soups, eng, name, ns):
    if name not in soups:
        soups[name] = Soup(eng, pc.inputs(name, ns)[0])
    return soups[name].mesh


def device(probe, eng, f, mesh):
    """the outputs of one probe's kernel, under the names of `probe_cases.define`: the entry its unit test calls"""
    if probe == 'normals':
        n, n_flat = mesh.vertex_normals(f, pc.NORMAL_EPS)
        return {'normal': np.array(n), 'n_flat': np.int64(n_flat)}
    if probe == 'thickness':
        th, status, steps = mesh.vertex_thickness(f, **pc.THICKNESS)
        return {'thickness': th, 'status': status, 'steps': steps}
    if probe == 'supports':
        raw = mesh.support_rays(f, pc.DIRECTION[None], **pc.SUPPORTS)
        tri, height, status, steps, origin = raw['rays'][0]
        assert raw['counts'].dtype == np.int64
        return {'triangle': tri, 'height': height, 'status': status, 'steps': steps, 'origin': origin, 'sums': raw['sums'][0],
                'counts': raw['counts'][0], 'lo': np.float64(raw['lo'][0]), 'hi': np.float64(raw['hi'][0])}
    if probe == 'deviation':
        dev, at, sumsq = mesh.triangle_deviation(f, pc.ORDER)
        return {'dev': dev, 'at': at, 'sumsq': sumsq}
    if probe == 'snap':
        moved = mesh.snap(f, **pc.SNAP)
        try:
            q, status, residual = moved.snap_result
            return {'points': q, 'status': status, 'residual': residual, 'evals': moved.snap_evals}
        finally:
            moved.close()
    if probe == 'render':
        frame, par = pc.render_setup()
        r = eng.render_buffers(f, frame, pc.WIDTH, pc.HEIGHT, **par)
        return {k: r[k] for k in ('depth', 'normal', 'steps', 'status')}
    raise KeyError(probe)


def differences(got, want, exact_nan):
    """the outputs that differ, as text: the same names, types and shapes; float64 by its bits (exact_nan) or with NaN == NaN,
    everything else exactly"""
    out = []
    if list(got) != list(want):
        return ['outputs %r / %r' % (list(got), list(want))]
    for key in want:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.dtype != w.dtype or g.shape != w.shape:
            out.append('%s: %s %r / %s %r' % (key, g.dtype, g.shape, w.dtype, w.shape))
            continue
        g, w = g.reshape(-1), w.reshape(-1)
        if g.dtype == np.float64:
            bad = bits(g) != bits(w)
            only_nan = bad & np.isnan(g) & np.isnan(w)
            if not exact_nan:
                bad = bad & ~only_nan
        else:
            bad = g != w
            only_nan = np.zeros(len(g), bool)
        if bad.any():
            i = np.flatnonzero(bad)[0]
            out.append('%s: %d of %d differ (%d of them NaN on both sides), first at %d: %r / %r' % (key, bad.sum(), bad.size, (bad & only_nan).sum(), i, g[i], w[i]))
    return out


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('probe', pc.PROBES)              # (the simplest kernel first: all cases of a probe, then the next probe)
def test_probe(probe, name, ns, eng, oracle_lib, soups):
    f, t = pc.model(name, ns)
    soup, pts = pc.inputs(name, ns)
    mesh = adopted(soups, eng, name, ns)
    assert mesh.n_triangles == len(soup)
    try:
        got = device(probe, eng, f, mesh)
        dt = eng.tape_for(f)
        with np.errstate(all='ignore'):
            want = pc.define(probe, lambda P: eng.eval_points(dt, P), soup, pts)
    except engine.SdfHipError as e:                         # a HIP error: this session starts nothing more on the device
        pytest.exit('%s %s: %s' % (probe, name, e), returncode=3)
    bad = ['over eval_points: ' + d for d in differences(got, want, exact_nan=True)]
    if not is_trig(t):
        with np.errstate(all='ignore'):
            want = pc.define(probe, lambda P: oracle_lib.evaluate(f, P), soup, pts)
        bad += ['over the checker: ' + d for d in differences(got, want, exact_nan=False)]
    assert not bad, '%s %s against the definition %s' % (probe, name, '; '.join(bad))


def test_the_weld_of_every_input_is_the_definitions(ns, eng, soups):
    """the vertex order the per-vertex kernels work in is np.unique's, which the definitions are given"""
    for name in CASES:
        got = adopted(soups, eng, name, ns).weld()[0]
        want = pc.inputs(name, ns)[1]
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), name
