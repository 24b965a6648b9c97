"""`SDF_PRECISION_F32` on the device: run_tape<float, ...> behind sdf_eval_points*, sdf_eval_grid_host, sdf_estimate_bounds,
sdf_skip_kinds and the two closure entry points, held to the float64 CPU checker within max(16, 4 E) units, E being what the float32
build of the same checker loses on the same model and points (float32_ref.py; test_float32_host.py pins E without a GPU).  The
kernels that exist in float only -- k_estimate_bounds_w<float>, k_skip<float>, k_eval_points_ext<float> -- are compared with the same
rule restated in NumPy over eval_points under F32, or with each other, bit for bit.  All need an MI355X."""
import contextlib
import os
import sys

import numpy as np
import pytest

import fixtures
import float32_ref as fr
import oracle
from conftest import GOLDEN, ROOT
from sdf_amd import core, engine, ir, mesh, tape
from test_register_slots import is_trig

pytestmark = pytest.mark.gpu

ALL = sorted(fixtures.FIXTURES) + sorted(fixtures.SLOT_FIXTURES)
TEXTURES = ('frame', 'blobs', 'noise')
GRIDS = ('torus', 'two_spheres', 'noise')


@contextlib.contextmanager
def float32(eng):
    eng.precision = engine.PRECISION_F32
    try:
        yield eng
    finally:
        eng.precision = engine.PRECISION_F64


@pytest.fixture(scope='module')
def P():
    return fr.points()


def _held_to_the_checker(eng, f, P, label):
    """the rule of this module: NaN where the float64 checker has NaN, else within max(16, 4 E) units of it"""
    v64, e = fr.envelope(oracle, f, P)
    T = fr.tolerance_units(e)
    with float32(eng):
        v = eng.eval_points(f, P)
    assert v.shape == (len(P),) and v.dtype == np.float64
    assert np.array_equal(np.isnan(v), np.isnan(v64)), label
    d = fr.in_units(v, v64, P)
    ok = ~np.isnan(d)
    worst = float(d[ok].max()) if ok.any() else 0.0
    print('%s: device %.2f units, checker E %.2f, bound %.1f' % (label, worst, fr.e_max(e), T))
    assert np.all(d[ok] <= T), (label, worst, T, P[ok][np.argmax(d[ok])])
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64), equal_nan=True), label    # float32 values, widened


# ---- a. values, every fixture ----------------------------------------------------------------

@pytest.mark.parametrize('name', ALL)
def test_float32_values_of_every_fixture(name, ns, eng, P):
    _held_to_the_checker(eng, fixtures.build(name, ns), P, name)


def _pictures():
    from test_oracle import _pictures as pictures
    return pictures()


def _grids():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_custom as mgc
    return mgc.grids()


def _texture_model(ns, name):
    arr, kw = _pictures()[name]
    return ns['image'](arr, **kw)


def _grid_model(name):
    X, Y, Z, A, bg, bb = _grids()[name]
    return mesh.grid_sdf((X, Y, Z), A, bg, bb), (X, Y, Z), bb


def test_the_float_trig_interpreter_is_reached(ns):
    """run_tape<float, FULL = true> is what LAUNCH_TAPE picks for a tape that `tape_needs_full` (csrc/sdf_ctx.hip; restated by
    test_register_slots.is_trig): several models of test a have one, and several the plain build"""
    full = [name for name in ALL if is_trig(tape.lower(fixtures.build(name, ns)))]
    assert len(full) >= 10 and len(ALL) - len(full) >= 10, full
    assert {'ex_gearlike', 'twist', 'circular_array', 'wrap_around', 'ease_in_out_elastic', 'slots_trig_8_8'} <= set(full)


def test_every_opcode_runs_in_float32(ns):
    """every opcode of csrc/opcodes.h except END, NOP and L_EXTERN occurs in a tape that tests a and b evaluate under F32.  The two
    sampled-field leaves are in the models of test b only.  LOAD_P / SAVE_P / PUSH_D reach the device as the RL / SV / PD prefixes
    of the instruction behind them (tape.peephole folds every one of them in these models): the prefix is counted as the opcode."""
    count = dict.fromkeys(tape.OP_NAMES, 0)
    models = [fixtures.build(name, ns) for name in ALL] + [_texture_model(ns, n).extrude(0.4) for n in TEXTURES] \
        + [_grid_model(n)[0] for n in GRIDS]
    for f in models:
        code = tape.lower(f).code
        for w0 in code[0::2]:
            w0 = int(w0)
            count[tape.OP_NAMES[w0 & 255]] += 1
            count['LOAD_P'] += bool(w0 & tape.RL_FLAG)
            count['SAVE_P'] += bool(w0 & tape.SV_FLAG)
            count['PUSH_D'] += bool(w0 & tape.PD_FLAG)
    assert len(count) == 69                                                                # OP_COUNT
    missing = sorted(op for op, n in count.items() if n == 0 and op not in ('END', 'NOP', 'L_EXTERN'))
    assert not missing, missing
    assert count['END'] == len(models)


# ---- b. texture and grid leaves: dimensions and strides carried as floats in d_c32 --------------

TEX = np.load(os.path.join(GOLDEN, 'texture.npz'))
GRID3D = np.load(os.path.join(GOLDEN, 'grid3d.npz'))


@pytest.mark.parametrize('name', TEXTURES)
def test_float32_image_leaf(name, ns, eng):
    f = _texture_model(ns, name)
    P2 = fr.part2_points(TEX['p2_' + name])
    x0, y0, x1, y1 = ir.unwrap(f).params[:4]                             # the texture's rectangle (oracle/sdf_oracle.c NODE_texture2d)
    inside = (P2[:, 0] > x0) & (P2[:, 0] < x1) & (P2[:, 1] > y0) & (P2[:, 1] < y1)
    assert inside.sum() >= 30 and (~inside).sum() >= 30                   # the bilinear look-up and the fallback rectangle
    _held_to_the_checker(eng, f, P2, 'image ' + name)
    P3 = np.concatenate([P2, np.linspace(-0.5, 0.5, len(P2)).reshape(-1, 1)], axis=1)
    _held_to_the_checker(eng, f.extrude(0.4), fr.part2_points(P3), 'extruded image ' + name)


@pytest.mark.parametrize('name', GRIDS)
def test_float32_grid_leaf(name, ns, eng):
    f, axes, bb = _grid_model(name)
    P = fr.part2_points(GRID3D['p_' + name])
    in_box = np.all((P > np.array(bb[0])) & (P < np.array(bb[1])), axis=1)
    in_grid = np.all((P > [a[0] for a in axes]) & (P < [a[-1] for a in axes]), axis=1)
    assert in_box.sum() >= 30 and (~in_grid).sum() >= 30                  # interpolated voxels, and the box distance outside them
    _held_to_the_checker(eng, f, P, 'grid ' + name)
    g = f.translate((0.05, -0.03, 0.02)) | ns['sphere'](0.2).translate((0, 0, 0.5))
    _held_to_the_checker(eng, g, P, 'grid under operators ' + name)


# ---- c. closures: k_eval_points_ext<float>, both passes ------------------------------------------

CUSTOM = np.load(os.path.join(GOLDEN, 'custom.npz'))


@pytest.mark.parametrize('name', sorted(fixtures.CUSTOM_FIXTURES))
def test_float32_closures_match_reference(name, ns, eng):
    """the float checker cannot run user code: the reference's own values (custom.npz) and the project's float32 bound,
    1e-5 max(1, |P|inf) (test_float32_mode_is_close).  custom.npz is sampled at the points of values.npz; the rows kept are
    part 2's, and rounding them to float32 -- which the kernel does anyway -- moves a value by 6e-8 |P| at most."""
    assert np.array_equal(CUSTOM['P'], np.load(os.path.join(GOLDEN, 'values.npz'))['P'])
    keep = np.abs(CUSTOM['P']).max(axis=1) <= 16.0
    P = fr.part2_points(CUSTOM['P'])
    ref = CUSTOM['v_' + name][keep]
    f = fixtures.build(name, ns)
    dt = eng.tape_for(f)
    assert dt.tape.externs
    with float32(eng):
        v = eng._eval_points_hybrid(dt, P)
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(v), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(v - ref)[ok] / np.maximum(1.0, np.abs(P).max(axis=1))[ok]
    print('%s: %.3g of the bound 1e-5' % (name, err.max() / 1e-5))
    assert np.all(err <= 1e-5)


# ---- d. grid indexing ------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(7, 5, 3), (1, 1, 1)], ids=['7x5x3', '1x1x1'])
@pytest.mark.parametrize('name', ['ex_example', 'twist'])
def test_float32_eval_grid_is_eval_points_on_the_product(name, shape, ns, eng):
    """the same interpreter on the same float32 inputs: the same bits, in the reference's order (first axis slowest)"""
    f = fixtures.build(name, ns)
    X = np.linspace(-1.13, 1.21, shape[0]); Y = np.linspace(-0.97, 1.07, shape[1]); Z = np.linspace(-1.31, 0.83, shape[2])
    with float32(eng):
        vol = eng.eval_grid(f, X, Y, Z)
        pts = eng.eval_points(f, core._cartesian_product(X, Y, Z))
    assert vol.shape == shape and pts.shape == (shape[0] * shape[1] * shape[2],)
    assert vol.tobytes() == pts.tobytes()
    assert np.array_equal(vol, vol.astype(np.float32).astype(np.float64))


# ---- e. the skip test: k_skip<float> ---------------------------------------------------------------

def _skip_rule(values, boxes):
    """reference sdf/core.py:28-43 for every batch at once.  values: (nb, 9), centre first, then the corners in
    itertools.product((x0, x1), (y0, y1), (z0, z1)) order; the centre distance in float64 as `skip_body` has it"""
    lo, hi = boxes
    mid = (lo + hi) / 2
    d = np.sqrt(((mid[:, 0] - lo[:, 0]) ** 2 + (mid[:, 1] - lo[:, 1]) ** 2) + (mid[:, 2] - lo[:, 2]) ** 2)
    r = np.abs(values[:, 0])
    corners = values[:, 1:]
    same = np.where(corners[:, :1] > 0, corners > 0, corners < 0).all(axis=1)
    return np.where(~(r <= d) & same, 0, 255).astype(np.uint8)


def _batch_probes(X, Y, Z, bs):
    """(nb, 9, 3) probes and the boxes of the batches, Z fastest (reference sdf/core.py:119)"""
    def spans(A):
        return [(A[o], A[min(o + bs, len(A) - 1)]) for o in range(0, len(A), bs)]
    lo, hi = [], []
    for x0, x1 in spans(X):
        for y0, y1 in spans(Y):
            for z0, z1 in spans(Z):
                lo.append((x0, y0, z0)); hi.append((x1, y1, z1))
    lo, hi = np.array(lo), np.array(hi)
    sel = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=bool)
    corners = np.where(sel[None, :, :], hi[:, None, :], lo[:, None, :])
    return np.concatenate([((lo + hi) / 2)[:, None, :], corners], axis=1), (lo, hi)


@pytest.mark.parametrize('name,bounds', [('ex_example', ((-2.05, -1.9, -2.2), (2.1, 2.3, 1.95))),
                                         ('ex_gearlike', ((-4.05, -3.9, -2.2), (4.1, 4.3, 1.95)))])
def test_float32_skip_verdicts_follow_the_reference_rule(name, bounds, ns, eng):
    import torch
    f = fixtures.build(name, ns)
    X, Y, Z, _ = core.grid_axes(bounds, samples=2 ** 15)
    bs = 8
    assert (len(X) - 1) % bs or (len(Y) - 1) % bs or (len(Z) - 1) % bs                       # ragged last batches
    probes, boxes = _batch_probes(X, Y, Z, bs)
    nb = len(probes)
    world = 3
    piece = -(-nb // world)
    buf = torch.full((piece * world,), 77, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    with float32(eng):
        for r in (2, 0, 1):
            eng.skip_kinds(f, X, Y, Z, bs, min(nb, piece * r), min(nb, piece * (r + 1)), buf.data_ptr())
        values = eng.eval_points(f, np.ascontiguousarray(probes.reshape(-1, 3))).reshape(nb, 9)
    got = buf.cpu().numpy()
    assert (got[nb:] == 77).all()
    want = _skip_rule(values, boxes)
    assert got[:nb].tobytes() == want.tobytes()
    assert (want == 0).sum() >= 3 and (want == 255).sum() >= 3


# ---- f. bounds: k_estimate_bounds_w<float> against the host loop around eval_grid --------------------

BOUNDS = np.load(os.path.join(GOLDEN, 'bounds.npz'))


@pytest.mark.parametrize('name', ['ex_example', 'ex_gearlike', 'torus'])
def test_float32_bounds_in_one_launch_equal_the_host_loop(name, ns, eng):
    assert engine.get_engine() is eng                                     # (core._estimate_bounds asks for the engine itself)
    f = fixtures.build(name, ns)
    with float32(eng):
        one_launch = eng.estimate_bounds(f)
        host_loop = core._estimate_bounds(f)                              # float32: the reference's loop, probes by eval_grid
    assert one_launch is not None
    a, b = np.array(one_launch), np.array(host_loop)
    assert a.shape == (2, 3) and a.tobytes() == b.tobytes()
    want = BOUNDS[name]
    last_cell = np.ptp(want, axis=0) / 14.0               # (test_device_bounds_match_reference_for_every_fixture: 16 probes, grown by half a cell)
    assert np.all(np.abs(a - want) <= 1.01 * last_cell + 1e-9), (name, a, want)
