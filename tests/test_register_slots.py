"""The register files of k_mesh without a GPU.  sdf_mesh_inst.hip instantiates the meshing kernel once per register file
(saved-point slots, saved-distance slots) and family (plain / trig); the host picks the smallest file that holds the tape.
These tests restate that choice and check that the models of fixtures.SLOT_FIXTURES reach the file they are named after,
that every (family, file) cell is reached by some model, that the checker agrees with the reference on those models, and
that the lowering refuses a ninth slot.  The GPU side (every cell and scheme against the checker) is in test_gpu.py."""
import os

import numpy as np
import pytest

import fixtures
from conftest import GOLDEN, value_tolerance
from sdf_amd import ease, tape

# csrc/sdf_generate.hip launch_mesh `kFile`: index = the register file's number (SDF_MESH_SLOTS)
REGISTER_FILES = ((1, 1), (2, 2), (4, 2), (2, 4), (4, 4), (8, 8))

_TRIG_EASES = {ease.EASING_IDS[n] for n in ('in_sine', 'out_sine', 'in_out_sine', 'in_expo', 'out_expo', 'in_out_expo',
                                            'in_elastic', 'out_elastic', 'in_out_elastic')}


def is_trig(t):
    """csrc/sdf_ctx.hip tape_needs_full: the tape is meshed by the trig family (sdf_launch_mesh_f64_full)"""
    for i in range(t.n_instr):
        op = tape.OP_NAMES[int(t.code[2 * i]) & 255]
        c = t.consts[(int(t.code[2 * i + 1]) & tape.COFF_MASK) + 1:]
        if op in ('TWIST', 'BEND', 'BEND_RADIAL', 'WRAP_AROUND', 'CIRC_PREP', 'CIRC_SET', 'TRANS_RAD_PRE'):
            return True
        if (op == 'BEND_LINEAR' and int(c[10]) in _TRIG_EASES) or (op == 'TRANS_LIN_PRE' and int(c[7]) in _TRIG_EASES) \
                or (op == 'EXTTO_PRE' and int(c[1]) in _TRIG_EASES):
            return True
    return False


def files_holding(t):
    """the register files whose slots hold the tape's, smallest first (the first one is launch_mesh's choice; SDF_MESH_SLOTS
    may force any of them)"""
    np_, nd = max(t.n_pslots, 1), max(t.n_dslots, 1)
    return [k for k, (p, d) in enumerate(REGISTER_FILES) if np_ <= p and nd <= d]


def mesh_cell(t):
    """(family, register file) of k_mesh that meshes tape t"""
    return ('trig' if is_trig(t) else 'plain', REGISTER_FILES[files_holding(t)[0]])


def named_cell(name):
    """slots_<family>_<P>_<D>[_...]: the cell a slot model is meant for"""
    parts = name.split('_')
    return parts[1], (int(parts[2]), int(parts[3]))


SLOTS = sorted(fixtures.SLOT_FIXTURES)


@pytest.fixture(scope='module')
def slot_tapes(ns):
    return {name: tape.lower(fixtures.build(name, ns)) for name in SLOTS}


@pytest.fixture(scope='module')
def values_slots():
    return np.load(os.path.join(GOLDEN, 'values_slots.npz'))


def test_slot_models_lower_to_the_register_file_they_are_named_after(slot_tapes):
    for name, t in slot_tapes.items():
        assert mesh_cell(t) == named_cell(name), (name, t.n_pslots, t.n_dslots)
    # the edges of the (8,8) file and the length at which the library picks the two-pass scheme by itself (n_instr > 96)
    big = [t for t in slot_tapes.values() if mesh_cell(t)[1] == (8, 8)]
    assert any(t.n_pslots == 8 for t in big) and any(t.n_dslots == 8 for t in big)
    assert any(max(t.n_pslots, t.n_dslots) == 5 for t in big)
    assert any(t.n_instr > 96 and max(t.n_pslots, t.n_dslots) >= 5 for t in slot_tapes.values())


def test_every_family_and_register_file_is_reached(ns, slot_tapes):
    """the value fixtures and the slot models together reach all 12 (family, register file) cells of k_mesh"""
    reached = {}
    for name in sorted(fixtures.FIXTURES):
        reached.setdefault(mesh_cell(tape.lower(fixtures.build(name, ns))), []).append(name)
    for name, t in slot_tapes.items():
        reached.setdefault(mesh_cell(t), []).append(name)
    want = {(fam, f) for fam in ('plain', 'trig') for f in REGISTER_FILES}
    missing = sorted(want - set(reached))
    assert not missing, 'k_mesh cells no model reaches: %r' % missing
    print('\n'.join('%-5s %s: %d models, e.g. %s' % (fam, f, len(reached[fam, f]), reached[fam, f][0])
                    for fam, f in sorted(want)))


@pytest.mark.parametrize('name', SLOTS)
def test_checker_matches_reference_on_slot_models(name, ns, values_slots, oracle_lib):
    P = values_slots['P']
    ref = values_slots['v_' + name]
    v = oracle_lib.evaluate(fixtures.build(name, ns), P)
    assert np.array_equal(np.isnan(v), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.all(np.abs(v[ok] - ref[ok]) <= value_tolerance(ref[ok], P[ok]))


def test_checker_bounds_match_reference_on_slot_models(ns, oracle_lib):
    b = np.load(os.path.join(GOLDEN, 'bounds_slots.npz'))
    assert sorted(b.files) == SLOTS
    for name in SLOTS:
        got = np.array(oracle_lib.estimate_bounds(fixtures.build(name, ns)))
        # (np.dot inside capsule / rotate: a probe value within a few ulp of the threshold may move a bound by one cell)
        cell = np.ptp(b[name], axis=0) / 14.0
        assert np.all(np.abs(got - b[name]) <= 1.01 * cell), name
        assert np.all(np.ptp(b[name], axis=0) < 10.0), name          # a surface within a few units of the origin


def _nested(ns, n, kind):
    f = ns['sphere'](0.3)
    for i in range(n + 1):
        if kind == 'p':       # a transform over a union whose left operand moves the point: one saved point per level
            f = (f | ns['sphere'](0.2).translate((0.3, 0, 0))).translate((0.05 * i, 0, 0))
        else:                 # a right operand that is itself a boolean: one saved distance per level
            f = ns['box'](0.8 + 0.2 * i) - f
    return f


def test_the_lowering_takes_eight_slots_and_refuses_a_ninth(ns):
    assert tape.MAX_P_SLOTS == 8 and tape.MAX_D_SLOTS == 8          # csrc/opcodes.h SDF_NP_SLOTS / SDF_ND_SLOTS
    t = tape.lower(_nested(ns, 8, 'p'))
    assert (t.n_pslots, t.n_dslots) == (8, 0)
    t = tape.lower(_nested(ns, 8, 'd'))
    assert (t.n_pslots, t.n_dslots) == (0, 8)
    with pytest.raises(ValueError, match='more than 8 saved-point slots'):
        tape.lower(_nested(ns, 9, 'p'))
    with pytest.raises(ValueError, match='more than 8 saved-distance slots'):
        tape.lower(_nested(ns, 9, 'd'))
