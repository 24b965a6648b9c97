"""What the dual-contouring sweep of tests/test_dual_sweep_gpu.py reaches, shown without a device: the definition (tests/dual_ref.py)
over the CPU checker on every swept case of tests/probe_cases.py, on the case's 24^3 grid (`pc.axes`) with eps = pc.NORMAL_EPS, for
both regularisations of the sweep.  Every one of the eight counters is non-zero somewhere, the mean fallback is taken only without
a regularisation, and the cases split into those with crossings and those that leave by the early return (the NaN, infinite and
degenerate models).  The numbers of cases with and without crossings are pinned as they are: a change of the table or of the
definition that moves them is to be looked at.  No GPU: both passes take a few seconds."""
import numpy as np
import pytest

import dual_ref as ref
import probe_cases as pc

REGS = (1e-3, 0.0)                                                     # the sweep's: the default, and none (the mean fallback)
WITH_CROSSINGS, WITHOUT_CROSSINGS = 229, 61


@pytest.fixture(scope='module')
def over_the_checker(ns, oracle_lib):
    """reg -> case -> the eight counters of the definition over the CPU checker"""
    out = {reg: {} for reg in REGS}
    with np.errstate(all='ignore'):
        for name in pc.CASES:
            if not pc.swept(name, ns):
                continue
            f = pc.model(name, ns)[0]
            X, Y, Z = pc.axes(name, ns)
            for reg in REGS:
                d = ref.dual(lambda P: oracle_lib.evaluate(f, P), X, Y, Z, pc.NORMAL_EPS, reg)
                # (no output holds a NaN or an infinity: the device comparison over the checker can be by bits, with no word on a NaN's sign)
                assert np.isfinite(d.points).all() and np.isfinite(d.normals).all() and np.isfinite(d.vertices).all(), (name, reg)
                assert d.cells.shape == (d.stats['triangles'], 3) and (len(d.points), len(d.vertices)) == (d.stats['crossings'], d.stats['cells'])
                out[reg][name] = d.stats
    return out


def reaching(stats, key):
    return sorted(n for n, st in stats.items() if st[key] > 0)


def test_the_sweep_reaches_every_counter(over_the_checker):
    R = over_the_checker
    assert list(R[1e-3]) == list(R[0.0]) and len(R[0.0]) >= 285
    for reg in REGS:
        for name, st in R[reg].items():
            assert list(st) == list(ref.STAT_KEYS) and min(st.values()) >= 0, (reg, name)
            assert st['triangles'] == 2 * (st['crossings'] - st['open_edges']), (reg, name)
            assert st['clamped'] + st['mean_fallback'] + st['flat'] <= st['cells'] <= 4 * st['crossings'], (reg, name)
            assert (st['crossings'] > 0) == (st['cells'] > 0), (reg, name)
    for reg in REGS:
        print('reg = %g: ' % reg + ', '.join('%s in %d cases' % (key, len(reaching(R[reg], key))) for key in ref.STAT_KEYS))
    for key in ref.STAT_KEYS:                                          # every counter is non-zero in at least one case
        assert any(reaching(R[reg], key) for reg in REGS), key
    # what does not depend on the regularisation: the crossings, the cells, the triangles, the two edge counters, the flat cells
    for name in R[0.0]:
        for key in ('crossings', 'cells', 'triangles', 'open_edges', 'nonfinite_edges', 'flat'):
            assert R[0.0][name][key] == R[1e-3][name][key], (name, key)
    # the mean fallback: a singular system, so only without a regularisation
    assert reaching(R[1e-3], 'mean_fallback') == []
    fallback = reaching(R[0.0], 'mean_fallback')
    assert fallback
    flat, nonfinite = reaching(R[1e-3], 'flat'), reaching(R[1e-3], 'nonfinite_edges')
    print('flat: %r; nonfinite_edges: %r; mean_fallback at reg = 0: %d cases' % (flat, nonfinite, len(fallback)))
    assert 'sphere_tiny' in flat
    assert {'ellipsoid', 'ellipsoid_flat'} <= set(nonfinite)
    for reg in REGS:
        assert len(reaching(R[reg], 'clamped')) >= 100 and len(reaching(R[reg], 'open_edges')) >= 50, reg


def test_cases_with_and_without_crossings(over_the_checker):
    """the early return (no crossing: nothing sized by the surface is allocated) and the full path both occur, in these numbers"""
    for reg in REGS:
        st = over_the_checker[reg]
        crossing = reaching(st, 'crossings')
        none = sorted(set(st) - set(crossing))
        print('reg = %g: %d cases with crossings, %d without: %r' % (reg, len(crossing), len(none), none))
        assert (len(crossing), len(none)) == (WITH_CROSSINGS, WITHOUT_CROSSINGS)
        for name in none:                                              # nothing but the non-finite edges is counted without a crossing
            assert {k: v for k, v in st[name].items() if k != 'nonfinite_edges'} == dict.fromkeys([k for k in ref.STAT_KEYS if k != 'nonfinite_edges'], 0), name
