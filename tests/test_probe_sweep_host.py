"""The probe sweep of tests/probe_cases.py on the host: the table is what it says, its inputs have the shapes the kernels can go
wrong at, the swept tapes hold every opcode a device kernel can meet, and the six definitions (normals_ref, thickness_ref,
supports_ref, deviation_ref x 2, render_ref) run over the CPU checker reach the states that make the device comparison of
tests/test_probe_sweep_gpu.py worth something.  No GPU: all definitions over all cases take a few seconds."""
import builtins
import os
import re

import numpy as np
import pytest

import deviation_ref
import fixtures
import param_cases
import probe_cases as pc
import supports_ref
import thickness_ref
from sdf_amd import ir, tape

OPCODES_H = os.path.join(pc.ROOT, 'sdf_amd', 'csrc', 'opcodes.h')

# The opcodes of csrc/opcodes.h that are the OP BYTE of no instruction of any swept tape, each with the reason.  A new opcode
# without a sweep case fails test_every_opcode_is_swept until a case holds it.
NEVER_AN_OP_BYTE = {
    'L_EXTERN': 'a user closure: the six kernels refuse such a tape, the definition runs on the host (probe_cases.swept)',
    'NOP': 'never lowered: only the interval prepass writes it, into its own pruned copy of a tape (sdf_prune.h), which no probe kernel reads',
    # tape.peephole folds every one of these three into a prefix of the instruction behind it -- in all 290 tapes, the 8 + 8 slot
    # models included, none is left as an instruction of its own -- and the prefixes RL, SV and PD all occur (asserted below): the
    # kernels run their work, through the prefix path of the dispatch
    'LOAD_P': 'always the RL prefix of the next instruction',
    'SAVE_P': 'always the SV prefix of the next instruction',
    'PUSH_D': 'always the PD prefix of the next instruction',
}


def _exception_class(name):
    return getattr(ir, name, None) or getattr(builtins, name)


def test_the_table_is_every_case_of_the_suite(ns, oracle_lib):
    names = set(pc.CASES)
    assert set(fixtures.FIXTURES) | set(fixtures.SLOT_FIXTURES) | set(pc.SAMPLED) | set(pc.EXTRA) <= names
    assert names & set(param_cases.CASES) == set(param_cases.CASES) - set(pc.RAISES) and set(pc.RAISES) <= set(param_cases.CASES)
    assert len(pc.SAMPLED) == 6 and len(pc.RAISES) == 6
    # the cases left out raise, in the builder, the lowering or the first evaluation, what RAISES says
    for name, cls in pc.RAISES.items():
        with pytest.raises(_exception_class(cls)) as info:
            f = param_cases.build(name, ns)
            tape.lower(f)
            oracle_lib.evaluate(f, np.zeros((1, 3)))
        assert type(info.value) is _exception_class(cls), (name, type(info.value))
    # every other one builds, lowers and has no closures: none is left to the host path
    not_swept = [n for n in pc.CASES if not pc.swept(n, ns)]
    assert not_swept == [] and 285 <= len(pc.CASES) <= 400, (not_swept, len(pc.CASES))
    for name in pc.SAMPLED:
        ops = pc.census(pc.model(name, ns)[1])[0]
        assert ('L_TEXTURE2D' if name.startswith('image_') else 'L_GRID3D') in ops, name


def test_the_inputs_have_ragged_sizes(ns, oracle_lib):
    sizes = {}
    for name in pc.CASES:
        soup, pts = pc.inputs(name, ns)
        assert soup.dtype == np.float64 and soup.ndim == 2 and soup.shape[1] == 9 and np.isfinite(soup).all(), name
        assert pc.N_RANDOM <= len(soup) <= pc.MAX_TRIS + pc.N_RANDOM and 3 * pc.N_RANDOM <= len(pts) <= 3 * len(soup), (name, soup.shape, pts.shape)
        assert not np.signbit(soup[soup == 0]).any(), name                 # (no -0.0: one weld order for np.unique and a sort by bits)
        sizes[name] = (len(soup), len(pts))
    T, U = (np.array([s[k] for s in sizes.values()]) for k in (0, 1))
    print('triangles %d .. %d, vertices %d .. %d; %d cases with only the random triangles' % (T.min(), T.max(), U.min(), U.max(), (T == pc.N_RANDOM).sum()))
    assert U.min() == 3 * pc.N_RANDOM and U.max() <= 999
    assert (U % 64 != 0).mean() > 0.9 and (T % 64 != 0).mean() > 0.9       # a partial last wave
    assert (U > 256).sum() >= 200 and (T > 256).sum() >= 200               # more than one workgroup
    assert all(sizes[n][0] > 256 for n in pc.SAMPLED), [sizes[n] for n in pc.SAMPLED]


def test_every_opcode_is_swept(ns):
    text = open(OPCODES_H).read()
    enum = re.findall(r'^\s*OP_(\w+) = (\d+),?$', text, re.M)
    opcodes = [n for n, _ in enum if n != 'COUNT']
    assert opcodes == list(tape.OP_NAMES) and dict(enum)['COUNT'] == str(len(opcodes))      # the header and the lowering agree
    n_post = len(re.findall(r'^\s*POST_\w+ = \d+,?$', text, re.M))
    n_ease = int(re.search(r'EASE_COUNT = (\d+)', text).group(1))
    assert (n_post, n_ease) == (8, 34)

    op_bytes, ops, posts, eases, by_op = set(), set(), set(), set(), {}
    for name in pc.CASES:
        t = pc.model(name, ns)[1]
        op_bytes |= {tape.OP_NAMES[int(w) & 255] for w in t.code[0::2]}
        o, p, e = pc.census(t)
        ops, posts, eases = ops | o, posts | p, eases | e
        for op in o:
            by_op.setdefault(op, []).append(name)
    assert set(opcodes) - op_bytes == set(NEVER_AN_OP_BYTE), sorted(set(opcodes) - op_bytes ^ set(NEVER_AN_OP_BYTE))
    assert {'LOAD_P', 'SAVE_P', 'PUSH_D'} <= ops                           # ... as prefixes
    assert set(opcodes) - ops == {'L_EXTERN', 'NOP'}
    assert posts == set(range(n_post)), sorted(posts)
    assert eases == set(range(n_ease)), sorted(set(range(n_ease)) - eases)
    rare = sorted((len(v), op) for op, v in by_op.items())[:6]
    print('%d of %d opcodes as op bytes, %d with the prefixes; %d post codes; %d easing ids; the rarest: %r' % (
        len(op_bytes), len(opcodes), len(ops), len(posts), len(eases), rare))

    # what the models of the five unit-test files reach (their MODELS and LIBM_FREE tuples): the gap this sweep closes
    unit = ('ex_example', 'ex_gearlike', 'twist', 'ex_blobby', 'ex_knurling', 'slots_plain_8_8_p8d8', 'torus')
    before = set()
    for name in unit:
        before |= {tape.OP_NAMES[int(w) & 255] for w in pc.model(name, ns)[1].code[0::2]}
    print('the unit tests\' models: %d opcodes as op bytes; the sweep: %d' % (len(before), len(op_bytes)))
    assert len(before) == 14 and before < op_bytes, sorted(before)


@pytest.fixture(scope='module')
def over_the_checker(ns, oracle_lib):
    """case -> probe -> outputs of the definition over the CPU checker"""
    out = {}
    with np.errstate(all='ignore'):
        for name in pc.CASES:
            f = pc.model(name, ns)[0]
            soup, pts = pc.inputs(name, ns)
            out[name] = {probe: pc.define(probe, lambda P: oracle_lib.evaluate(f, P), soup, pts) for probe in pc.PROBES}
    return out


def test_the_definitions_run_on_every_case(ns, over_the_checker):
    """shapes, statuses in range, no more steps than max_steps"""
    for name, r in over_the_checker.items():
        soup, pts = pc.inputs(name, ns)
        T, U = len(soup), len(pts)
        assert r['normals']['normal'].shape == (U, 3) and 0 <= r['normals']['n_flat'] <= U, name
        th = r['thickness']
        assert th['thickness'].shape == th['status'].shape == th['steps'].shape == (U,) and th['status'].max() <= thickness_ref.NAN, name
        assert 0 <= th['steps'].min() and th['steps'].max() <= pc.MAX_STEPS, name
        s = r['supports']
        M = len(s['triangle'])
        assert s['height'].shape == s['status'].shape == s['steps'].shape == (M,) and s['origin'].shape == (M, 3) and M <= T, name
        assert s['status'].max() <= supports_ref.NAN and s['steps'].max() <= pc.MAX_STEPS and s['counts'].sum() == M, name
        assert (np.diff(s['triangle']) > 0).all() and s['sums'].shape == (5,), name
        d = r['deviation']
        assert d['dev'].shape == d['at'].shape == d['sumsq'].shape == (T,) and 0 <= d['at'].min() and d['at'].max() < deviation_ref.n_samples(pc.ORDER), name
        q = r['snap']
        assert q['points'].shape == (U, 3) and q['status'].shape == q['residual'].shape == q['evals'].shape == (U,), name
        assert q['status'].max() <= deviation_ref.NAN and 1 <= q['evals'].min() and q['evals'].max() <= 7 * pc.SNAP['iters'] + 1, name
        im = r['render']
        assert im['depth'].shape == im['steps'].shape == im['status'].shape == (pc.HEIGHT, pc.WIDTH) and im['normal'].shape == (pc.HEIGHT, pc.WIDTH, 3), name
        assert im['status'].max() <= 1 and 1 <= im['steps'].min() and im['steps'].max() <= pc.MAX_STEPS, name


def test_the_sweep_is_not_vacuous(over_the_checker):
    """most cases have a wall to measure and a surface to hit, every case has a support ray, and over the whole sweep every
    status of the thickness probe, of the snap and of the support rays occurs -- UNRESOLVED through the case made for it
    (probe_cases.EXTRA says why no other one reaches it)"""
    R = over_the_checker
    thick = sum((r['thickness']['status'] == thickness_ref.THICK).any() for r in R.values())
    hit = sum((r['render']['status'] == 1).any() for r in R.values())
    rays = sum(len(r['supports']['triangle']) > 0 for r in R.values())
    seen = {probe: set() for probe in ('thickness', 'supports', 'snap')}
    for r in R.values():
        for probe in seen:
            seen[probe] |= set(r[probe]['status'].tolist())
    nan_dev = sum(np.isnan(r['deviation']['dev']).any() for r in R.values())
    refined = sum(((r['render']['status'] == 1) & (r['render']['steps'] > 1)).any() for r in R.values())
    print('%d cases: %d with a THICK vertex, %d with a render hit (%d after more than one step), %d with a support ray, %d with a NaN deviation; statuses %r' % (
        len(R), thick, hit, refined, rays, nan_dev, seen))
    assert thick >= 200 and hit >= 220 and rays == len(R)
    assert nan_dev >= len(param_cases.NAN_MODELS)                          # (each of them is NaN at every point)
    assert refined >= 200                                                  # (the rays start outside the bounds: a hit takes steps)
    assert seen['thickness'] == {thickness_ref.OPEN, thickness_ref.THICK, thickness_ref.THIN, thickness_ref.FLAT, thickness_ref.NAN}
    assert seen['snap'] == {deviation_ref.LEFT, deviation_ref.SNAPPED, deviation_ref.HELD, deviation_ref.FLAT, deviation_ref.NAN}
    assert seen['supports'] == {supports_ref.BED, supports_ref.PART, supports_ref.BURIED, supports_ref.UNRESOLVED, supports_ref.NAN}
    s = R['march_at_min_step']['supports']
    unresolved = s['status'] == supports_ref.UNRESOLVED
    assert unresolved.any() and (s['steps'][unresolved] == pc.MAX_STEPS).all()
    assert not any((r['supports']['status'] == supports_ref.UNRESOLVED).any() for n, r in R.items() if n != 'march_at_min_step')
