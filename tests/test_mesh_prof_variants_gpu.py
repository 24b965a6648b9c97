"""The instrumented and the plain instantiation of k_mesh give the same soup, and both give the checker's.

k_mesh's per-phase cycle counters and workgroup timelines (SDF_MESH_PROF=1) are compiled into kernels of their own (k_mesh_prof,
the same body: csrc/sdf_mesh_inst.hip with -DMESH_PROF=1), which launch_mesh takes when the context has a `prof` buffer; the kernels
of a normal call hold none of it.  A context reads SDF_MESH_PROF (and SDF_DEFER) when it is created, so every run here is a fresh child
process with a time limit of its own:
  * no SDF_MESH_PROF      the plain kernels, no buffer: nothing is reported;
  * SDF_MESH_PROF=1       the instrumented kernels: every call reports k_mesh words that are not zero;
  * SDF_MESH_PROF=2       the buffer and the report with the PLAIN kernels: k_mesh's words stay zero (k_cull's are its own).
The shapes are the smallest that reach every path the switch touches: one-pass batches of file (1,1) (one at 2^15 samples, eight at 150000, with ragged last tiles), the files
(2,2) and (2,4), and the two-pass scheme of the trig family with file (4,2); each with deferred emission on and off.  Soup (sha256) and
the five counts of the three runs are equal, and equal to oracle.generate's -- bit for bit, except the trig model, whose sines the
checker takes from libm: there the suite's tolerance for trig models holds (tests/test_gpu.py: 1e-5 of the extent, 99.9 % of the
coordinates equal), applied to the plain run's soup, which the other two must match bit for bit."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fixtures
from sdf_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('ex_example', 2 ** 15), ('ex_example', 150000), ('ex_blobby', 2 ** 15), ('ex_pawn', 2 ** 15), ('ex_weave', 2 ** 16)]
TRIG = {'ex_weave'}
COUNTS = ('batches', 'skipped', 'empty', 'nonempty', 'triangles')

CHILD = r'''
import hashlib, json, os, sys
import numpy as np
root, grids, soup_dir = sys.argv[1:4]
sys.path[:0] = [root, os.path.join(root, 'tests')]
import sdf_amd, fixtures
from sdf_amd import engine
ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
eng = engine.get_engine(0)
g = np.load(grids)
out = []
for i, name in enumerate(json.loads(sys.argv[4])):
    f = fixtures.build(name, ns)
    sys.stderr.write('[case %d]\n' % i); sys.stderr.flush()
    m = eng.generate(f, g['X%d' % i], g['Y%d' % i], g['Z%d' % i], 32, True)
    pts, st = m.points(), m.stats()
    m.close()
    if soup_dir:
        np.save(os.path.join(soup_dir, 'soup%d.npy' % i), pts)
    out.append({'sha256': hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest(), 'counts': [int(st[k]) for k in COUNTS]})
print(json.dumps(out))
'''.replace('COUNTS', repr(COUNTS))

_CHECKER = {}


@pytest.fixture(scope='module')
def grids(ns, eng, tmp_path_factory):
    """the axes of every case (the reference's step rule over the estimated bounds), in one file for the children"""
    arrays = {}
    for i, (name, samples) in enumerate(CASES):
        f = fixtures.build(name, ns)
        X, Y, Z, _ = core.grid_axes(core._estimate_bounds(f), samples=samples)
        arrays.update({'X%d' % i: X, 'Y%d' % i: Y, 'Z%d' % i: Z})
    path = str(tmp_path_factory.mktemp('prof_variants') / 'grids.npz')
    np.savez(path, **arrays)
    return path, arrays


def checker(i, ns, oracle_lib, arrays):
    if i not in _CHECKER:
        f = fixtures.build(CASES[i][0], ns)
        o = oracle_lib.generate(f, arrays['X%d' % i], arrays['Y%d' % i], arrays['Z%d' % i], 32, True)
        _CHECKER[i] = (o.points, [len(o.kinds)] + [int((o.kinds == k).sum()) for k in (0, 1, 2)] + [len(o.points) // 3])
    return _CHECKER[i]


def run_child(grids_path, soup_dir, defer, prof):
    env = dict(os.environ, SDF_DEFER=str(defer))
    env.pop('SDF_MESH_PROF', None)
    if prof:
        env['SDF_MESH_PROF'] = str(prof)
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, grids_path, soup_dir, json.dumps([c[0] for c in CASES])],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (prof, r.returncode, r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    # the report of each case: the numbers of every `[k_mesh prof]` line between its marker and the next
    reports = [re.findall(r'^\[k_mesh prof\] (.*)$', part, re.M) for part in re.split(r'^\[case \d+\]$', r.stderr, flags=re.M)[1:]]
    assert len(res) == len(CASES) == len(reports)
    return res, reports


def words(line):
    """the integers of a report line (its label before the colon dropped; the timeline's microseconds are no integers)"""
    return [int(x) for x in re.findall(r'(?<![\d.])\d+(?![\d.])', line.split(':', 1)[1])]


@pytest.mark.gpu
@pytest.mark.parametrize('defer', [1, 0], ids=['deferred', 'not_deferred'])
def test_instrumented_and_plain_kernels_give_the_checkers_soup(defer, grids, ns, oracle_lib, tmp_path):
    grids_path, arrays = grids
    plain, rep_plain = run_child(grids_path, str(tmp_path), defer, 0)
    instr, rep_instr = run_child(grids_path, '', defer, 1)
    quiet, rep_quiet = run_child(grids_path, '', defer, 2)
    for i, (name, samples) in enumerate(CASES):
        where = (name, samples, defer)
        print(where, plain[i]['counts'], plain[i]['sha256'][:16])
        want_pts, want_counts = checker(i, ns, oracle_lib, arrays)
        assert want_counts[3] >= 1 and want_counts[4] > 0, where                   # (at batch size 32 the first case is ONE batch; the others are several)
        assert plain[i] == instr[i] == quiet[i], where                             # sha256 of the soup and the five counts
        assert plain[i]['counts'] == want_counts, where
        pts = np.load(str(tmp_path / ('soup%d.npy' % i)))
        assert hashlib.sha256(np.ascontiguousarray(pts).tobytes()).hexdigest() == plain[i]['sha256'] and pts.shape == want_pts.shape, where
        if name in TRIG:
            extent = max(arrays[a + str(i)][-1] - arrays[a + str(i)][0] for a in 'XYZ')
            assert np.abs(pts - want_pts).max() <= 1e-5 * extent and (pts == want_pts).mean() > 0.999, where
        else:
            assert np.array_equal(pts, want_pts), where
        # the prof words: none without the buffer; not zero from the instrumented kernels; zero from the plain kernels with the buffer
        assert rep_plain[i] == [], where
        for rep, nonzero in ((rep_instr[i], True), (rep_quiet[i], False)):
            cyc = [l for l in rep if l.startswith(tuple('0123456789')) and 'cycles/WG-sum' in l]     # "<ms> ms; cycles/WG-sum: grab .. sample .."
            fine = [l for l in rep if l.startswith('fine:')]
            smp = [l for l in rep if l.startswith('sampling:')]
            assert cyc and len(cyc) == len(fine) == len(smp), (where, rep)
            for l in cyc:
                grab, sample, count = words(l)[:3]
                assert (grab > 0 and sample > 0 and count > 0) if nonzero else not any(words(l)), (where, l)
            for l in fine + smp:
                assert any(words(l)) if nonzero else not any(words(l)), (where, l)
