#!/usr/bin/env python3
"""One hash over what the interval passes see and say for every well-formed model of the suite: for each tape of
tests/fixtures.py FIXTURES and SLOT_FIXTURES, its code, constants and operand ranges (sdf_amd/tape.py lower) and the
intervals the host build of ia_run_tape (tests/native/interval_tape_host.hip) gives the boxes that
tests/test_interval_host.py::_check_tape_enclosure draws for it (same generator, same seeds, 1500 boxes per tape).

    python tools/interval_fixture_hash.py [--root TREE]

Run on two trees (--root: a checkout of another commit), equal hashes say that a change of the lowering or of the
interval forms moved nothing for these models: profiles/params01_intervals.md records such a comparison.
"""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np


def boxes_for(t, centres, seed, nb=1500):
    """the boxes of _check_tape_enclosure (tests/test_interval_host.py), draw for draw"""
    rng = np.random.default_rng(seed)
    c = centres[rng.integers(0, len(centres), nb)].astype(np.float64)
    if t.dim == 2:
        c[:, 2] = 0.0
    size = 10.0 ** rng.uniform(-3.5, 0.0, (nb, 1)) * rng.uniform(0.2, 1.0, (nb, 3))
    size[rng.random(nb) < 0.1] *= np.array([1.0, 0.0, 1.0])
    lo, hi = c - size * rng.random((nb, 3)), c + size * rng.random((nb, 3))
    if t.dim == 2:
        lo[:, 2] = hi[:, 2] = 0.0
    return np.ascontiguousarray(np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--verbose', action='store_true')
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    import fixtures
    import sdf_amd
    from sdf_amd import tape as tape_mod
    assert os.path.abspath(sdf_amd.__file__).startswith(root + os.sep), sdf_amd.__file__
    ns = {k: getattr(sdf_amd, k) for k in dir(sdf_amd) if not k.startswith('_')}
    P = np.load(os.path.join(root, 'tests', 'golden', 'values.npz'))['P']
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    total = hashlib.sha256()
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, 'libia_tape.so')
        subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-std=c++17', '-ffp-contract=off', '-w', '-fPIC', '-shared',
                               '-I', os.path.join(root, 'sdf_amd', 'csrc'), '-o', so,
                               os.path.join(root, 'tests', 'native', 'interval_tape_host.hip')])
        lib = ctypes.CDLL(so)
        lib.ia_tape_boxes.restype = ctypes.c_int
        lib.ia_tape_boxes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        names = sorted(fixtures.FIXTURES) + sorted(fixtures.SLOT_FIXTURES)
        for name in names:
            t = tape_mod.lower(fixtures.build(name, ns))
            boxes = boxes_for(t, P, zlib.crc32(name.encode()))
            out = np.empty((len(boxes), 2))
            code = np.ascontiguousarray(t.code, dtype=np.uint32)
            consts = np.ascontiguousarray(np.concatenate([t.consts, [0.0]]))
            if getattr(t, 'intervals', True):
                assert lib.ia_tape_boxes(code.ctypes.data, consts.ctypes.data, t.n_instr, t.n_pslots, t.n_dslots,
                                         boxes.ctypes.data, len(boxes), out.ctypes.data) == 0
            else:                      # no interval pass runs for this tape: nothing is decided for any box
                out[:] = (-np.inf, np.inf)
            h = hashlib.sha256()
            for part in (name.encode(), code.tobytes(), t.consts.tobytes(),
                         b'none' if t.rstart is None else t.rstart.tobytes() + t.lstart.tobytes(), boxes.tobytes(), out.tobytes()):
                h.update(part)
            total.update(h.digest())
            if a.verbose:
                print('%-24s %4d instr  finite %5.1f %%  %s' % (name, t.n_instr, 100.0 * np.isfinite(out).all(axis=1).mean(), h.hexdigest()[:16]))
    print('%d tapes  sha256 %s' % (len(names), total.hexdigest()))


if __name__ == '__main__':
    main()
