#!/opt/conda/bin/python3.9
"""tests/golden/stl_soups.npz: what the unmodified reference's STL writer makes of the constructed soups of tests/soups_ref.py and of
two models whose meshes are full of degenerate triangles.  Run it under the reference's own interpreter, like tools/make_golden.py:

    env -u PYTHONPATH /opt/conda/bin/python3.9 -W ignore tools/make_golden_stl.py [--check]

(SDF_REFERENCE names the reference's checkout where it is not /root/reference.)  Nothing here is imported by the product or by the
tests; the tests read the .npz.  Every value comes from correctly rounded float32 operations of NumPy (np.cross, np.linalg.norm,
the division; reference sdf/stl.py:4-24) and, for the two models, from the reference's `generate` on models without BLAS or libm on
the way (box, octahedron): the file is reproducible bit for bit.  --check compares with the committed file and writes nothing.

  keys       the soups' names, in order: <case>_<T> for class A, b_<case>_<T> for class B
  sha_<key>  sha256 of the float64 soup's bytes: the tests notice a builder that drifts between NumPy versions
  rec_<key>  the T x 50 bytes of records `sdf.stl.write_binary_stl` wrote for it (the file without header and count)
  stl_box, stl_octahedron   the whole files of box(1) and octahedron(1):
             write_binary_stl(generate(f, step=0.125, bounds=((-1, -1, -1), (1, 1, 1)), sparse=False))
"""
import hashlib
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get('SDF_REFERENCE', '/root/reference'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import sdf  # the reference  # noqa: E402
from sdf import core  # noqa: E402

import soups_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'stl_soups.npz')
LATTICE = dict(step=0.125, bounds=((-1, -1, -1), (1, 1, 1)), sparse=False)


def written(points):
    """the bytes of the file the reference writes for a list of points"""
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, 'a.stl')
        with np.errstate(all='ignore'):
            sdf.write_binary_stl(p, points)
        with open(p, 'rb') as fp:
            return fp.read()


def make():
    out = {}
    keys = []
    for key, cls, soup in soups_ref.stl_cases():
        raw = written(list(soup))
        T = len(soup) // 3
        assert raw[:80] == b'\x00' * 80 and struct.unpack('<I', raw[80:84])[0] == T and len(raw) == 84 + 50 * T
        keys.append(key)
        out['sha_' + key] = np.frombuffer(hashlib.sha256(soup.tobytes()).digest(), np.uint8)
        out['rec_' + key] = np.frombuffer(raw[84:], np.uint8)
        nan = np.isnan(np.frombuffer(raw[84:], np.uint8).reshape(T, 50)[:, :48].copy().view('<f4'))
        print('%-20s class %s  %4d triangles, %4d with a NaN word' % (key, cls, T, int(nan.any(axis=1).sum())))
    out['keys'] = np.array(keys)
    for name in ('box', 'octahedron'):
        with np.errstate(all='ignore'):
            points = core.generate(getattr(sdf, name)(1), workers=1, verbose=False, **LATTICE)
        raw = written(points)
        out['stl_' + name] = np.frombuffer(raw, np.uint8)
        nrm = np.frombuffer(raw[84:], np.uint8).reshape(-1, 50)[:, :12].copy().view('<u4')
        print('%-20s %d triangles, %d with a NaN normal, its words %s' % (
            name, len(points) // 3, int(np.isnan(nrm.view('<f4')).any(axis=1).sum()),
            sorted(set('%08x' % w for w in nrm[np.isnan(nrm.view('<f4'))].tolist()))))
    return out


def main():
    out = make()
    if '--check' in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        bad = [k for k in out if not (old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k]))]
        print('%s: %d arrays, %s' % (OUT, len(out), 'differ: %s' % bad if bad else 'all reproduced'))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
