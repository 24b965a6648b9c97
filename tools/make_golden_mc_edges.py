#!/opt/conda/bin/python3.9
"""tests/golden/mc_edges.npz: what the unmodified reference makes of the cases of tests/mc_cases.py -- skimage 0.18.3 through
the reference's own `_marching_cubes` (sdf/core.py:16-18) for the volume families, its `generate` for the on_surface family.

    env -u PYTHONPATH /opt/conda/bin/python3.9 -W ignore tools/make_golden_mc_edges.py

Per volume case <key>:
  sha_<key>              sha256 of the volume (mc_cases.sha256); the volumes themselves are not stored
  v_<key>, i_<key>       the float32 soup as its distinct rows and a back-reference code per row (mc_cases.pack_soup;
                         mc_cases.unpack_soup(v, i) is the soup, bit for bit)
  e_<key>                instead of the soup: the class name of the exception skimage raised
Per on_surface case <key> (sparse=True; dense gives the same soup, which is asserted here, and its own kinds):
  gv_<key>, gi_<key>     the float64 soup in world coordinates, packed the same way
  gk_<key>, gkd_<key>    0 skipped / 1 empty / 2 nonempty per batch, sparse and dense
  gvd_<key>, gid_<key>   the dense soup of the nan_plane cases, where it is not the sparse one
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sdf  # the reference  # noqa: E402
from sdf import core  # noqa: E402

import mc_cases  # noqa: E402

NS = {k: getattr(sdf, k) for k in dir(sdf) if not k.startswith('_')}
NS['np'] = np


def run_generate(f, axis, sparse):
    bounds, step = mc_cases.reference_grid(axis)
    kinds = []
    orig = core._worker

    def worker(sdf_, job, step, sparse):          # (the reference passes step and sparse by keyword)
        r = orig(sdf_, job, step, sparse)
        kinds.append(0 if r is None else (1 if len(r) == 0 else 2))
        return r
    core._worker = worker
    try:
        with np.errstate(all='ignore'):
            pts = core.generate(f, step=step, bounds=bounds, workers=1, batch_size=mc_cases.BATCH, verbose=False, sparse=sparse)
    finally:
        core._worker = orig
    return np.array(pts, dtype=np.float64).reshape(-1, 3), np.array(kinds, np.uint8)


def main():
    out = {}
    for key in mc_cases.volume_keys():
        vol = mc_cases.volume(key)
        out['sha_' + key] = np.array(mc_cases.sha256(vol))
        try:
            with np.errstate(all='ignore'):
                soup = np.ascontiguousarray(core._marching_cubes(vol), dtype=np.float32)
        except Exception as e:
            out['e_' + key] = np.array(type(e).__name__)
            print('%-24s %-14s raises %s: %s' % (key, vol.shape, type(e).__name__, e))
            continue
        out['v_' + key], out['i_' + key] = mc_cases.pack_soup(soup)
        assert np.array_equal(mc_cases.unpack_soup(out['v_' + key], out['i_' + key]).view(np.uint32), soup.view(np.uint32))
        print('%-24s %-14s %6d triangles, %5d coordinates NaN' % (key, vol.shape, len(soup) // 3, int(np.isnan(soup).sum())))
    for key in mc_cases.surface_keys():
        program, axis = mc_cases.surface_case(key)
        f = mc_cases.build_model(program, NS)
        pts, kinds = run_generate(f, axis, True)
        dense, kinds_dense = run_generate(f, axis, False)
        if key.startswith('nan_plane'):           # the sparse pass may skip a batch the dense one marches: the NaN sits at the
            out['gvd_' + key], out['gid_' + key] = mc_cases.pack_soup(dense)      # centre and the eight corners are positive
        else:
            assert dense.shape == pts.shape and np.array_equal(dense.view(np.uint64), pts.view(np.uint64)), key
        out['gv_' + key], out['gi_' + key] = mc_cases.pack_soup(pts)
        out['gk_' + key], out['gkd_' + key] = kinds, kinds_dense
        print('%-24s %6d triangles, %5d coordinates NaN, batches %s sparse, %s dense'
              % (key, len(pts) // 3, int(np.isnan(pts).sum()), np.bincount(kinds, minlength=3), np.bincount(kinds_dense, minlength=3)))
    path = os.path.join(ROOT, 'tests', 'golden', 'mc_edges.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
