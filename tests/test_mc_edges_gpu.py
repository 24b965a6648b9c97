"""The device's marching cubes held to skimage (tests/golden/mc_edges.npz) and to the CPU checker on the cases of
tests/mc_cases.py -- the volume path (k_mc_rows / k_scan_rows / k_mc_emit), the field-tile path of a model with user closures
(k_field_emit) and the tape path (k_mesh) -- where the vertex arithmetic is fragile: float32 ties, grid indices up to 4094,
NaN / infinite / denormal samples, row counts at the block boundaries, samples exactly on the surface."""
import ctypes

import numpy as np
import pytest

import mc_cases
from test_mc_edges_host import golden_generate, golden_soup, surface_axes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('key', mc_cases.volume_keys())
def test_device_matches_skimage_and_checker(key, eng, oracle_lib):
    vol = mc_cases.volume(key)
    with np.errstate(all='ignore'):                        # (the float32 cast of 1e39 warns)
        got = eng.marching_cubes(vol)
        want, _ = oracle_lib.marching_cubes(vol)
    mc_cases.assert_same_soup(got, golden_soup(key), key + ' against skimage')
    mc_cases.assert_same_soup(got, want, key + ' against the checker')


@pytest.mark.parametrize('sparse', (True, False), ids=('sparse', 'dense'))
@pytest.mark.parametrize('key', mc_cases.surface_keys())
def test_generate_on_surface(key, sparse, ns, eng, oracle_lib):
    """k_mesh on fields with whole planes of samples at exactly 0.0 -- and, nan_plane, at NaN: the tape model that is NaN on
    part of the grid and positive elsewhere (its sparse pass skips the one batch of the small grid, like the reference's)"""
    f, axis = surface_axes(key, ns)
    m = eng.generate(f, axis, axis, axis, mc_cases.BATCH, sparse)
    pts, kinds, st = m.points(), m.kinds(), m.stats()
    m.close()
    o = oracle_lib.generate(f, axis, axis, axis, mc_cases.BATCH, sparse)
    assert np.array_equal(kinds, o.kinds) and st['n_eval_voxels'] == o.n_eval
    mc_cases.assert_same_soup(pts, o.points, key + ' against the checker')
    want, want_kinds = golden_generate(key, sparse)
    assert np.array_equal(kinds, want_kinds)
    mc_cases.assert_same_soup(pts, want, key + ' against the reference')


def _volume_closure(ns, vol):
    """a user closure whose values on the grid arange(n0) x arange(n1) x arange(n2) are the volume's"""
    @ns['sdf3']
    def lookup():
        def f(p):
            i = np.clip(np.rint(p).astype(np.int64), 0, np.array(vol.shape) - 1)
            return vol[i[:, 0], i[:, 1], i[:, 2]]
        return f
    return lookup()


@pytest.mark.parametrize('key', mc_cases.volume_keys('special'))
def test_field_tiles_on_special_values(key, ns, eng):
    """the same volumes through the meshing of a model with user closures (k_field_emit): one dense batch on the volume's own
    grid, whose soup in world coordinates is the volume's soup"""
    vol = mc_cases.volume(key)
    X, Y, Z = (np.arange(n, dtype=np.float64) for n in vol.shape)
    with np.errstate(all='ignore'):
        m = eng.generate(_volume_closure(ns, vol), X, Y, Z, mc_cases.BATCH, False)
        pts, kinds = m.points(), m.kinds()
        m.close()
    want = golden_soup(key).astype(np.float64)
    assert kinds.tolist() == [2 if len(want) else 1]
    mc_cases.assert_same_soup(pts, want, key)


def test_marching_cubes_host_with_a_short_buffer(eng):
    """`cap` below the triangle count (Engine.marching_cubes asks again with the count and so never shows this): the count
    returned is the whole soup's, the first `cap` triangles are the soup's first, nothing is written behind them"""
    from sdf_amd.engine import _check, _dp, _f32p
    key = 'shape_26x42x3'                                   # 1025 rows: five workgroups of k_mc_emit stop at the cap
    vol = np.ascontiguousarray(mc_cases.volume(key), dtype=np.float32)
    full = golden_soup(key).reshape(-1, 9)
    for cap in (1, 1000, len(full) - 1):
        out = np.full((cap + 64, 9), -7.5, np.float32)
        nt = ctypes.c_int64(0)
        _check(eng.lib, eng.lib.sdf_marching_cubes_host(eng.ctx, _dp(vol, _f32p), vol.shape[0], vol.shape[1], vol.shape[2],
                                                        _dp(out, _f32p), cap, ctypes.byref(nt)))
        assert nt.value == len(full)
        assert np.array_equal(out[:cap].view(np.uint32), full[:cap].view(np.uint32))
        assert (out[cap:] == -7.5).all()
