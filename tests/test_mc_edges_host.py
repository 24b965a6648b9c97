"""The CPU checker's marching cubes held to skimage (tests/golden/mc_edges.npz, tools/make_golden_mc_edges.py) on the cases of
tests/mc_cases.py: float32 ties of the vertex coordinate, grid indices up to 4094, NaN / infinite / denormal samples, row
counts at the device kernels' block boundaries, models sampled exactly on their surface.  No GPU.

Before the checker's `mc_vertex` made the whole vertex NaN where skimage does, test_checker_matches_skimage failed on
special_nan, special_overflow (+inf next to -inf: 0 / 0), special_mixed and corner_nan, and test_checker_generate on nan_plane_g8
(dense) and nan_plane_g32 (both): a third of the NaN coordinates were there."""
import os

import numpy as np
import pytest

import mc_cases
from conftest import GOLDEN

G = np.load(os.path.join(GOLDEN, 'mc_edges.npz'))


def golden_soup(key):
    """the reference's float32 soup of a volume case; (0, 3) where skimage raised (the drop-in returns an empty soup there)"""
    if 'e_' + key in G.files:
        assert str(G['e_' + key]) in ('RuntimeError', 'ValueError')
        return np.zeros((0, 3), np.float32)
    return mc_cases.unpack_soup(G['v_' + key], G['i_' + key])


def golden_generate(key, sparse):
    """(float64 soup in world coordinates, kinds) of an on_surface case"""
    dense = not sparse and 'gvd_' + key in G.files
    soup = mc_cases.unpack_soup(G[('gvd_' if dense else 'gv_') + key], G[('gid_' if dense else 'gi_') + key])
    return soup, G[('gk_' if sparse else 'gkd_') + key]


def surface_axes(key, ns):
    program, axis = mc_cases.surface_case(key)
    return mc_cases.build_model(program, dict(ns, np=np)), axis


@pytest.mark.parametrize('key', mc_cases.volume_keys())
def test_checker_matches_skimage(key, oracle_lib):
    with np.errstate(all='ignore'):                        # (the float32 cast of 1e39 warns)
        got, _ = oracle_lib.marching_cubes(mc_cases.volume(key))
    mc_cases.assert_same_soup(got, golden_soup(key), key)


@pytest.mark.parametrize('sparse', (True, False), ids=('sparse', 'dense'))
@pytest.mark.parametrize('key', mc_cases.surface_keys())
def test_checker_generate(key, sparse, ns, oracle_lib):
    f, axis = surface_axes(key, ns)
    r = oracle_lib.generate(f, axis, axis, axis, mc_cases.BATCH, sparse)
    want, kinds = golden_generate(key, sparse)
    assert np.array_equal(r.kinds, kinds)
    mc_cases.assert_same_soup(r.points, want, key)


def test_case_module():
    """the builders have not drifted from what the golden was recorded on, the pairs are float32 numbers, and the coordinate
    skimage gave every pair is the three-division formula's, computed here in NumPy float64"""
    assert mc_cases.CASE_COUNTS == {'ties': 12, 'large_index': 27, 'special': 18, 'shapes': 10, 'on_surface': 20}
    for key in mc_cases.volume_keys():
        assert mc_cases.sha256(mc_cases.volume(key)) == str(G['sha_' + key]), key
    for key in mc_cases.volume_keys('ties') + mc_cases.volume_keys('large_index'):
        i, ax, pairs = mc_cases.pair_case(key)
        assert pairs.shape == (mc_cases.ROWS, 2) and np.array_equal(pairs.astype(np.float32).astype(np.float64), pairs), key
        assert (pairs[:, 0] > 0).all() and (pairs[:, 1] < 0).all()
        vol = mc_cases.volume(key)
        assert vol.dtype == np.float32 and vol.shape[ax] == i + 2 and sorted(vol.shape) == sorted((mc_cases.ROWS, 2, i + 2))
        # the sheet: every soup vertex lies on an edge along `ax`, in row r of the pairs -- r is its coordinate on the ROWS axis
        soup = golden_soup(key)
        assert len(soup) == 3 * 2 * (mc_cases.ROWS - 1)
        row_axis = {0: 2, 1: 2, 2: 0}[ax]
        r = soup[:, row_axis].astype(np.int64)
        assert np.array_equal(r, soup[:, row_axis]) and set(r) == set(range(mc_cases.ROWS))
        want = mc_cases.edge_positions(i, pairs[:, 0], pairs[:, 1])
        assert np.array_equal(soup[:, ax].view(np.uint32), want[r].view(np.uint32)), key
    # ties: the exact quotient is on the float32 tie; where the three roundings of t leave the float64 sum on it, the result is even
    for i in mc_cases.TIE_INDICES:
        p = mc_cases.tie_pairs(i)
        m = 24 - int(np.floor(np.log2(i)))
        k = p[:, 0] / (p[:, 0] - p[:, 1]) * 2 ** m
        assert np.array_equal(k, np.rint(k)) and (k % 2 == 1).all()
    for i in mc_cases.LARGE_INDICES:
        rec = mc_cases.NEAR_TIES[i]
        if i >= 512:
            assert len(rec) >= 32 and all(any(m >> bit & 1 for _, _, m in rec) for bit in range(3)), i
        assert len(mc_cases.large_index_pairs(i)) - len(rec) >= mc_cases.RANDOM_PAIRS
    i, v_lo, v_hi, pos = mc_cases.QUOTED_PAIR
    assert (v_lo, v_hi, 3) in mc_cases.NEAR_TIES[i]
    assert mc_cases.edge_positions(i, v_lo, v_hi) == np.float32(pos) and np.float32(pos) != np.float32(i + 1)
    # a correctly rounded quotient would put the float64 sum on the tie, and the tie rounds to the even float32: i + 1
    assert np.float32(np.float64(i) + np.float64(v_lo) / (np.float64(v_lo) - np.float64(v_hi))) == np.float32(i + 1)


def test_pack_soup_round_trip():
    rng = np.random.RandomState(5)
    for dtype, bits in ((np.float32, np.uint32), (np.float64, np.uint64)):
        rows = rng.standard_normal((40, 3)).astype(dtype)
        rows[3] = (0.0, -0.0, np.nan)
        rows[4] = (-0.0, 0.0, np.nan)
        rows[5, 1] = np.array([0x7fc00001 if dtype is np.float32 else 0x7ff8000000000001], bits).view(dtype)[0]
        soup = rows[rng.randint(0, 40, 300)]
        v, c = mc_cases.pack_soup(soup)
        assert v.shape[0] == 3 and v.shape[1] <= 40 and np.array_equal(mc_cases.unpack_soup(v, c).view(bits), soup.view(bits))
    v, c = mc_cases.pack_soup(np.zeros((0, 3), np.float32))
    assert mc_cases.unpack_soup(v, c).shape == (0, 3)
