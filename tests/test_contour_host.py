"""The definition of the contours (tests/contour_ref.py) on constructed grids and closed-form fields, the case table of the device
header against the definition's, the SVG and DXF writers, and the ABI's new names.  No device is needed: the writers are driven
with the definition's arrays."""
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import contour_cases as cases
import contour_ref as ref
from sdf_amd import contour, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run(name):
    V, X, Y, level = cases.GRIDS[name]()
    return ref.contours(V, X, Y, level), V, X, Y, level


def loops(c):
    return [c['points'][c['offsets'][i]:c['offsets'][i + 1]] for i in range(len(c['closed']))]


def cross(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])


@pytest.mark.parametrize('name,V,inside,centre', cases.two_by_two(), ids=[c[0] for c in cases.two_by_two()])
def test_the_sixteen_cases(name, V, inside, centre):
    """every case on a 2 x 2 grid, the saddles with the centre inside and outside: the number of segments, and their orientation by
    the sign of the cross product -- an inside corner lies to the LEFT of a segment, an outside corner to its right.  A saddle whose
    centre is inside has its two inside corners joined, so they lie left of both segments; one whose centre is outside has the two
    outside corners joined, right of both"""
    X, Y = np.array([0.0, 1.0]), np.array([0.0, 1.0])
    c = ref.contours(V, X, Y, 0.0)
    corners = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    n_in = sum(inside)
    want = 0 if n_in in (0, 4) else (2 if centre is not None else 1)
    assert c['n_segments'] == want == len(c['closed']) and not c['closed'].any() and c['nonfinite_cells'] == 0
    assert (c['area'] == 0).all() and len(c['points']) == 2 * want
    for a, b in zip(c['seg_start'], c['seg_end']):
        for k in range(4):
            s = cross(a, b, corners[k])
            if inside[k] and centre is not False:
                assert s > 0, (name, k, s)
            if not inside[k] and centre is not True:
                assert s < 0, (name, k, s)


def test_the_saddle_decisions_join_different_corners():
    got = {}
    for name, V, inside, centre in cases.two_by_two():
        if name.startswith('case5'):
            c = ref.contours(V, np.array([0.0, 1.0]), np.array([0.0, 1.0]), 0.0)
            got[centre] = sorted((tuple(a), tuple(b)) for a, b in zip(c['seg_start'], c['seg_end']))
    assert got[True] != got[False]
    # centre inside: the segment that starts on the bottom edge ends on the right one (it cuts c1 off); outside: on the left one
    assert [b[0] for a, b in got[True] if a[1] == 0.0] == [1.0] and [b[0] for a, b in got[False] if a[1] == 0.0] == [0.0]


def test_ties_keep_their_segments_of_length_zero():
    c, V, X, Y, level = run('ties')
    assert c['n_segments'] == 4 and len(c['closed']) == 1 and c['closed'][0]
    assert (c['points'] == [X[1], Y[1]]).all() and len(c['points']) == 4 and c['area'][0] == 0.0
    assert (c['seg_start'] == c['seg_end']).all()                    # every one of them has length zero


def test_circle():
    """hypot(x, y) - 1 at h = 0.05: one closed loop, positive area, and every vertex v has |f(v)| <= h^2 / (8 (r - h)) = 3.3e-4.
    Why: a vertex is the zero of the linear interpolant l of f along a grid edge of length h, and |f - l| <= h^2 / 8 max |f''| on the
    edge (the interpolation error of a C^2 function).  Along a straight line the second derivative of the distance to the origin is
    sin^2(angle) / rho <= 1 / rho, and every point of an edge that crosses the circle has rho >= r - h.  So |f(v)| = |f(v) - l(v)| <=
    h^2 / (8 (r - h)); the rounding of t and of the vertex is twelve orders of magnitude below that."""
    c, V, X, Y, level = run('circle')
    assert len(c['closed']) == 1 and c['closed'][0] and c['area'][0] > 0 and c['layer'][0] == 0
    h, r = cases.H, 1.0
    err = np.abs(np.hypot(c['points'][:, 0], c['points'][:, 1]) - r)
    print('circle: max |f(v)| = %.3e, bound %.3e, area %.6f' % (err.max(), h * h / (8 * (r - h)), c['area'][0]))
    assert err.max() <= h * h / (8 * (r - h))
    assert abs(c['area'][0] - np.pi) < 2 * np.pi * r * h * h / (8 * (r - h)) + 0.01      # (an inscribed polygon: a little below pi)
    assert len(c['points']) == c['n_segments'] and c['offsets'].tolist() == [0, c['n_segments']]


def test_annulus_outer_loop_first():
    """two loops of opposite sign.  The leader rule orders them by their smallest segment index, and cells are numbered ix first: the
    outer loop reaches the smallest ix, so it comes first"""
    c, V, X, Y, level = run('annulus')
    assert c['closed'].tolist() == [True, True]
    assert c['area'][0] > 0 > c['area'][1]
    assert abs(c['area'][0] - np.pi) < 0.02 and abs(c['area'][1] + np.pi * 0.25) < 0.02
    assert c['leaders'][0] < c['leaders'][1] and loops(c)[0][:, 0].min() < loops(c)[1][:, 0].min()


def test_two_layers():
    c, V, X, Y, level = run('two_layers')
    assert c['layer'].tolist() == [0, 1] and c['layer'].dtype == np.int32 and c['closed'].all()
    assert abs(c['area'][0] - np.pi) < 0.02 and abs(c['area'][1] - np.pi * 0.36) < 0.02
    one = ref.contours(V[1:], X, Y, level)                            # a layer alone gives the same loop
    assert (bits(loops(c)[1]) == bits(one['points'])).all() and bits(c['area'][1]) == bits(one['area'][0])


def test_clipped_circle_gives_open_chains():
    c, V, X, Y, level = run('clipped')
    assert len(c['closed']) == 4 and not c['closed'].any() and (c['area'] == 0).all()
    has_pred = np.zeros(c['n_segments'], bool)
    has_pred[c['next'][c['next'] >= 0]] = True
    assert sorted(np.flatnonzero(~has_pred)) == c['leaders'].tolist()                       # the heads, ascending
    assert len(c['points']) == c['n_segments'] + 4
    for i, p in enumerate(loops(c)):
        n = 0
        s = c['leaders'][i]
        while s >= 0:
            n, s = n + 1, c['next'][s]
        assert len(p) == n + 1
        on_border = lambda q: q[0] in (X[0], X[-1]) or q[1] in (Y[0], Y[-1])
        assert on_border(p[0]) and on_border(p[-1]) and not any(on_border(q) for q in p[1:-1])


def test_a_nan_sample_opens_the_loop():
    c, V, X, Y, level = run('with_nan')
    assert c['nonfinite_cells'] == 4
    assert len(c['closed']) == 1 and not c['closed'][0] and c['area'][0] == 0.0
    assert len(c['points']) == c['n_segments'] + 1 and np.isfinite(c['points']).all()
    whole = ref.contours(*cases.circle())
    assert c['n_segments'] < whole['n_segments']


def test_a_level_other_than_zero():
    c, V, X, Y, level = run('shifted_level')
    assert len(c['closed']) == 1 and c['closed'][0] and abs(c['area'][0] - np.pi) < 0.02


@pytest.mark.parametrize('make', [cases.annulus, cases.clipped, cases.with_nan, cases.random_field, lambda: cases.random_field(9, 7, 3, 1)],
                         ids=['annulus', 'clipped', 'with_nan', 'random', 'random_layers'])
def test_the_linking_walked_naively(make):
    """`next` re-walked without the definition's bookkeeping: where s ends, next[s] starts, bit for bit; every segment is in exactly
    one contour; a closed loop returns to its smallest index and an open chain runs from the segment nobody points at to one that
    points nowhere"""
    V, X, Y, level = make()
    c = ref.contours(V, X, Y, level)
    nxt, n = c['next'], c['n_segments']
    linked = np.flatnonzero(nxt >= 0)
    assert (bits(c['seg_end'][linked]) == bits(c['seg_start'][nxt[linked]])).all()
    assert len(set(nxt[linked].tolist())) == len(linked)                                    # at most one predecessor
    pred = np.full(n, -1)
    pred[nxt[linked]] = linked
    seen = np.zeros(n, int)
    for i, p in enumerate(loops(c)):
        s, walk = int(c['leaders'][i]), []
        while s >= 0 and not (walk and s == walk[0]):
            walk.append(s); seen[s] += 1
            s = int(nxt[s])
        closed = s >= 0
        assert closed == bool(c['closed'][i])
        assert walk[0] == (min(walk) if closed else [w for w in walk if pred[w] < 0][0])
        want = c['seg_start'][walk] if closed else np.vstack([c['seg_start'][walk], c['seg_end'][walk[-1:]]])
        assert (bits(p) == bits(want)).all()
    assert (seen == 1).all() and (np.diff(c['leaders']) > 0).all()
    if make is cases.random_field:
        assert len(c['closed']) > 100 and c['closed'].any() and not c['closed'].all()


def test_the_device_header_carries_the_same_table():
    text = open(os.path.join(ROOT, 'sdf_amd', 'csrc', 'sdf_contour.h')).read()
    body = re.search(r'CONTOUR_CASES\[16\]\[5\]\s*=\s*\{(.*?)\};', text, re.S).group(1)
    rows = np.array([int(v) for v in re.findall(r'\d+', body)]).reshape(16, 5)
    assert rows.tolist() == [list(r) for r in ref.CASES]
    for case, (n, f0, t0, f1, t1) in enumerate(ref.CASES):           # and the table against the rule it follows from
        ins = [bool(case >> k & 1) for k in range(4)]
        starts = [e for e in range(4) if ins[e] and not ins[(e + 1) % 4]]
        ends = [e for e in range(4) if not ins[e] and ins[(e + 1) % 4]]
        assert n == len(starts) and [f0, f1][:n] == starts and sorted([t0, t1][:n]) == ends


# ---- the writers ----
def as_contours(c, X, Y, z):
    return contour.Contours(c['points'], c['offsets'], c['closed'], c['layer'], c['area'], z, {}, X, Y)


def writer_input():
    """two layers, the second clipped by a border of NaN samples so that it holds open chains"""
    V, X, Y, level = cases.two_layers()
    V = V.copy()
    V[1, :, :18] = np.nan
    c = ref.contours(V, X, Y, level)
    assert c['closed'].any() and not c['closed'].all() and set(c['layer'].tolist()) == {0, 1}
    return c, as_contours(c, X, Y, np.array([0.1, 0.30000000000000004]))


def test_svg(tmp_path):
    c, obj = writer_input()
    path = str(tmp_path / 'out.svg')
    obj.save(path)
    root = ET.parse(path).getroot()
    ns = '{http://www.w3.org/2000/svg}'
    paths = list(root.iter(ns + 'path'))
    assert len(paths) == 2 and all(p.get('fill-rule') == 'evenodd' for p in paths)
    d = ' '.join(p.get('d') for p in paths)
    assert d.count('M') == len(c['closed']) and d.count('Z') == int(c['closed'].sum())
    xy = np.array([float(v) for v in re.findall(r'[ML]([^, ]+),([^, ]+)', d) for v in v]).reshape(-1, 2)
    assert (bits(xy) == bits(c['points'])).all()
    for k, p in enumerate(paths):                                    # one path per layer, in order, open chains without Z
        subs = [s for s in p.get('d').split('M') if s]
        mine = np.flatnonzero(c['layer'] == k)
        assert len(subs) == len(mine) and [s.rstrip().endswith('Z') for s in subs] == c['closed'][mine].tolist()
        assert float(p.get('data-z')) == obj.z[k]
    vb = [float(v) for v in root.get('viewBox').split()]
    (x0, y0), (x1, y1) = obj.bounds
    assert vb == [x0, -y1, x1 - x0, y1 - y0]
    assert 'scale(1,-1)' in next(root.iter(ns + 'g')).get('transform')                      # up is up


def test_dxf(tmp_path):
    c, obj = writer_input()
    path = str(tmp_path / 'out.dxf')
    obj.save(path)
    lines = open(path).read().split('\n')
    assert lines[-1] == '' and len(lines) % 2 == 1
    pairs = [(int(lines[i]), lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
    assert pairs[-1] == (0, 'EOF') and (1, 'AC1009') in pairs
    ents, cur = [], None
    for code, val in pairs:
        if code == 0:
            cur = {'type': val}
            ents.append(cur)
        elif cur is not None:
            cur[code] = val
    poly = [e for e in ents if e['type'] == 'POLYLINE']
    verts = [e for e in ents if e['type'] == 'VERTEX']
    assert len(poly) == len(c['closed']) == sum(e['type'] == 'SEQEND' for e in ents)
    assert [int(e[70]) for e in poly] == c['closed'].astype(int).tolist()
    assert [e[8] for e in poly] == ['L%d' % k for k in c['layer']]
    assert [float(e[30]) for e in poly] == [obj.z[k] for k in c['layer']]
    xy = np.array([[float(e[10]), float(e[20])] for e in verts])
    assert (bits(xy) == bits(c['points'])).all()
    n = 0
    for e in ents:                                                    # the vertices of a polyline follow it, then its SEQEND
        if e['type'] == 'POLYLINE':
            n += 1
            count = 0
        elif e['type'] == 'VERTEX':
            count += 1
        elif e['type'] == 'SEQEND':
            assert count == c['offsets'][n] - c['offsets'][n - 1]


def test_save_refuses_other_extensions(tmp_path):
    c, obj = writer_input()
    with pytest.raises(ValueError, match='svg'):
        obj.save(str(tmp_path / 'out.stl'))
    import sdf_amd
    with pytest.raises(ValueError, match='svg'):                      # before anything is sampled
        sdf_amd.circle(1).save(str(tmp_path / 'out.stl'))
    assert not os.listdir(str(tmp_path))


def test_what_is_refused_before_the_engine_is_asked_for():
    import sdf_amd
    with pytest.raises(ValueError, match='z'):
        contour.contours(sdf_amd.sphere(1))
    with pytest.raises(ValueError, match='z'):
        contour.contours(sdf_amd.circle(1), z=0.0)
    with pytest.raises(ValueError, match='level'):
        contour.contours(sdf_amd.circle(1), level=np.nan, bounds=((-1, -1), (1, 1)))
    with pytest.raises(ValueError, match='model'):
        contour.contours(lambda p: p)


def test_the_axes_reach_past_the_bounds():
    a = contour.axis(-1.0, 1.0, 0.3)
    assert a[0] == -1.0 and a[-2] < 1.0 <= a[-1] and np.allclose(np.diff(a), 0.3)
    b = contour.axis(0.0, 1.0, 0.25)                                  # arange stops short of hi: one more sample, on hi
    assert b.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]


def test_the_public_names():
    import sdf_amd
    from sdf_amd import d2, d3
    assert callable(d2.SDF2.contours) and callable(d2.SDF2.save) and callable(d3.SDF3.slices)
    for name in ('contours', 'Contours', 'slices', 'contour'):
        assert name not in dir(sdf_amd) or name == 'contour'          # (the submodule's own name appears once it is imported)
    assert 'contours' not in d2._ops and 'slices' not in d3._ops      # methods, not ops: `slice` stays the op it is
    assert callable(sdf_amd.sphere(1).slice)


def test_the_abi_names_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'sdf_hip.h')).read()
    version = int(re.search(r'#define\s+SDF_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert version == engine.ABI_VERSION == 17                    # added under ABI 17
    for name in ('sdf_contour_grid_host', 'sdf_contour_host', 'sdf_contours_fetch', 'sdf_contours_destroy', 'sdf_contour_last_kernel_ms'):
        assert name in engine.ABI and re.search(r'\b%s\s*\(' % name, hdr), name
    lib = engine.load_library()
    assert lib.sdf_abi_version() == 17 and all(hasattr(lib, n) for n in engine.ABI)
    fields = list(engine.CONTOUR_COUNTS)
    assert [k for k, _ in engine.SdfContourCounts._fields_] == fields
    m = re.search(r'typedef struct sdf_contour_counts \{(.*?)\} sdf_contour_counts;', hdr, re.S).group(1)
    assert re.findall(r'\b(%s)\b' % '|'.join(fields), m) == fields
