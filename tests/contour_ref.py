"""The definition of the contours of a sampled 2-D field: marching squares with closed, oriented, ORDERED
polylines.  NumPy for the cells, plain loops for the chains; sdf_amd/csrc/sdf_contour.hip reproduces every output bit for bit.

Samples V[nw, nx, ny] (nw layers), axes X[nx], Y[ny], a level.

Inside.  A sample is inside iff v < level, strictly: a sample equal to the level is outside.  A cell with a non-finite corner emits
nothing and is counted in `nonfinite_cells`.

Cell (ix, iy) has the corners c0 = V[ix, iy], c1 = V[ix + 1, iy], c2 = V[ix + 1, iy + 1], c3 = V[ix, iy + 1] -- counter-clockwise in
x-right / y-up -- and the edges e = 0 bottom (c0 c1), 1 right (c1 c2), 2 top (c2 c3), 3 left (c3 c0).  Its case is the sum of 1 << k over
its inside corners.  A segment runs from edge to edge with the inside on its LEFT: it starts on the edge where, going round the cell
counter-clockwise, the samples turn from inside to outside, and ends where they turn back.  Outer boundaries therefore run
counter-clockwise (positive area) and holes clockwise (negative area).  CASES[case] = (n, from0, to0, from1, to1) is the whole
table; the two saddles, 5 and 10, are listed for a centre value ((c0 + c1) + (c3 + c2)) * 0.25 that is inside (it joins the inside
corners), and a centre that is outside swaps the two `to` edges.  The slots of a cell are in the table's order.

Vertices.  A vertex on a grid edge is computed from the lower-index sample a (coordinate ca) to the higher-index one b:
t = (a - level) / (a - b), c = ca + t * (cb - ca), every operation rounded on its own; the other coordinate is the axis value.  Both
cells that share the edge get the same bits.  Where a sample equals the level, t is 0 or 1 and segments of length zero arise: they
are KEPT -- dropping them would make the number of points depend on ties, and a cutter does not mind a repeated point.

Segment index: by layer, then by cell ix * (ny - 1) + iy, then by slot.  next[s] is the segment of the neighbouring cell across the
edge where s ends that starts on that edge; -1 at the border of the grid and beside a non-finite cell.  It follows from the tables
and the cells' offsets alone.

Chains.  A closed loop starts at its smallest segment index and lists one point per segment (its start); an open chain starts at the
segment without a predecessor and lists n + 1 points (the starts and the last segment's end).  Contours are ordered by ascending
leader index, which groups them by layer.  area = 0.5 * sum(x_i * y_{i+1} - x_{i+1} * y_i), summed left to right from the first
point, the last term wrapping round to the first point; 0 for an open chain."""
import numpy as np

CASES = (
    (0, 0, 0, 0, 0),
    (1, 0, 3, 0, 0),
    (1, 1, 0, 0, 0),
    (1, 1, 3, 0, 0),
    (1, 2, 1, 0, 0),
    (2, 0, 1, 2, 3),
    (1, 2, 0, 0, 0),
    (1, 2, 3, 0, 0),
    (1, 3, 2, 0, 0),
    (1, 0, 2, 0, 0),
    (2, 1, 2, 3, 0),
    (1, 1, 2, 0, 0),
    (1, 3, 1, 0, 0),
    (1, 0, 1, 0, 0),
    (1, 3, 0, 0, 0),
    (0, 0, 0, 0, 0),
)
NEIGHBOUR = ((0, -1), (1, 0), (0, 1), (-1, 0))       # the cell across edge e; it sees the edge as (e + 2) % 4


def cell_segments(case, centre_inside):
    """[(from, to), ...] of a cell: the table, with the saddles' `to` edges swapped for a centre that is outside"""
    n, f0, t0, f1, t1 = CASES[case]
    if n == 2 and not centre_inside:
        t0, t1 = t1, t0
    return [(f0, t0), (f1, t1)][:n]


def edge_vertex(V2, X, Y, ix, iy, e, level):
    """the vertex on edge e of cell (ix, iy) of one layer: always from the lower-index sample to the higher-index one"""
    if e == 0 or e == 2:
        j = iy + (1 if e == 2 else 0)
        a, b = V2[ix, j], V2[ix + 1, j]
        t = (a - level) / (a - b)
        return X[ix] + t * (X[ix + 1] - X[ix]), Y[j]
    i = ix + (1 if e == 1 else 0)
    a, b = V2[i, iy], V2[i, iy + 1]
    t = (a - level) / (a - b)
    return X[i], Y[iy] + t * (Y[iy + 1] - Y[iy])


def cell_codes(V, level):
    """per cell (nw, nx - 1, ny - 1): the case (0 for a cell with a non-finite corner), whether the centre is inside, whether the
    cell is finite"""
    c0, c1, c2, c3 = V[:, :-1, :-1], V[:, 1:, :-1], V[:, 1:, 1:], V[:, :-1, 1:]
    finite = np.isfinite(c0) & np.isfinite(c1) & np.isfinite(c2) & np.isfinite(c3)
    with np.errstate(all='ignore'):
        case = (c0 < level) * 1 + (c1 < level) * 2 + (c2 < level) * 4 + (c3 < level) * 8
        centre = ((c0 + c1) + (c3 + c2)) * 0.25
        centre_inside = centre < level
    return np.where(finite, case, 0).astype(np.int64), centre_inside, finite


def contours(V, X, Y, level=0.0):
    V = np.ascontiguousarray(V, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    level = np.float64(level)
    nw, nx, ny = V.shape
    assert X.shape == (nx,) and Y.shape == (ny,) and nx >= 2 and ny >= 2 and nw >= 1
    cy = ny - 1
    ncell = (nx - 1) * cy
    case, centre_inside, finite = cell_codes(V, level)
    case, centre_inside = case.reshape(-1), centre_inside.reshape(-1)
    count = np.array([c[0] for c in CASES], dtype=np.int64)[case]
    offset = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_seg = int(offset[-1])

    start = np.zeros((n_seg, 2), np.float64)
    end = np.zeros((n_seg, 2), np.float64)
    nxt = np.full(n_seg, -1, np.int64)
    seg_layer = np.zeros(n_seg, np.int32)
    with np.errstate(all='ignore'):
        for g in np.flatnonzero(count):
            w, c = divmod(int(g), ncell)
            ix, iy = divmod(c, cy)
            for k, (f, t) in enumerate(cell_segments(int(case[g]), bool(centre_inside[g]))):
                s = int(offset[g]) + k
                start[s] = edge_vertex(V[w], X, Y, ix, iy, f, level)
                end[s] = edge_vertex(V[w], X, Y, ix, iy, t, level)
                seg_layer[s] = w
                jx, jy = ix + NEIGHBOUR[t][0], iy + NEIGHBOUR[t][1]
                if 0 <= jx < nx - 1 and 0 <= jy < cy:
                    h = w * ncell + jx * cy + jy
                    for k2, (f2, _) in enumerate(cell_segments(int(case[h]), bool(centre_inside[h]))):
                        if f2 == (t + 2) % 4:
                            nxt[s] = int(offset[h]) + k2

    has_pred = np.zeros(n_seg, bool)
    has_pred[nxt[nxt >= 0]] = True
    done = np.zeros(n_seg, bool)
    chains = []                                          # (leader, [segments in order], closed)
    for s in np.flatnonzero(~has_pred):                  # open chains: from the segment without a predecessor
        run = []
        while s >= 0:
            run.append(int(s)); done[s] = True
            s = nxt[s]
        chains.append((run[0], run, False))
    for s in range(n_seg):                               # closed loops: ascending, so the first segment met is the smallest
        if done[s]:
            continue
        run = []
        while not done[s]:
            run.append(int(s)); done[s] = True
            s = int(nxt[s])
        assert s == run[0]
        chains.append((run[0], run, True))
    chains.sort(key=lambda c: c[0])

    points, offsets, closed, layer, area = [], [0], [], [], []
    for leader, run, is_closed in chains:
        p = [start[s] for s in run]
        if not is_closed:
            p.append(end[run[-1]])
        p = np.array(p, np.float64).reshape(-1, 2)
        acc = 0.0
        if is_closed:
            x, y = p[:, 0], p[:, 1]
            x1, y1 = np.roll(x, -1), np.roll(y, -1)
            with np.errstate(all='ignore'):
                for term in (x * y1 - x1 * y).tolist():
                    acc = acc + term
            acc = 0.5 * acc
        points.append(p); offsets.append(offsets[-1] + len(p)); closed.append(is_closed)
        layer.append(seg_layer[leader]); area.append(acc)
    return {
        'points': np.concatenate(points).reshape(-1, 2) if points else np.zeros((0, 2), np.float64),
        'offsets': np.array(offsets, np.int64),
        'closed': np.array(closed, bool),
        'layer': np.array(layer, np.int32),
        'area': np.array(area, np.float64),
        'n_segments': n_seg,
        'nonfinite_cells': int((~finite).sum()),
        # what the outputs follow from, for the tests of the linking
        'next': nxt, 'seg_start': start, 'seg_end': end, 'leaders': np.array([c[0] for c in chains], np.int64),
    }


ARRAYS = ('points', 'offsets', 'closed', 'layer', 'area')
