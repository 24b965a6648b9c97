"""The four stages of `core.meshed` -- keep, simplify, snap, mend -- in ONE call, against the four `engine.Mesh`
calls made by hand in that order: the soup bit for bit, and the statistics of every stage where a caller looks for them (simplify's
on the `Meshed`, snap's and mend's riding on the final mesh; `kernel_ms` is a time and is left out).  The model is two disjoint
spheres at step 0.1 with simplify=2: 1284 triangles in two shells, clusters that collapse three quarters of them (the mend finds
nothing to drop on these spheres: its statistics are compared all the same, and tests/test_mend_gpu.py has the meshes it works on)."""
import numpy as np
import pytest

from sdf_amd import core
from sdf_amd.deviation import snap_params
from sdf_amd.shells import resolve_keep
from sdf_amd.simplify import resolve_cell

pytestmark = pytest.mark.gpu

STEP, CLUSTER = 0.1, 2


def timeless(stats):
    return {k: v for k, v in stats.items() if k != 'kernel_ms'}


def by_hand(f, eng, keep):
    """(soup, weld, simplify_stats, snap_stats, mend_stats) of the four calls in the order of `meshed`"""
    bounds = core._estimate_bounds(f)
    X, Y, Z, steps = core.grid_axes(bounds, STEP)
    made = [eng.generate(f, X, Y, Z, core.BATCH_SIZE, True)]
    try:
        made.append(made[-1].select(resolve_keep(keep, made[-1].shell_summary()['triangles'])))
        made.append(made[-1].simplify(*resolve_cell(float(CLUSTER), X, Y, Z, steps)))
        made.append(made[-1].snap(f, **snap_params({}, bounds, steps, float(CLUSTER))))
        made.append(made[-1].mend())
        assert made[0].shell_summary()['count'] == 2
        return (np.array(made[4].points()), made[4].weld(), timeless(made[2].simplify_stats), timeless(made[3].snap_stats),
                timeless(made[4].mend_stats))
    finally:
        for m in made:
            m.close()


@pytest.mark.parametrize('keep', ['largest', 2])
def test_four_stages_in_one_call(keep, ns, eng):
    f = ns['sphere'](0.5) | ns['sphere'](0.3).translate((1.2, 0, 0))
    soup, (pts, cells), simplify_stats, snap_stats, mend_stats = by_hand(f, eng, keep)
    print('keep=%r: %d triangles; simplify %r; snap %r; mend %r' % (keep, len(soup) // 3, simplify_stats, snap_stats, mend_stats))
    assert len(soup) and simplify_stats['collapsed'] > 0 and snap_stats['vertices'] > 0
    options = dict(keep=keep, simplify=CLUSTER, snap=True, mend=True, step=STEP, verbose=False)

    with core.meshed(f, **options) as m:
        got = np.array(m.mesh.points())
        assert got.dtype == soup.dtype and got.shape == soup.shape and np.array_equal(got.view(np.uint64), soup.view(np.uint64))
        assert timeless(m.simplify_stats) == simplify_stats
        assert timeless(m.mesh.snap_stats) == snap_stats          # (carried through the mend)
        assert timeless(m.mesh.mend_stats) == mend_stats and m.mesh.n_triangles == mend_stats['triangles_out']

    p, c, _ = core.generate_mesh(f, **options)
    assert np.array_equal(p.view(np.uint64), pts.view(np.uint64)) and np.array_equal(c, cells)
    assert timeless(core.generate_mesh.last_simplify) == simplify_stats and timeless(core.generate_mesh.last_snap) == snap_stats
    assert timeless(core.generate_mesh.last_mend) == mend_stats
