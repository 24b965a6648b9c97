"""The keywords that reach `core.meshed` from every facade of the post-meshing pipeline, pinned as literals.
`core.meshed` is replaced by a recorder that notes its arguments and stops the call, so nothing here needs a device.  A default is
LEFT OUT of the call (simplify=None, mend=False, snap=False, simplify_tolerance=None with simplify_levels=5), anything else travels
as it was given -- tests/test_export_host.py, whose stand-in for `meshed` expects `{}`, depends on the same property."""
import importlib

import pytest

# (by module name: the package's attributes `thickness`, `curvature`, ... are the functions)
core, curvature, deviation, measure, overhang, shells, supports, thickness = (importlib.import_module('sdf_amd.' + name) for name in (
    'core', 'curvature', 'deviation', 'measure', 'overhang', 'shells', 'supports', 'thickness'))


REAL_MESHED = core.meshed


class Reached(Exception):
    """the recorder's way out: the facade has made its call of `meshed`"""


@pytest.fixture
def calls(monkeypatch):
    seen = []

    def recorder(*args, **kwargs):
        seen.append((args, kwargs))
        raise Reached

    monkeypatch.setattr(core, 'meshed', recorder)
    return seen


# name -> (the call with the model 'model', what reaches `meshed` without any pipeline option, whether the facade has `snap=`)
PLAIN = {'keep': None}
QUIET = {'keep': None, 'simplify': None, 'mend': False, 'to_host': False, 'verbose': False}      # (`shells._meshed` names these four every time)
FACADES = {
    'generate_mesh': (lambda **kw: core.generate_mesh('model', **kw), PLAIN, True),
    'save': (lambda **kw: core.save('a.stl', 'model', **kw), PLAIN, True),
    'measure': (lambda **kw: measure.measure('model', **kw), PLAIN, True),
    'thickness': (lambda **kw: thickness.thickness('model', **kw), PLAIN, True),
    'curvature': (lambda **kw: curvature.curvature('model', **kw), PLAIN, True),
    'deviation': (lambda **kw: deviation.deviation('model', **kw), PLAIN, True),
    'overhangs': (lambda **kw: overhang.overhangs('model', **kw), PLAIN, False),
    'supports': (lambda **kw: supports.supports('model', **kw), PLAIN, False),
    'shells': (lambda **kw: shells.shells('model', **kw), QUIET, None),
    'measure_shells': (lambda **kw: shells.measure_shells('model', **kw), QUIET, None),
}

# (the options of the call, what they add to the keywords of `meshed`, whether the row needs `snap=`)
ROWS = [
    ({}, {}, False),
    ({'simplify': 2}, {'simplify': 2}, False),
    ({'simplify_tolerance': 0.01}, {'simplify_tolerance': 0.01, 'simplify_levels': 5}, False),
    ({'simplify_levels': 3}, {'simplify_tolerance': None, 'simplify_levels': 3}, False),
    ({'mend': True}, {'mend': True}, False),
    ({'snap': True}, {'snap': True}, True),
    ({'snap': {'iters': 2, 'tol': 0.0}}, {'snap': {'iters': 2, 'tol': 0.0}}, True),
    ({'simplify': 2, 'simplify_tolerance': 0.01, 'simplify_levels': 3, 'mend': True, 'snap': {'eps': 1e-3}},
     {'simplify': 2, 'simplify_tolerance': 0.01, 'simplify_levels': 3, 'mend': True, 'snap': {'eps': 1e-3}}, True),
    # the defaults, spelt out, are the call without them ...
    ({'simplify': None, 'simplify_tolerance': None, 'simplify_levels': 5, 'mend': False}, {}, False),
    ({'snap': False}, {}, True),
    # ... and only they: what merely compares equal to a default travels on, for `meshed` to judge
    ({'simplify_levels': 5.0}, {'simplify_tolerance': None, 'simplify_levels': 5.0}, False),
    ({'simplify_levels': True}, {'simplify_tolerance': None, 'simplify_levels': True}, False),
    ({'snap': None}, {'snap': None}, True),
    # the arguments of `generate` pass through untouched
    ({'step': 0.1, 'bounds': ((0, 0, 0), (1, 1, 1)), 'samples': 64, 'batch_size': 16, 'sparse': False, 'simplify': 3},
     {'step': 0.1, 'bounds': ((0, 0, 0), (1, 1, 1)), 'samples': 64, 'batch_size': 16, 'sparse': False, 'simplify': 3}, False),
]


@pytest.mark.parametrize('name', sorted(FACADES))
def test_the_keywords_that_reach_meshed(name, calls):
    call, base, has_snap = FACADES[name]
    for given, added, needs_snap in ROWS:
        if needs_snap and not has_snap:
            continue
        del calls[:]
        with pytest.raises(Reached):
            call(**given)
        assert calls == [(('model',), dict(base, **added))], (name, given)


def test_mend_none_is_not_the_default(calls):
    """mend=None is not mend=False: the six facades that fold it hand it on; the two of `shells`, which check it first, refuse it"""
    for name in ('generate_mesh', 'save', 'measure', 'thickness', 'curvature', 'deviation', 'overhangs', 'supports'):
        del calls[:]
        with pytest.raises(Reached):
            FACADES[name][0](mend=None)
        assert calls == [(('model',), {'keep': None, 'mend': None})], name
    for name in ('shells', 'measure_shells'):
        del calls[:]
        with pytest.raises(ValueError, match='mend'):
            FACADES[name][0](mend=None)
        assert calls == []


def test_verbose_cannot_be_given_to_shells(calls):
    """`shells` and `measure_shells` mesh quietly: a `verbose=` of the caller's is overridden, and `keep=` is not theirs to give"""
    for name in ('shells', 'measure_shells'):
        del calls[:]
        with pytest.raises(Reached):
            FACADES[name][0](verbose=True, step=0.2)
        assert calls == [(('model',), dict(QUIET, step=0.2))], name
        with pytest.raises(TypeError, match='keep'):
            FACADES[name][0](keep='largest')


def test_keep_and_positional_arguments(calls):
    with pytest.raises(Reached):
        core.save('a.stl', 'model', 0.1, None, 64, keep='largest', mend=True)
    assert calls.pop() == (('model', 0.1, None, 64), {'keep': 'largest', 'mend': True})
    with pytest.raises(Reached):
        curvature.curvature('model', 0.1, 0.05, keep=2)          # (step and eps are curvature's own: step is folded back in)
    assert calls.pop() == (('model',), {'keep': 2, 'step': 0.1})
    with pytest.raises(Reached):
        measure.measure('model', (0, 0, 0), 'largest', 2, True, 0.01, 3, {'iters': 1}, verbose=False)
    assert calls.pop() == (('model',), {'keep': 'largest', 'simplify': 2, 'mend': True, 'simplify_tolerance': 0.01, 'simplify_levels': 3,
                                        'snap': {'iters': 1}, 'verbose': False})


def test_overhangs_and_supports_have_no_snap_of_their_own(calls):
    """neither signature names `snap`: one that is given rides in **generate_kwargs, untouched -- False included, which the six
    facades with a `snap=` of their own leave out -- and it is `meshed` that checks it"""
    import inspect
    for name in ('overhangs', 'supports'):
        fn = getattr(overhang if name == 'overhangs' else supports, name)
        assert 'snap' not in inspect.signature(fn).parameters
        for value in (True, False, {'iters': 2}, 'no'):
            del calls[:]
            with pytest.raises(Reached):
                FACADES[name][0](snap=value, mend=True)
            assert calls == [(('model',), {'keep': None, 'snap': value, 'mend': True})], (name, value)
    with pytest.raises(ValueError, match='snap: True, False or a dict'):
        next(REAL_MESHED.__wrapped__('model', snap='no'))          # (a generator function: the check runs on its first step)
