"""The arena helper of the view-contract suite (tests/view_arena_common.py), on CPU tensors: the windows are what their kinds promise, the checker
sees a store outside a window (guards, pitch pads, neighbouring trials), the coverage table lists every reachable store path under the path
its launcher predicate picks, and the FAIL-injected inputs of tests/test_gpu_view_bounds.py FAIL where planned on oracle/c."""
import collections

import numpy as np
import pytest

import closed_shapes_common as cs
import gpu_harness as gh
import view_arena_common as va

SHAPES = [(70, 60, 48), (69, 60, 8), (2, 5, 6), (1, 1, 1), (4, 80, 224), (35, 12, 8), (257, 1, 3)]


def _elements(window):
    """Offsets into the allocation of the elements the window addresses, (T, K, comp)."""
    T, K, comp = window.shape
    st, sk, sc = window.stride()
    return window.storage_offset() + st * np.arange(T)[:, None, None] + sk * np.arange(K)[None, :, None] + sc * np.arange(comp)[None, None, :]


@pytest.mark.parametrize('kind', va.KINDS)
@pytest.mark.parametrize('T,K,comp', SHAPES)
def test_every_kind_gives_a_valid_window_between_two_guards(kind, T, K, comp):
    import torch
    assert va.POISON_INT == gh.POISON_INT
    whole, window, before = va.arena(T, K, comp, kind)
    geo = va.geometry(T, K, comp, kind)
    idx = _elements(window)
    assert window.shape == (T, K, comp) and len(np.unique(idx)) == T * K * comp                     # distinct elements
    assert (idx.min() - 0) * 8 >= va.GUARD_BYTES and (whole.numel() - 1 - idx.max()) * 8 >= va.GUARD_BYTES
    assert torch.isnan(whole).all() and torch.isnan(before).all() and before.data_ptr() != whole.data_ptr()
    assert window.stride() == (geo.st, geo.sk, geo.sc) and window.storage_offset() == geo.offset
    assert window.data_ptr() % 16 == (8 if kind.endswith('base8') or (kind == 'ktc_slice' and comp % 2) else 0)
    st, sk, sc = window.stride()
    if kind.startswith('kct'):
        pitch = T + {'kct_pitch_even': 6, 'kct_pitch_odd': 5}.get(kind, 0)
        assert (st, sk, sc) == (1, comp * pitch, pitch)
    elif kind.startswith('ktc'):
        assert (st, sk, sc) == (comp, (T + (8 if kind == 'ktc_slice' else 0)) * comp, 1)
    else:
        assert (st, sk, sc) == ((K + (1 if kind == 'tkc_slice' else 0)) * comp, comp, 1)
    # integers: poisoned with POISON_INT, guards as wide in bytes
    iw, iwin, _ = va.arena(T, 1, 1, kind, dtype=torch.int32)
    assert (iw == gh.POISON_INT).all() and iwin.storage_offset() * 4 >= va.GUARD_BYTES


def _outside_targets(kind, T, K, comp, window, whole):
    """Offsets outside the window that a kernel one trial, row or record off would hit: (name, offset)."""
    first, last = int(_elements(window).min()), int(_elements(window).max())
    out = [('front guard', first - 1), ('front guard, a wavefront back', first - 1536), ('back guard', last + 1), ('end of the allocation', whole.numel() - 1),
           ('start of the allocation', 0)]
    st, sk, sc = window.stride()
    if 'pitch' in kind:
        out += [('pitch pad after trial T - 1', window.storage_offset() + T), ('pitch pad of the last row', last + 2)]
    if kind == 'ktc_slice':
        out += [('the record before trial 0', window.storage_offset() - 1), ('the record after trial T - 1', window.storage_offset() + T * st),
                ('trial T of the last step', last + 1)]
    if kind == 'tkc_slice':
        out += [('row K of trial 0', window.storage_offset() + K * sk), ('trial -1', window.storage_offset() - 1), ('trial T', window.storage_offset() + T * st)]
    return out


@pytest.mark.parametrize('kind', va.KINDS)
@pytest.mark.parametrize('T,K,comp', [(70, 60, 48), (69, 7, 8), (2, 3, 6)])
def test_the_checker_passes_a_written_window_and_sees_one_element_outside(kind, T, K, comp):
    whole, window, before = va.arena(T, K, comp, kind)
    window.fill_(1.5)
    va.assert_only_the_window_changed(whole, window, before, (kind,))
    with pytest.raises(AssertionError):                                                            # the same buffer as an input: it changed
        va.assert_only_the_window_changed(whole, None, before, (kind,))
    for name, off in _outside_targets(kind, T, K, comp, window, whole):
        assert off not in set(_elements(window).ravel().tolist()), (name, 'is no outside target')
        keep = whole[off].clone()
        whole[off] = 2.5
        assert va.strays(whole, window, before).tolist() == [off], (kind, name)
        with pytest.raises(AssertionError, match='outside the view'):
            va.assert_only_the_window_changed(whole, window, before, (kind, name))
        whole[off] = keep
    # a NaN with another payload is a change too: bytes are compared, not values
    whole.view(__import__('torch').int64)[0] ^= 1
    assert va.strays(whole, window, before).tolist() == [0]


@pytest.mark.parametrize('kind', ['kct', 'kct_pitch_even', 'ktc', 'ktc_slice', 'tkc', 'tkc_slice'])
def test_a_window_written_for_one_trial_too_many_is_reported_as_that_trial(kind):
    """Checker sensitivity without a broken kernel: T trials written, checked against the window of T - 1."""
    T, K, comp = 70, 9, 8
    whole, window, before = va.arena(T, K, comp, kind)
    window.fill_(3.0)
    idx = va.strays(whole, window[:T - 1], before)
    assert sorted(idx.tolist()) == sorted(_elements(window)[T - 1].ravel().tolist())
    with pytest.raises(AssertionError, match=f'{K * comp} elements changed outside the view'):
        va.assert_only_the_window_changed(whole, window[:T - 1], before, (kind,))
    va.assert_only_the_window_changed(whole, window, before, (kind,))


def test_integer_and_byte_arenas():
    import torch
    whole, window, before = va.arena(70, 1, 1, 'ktc_slice', dtype=torch.int32)
    window.fill_(0)
    va.assert_only_the_window_changed(whole, window, before, ())
    whole[window.storage_offset() + 70] = 0                                                        # trial T of somebody else's status
    with pytest.raises(AssertionError):
        va.assert_only_the_window_changed(whole, window, before, ())
    whole, window, before = va.byte_arena(1000)
    assert window.data_ptr() % 256 == 0 and window.numel() == 1000
    lead = window.data_ptr() - whole.data_ptr()
    assert lead >= va.GUARD_BYTES and whole.numel() - lead - 1000 >= va.GUARD_BYTES
    window.fill_(0)
    va.assert_only_the_window_changed(whole, window, before, ())
    whole[lead + 1000] = 0
    assert va.strays(whole, window, before).tolist() == [lead + 1000]


def test_the_predictors_on_tensors_and_geometries_agree():
    for kind in va.KINDS:
        for T in va.CLOSED_T:
            _, window, _ = va.arena(T, 60, 48, kind)
            geo = va.geometry(T, 60, 48, kind)
            assert va._facts(window) == va._facts(geo), (kind, T)
    # what each kind is named for, at the headline kernel (KF, two lanes, DH plant)
    path = lambda kind, T, **kw: va.closed_x_path(8, 6, 2, 'KF', 'dh', kw.get('per_trial', False), kw.get('strict', False), T, va.geometry(T, 60, 48, kind))   # noqa: E731
    assert [path('kct', T) for T in (64, 70, 69, 2)] == ['pairs', 'pairs', 'plain', 'pairs']
    assert path('kct_pitch_even', 70) == 'pairs' and path('kct_pitch_odd', 70) == 'plain' and path('kct_base8', 70) == 'plain'
    assert path('ktc', 69) == 'records' and path('ktc_slice', 69) == 'records' and path('ktc_base8', 64) == 'plain'
    assert path('tkc', 64) == 'plain' and path('tkc_slice', 64) == 'plain'
    assert path('ktc', 64, strict=True) == 'plain' and path('ktc', 64, per_trial=True) == 'plain'
    assert va.closed_x_path(8, 6, 2, 'GMCKF', 'dh', False, False, 64, va.geometry(64, 60, 48, 'ktc')) == 'plain'
    assert va.closed_x_path(8, 6, 2, 'KF', 'linear', False, False, 64, va.geometry(64, 60, 48, 'ktc')) == 'plain'
    assert va.closed_x_path(8, 6, 4, 'KF', 'dh', False, False, 64, va.geometry(64, 60, 48, 'ktc')) == 'plain'


def test_the_coverage_table_lists_every_reachable_cell_under_its_predicted_path():
    paths = {'closed': ('records', 'pairs', 'plain'), 'wide': ('records', 'plain'),
             'replay': ('records', 'rowgroups', 'lanegroups', 'control', 'twolane', 'generic')}
    rags = {'closed': ('whole', 'ragged_even', 'ragged_odd', 'single'), 'wide': ('whole', 'single'), 'replay': ('whole', 'ragged_odd')}
    for entry in paths:
        listed = collections.Counter()
        for path, rag, combo in va.cells_of(entry):
            assert va.predicted(entry, combo) == (path, rag), (entry, combo)
            listed[combo] += 1
        assert set(listed) == set(va.universe(entry)) and set(listed.values()) == {1}, entry       # every combination of the axes, once
        for path in paths[entry]:
            for rag in rags[entry]:
                if (entry, path, rag) in va.UNREACHABLE:
                    assert (entry, path, rag) not in va.CELLS
                    continue
                assert len(va.CELLS[(entry, path, rag)]) >= 1, (entry, path, rag)
    assert all(key[0] in paths and key[1] in paths[key[0]] and key[2] in rags[key[0]] for key in va.CELLS)
    # the unreachable cells are unreachable by the predicates, not by the table: no view kind changes that
    for kind in va.KINDS:
        assert va.closed_x_path(8, 6, 2, 'KF', 'dh', False, False, 69, va.geometry(69, 60, 48, kind)) != 'pairs'
        assert va.wide_x_path(8, 4, va.geometry(4, 80, 224, kind)) == 'plain'
        assert va.replay_path('KF', 0, ('x', 'err'), 35, va.geometry(35, 12, 48, kind), va.geometry(35, 12, 8, kind)) != 'records'


@pytest.mark.parametrize('method', ['KF', 'GMCKF'])
def test_the_injected_fails_land_where_planned_on_the_c_oracle(method):
    from oracle import c_oracle
    inp = cs.inputs('dh86')
    base = cs.c_reference('dh86', method, False)
    assert not base['status'].any() and np.all(base['k_done'] == inp['K'])
    noise = va.inject_fails(inp['noise'])
    assert np.isnan(noise).sum() == len(va.FAIL_PLAN) and set(va.FAIL_PLAN) >= set(range(64, 70)) and 17 in va.FAIL_PLAN.values() and 0 in va.FAIL_PLAN.values()
    ref = c_oracle.closed_loop_batch(inp['q0'], noise, inp['desired'], method=method, kernel_bw=inp['bw'], annealing=False, dt=cs.DT, t_max=inp['t_max'],
                                     gain=cs.GAIN, steps=inp['K'], want_x=True, plant=cs.c_plant(inp), fpi_threshold=cs.FPI_THRESHOLD)
    assert np.flatnonzero(ref['status']).tolist() == sorted(va.FAIL_PLAN)
    for t in range(inp['T']):
        assert ref['k_done'][t] == va.FAIL_PLAN.get(t, inp['K']), t
        if t not in va.FAIL_PLAN:                                                                  # nobody else notices
            assert all(gh.same_bits(ref[k][t], base[k][t]) for k in ('err', 'q', 'X', 'stats', 'status'))
