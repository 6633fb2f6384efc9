"""uvs_filter_params.reg and .anneal_span, launch-wide, and uvs_trial_params.reg / .fpi_threshold, per trial, on every route that reads
them.  engine.make_params writes reg = 1e-6 and anneal_span = 100 into every block the rest of the suite builds, so a kernel that used
the literals instead of the fields would pass everything else; here the fields are set on the struct after make_params and the kernels
are held to CPU references computed with the same values (tests/estimator_params_common.py: oracle/c and oracle/rmckf_block, held to
each other -- and shown to be far from their default-valued runs -- by tests/test_oracle_c.py).

Every output buffer is filled with NaN (-7 for the integers) before the launch.  Gates are the routes' own: closed loop 1e-8 on err, q, X
and the statistics with status and k_done exact (test_gpu_closed_shapes.TOL); single step X 1e-10, P 1e-9, command 1e-7, kappa 1e-9
(test_gpu_step); replay X 1e-10, command 1e-8, kappa 1e-9, final P 1e-10 (test_replay_other_shapes_match_block_oracle); fp32 replay 1e-5.
The worst deviation per route is printed when the module finishes (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import closed_shapes_common as cs
import estimator_params_common as ep
from sweep_common import STATS_TOL
from test_gpu_closed_shapes import (BLOCK_TRIALS, LATENCY, POISON_INT, STREAMS, STRICT, TOL, TOL_MODES, _assert_everything_was_stored,
                                    _assert_same_launch, _assert_twins, _cuda, _live, _per_trial_rel, _poisoned, _same_bits)
from test_gpu_step import DEFAULT_LANES, K_MAX, SHAPES, TOL_DQ, TOL_KAPPA, TOL_P, TOL_X

pytestmark = pytest.mark.gpu

REG, SPAN = ep.REG, ep.ANNEAL_SPAN
WORST = {}                                                   # route -> quantity -> worst relative deviation from the references so far
NOTES = []
_PLANTS, _LAUNCHES = {}, {}
CLOSED_SETS = [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF'), ('A25', 'MCKF')]
SQUARE_SETS = [('R3', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF'), ('A25', 'MCKF')]     # (6,6) on the DH plant: R3 in place of R25


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    for route, worst in WORST.items():
        print(f'estimator params, {route}: worst relative deviations', {k: f'{v:.1e}' for k, v in worst.items()})
    print('estimator params: trials left out of the gates (the CPU oracles disagree there):', {k: list(v) for k, v in ep.EXCLUDED.items()})
    for note in NOTES:
        print('estimator params:', note)


def _note(route, key, value):
    worst = WORST.setdefault(route, {})
    worst[key] = max(worst.get(key, 0.0), float(value))


# ---------------------------------------------------------------------------------------------- closed-loop launches and their references
def _inputs(case):
    """cs.inputs(case), or for 'wide' the (32,7) linear plant: (inputs, steps, kernel_bw)."""
    return (ep.wide_inputs(), ep.WIDE_K, ep.WIDE_BW) if case == 'wide' else (cs.inputs(case), cs.K, cs.BW)


def _plant(uvs, case):
    if case not in _PLANTS:
        inp = _inputs(case)[0]
        if inp.get('kind') == 'dh':
            plant = uvs.SyntheticPlant.ur10(inp['desired'])
            assert np.allclose(plant.points[:len(inp['discs'])], inp['discs'], rtol=0, atol=1e-15)
        else:
            plant = uvs.LinearPlant(*inp['lin'])
        _PLANTS[case] = plant
    return _PLANTS[case]


def _closed(uvs, case, method, anneal, reg, span, lanes=0, reserved=0, want=('x', 'err', 'q')):
    """One closed-loop launch (uvs_rmckf_closed_loop_ws_f64) on every trial of the case with fp.reg and fp.anneal_span set after
    make_params; numpy arrays in [trial][step][component] order plus what the host-side queries say.  Launches are kept."""
    key = (case, method, anneal, reg, span, lanes, reserved, want)
    if key in _LAUNCHES:
        return _LAUNCHES[key]
    import torch
    inp, K, bw = _inputs(case)
    m, n, guess = inp['m'], inp['n'], inp.get('guess', False)
    T = len(inp['q0'])
    fp = uvs.engine.make_params(m, n, method, bw, anneal, cs.DT, cs.DT * (K + 0.5), cs.GAIN, inp['desired'], guess, lanes, K, cs.FPI_THRESHOLD, 1000)
    assert fp.k_max == K and fp.reg == REG and fp.anneal_span == SPAN
    fp.reg, fp.anneal_span, fp.reserved = reg, span, reserved
    ps = _plant(uvs, case).to_struct()
    noise, q0 = _cuda(inp['noise'].transpose(1, 2, 0)), _cuda(inp['q0'])
    start = None if guess else _cuda(inp['x0'])
    comps = {'x': m * n, 'err': m, 'q': n, 'f': m, 'dq': n}
    dev = {k: _poisoned(T, K, comps[k], 'kct') if k in want else None for k in STREAMS}
    dev.update(stats=torch.full((T, 3), float('nan'), dtype=torch.float64, device='cuda'),
               status=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'), k_done=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'))
    flat = lambda t: uvs._lib.NULL_VIEW if t is None else uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))      # noqa: E731
    rc = uvs.engine.launch_closed_loop(fp, ps, T, flat(q0), uvs.engine.stream_view(noise), flat(start), *(uvs.engine.stream_view(dev[k]) for k in STREAMS),
                                       dev['stats'].data_ptr(), dev['status'].data_ptr(), dev['k_done'].data_ptr(), uvs._lib.NULL_VIEW, uvs._lib.NULL_VIEW)
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    assert (fp.reg, fp.anneal_span) == (reg, span)
    out = {'lanes': int(uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp), C.byref(ps), T)),
           'segments': int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(fp), C.byref(ps), T)),
           'workspace': int(uvs.lib().uvs_rmckf_closed_loop_workspace_bytes(C.byref(fp), C.byref(ps), T)),
           'fallbacks': uvs.engine.hand_over_fallbacks(fp, ps, T)}
    for k in STREAMS:
        out[k] = None if dev[k] is None else np.ascontiguousarray(uvs.engine.as_tkc(dev[k]).cpu().numpy())
    for k in ('stats', 'status', 'k_done'):
        out[k] = dev[k].cpu().numpy()
    _assert_everything_was_stored(out, key)
    _LAUNCHES[key] = out
    return out


def _launch_set(uvs, case, name, method, lanes=0, reserved=0):
    anneal, reg, span = ep.estimator(name, method)
    return _closed(uvs, case, method, anneal, reg, span, lanes, reserved)


def _assert_matches(out, ref, kept, block_of, block_trials, route, tag):
    """status and k_done on every trial; err, q, X and the statistics on the trials `kept` against oracle/c (`ref`), and on `block_trials`
    against oracle/rmckf_block (numpy pinv)."""
    T, K = out['err'].shape[:2]
    assert np.array_equal(out['status'], ref['status'][:T]) and np.array_equal(out['k_done'], ref['k_done'][:T]), tag
    kept = list(kept)
    live = np.arange(K)[None, :, None] < ref['k_done'][:T, None, None]
    for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
        d = _per_trial_rel(_live(out, key), np.where(live, ref[rk][:T], 0.0))[kept]
        _note(route, key, d.max())
        assert d.max() <= TOL, (key, float(d.max()), kept[int(d.argmax())]) + tuple(tag)
    ok = [t for t in kept if ref['status'][t] == 0]
    d = _per_trial_rel(out['stats'][ok], ref['stats'][ok])
    _note(route, 'stats', d.max())
    assert d.max() <= TOL, ('stats', float(d.max())) + tuple(tag)
    for t in block_trials:
        blk = block_of(t)
        k = blk['k_done']
        assert out['status'][t] == blk['status'] and out['k_done'][t] == k and k > 0, (t,) + tuple(tag)
        for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
            d = cs.rel(out[key][t, :k], blk[rk])
            _note(route, key + ' (numpy)', d)
            assert d <= TOL, (key, d, t) + tuple(tag)
        assert cs.rel(out['stats'][t], blk['stats']) <= TOL, (t,) + tuple(tag)


def _hold(out, case, name, method, route, tag=()):
    """The launch against the two oracles run at parameter set `name` (every estimator of the set's; KF: any set, it reads neither field)."""
    tag = (case, name, method, route) + tuple(tag)
    if case == 'wide':
        _assert_matches(out, ep.wide_c_reference(name, method), range(ep.WIDE_T), lambda t: ep.wide_block_reference(name, method, t), range(ep.WIDE_T), route, tag)
    else:
        kept = ep.kept_trials(case, name, method)
        _assert_matches(out, ep.c_reference(case, name, method), kept, lambda t: ep.block_reference(case, name, method, t),
                        [t for t in BLOCK_TRIALS if t in kept], route, tag)
        _assert_twins(out, tag)


# ---------------------------------------------------------------------------------------------- a. closed loop, launch-wide values
# route -> (lanes_per_filter, option bits, lanes the plan reports)
DH86_ROUTES = {'tuned L1': (1, 0, 1), 'tuned L2': (2, 0, 2), 'tuned L4': (4, 0, 4), 'small batch': (0, 0, 4), 'UVS_OPT_LATENCY': (0, LATENCY, 4),
               'wide L8': (8, 0, 8), 'generic L1': (-1, 0, 1), 'generic L2': (-2, 0, 2), 'generic L4': (-4, 0, 4)}


DH86_CASES = [(route, name, method) for route in DH86_ROUTES for name, method in CLOSED_SETS if not (method == 'MCKF' and route == 'wide L8')]


@pytest.mark.parametrize('route,name,method', DH86_CASES)
def test_dh86_every_route_reads_reg_and_anneal_span(uvs, route, name, method):
    """(8,6) on the DH plant from the analytic guess, T = 70: closed_loop_tuned_kernel<8, 6, {1, 2, 4}>, the four-lane small-batch kernels that
    lanes_per_filter 0 takes at this size (the two-lane kernel's bits), the plain four-lane kernels under UVS_OPT_LATENCY, the wide kernel's DH
    instantiation at eight lanes and the generic templates.  MCKF has a tuned kernel on two lanes only: 1, 4 and UVS_OPT_LATENCY (which
    keeps it on two lanes) are held all the same, eight lanes are left out (the wide kernel has no MCKF)."""
    lanes, reserved, L = DH86_ROUTES[route]
    out = _launch_set(uvs, 'dh86', name, method, lanes, reserved)
    assert out['lanes'] == (2 if method == 'MCKF' and route == 'UVS_OPT_LATENCY' else L) and out['segments'] == 1
    _hold(out, 'dh86', name, method, f'(8,6) DH {route}')
    if route == 'small batch':
        _assert_same_launch(_launch_set(uvs, 'dh86', name, method, 2), out, (name, method, 'small batch = two lanes'))


@pytest.mark.parametrize('name', ['R25', 'A25'])
def test_dh86_rmckf_under_strict_pinv(uvs, name):
    """UVS_OPT_STRICT_PINV at two lanes: the certifying instantiation of the tuned kernel.  Inside the oracle gates and within 1e-9 of the
    default mode."""
    fast, strict = _launch_set(uvs, 'dh86', name, 'GMCKF', 2), _launch_set(uvs, 'dh86', name, 'GMCKF', 2, STRICT)
    assert strict['lanes'] == 2 and strict['segments'] == 1
    _hold(strict, 'dh86', name, 'GMCKF', '(8,6) DH strict pinv')
    for key in ('err', 'q'):
        assert cs.rel(_live(strict, key), _live(fast, key)) <= TOL_MODES, (key, name)
    NOTES.append(f'strict pinv, dh86 {name}: the bits of the default mode: {_same_bits(_live(strict, "x"), _live(fast, "x"))}')


@pytest.mark.parametrize('name', ['A25', 'A400'])
def test_dh86_mckf_in_four_segments(uvs, name):
    """fp.reserved = 4 << 8: the two-lane MCKF kernel runs every trial as four work items whose state crosses through the workspace and
    every one of which forms its own bandwidths.  The bits of whole trials, no work item fell back, inside the oracle gates."""
    whole = _launch_set(uvs, 'dh86', name, 'MCKF', 2)
    assert whole['segments'] == 1 and whole['workspace'] == 0 and whole['fallbacks'] is None
    for lanes in (0, 2):
        cut = _launch_set(uvs, 'dh86', name, 'MCKF', lanes, 4 << 8)
        assert cut['lanes'] == 2 and cut['segments'] == 4 and cut['workspace'] > 0 and cut['fallbacks'] == 0
        _assert_same_launch(whole, cut, (name, lanes, 'segments'))
        _hold(cut, 'dh86', name, 'MCKF', '(8,6) DH MCKF in 4 segments')


@pytest.mark.parametrize('name,method', SQUARE_SETS)
@pytest.mark.parametrize('case', ['dh66', 'dh66_x0'])
def test_dh66_reads_reg_and_anneal_span(uvs, case, name, method):
    """(6,6) on the DH plant: the tuned two-lane kernel and the generic (6,6,1) and (6,6,2) templates."""
    for lanes in (2, -1, -2):
        out = _launch_set(uvs, case, name, method, lanes)
        assert out['lanes'] == abs(lanes) and out['segments'] == 1
        _hold(out, case, name, method, f'(6,6) DH {"tuned" if lanes > 0 else "generic L" + str(-lanes)}')


@pytest.mark.parametrize('name,method', CLOSED_SETS)
def test_dh26_reads_reg_and_anneal_span(uvs, name, method):
    """(2,6), m < n: the generic (2,6,1) kernel.  R3 and A400 with IMCC-KF move this one-point loop least (tests/test_oracle_c.py prints by how
    much); R25 and A25 with RMCKF are the sets with the margin."""
    out = _launch_set(uvs, 'dh26', name, method, 1)
    assert out['lanes'] == 1
    _hold(out, 'dh26', name, method, '(2,6) DH generic')


@pytest.mark.parametrize('name,method', CLOSED_SETS)
@pytest.mark.parametrize('case,lanes_tried', [('lin86', (1, 2, 4)), ('lin66', (2,))])
def test_linear_plant_reads_reg_and_anneal_span(uvs, case, lanes_tried, name, method):
    """The UVS_PLANT_LINEAR instantiations of the tuned kernels (MCKF: tuned on two lanes, generic on one and four)."""
    for lanes in lanes_tried:
        out = _launch_set(uvs, case, name, method, lanes)
        assert out['lanes'] == lanes and out['segments'] == 1 and out['workspace'] == 0
        _hold(out, case, name, method, f'{"(8,6)" if case == "lin86" else "(6,6)"} linear L{lanes}')


@pytest.mark.parametrize('name,method', [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF')])
@pytest.mark.parametrize('lanes', [0, 8, 16, 32, -8])
def test_wide_shape_reads_reg_and_anneal_span(uvs, lanes, name, method):
    """(32,7) on the linear plant (the inputs of test_closed_loop_stress_plant, T = 4, K = 80, k_max = K): the wide kernel at 8 (the default)
    and 16 lanes, the generic template at 32 and at a forced 8."""
    out = _launch_set(uvs, 'wide', name, method, lanes)
    assert out['lanes'] == (abs(lanes) or 8)
    _hold(out, 'wide', name, method, f'(32,7) {"wide" if lanes in (0, 8, 16) else "generic"} L{abs(lanes) or 8}')
    if lanes == 8:
        _assert_same_launch(_launch_set(uvs, 'wide', name, method, 0), out, (name, method, '0 = 8'))


# ---------------------------------------------------------------------------------------------- b. what must not depend on them
INDEPENDENCE_ROUTES = [('dh86', 2), ('dh86', -2), ('wide', 0)]      # a tuned kernel, a generic template, the wide kernel


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_kf_reads_neither_field_nor_the_annealing_flag(uvs, case, lanes):
    """KF has no correntropy weight: identical bits for (reg, anneal_span, annealing) = (default, default, off), (0.25, 25, on) and
    (1e-3, 400, on), and inside the gates of the KF oracle."""
    base = _closed(uvs, case, 'KF', False, REG, SPAN, lanes)
    _hold(base, case, 'R25', 'KF', f'KF, {case} lanes {lanes}')                              # estimator('R25', 'KF'): annealing off, the defaults
    for anneal, reg, span in ((True, 0.25, 25.0), (True, 1e-3, 400.0)):
        _assert_same_launch(base, _closed(uvs, case, 'KF', anneal, reg, span, lanes), (case, lanes, anneal, reg, span))


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_imcckf_and_mckf_do_not_read_reg(uvs, case, lanes):
    """Only RMCKF regularises its weights (experiment.py:280): IMCC-KF and MCKF (not on the wide kernel) give identical bits for
    reg = default and reg = 0.25, with annealing over a span of 25 and without."""
    for method in ('IMCCKF',) if case == 'wide' else ('IMCCKF', 'MCKF'):
        for anneal, span in ((True, 25.0), (False, SPAN)):
            a, b = _closed(uvs, case, method, anneal, REG, span, lanes), _closed(uvs, case, method, anneal, 0.25, span, lanes)
            _assert_same_launch(a, b, (case, lanes, method, anneal))
        _hold(_closed(uvs, case, method, True, 0.25, 25.0, lanes), case, 'A25', method, f'{method} with reg = 0.25, {case} lanes {lanes}')


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_annealing_over_a_zero_span_is_no_annealing(uvs, case, lanes):
    """annealing = 1 with anneal_span = 0: sigma_k = kernel_bw at every step, so the launch passes the oracle gates of annealing off (RMCKF at
    reg = 0.25: set R25; IMCC-KF).  Whether the bits are those of annealing off too is printed, not asserted."""
    for method, reg in (('GMCKF', 0.25), ('IMCCKF', REG)):
        on = _closed(uvs, case, method, True, reg, 0.0, lanes)
        _hold(on, case, 'R25', method, f'anneal_span = 0, {case} lanes {lanes}')
        off = _closed(uvs, case, method, False, reg, SPAN, lanes)
        NOTES.append(f'anneal_span = 0 against annealing off, {case} lanes {lanes} {method}: same bits: {_same_bits(_live(on, "x"), _live(off, "x"))}')


# ---------------------------------------------------------------------------------------------- c. replay
REPLAY_T = 35                                                # (8,6) at four lanes per filter: two wavefronts and three trials
REPLAY_SETS = [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF')]
FULL, ALONE = ('x', 'err', 'kappa', 'dqcmd'), ('x', 'err', 'kappa')


@functools.lru_cache(maxsize=None)
def _replay_case(case, name, method):
    """Streams recorded from the block oracle's closed loop at the set: f (T, K + 1, m) with row 0 the first f_old, dq (T, K, n) the regressor
    of every step (the command before it: the difference quotient of q), x0, desired -- and rmckf_block.run_replay on them, at the set."""
    from oracle import rmckf_block
    inp, K, bw = _inputs(case)
    T = min(REPLAY_T, len(inp['q0']))
    m, n = inp['m'], inp['n']
    anneal, reg, span = ep.estimator(name, method)
    f, dq = np.zeros((T, K + 1, m)), np.zeros((T, K, n))
    for t in range(T):
        run = ep.wide_block_reference(name, method, t) if case == 'wide' else ep.block_reference(case, name, method, t)
        assert run['status'] == 0 and run['k_done'] == K
        f[t, 0] = inp['features'](inp['q0'][t]) if inp.get('guess', False) else 0.0
        f[t, 1:] = run['err'] + inp['desired']
        dq[t, 1:] = np.diff(run['q'], axis=0) / cs.DT
    x0 = np.array(inp['x0'][:T])
    refs = [rmckf_block.run_replay(f[t], dq[t], x0[t], inp['desired'], cs.GAIN, method, bw, anneal, K, cs.FPI_THRESHOLD, reg=reg, anneal_span=span)
            for t in range(T)]
    return f, dq, x0, refs


def _replay(uvs, case, name, method, lanes, want, reg=None, span=None):
    """uvs_rmckf_replay_f64 on the streams of _replay_case with fp.reg / fp.anneal_span of the set (or as given), into NaN-filled buffers."""
    import torch
    inp, K, bw = _inputs(case)
    f, dq, x0, _ = _replay_case(case, name, method)
    T, m, n = len(x0), inp['m'], inp['n']
    anneal, set_reg, set_span = ep.estimator(name, method)
    fp = uvs.engine.make_params(m, n, method, bw, anneal, cs.DT, cs.DT * (K + 0.5), cs.GAIN, inp['desired'], False, lanes, K, cs.FPI_THRESHOLD, 1000)
    assert fp.k_max == K
    fp.reg, fp.anneal_span = set_reg if reg is None else reg, set_span if span is None else span
    f_dev, dq_dev, x0_dev = _cuda(f.transpose(1, 2, 0)), _cuda(dq.transpose(1, 2, 0)), _cuda(x0)
    comps = {'x': m * n, 'err': m, 'kappa': m, 'dqcmd': n}
    dev = {k: _poisoned(T, K, comps[k], 'kct') if k in want else None for k in comps}
    dev.update(status=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'), k_done=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'),
               x_final=torch.full((T, m * n), float('nan'), dtype=torch.float64, device='cuda'),
               p_final=torch.full((T, m * n * n), float('nan'), dtype=torch.float64, device='cuda'))
    flat = lambda t: uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))                # noqa: E731
    view = uvs.engine.stream_view
    rc = uvs.lib().uvs_rmckf_replay_f64(C.byref(fp), T, view(f_dev), view(dq_dev), flat(x0_dev), *(view(dev[k]) for k in comps),
                                        dev['status'].data_ptr(), dev['k_done'].data_ptr(), flat(dev['x_final']), flat(dev['p_final']),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    out = {k: None if dev[k] is None else np.ascontiguousarray(uvs.engine.as_tkc(dev[k]).cpu().numpy()) for k in comps}
    out.update({k: dev[k].cpu().numpy() for k in ('status', 'k_done', 'x_final', 'p_final')})
    for k, v in out.items():
        if v is not None:
            assert not (np.isnan(v).any() if v.dtype.kind == 'f' else (v == POISON_INT).any()), (k, 'not stored', case, name, method, lanes, want)
    assert not out['status'].any() and np.all(out['k_done'] == K), (case, name, method, lanes, want)
    return out


def _assert_replay(out, case, name, method, route, tag):
    inp = _inputs(case)[0]
    m, n = inp['m'], inp['n']
    refs = _replay_case(case, name, method)[3]
    for t, ref in enumerate(refs):
        checks = [('p_final', out['p_final'][t].reshape(m, n, n), ref['P_final'], 1e-10), ('x_final', out['x_final'][t], ref['X'][-1], 1e-10)]
        if out['x'] is not None:
            checks += [('x', out['x'][t], ref['X'], 1e-10), ('kappa', out['kappa'][t], ref['kappa'], 1e-9)]
        if out['dqcmd'] is not None:
            checks.append(('dqcmd', out['dqcmd'][t], ref['dq_cmd'], 1e-8))
        for key, a, b, tol in checks:
            d = cs.rel(a, b)
            _note(route, key, d)
            assert d <= tol, (key, d, t, case, name, method) + tuple(tag)


@pytest.mark.parametrize('name,method', REPLAY_SETS)
def test_replay_at_86_reads_reg_and_anneal_span(uvs, name, method):
    """(8,6), T = 35: the estimator-only kernels at lanes_per_filter 0 and 4, the same requests with the command wanted (the control
    wavefronts of replay_tuned_kernel), and the generic template at -1."""
    for lanes, want in ((0, ALONE), (4, ALONE), (0, FULL), (4, FULL), (-1, FULL)):
        out = _replay(uvs, 'dh86', name, method, lanes, want)
        _assert_replay(out, 'dh86', name, method, f'(8,6) replay {"with the command" if want == FULL else "estimator only"}{" generic" if lanes < 0 else ""}', (lanes, want))


@pytest.mark.parametrize('name,method', SQUARE_SETS[:3])
def test_replay_at_66_reads_reg_and_anneal_span(uvs, name, method):
    """replay_tuned_kernel<6, 6, ...> on the streams of the (6,6) DH closed loop (open loop: no trial is left out)."""
    for want in (FULL, ALONE):
        _assert_replay(_replay(uvs, 'dh66', name, method, 0, want), 'dh66', name, method, '(6,6) replay', (want,))


@pytest.mark.parametrize('name,method', [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF')])
def test_replay_at_32_7_reads_reg_and_anneal_span(uvs, name, method):
    for lanes in (8, 32):
        _assert_replay(_replay(uvs, 'wide', name, method, lanes, FULL), 'wide', name, method, f'(32,7) replay L{lanes}', (lanes,))


def _replay_f32(uvs, name, method, reg, span):
    """uvs_rmckf_replay_f32 on the float32-rounded (8,6) streams; per-trial relative error of its X stream against the fp64 block oracle run
    with (reg, span) on the fp64 streams."""
    import torch
    from oracle import rmckf_block
    inp, K, bw = _inputs('dh86')
    f, dq, x0, refs = _replay_case('dh86', name, method)
    T = len(x0)
    anneal, set_reg, set_span = ep.estimator(name, method)
    if (reg, span) != (set_reg, set_span):
        refs = [rmckf_block.run_replay(f[t], dq[t], x0[t], inp['desired'], cs.GAIN, method, bw, anneal, K, reg=reg, anneal_span=span) for t in range(T)]
    fp = uvs.engine.make_params(8, 6, method, bw, anneal, cs.DT, cs.DT * (K + 0.5), cs.GAIN, inp['desired'], False, 0, K)
    fp.reg, fp.anneal_span = reg, span
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')      # noqa: E731
    x = torch.full((K, 48, T), float('nan'), dtype=torch.float32, device='cuda')
    err = torch.full((K, 8, T), float('nan'), dtype=torch.float32, device='cuda')
    status, k_done = (torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda') for _ in range(2))
    f_dev, dq_dev, x0_dev = cu(f.transpose(1, 2, 0)), cu(dq.transpose(1, 2, 0)), cu(x0)
    view = uvs.engine.stream_view
    rc = uvs.lib().uvs_rmckf_replay_f32(C.byref(fp), T, view(f_dev), view(dq_dev),
                                        uvs._lib.View(x0_dev.data_ptr(), x0_dev.stride(0), 0, x0_dev.stride(1)), view(x), view(err),
                                        status.data_ptr(), k_done.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * T and k_done.cpu().tolist() == [K] * T
    X = x.cpu().numpy().astype(np.float64).transpose(2, 0, 1)
    assert not np.isnan(X).any() and not np.isnan(err.cpu().numpy()).any()
    return max(cs.rel(X[t], refs[t]['X']) for t in range(T))


@pytest.mark.parametrize('name', ['R25', 'A25'])
def test_fp32_replay_reads_reg_and_anneal_span(uvs, name):
    """The single-precision replay casts fp.reg to float: against the fp64 oracle at the set's values within the contract's 1e-5.  Printed next
    to the error of the same kernel and streams at the default values, the figure tests/test_gpu_replay_f32.py reports."""
    anneal, reg, span = ep.estimator(name, 'GMCKF')
    at_set, at_default = _replay_f32(uvs, name, 'GMCKF', reg, span), _replay_f32(uvs, name, 'GMCKF', REG, SPAN)
    NOTES.append(f'fp32 replay, streams of dh86 {name}: X rel err {at_set:.2e} at the set, {at_default:.2e} at the default reg and anneal_span')
    _note('(8,6) fp32 replay', 'x', at_set)
    assert at_set <= 1e-5 and at_default <= 1e-5, (at_set, at_default)


# ---------------------------------------------------------------------------------------------- d. single step
def _step_case(m, n, lanes, method, k0, scale, bw, anneal, reg, span, steps=4):
    """Inputs and oracle results of `steps` steps of a bank of T = 64 // L + 3 filters (two blocks, the second ragged) from k0, by the recipe
    of test_gpu_step._parity_run: every step starts from the oracle's state and command of the step before.  Per step a dict of the
    operands, the state going in, BlockFilter.step's results at (reg, span), and `teeth`: how far X would be at the default values."""
    import copy
    import zlib
    from oracle import rmckf_block
    rng = np.random.default_rng(zlib.crc32(repr((m, n, lanes, method, k0, scale, reg, span)).encode()))
    L = abs(lanes) or DEFAULT_LANES[(m, n)]
    T = 64 // L + 3
    gain = float(rng.uniform(0.05, 0.6))
    desired = 128 + 10 * rng.standard_normal(m)
    J = rng.standard_normal((T, m, n)) * 50
    x0 = J.reshape(T, m * n)
    fresh = lambda t: rmckf_block.BlockFilter(m, n, x0[t], method, bw, anneal, K_MAX, reg=reg, anneal_span=span)     # noqa: E731
    filt = [fresh(t) for t in range(T)]
    f_old, dq = 128 + 20 * rng.standard_normal((T, m)), np.zeros((T, n))
    out = []
    for s in range(steps):
        f = f_old + np.einsum('tmn,tn->tm', J, dq) * 0.05 + scale * rng.standard_t(2.0, size=(T, m))
        st = dict(k=k0 + s, f=f, f_old=f_old, dq=dq, X_in=np.stack([fl.X.ravel() for fl in filt]), P_in=np.stack([fl.P for fl in filt]),
                  X=np.zeros((T, m * n)), P=np.zeros((T, m, n, n)), cmd=np.zeros((T, n)), kappa=np.zeros((T, m)), finite=np.ones(T, bool), teeth=0.0)
        for t in range(T):
            twin = copy.deepcopy(filt[t])
            twin.reg, twin.anneal_span = REG, SPAN
            with np.errstate(all='ignore'):
                st['kappa'][t] = filt[t].step(f[t] - f_old[t], dq[t], st['k'])
                twin.step(f[t] - f_old[t], dq[t], st['k'])
            st['finite'][t] = np.all(np.isfinite(filt[t].X))
            if not st['finite'][t]:
                filt[t] = fresh(t)
                filt[t].first = False
                continue
            st['X'][t], st['P'][t] = filt[t].X.ravel(), filt[t].P
            st['cmd'][t] = rmckf_block.control_law(filt[t].X, f[t] - desired, st['kappa'][t], gain)
            st['teeth'] = max(st['teeth'], cs.rel(twin.X, filt[t].X))
        out.append(st)
        f_old, dq = f, np.clip(st['cmd'], -5, 5)
    return dict(T=T, gain=gain, desired=desired, x0=x0, steps=out)


def _assert_steps(uvs, m, n, lanes, method, case, bw, anneal, reg, span, route):
    import torch
    T = case['T']
    fp = uvs.engine.make_params(m, n, method, bw, anneal, 0.05, 15.0, case['gain'], case['desired'], False, lanes, 0)
    assert fp.k_max == K_MAX
    fp.reg, fp.anneal_span = reg, span
    bank = uvs.engine.FilterBank(fp, T, case['x0'])
    for s, st in enumerate(case['steps']):
        if s:
            bank.X.copy_(_cuda(st['X_in']))
            bank.P.copy_(_cuda(st['P_in']).reshape(bank.P.shape))
        for buf in (bank.dq, bank.err, bank.kappa):
            buf.fill_(float('nan'))
        bank.status.fill_(POISON_INT)
        cmd, err, kap, status = (o.cpu().numpy().copy() for o in bank.step(_cuda(st['f']), _cuda(st['f_old']), _cuda(st['dq']), st['k']))
        torch.cuda.synchronize()
        X, P = bank.X.cpu().numpy(), bank.P.cpu().numpy().reshape(T, m, n, n)
        assert _same_bits(err, st['f'] - case['desired']), (route, s)
        assert np.array_equal(status == 0, st['finite']) and set(status.tolist()) <= {0, 1}, (route, s, status.tolist())
        for t in np.flatnonzero(st['finite']):
            d = {'X': cs.rel(X[t], st['X'][t]), 'P': cs.rel(P[t], st['P'][t]), 'dq': cs.rel(cmd[t], st['cmd'][t]), 'kappa': cs.rel(kap[t], st['kappa'][t])}
            for key, tol in (('X', TOL_X), ('P', TOL_P), ('dq', TOL_DQ), ('kappa', TOL_KAPPA)):
                _note(route, key, d[key])
                assert d[key] <= tol, (key, d[key], route, m, n, lanes, method, s, int(t), reg, span)


@pytest.mark.parametrize('m,n,lanes', SHAPES)
def test_step_rmckf_reads_reg_and_anneal_span(uvs, m, n, lanes):
    """step_kernel on every instantiated (m, n, L) against BlockFilter.step and numpy's pinv, four steps each:
    R25 at k = 0; A25 from k = 30 of 300 (sigma = kernel_bw + 22.5); reg = 1e-12 at noise scale 400 and kernel_bw 1, where weights
    underflow to 0 and the kernel's d / (a d + 1) must agree with the reference's 1 / (a + 1 / d) at d = 1e-12; reg = 0 at noise scale 1 and
    kernel_bw 50, where -- asserted on the oracle first -- every weight is above 0 (with a zero weight the reference's inv(Cy) raises and
    nothing is specified).  The first three are also shown to be at least 100 gates (X: 1e-10) from their default-valued step."""
    runs = {'R25 at k = 0': (0, 1.0, 10.0, False, 0.25, SPAN), 'A25 at k = 30': (30, 1.0, 10.0, True, 0.25, 25.0),
            'reg = 1e-12, zero weights': (0, 400.0, 1.0, False, 1e-12, SPAN), 'reg = 0': (0, 1.0, 50.0, False, 0.0, SPAN)}
    for what, (k0, scale, bw, anneal, reg, span) in runs.items():
        case = _step_case(m, n, lanes, 'GMCKF', k0, scale, bw, anneal, reg, span)
        kappas = np.concatenate([st['kappa'][st['finite']].ravel() for st in case['steps'][1:]])
        if reg == 0.0:
            assert kappas.min() > 0.0, (what, kappas.min())
        else:
            assert max(st['teeth'] for st in case['steps']) >= 100 * TOL_X, (what, [st['teeth'] for st in case['steps']])
        if reg == 1e-12:
            assert (kappas == 0.0).any(), what
        _assert_steps(uvs, m, n, lanes, 'GMCKF', case, bw, anneal, reg, span, f'step, {what}')


@pytest.mark.parametrize('method', ['IMCCKF', 'MCKF'])
@pytest.mark.parametrize('m,n', list(DEFAULT_LANES))
def test_step_imcckf_and_mckf_read_anneal_span(uvs, m, n, method):
    """A400 from k = 30 (sigma = kernel_bw + 360) at the default lanes of each shape."""
    case = _step_case(m, n, 0, method, 30, 1.0, 10.0, True, REG, 400.0)
    assert max(st['teeth'] for st in case['steps']) >= 100 * TOL_X
    _assert_steps(uvs, m, n, 0, method, case, 10.0, True, REG, 400.0, f'step, A400 {method}')


# ---------------------------------------------------------------------------------------------- e. per-trial reg and fpi_threshold
def _grid(uvs, fp, plant, q0, noise, want, tp=None, x0=None):
    """engine.closed_loop (the grid entry point when tp is given) into NaN-filled buffers handed over as `reuse`; host arrays."""
    import torch
    from test_gpu_grid import _host
    T = q0.shape[0] if tp is None or tp.get('source') is None else tp['source'].shape[0]
    comps = {'x': fp.m * fp.n, 'err': fp.m, 'q': fp.n, 'f': fp.m, 'dq': fp.n}
    reuse = {k: _poisoned(T, fp.steps, comps[k], 'kct') for k in want}
    reuse.update(stats=torch.full((T, 3), float('nan'), dtype=torch.float64, device='cuda'),
                 status=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'), k_done=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'))
    out = uvs.engine.closed_loop(fp, plant, q0, noise, x0, want=want, reuse=reuse, trial_params=tp)
    torch.cuda.synchronize()
    got = _host(out, tuple(want))
    assert set(got['status'].tolist()) <= {0, 1} and got['k_done'].min() >= 0
    assert not np.isnan(got['stats'][got['status'] == 0]).any()
    logged = np.arange(fp.steps)[:, None] < got['k_done'][None, :]
    for key in want:
        assert not np.isnan(got[key][np.broadcast_to(logged[:, None, :], got[key].shape)]).any(), (key, 'not stored')
    return got


def _grid_against_uniform(uvs, method, cells, E=100, annealing=False, segments=0, span=SPAN, want=('x', 'err', 'q')):
    """One grid launch over `cells` (dicts of per-trial values, E trials each, inputs read through `source`) against one uniform launch per
    cell whose parameter block carries the cell's values: the same bits.  `span`: fp.anneal_span of every launch."""
    from test_gpu_grid import _assert_same_bits, _setup
    cfg, plan, q0, noise, plant, fp = _setup(uvs, method, E, annealing)
    H = len(cells)
    tp = {key: _cuda(np.repeat([float(c[key]) for c in cells], E)) for key in cells[0]}
    tp['source'] = _cuda((np.arange(H * E) % E).astype(np.int32))
    fp_grid = fp(2, segments=segments)
    fp_grid.anneal_span = span
    got = _grid(uvs, fp_grid, plant, q0, noise, want, tp)
    if segments:
        assert int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(fp_grid), C.byref(plant), H * E)) == segments
        assert uvs.engine.hand_over_fallbacks(fp_grid, plant, H * E) == 0
    refs = []
    for h, cell in enumerate(cells):
        one = fp(2, segments=segments)
        one.anneal_span = span
        for key, value in cell.items():
            setattr(one, key, value)
        refs.append(_grid(uvs, one, plant, q0, noise, want))
        _assert_same_bits(got, h * E, refs[-1], (method, annealing, segments, cell))
    return got, refs


REG_CELLS = [dict(reg=r, kernel_bw=b) for r in (1e-12, 1e-6, 1e-3, 0.25) for b in (5.0, 20.0)]


@pytest.mark.parametrize('annealing,segments,span', [(False, 0, SPAN), (True, 0, SPAN), (False, 4, SPAN), (True, 4, 25.0)])
def test_per_trial_reg_has_the_bits_of_uniform_launches(uvs, annealing, segments, span):
    """reg {1e-12, 1e-6, 1e-3, 0.25} x kernel_bw {5, 20}, 100 trials per cell (wavefronts of 32 trials mix cells), RMCKF: every cell has the bits
    of the uniform launch whose fp.reg carries its value -- without and with annealing, in four forced segments, each of which reads the
    per-trial values again, and in four segments annealed over fp.anneal_span = 25 (the per-trial kernels form sigma_k in bandwidth_of(), the
    uniform ones, which the oracles hold above, in bandwidth()).  The uniform launches differ from each other, so reading fp.reg for every
    trial could not pass."""
    got, refs = _grid_against_uniform(uvs, 'GMCKF', REG_CELLS, annealing=annealing, segments=segments, span=span)
    for a, b in ((0, 2), (2, 4), (4, 6), (1, 3)):                                           # neighbouring reg values at the same kernel_bw
        assert not np.array_equal(refs[a]['stats'], refs[b]['stats']), (REG_CELLS[a], REG_CELLS[b])


@pytest.mark.parametrize('method', ['KF', 'IMCCKF', 'MCKF'])
def test_per_trial_reg_is_ignored_by_the_other_estimators(uvs, method):
    """The launch with a per-trial reg array has the bits of the launch without it."""
    from test_gpu_grid import _assert_same_bits, _setup
    E, want = 100, ('x', 'err', 'q')
    cfg, plan, q0, noise, plant, fp = _setup(uvs, method, E)
    H = len(REG_CELLS)
    tp = dict(kernel_bw=_cuda(np.repeat([c['kernel_bw'] for c in REG_CELLS], E)), source=_cuda((np.arange(H * E) % E).astype(np.int32)))
    without = _grid(uvs, fp(2), plant, q0, noise, want, tp)
    with_reg = _grid(uvs, fp(2), plant, q0, noise, want, dict(tp, reg=_cuda(np.repeat([c['reg'] for c in REG_CELLS], E))))
    _assert_same_bits(with_reg, 0, without, method)


@pytest.mark.parametrize('method', ['IMCCKF', 'MCKF', 'KF'])
def test_per_trial_bandwidth_anneals_over_the_launch_wide_span(uvs, method):
    """kernel_bw {5, 20} per trial, annealing on, fp.anneal_span = 400: sigma_k = kernel_bw[t] + anneal_span (1 - k / k_max) in the per-trial
    flavour of every estimator's kernel (IMCC-KF reads its sigma_0 back from LDS) -- the bits of the uniform launches at that span, which
    are not those at the default span (KF: they are; it has no bandwidth)."""
    from test_gpu_grid import _setup
    cells = [dict(kernel_bw=5.0), dict(kernel_bw=20.0)]
    got, refs = _grid_against_uniform(uvs, method, cells, annealing=True, span=400.0)
    cfg, plan, q0, noise, plant, fp = _setup(uvs, method, 100, True)
    at_default = fp(2, kernel_bw=5.0)
    assert at_default.anneal_span == SPAN
    assert np.array_equal(_grid(uvs, at_default, plant, q0, noise, ('x', 'err', 'q'))['stats'], refs[0]['stats']) == (method == 'KF')


@pytest.mark.parametrize('segments', [0, 4])
def test_per_trial_fpi_threshold_has_the_bits_of_uniform_launches(uvs, segments):
    """fpi_threshold {0.1, 1e-2, 1e-4} per trial, MCKF, whole trials and four forced segments."""
    got, refs = _grid_against_uniform(uvs, 'MCKF', [dict(fpi_threshold=thr) for thr in (0.1, 1e-2, 1e-4)], segments=segments)
    assert not np.array_equal(refs[0]['stats'], refs[1]['stats']) and not np.array_equal(refs[1]['stats'], refs[2]['stats'])


@pytest.mark.parametrize('method', ['GMCKF', 'MCKF'])
def test_per_trial_reg_and_fpi_threshold_against_the_oracle(uvs, method):
    """Independent of the uniform kernels: RMCKF reg {1e-3, 0.25} x kernel_bw {5, 20}, MCKF fpi_threshold {0.1, 1e-4}, 32 trials per cell, against
    oracle/c called per cell with the cell's values.  The rule of test_grid_against_the_oracle: status and k_done exact and the statistics to
    STATS_TOL on every trial the oracle reproduces from a 1e-14-moved start; at least 95 % of the trials must be such (the oracle alone, on
    the host's noise: 124 of 128 for RMCKF, 64 of 64 for MCKF -- tests/test_oracle_c.py)."""
    from test_gpu_grid import _setup
    E, cells = ep.GRID_E, ep.GRID_CELLS[method]
    cfg, plan, q0, noise, plant, fp = _setup(uvs, method, E)
    H = len(cells)
    tp = {key: _cuda(np.repeat([float(c[key]) for c in cells], E)) for key in cells[0]}
    tp['source'] = _cuda((np.arange(H * E) % E).astype(np.int32))
    got = _grid(uvs, fp(0), plant, q0, noise, (), tp)
    host_noise = np.ascontiguousarray(noise.cpu().numpy().transpose(2, 0, 1))               # (E, K, m)
    calm_total = 0
    for h, cell in enumerate(cells):
        a, calm = ep.grid_oracle(cfg, plan.q_start, host_noise, cell)
        sl = slice(h * E, (h + 1) * E)
        dev = np.abs(got['stats'][sl] - a['stats']).max(axis=1) / np.abs(a['stats']).max(axis=1)
        print(f'{method} {cell}: calm {int(calm.sum())}/{E}, max deviation on calm trials {dev[calm].max() if calm.any() else 0.0:.3e}')
        assert np.array_equal(got['status'][sl][calm], a['status'][calm]) and np.array_equal(got['k_done'][sl][calm], a['k_done'][calm]), cell
        ok = calm & (a['status'] == 0)
        _note(f'per-trial values against oracle/c, {method}', 'stats', dev[ok].max())
        assert (dev[ok] <= STATS_TOL).all(), (cell, dev[ok].max())
        calm_total += int(calm.sum())
    assert calm_total >= ep.GRID_MIN_CALM * H * E, calm_total


def test_careful_pass_reads_the_per_trial_reg(uvs):
    """The Kahan fixture's start state (every trial marked at its first solve, so the careful pass computes everything) with three per-trial
    regs -- 1e-3, the fixture's 1e-6, 0.25: equal to three uniform launches bit for bit, status included, and those three differ from each
    other in bits.  The middle trial follows the fixture within the gates of test_careful_pass_reads_the_per_trial_values.  On this fixture
    the loop hardly moves (the commands of a rank-deficient estimate are small), so reg moves it little: oracle/c at reg = 1e-3 stays within
    1.0e-11 (err), 3.2e-12 (q) and 2.2e-8 (X) of the fixture, at 0.25 within 2.5e-9, 8.1e-10 and 5.4e-6 -- only X at 0.25 leaves the 1e-7
    gate, which is asserted; that the outer trials are not the middle one rests on the bits."""
    from conftest import load_golden, rel_err, scene_desired
    from test_gpu_grid import _assert_same_bits
    g = load_golden('rankdef_gmckf_kahan_c1000')
    meta, p = g['meta'], g['meta']['params']
    regs = (1e-3, REG, 0.25)
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    mk = lambda: uvs.engine.make_params(8, 6, meta['method'], p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], meta['gain'], g['desired'], False)   # noqa: E731
    T = 3
    q0, noise, x0 = _cuda(np.tile(g['q_start'], (T, 1))), _cuda(np.repeat(g['noise'][:, :, None], T, axis=2)), _cuda(np.tile(g['X'][0], (T, 1)))
    want = ('x', 'err', 'q', 'dq')
    launch_wide = mk()
    launch_wide.reg = 0.5                                                                   # no trial's value: must not be read
    got = _grid(uvs, launch_wide, plant, q0, noise, want, {'reg': _cuda(np.asarray(regs))}, x0)
    assert got['status'].tolist() == [0, 0, 0]
    refs = []
    for i, reg in enumerate(regs):
        fp = mk()
        fp.reg = reg
        refs.append(_grid(uvs, fp, plant, q0, noise, want, None, x0))
        sub = {k: (v[[i] * T] if k in ('stats', 'status', 'k_done') else v[:, :, [i] * T]) for k, v in got.items()}
        _assert_same_bits(sub, 0, refs[-1], reg)
    assert not np.array_equal(refs[0]['x'], refs[1]['x']) and not np.array_equal(refs[2]['x'], refs[1]['x'])
    K = len(g['t'])
    assert rel_err(got['err'][:, :, 1], g['err']) <= 1e-7 and rel_err(got['q'][:, :, 1], g['q']) <= 1e-7 and rel_err(got['x'][g['X_steps'], :, 1], g['X']) <= 1e-7
    assert rel_err(got['dq'][:K - 1, :, 1], g['dq_prev'][1:]) <= 1e-6
    for i in (0, 2):
        NOTES.append(f'careful pass, reg {regs[i]}: from the fixture err {rel_err(got["err"][:, :, i], g["err"]):.1e} q {rel_err(got["q"][:, :, i], g["q"]):.1e} '
                     f'X {rel_err(got["x"][g["X_steps"], :, i], g["X"]):.1e}')
    assert rel_err(got['x'][g['X_steps'], :, 2], g['X']) > 1e-7
