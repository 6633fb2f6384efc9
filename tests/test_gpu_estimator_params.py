"""uvs_filter_params.reg and .anneal_span, launch-wide, and uvs_trial_params.reg / .fpi_threshold, per trial, on every route that reads
them.  engine.make_params writes reg = 1e-6 and anneal_span = 100 into every block the rest of the suite builds, so a kernel that used
the literals instead of the fields would pass everything else; here the fields are set on the struct after make_params and the kernels
are held to CPU references computed with the same values (tests/estimator_params_common.py: oracle/c and oracle/rmckf_block, held to
each other -- and shown to be far from their default-valued runs -- by tests/test_oracle_c.py).

Every output buffer is filled with NaN (-7 for the integers) before the launch.  Gates are the routes' own: closed loop 1e-8 on err, q, X
and the statistics with status and k_done exact (gpu_harness.TOL); single step X 1e-10, P 1e-9, command 1e-7, kappa 1e-9
(gpu_harness.STEP_GATES); replay X 1e-10, command 1e-8, kappa 1e-9, final P 1e-10 (test_replay_other_shapes_match_block_oracle); fp32 replay 1e-5.
The worst deviation per route is printed when the module finishes (pytest -s)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import closed_shapes_common as cs
import estimator_params_common as ep
import gpu_harness as gh
from gpu_harness import BLOCK_TRIALS, DEFAULT_LANES, K_MAX, LATENCY, POISON_INT, SHAPES, STRICT, TOL_MODES, TOL_X
from sweep_common import STATS_TOL

pytestmark = pytest.mark.gpu

REG, SPAN = ep.REG, ep.ANNEAL_SPAN
WORST = gh.Worst()                                           # route -> quantity -> worst relative deviation from the references so far
NOTES = []
CLOSED_SETS = [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF'), ('A25', 'MCKF')]
SQUARE_SETS = [('R3', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF'), ('A25', 'MCKF')]     # (6,6) on the DH plant: R3 in place of R25


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    WORST.report('estimator params')
    print('estimator params: trials left out of the gates (the CPU oracles disagree there):', {k: list(v) for k, v in ep.EXCLUDED.items()})
    for note in NOTES:
        print('estimator params:', note)


# ---------------------------------------------------------------------------------------------- closed-loop launches and their references
def _closed(uvs, case, method, anneal, reg, span, lanes=0, reserved=0):
    """gh.launch with the arguments in the order of ep.estimator's result."""
    return gh.launch(uvs, case, method, anneal, lanes, reserved, reg=reg, anneal_span=span)


def _launch_set(uvs, case, name, method, lanes=0, reserved=0):
    return _closed(uvs, case, method, *ep.estimator(name, method), lanes, reserved)


def _hold(out, case, name, method, route, tag=()):
    """The launch against the two oracles run at parameter set `name` (every estimator of the set's; KF: any set, it reads neither field):
    status and k_done on every trial; err, q, X and the statistics on the kept trials against oracle/c, and on those of BLOCK_TRIALS (every
    trial of 'wide') against oracle/rmckf_block."""
    tag = (case, name, method, route) + tuple(tag)
    kept, run = cs.kept_trials((case, name, method), ep.EXCLUDED), ep.run(name, method)
    gh.assert_matches_c(out, cs.c_reference(case, **run), kept, WORST, route, tag, strict=True)
    gh.assert_matches_block(out, lambda t: cs.block_reference(case, t=t, **run), kept if case == 'wide' else [t for t in BLOCK_TRIALS if t in kept],
                            WORST, route, tag, strict=True)
    gh.assert_twins(out, tag, cs.inputs(case)['twins'])


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
        gh.assert_same_launch(_launch_set(uvs, 'dh86', name, method, 2), out, (name, method, 'small batch = two lanes'))


@pytest.mark.parametrize('name', ['R25', 'A25'])
def test_dh86_rmckf_under_strict_pinv(uvs, name):
    """UVS_OPT_STRICT_PINV at two lanes: the certifying instantiation of the tuned kernel.  Inside the oracle gates and within 1e-9 of the
    default mode."""
    fast, strict = _launch_set(uvs, 'dh86', name, 'GMCKF', 2), _launch_set(uvs, 'dh86', name, 'GMCKF', 2, STRICT)
    assert strict['lanes'] == 2 and strict['segments'] == 1
    _hold(strict, 'dh86', name, 'GMCKF', '(8,6) DH strict pinv')
    for key in ('err', 'q'):
        assert cs.rel(gh.live(strict, key), gh.live(fast, key)) <= TOL_MODES, (key, name)
    NOTES.append(f'strict pinv, dh86 {name}: the bits of the default mode: {gh.same_bits(gh.live(strict, "x"), gh.live(fast, "x"))}')


@pytest.mark.parametrize('name', ['A25', 'A400'])
def test_dh86_mckf_in_four_segments(uvs, name):
    """fp.reserved = 4 << 8: the two-lane MCKF kernel runs every trial as four work items whose state crosses through the workspace and
    every one of which forms its own bandwidths.  The bits of whole trials, no work item fell back, inside the oracle gates."""
    whole = _launch_set(uvs, 'dh86', name, 'MCKF', 2)
    assert whole['segments'] == 1 and whole['workspace'] == 0 and whole['fallbacks'] is None
    for lanes in (0, 2):
        cut = _launch_set(uvs, 'dh86', name, 'MCKF', lanes, 4 << 8)
        assert cut['lanes'] == 2 and cut['segments'] == 4 and cut['workspace'] > 0 and cut['fallbacks'] == 0
        gh.assert_same_launch(whole, cut, (name, lanes, 'segments'))
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
        gh.assert_same_launch(_launch_set(uvs, 'wide', name, method, 0), out, (name, method, '0 = 8'))


# ---------------------------------------------------------------------------------------------- b. what must not depend on them
INDEPENDENCE_ROUTES = [('dh86', 2), ('dh86', -2), ('wide', 0)]      # a tuned kernel, a generic template, the wide kernel


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_kf_reads_neither_field_nor_the_annealing_flag(uvs, case, lanes):
    """KF has no correntropy weight: identical bits for (reg, anneal_span, annealing) = (default, default, off), (0.25, 25, on) and
    (1e-3, 400, on), and inside the gates of the KF oracle."""
    base = _closed(uvs, case, 'KF', False, REG, SPAN, lanes)
    _hold(base, case, 'R25', 'KF', f'KF, {case} lanes {lanes}')                              # estimator('R25', 'KF'): annealing off, the defaults
    for anneal, reg, span in ((True, 0.25, 25.0), (True, 1e-3, 400.0)):
        gh.assert_same_launch(base, _closed(uvs, case, 'KF', anneal, reg, span, lanes), (case, lanes, anneal, reg, span))


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_imcckf_and_mckf_do_not_read_reg(uvs, case, lanes):
    """Only RMCKF regularises its weights (experiment.py:280): IMCC-KF and MCKF (not on the wide kernel) give identical bits for
    reg = default and reg = 0.25, with annealing over a span of 25 and without."""
    for method in ('IMCCKF',) if case == 'wide' else ('IMCCKF', 'MCKF'):
        for anneal, span in ((True, 25.0), (False, SPAN)):
            a, b = _closed(uvs, case, method, anneal, REG, span, lanes), _closed(uvs, case, method, anneal, 0.25, span, lanes)
            gh.assert_same_launch(a, b, (case, lanes, method, anneal))
        _hold(_closed(uvs, case, method, True, 0.25, 25.0, lanes), case, 'A25', method, f'{method} with reg = 0.25, {case} lanes {lanes}')


@pytest.mark.parametrize('case,lanes', INDEPENDENCE_ROUTES)
def test_annealing_over_a_zero_span_is_no_annealing(uvs, case, lanes):
    """annealing = 1 with anneal_span = 0: sigma_k = kernel_bw at every step, so the launch passes the oracle gates of annealing off (RMCKF at
    reg = 0.25: set R25; IMCC-KF).  Whether the bits are those of annealing off too is printed, not asserted."""
    for method, reg in (('GMCKF', 0.25), ('IMCCKF', REG)):
        on = _closed(uvs, case, method, True, reg, 0.0, lanes)
        _hold(on, case, 'R25', method, f'anneal_span = 0, {case} lanes {lanes}')
        off = _closed(uvs, case, method, False, reg, SPAN, lanes)
        NOTES.append(f'anneal_span = 0 against annealing off, {case} lanes {lanes} {method}: same bits: {gh.same_bits(gh.live(on, "x"), gh.live(off, "x"))}')


# ---------------------------------------------------------------------------------------------- c. replay
REPLAY_T = 35                                                # (8,6) at four lanes per filter: two wavefronts and three trials
REPLAY_SETS = [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF')]
FULL, ALONE = ('x', 'err', 'kappa', 'dqcmd'), ('x', 'err', 'kappa')


@functools.lru_cache(maxsize=None)
def _replay_case(case, name, method):
    """Streams recorded from the block oracle's closed loop at the set: f (T, K + 1, m) with row 0 the first f_old, dq (T, K, n) the regressor
    of every step (the command before it: the difference quotient of q), x0, desired -- and rmckf_block.run_replay on them, at the set."""
    from oracle import rmckf_block
    inp = cs.inputs(case)
    T, K, m, n = min(REPLAY_T, inp['T']), inp['K'], inp['m'], inp['n']
    anneal, reg, span = ep.estimator(name, method)
    f, dq = np.zeros((T, K + 1, m)), np.zeros((T, K, n))
    for t in range(T):
        run = cs.block_reference(case, t=t, **ep.run(name, method))
        assert run['status'] == 0 and run['k_done'] == K
        f[t, 0] = inp['features'](inp['q0'][t]) if inp['guess'] else 0.0
        f[t, 1:] = run['err'] + inp['desired']
        dq[t, 1:] = np.diff(run['q'], axis=0) / cs.DT
    x0 = np.array(inp['x0'][:T])
    refs = [rmckf_block.run_replay(f[t], dq[t], x0[t], inp['desired'], cs.GAIN, method, inp['bw'], anneal, K, cs.FPI_THRESHOLD, reg=reg, anneal_span=span)
            for t in range(T)]
    return f, dq, x0, refs


def _hold_replay(uvs, case, name, method, lanes, want, route):
    """uvs_rmckf_replay_f64 on the streams of _replay_case with fp.reg / fp.anneal_span of the set, into NaN-filled buffers, against the
    block oracle's replay of them."""
    f, dq, x0, refs = _replay_case(case, name, method)
    anneal, reg, span = ep.estimator(name, method)
    fp = gh.params(uvs, case, method, anneal, lanes, guess=False)
    fp.reg, fp.anneal_span = reg, span
    out = gh.replay(uvs, fp, f, dq, x0, want)
    assert not out['status'].any() and np.all(out['k_done'] == fp.steps), (case, name, method, lanes, want)
    gh.assert_replay(out, refs, WORST, route, (case, name, method, lanes, want))


@pytest.mark.parametrize('name,method', REPLAY_SETS)
def test_replay_at_86_reads_reg_and_anneal_span(uvs, name, method):
    """(8,6), T = 35: the estimator-only kernels at lanes_per_filter 0 and 4, the same requests with the command wanted (the control
    wavefronts of replay_tuned_kernel), and the generic template at -1."""
    for lanes, want in ((0, ALONE), (4, ALONE), (0, FULL), (4, FULL), (-1, FULL)):
        _hold_replay(uvs, 'dh86', name, method, lanes, want, f'(8,6) replay {"with the command" if want == FULL else "estimator only"}{" generic" if lanes < 0 else ""}')


@pytest.mark.parametrize('name,method', SQUARE_SETS[:3])
def test_replay_at_66_reads_reg_and_anneal_span(uvs, name, method):
    """replay_tuned_kernel<6, 6, ...> on the streams of the (6,6) DH closed loop (open loop: no trial is left out)."""
    for want in (FULL, ALONE):
        _hold_replay(uvs, 'dh66', name, method, 0, want, '(6,6) replay')


@pytest.mark.parametrize('name,method', [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A400', 'IMCCKF')])
def test_replay_at_32_7_reads_reg_and_anneal_span(uvs, name, method):
    for lanes in (8, 32):
        _hold_replay(uvs, 'wide', name, method, lanes, FULL, f'(32,7) replay L{lanes}')


def _replay_f32(uvs, name, method, reg, span):
    """uvs_rmckf_replay_f32 on the float32-rounded (8,6) streams; per-trial relative error of its X stream against the fp64 block oracle run
    with (reg, span) on the fp64 streams."""
    import torch
    from oracle import rmckf_block
    inp = cs.inputs('dh86')
    K, bw = inp['K'], inp['bw']
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
    WORST.note('(8,6) fp32 replay', 'x', at_set)
    assert at_set <= 1e-5 and at_default <= 1e-5, (at_set, at_default)


# ---------------------------------------------------------------------------------------------- d. single step
def _step_case(m, n, lanes, method, k0, scale, bw, anneal, reg, span):
    """Four steps of gh.step_recipe at (reg, span) from k0: dict(T, gain, desired, x0, steps: per step the operands, the state going in,
    BlockFilter.step's results, and `teeth`: how far X would be at the default values)."""
    rng = np.random.default_rng(zlib.crc32(repr((m, n, lanes, method, k0, scale, reg, span)).encode()))
    head, *steps = gh.step_recipe(rng, m, n, lanes, method, k0, scale, bw, anneal, 4, default_twin=True, reg=reg, anneal_span=span)
    return dict(head, steps=steps)


def _assert_steps(uvs, m, n, lanes, method, case, bw, anneal, reg, span, route):
    fp = uvs.engine.make_params(m, n, method, bw, anneal, 0.05, 15.0, case['gain'], case['desired'], False, lanes, 0)
    assert fp.k_max == K_MAX
    fp.reg, fp.anneal_span = reg, span
    bank = uvs.engine.FilterBank(fp, case['T'], case['x0'])
    for s, st in enumerate(case['steps']):
        gh.assert_step(bank, st, case['desired'], WORST, (route,), (route, m, n, lanes, method, reg, span), fresh=s == 0)


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
    T = q0.shape[0] if tp is None or tp.get('source') is None else tp['source'].shape[0]
    comps = {'x': fp.m * fp.n, 'err': fp.m, 'q': fp.n, 'f': fp.m, 'dq': fp.n}
    reuse = {k: gh.poisoned(T, fp.steps, comps[k], 'kct') for k in want}
    reuse.update(gh.poisoned_trials(T))
    out = uvs.engine.closed_loop(fp, plant, q0, noise, x0, want=want, reuse=reuse, trial_params=tp)
    torch.cuda.synchronize()
    got = gh.host(out, tuple(want))
    assert set(got['status'].tolist()) <= {0, 1} and got['k_done'].min() >= 0
    assert not np.isnan(got['stats'][got['status'] == 0]).any()
    logged = np.arange(fp.steps)[:, None] < got['k_done'][None, :]
    for key in want:
        assert not np.isnan(got[key][np.broadcast_to(logged[:, None, :], got[key].shape)]).any(), (key, 'not stored')
    return got


def _grid_against_uniform(uvs, method, cells, E=100, annealing=False, segments=0, span=SPAN, want=('x', 'err', 'q')):
    """One grid launch over `cells` (dicts of per-trial values, E trials each, inputs read through `source`) against one uniform launch per
    cell whose parameter block carries the cell's values: the same bits.  `span`: fp.anneal_span of every launch."""
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E, annealing)
    H = len(cells)
    tp = {key: gh.cuda(np.repeat([float(c[key]) for c in cells], E)) for key in cells[0]}
    tp['source'] = gh.cuda((np.arange(H * E) % E).astype(np.int32))
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
        gh.assert_same_bits(got, h * E, refs[-1], (method, annealing, segments, cell))
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
    E, want = 100, ('x', 'err', 'q')
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    H = len(REG_CELLS)
    tp = dict(kernel_bw=gh.cuda(np.repeat([c['kernel_bw'] for c in REG_CELLS], E)), source=gh.cuda((np.arange(H * E) % E).astype(np.int32)))
    without = _grid(uvs, fp(2), plant, q0, noise, want, tp)
    with_reg = _grid(uvs, fp(2), plant, q0, noise, want, dict(tp, reg=gh.cuda(np.repeat([c['reg'] for c in REG_CELLS], E))))
    gh.assert_same_bits(with_reg, 0, without, method)


@pytest.mark.parametrize('method', ['IMCCKF', 'MCKF', 'KF'])
def test_per_trial_bandwidth_anneals_over_the_launch_wide_span(uvs, method):
    """kernel_bw {5, 20} per trial, annealing on, fp.anneal_span = 400: sigma_k = kernel_bw[t] + anneal_span (1 - k / k_max) in the per-trial
    flavour of every estimator's kernel (IMCC-KF reads its sigma_0 back from LDS) -- the bits of the uniform launches at that span, which
    are not those at the default span (KF: they are; it has no bandwidth)."""
    cells = [dict(kernel_bw=5.0), dict(kernel_bw=20.0)]
    got, refs = _grid_against_uniform(uvs, method, cells, annealing=True, span=400.0)
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, 100, True)
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
    E, cells = ep.GRID_E, ep.GRID_CELLS[method]
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    H = len(cells)
    tp = {key: gh.cuda(np.repeat([float(c[key]) for c in cells], E)) for key in cells[0]}
    tp['source'] = gh.cuda((np.arange(H * E) % E).astype(np.int32))
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
        WORST.note(f'per-trial values against oracle/c, {method}', 'stats', dev[ok].max())
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
    g = load_golden('rankdef_gmckf_kahan_c1000')
    meta, p = g['meta'], g['meta']['params']
    regs = (1e-3, REG, 0.25)
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    mk = lambda: uvs.engine.make_params(8, 6, meta['method'], p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], meta['gain'], g['desired'], False)   # noqa: E731
    T = 3
    q0, noise, x0 = gh.cuda(np.tile(g['q_start'], (T, 1))), gh.cuda(np.repeat(g['noise'][:, :, None], T, axis=2)), gh.cuda(np.tile(g['X'][0], (T, 1)))
    want = ('x', 'err', 'q', 'dq')
    launch_wide = mk()
    launch_wide.reg = 0.5                                                                   # no trial's value: must not be read
    got = _grid(uvs, launch_wide, plant, q0, noise, want, {'reg': gh.cuda(np.asarray(regs))}, x0)
    assert got['status'].tolist() == [0, 0, 0]
    refs = []
    for i, reg in enumerate(regs):
        fp = mk()
        fp.reg = reg
        refs.append(_grid(uvs, fp, plant, q0, noise, want, None, x0))
        sub = {k: (v[[i] * T] if k in ('stats', 'status', 'k_done') else v[:, :, [i] * T]) for k, v in got.items()}
        gh.assert_same_bits(sub, 0, refs[-1], reg)
    assert not np.array_equal(refs[0]['x'], refs[1]['x']) and not np.array_equal(refs[2]['x'], refs[1]['x'])
    K = len(g['t'])
    assert rel_err(got['err'][:, :, 1], g['err']) <= 1e-7 and rel_err(got['q'][:, :, 1], g['q']) <= 1e-7 and rel_err(got['x'][g['X_steps'], :, 1], g['X']) <= 1e-7
    assert rel_err(got['dq'][:K - 1, :, 1], g['dq_prev'][1:]) <= 1e-6
    for i in (0, 2):
        NOTES.append(f'careful pass, reg {regs[i]}: from the fixture err {rel_err(got["err"][:, :, i], g["err"]):.1e} q {rel_err(got["q"][:, :, i], g["q"]):.1e} '
                     f'X {rel_err(got["x"][g["X_steps"], :, i], g["X"]):.1e}')
    assert rel_err(got['x'][g['X_steps'], :, 2], g['X']) > 1e-7
