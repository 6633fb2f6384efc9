"""The closed-loop route (uvs_rmckf_closed_loop_ws_f64) and the tuned replay at the shapes no GPU test launched before: (6,6) and (2,6) on
the DH / pinhole plant, (8,6) and (6,6) on the linear plant -- every estimator, every lane mapping the plan can pick there (the tuned
two-lane kernels and their four- / one-lane relatives on the linear plant, the generic templates, the careful pass alone under
UVS_OPT_STRICT_PINV), MCKF with a fixed-point loop that iterates.

Inputs and references: tests/closed_shapes_common.py, launches and comparisons: tests/gpu_harness.py (T = 70, K = 60; oracle/c on every trial, oracle/rmckf_block -- numpy pinv -- on a
sample; tests/test_oracle_c.py holds the two to 1e-11 of each other and lists the few (6,6) trials that miss it, which are left out here).
Gates (test_gpu_fuzz.py, test_closed_loop_stress_plant): status and k_done exact on every trial; err, q, x and stats <= 1e-8 relative,
per trial.  Every batch carries one trial three times -- in the first, a middle and the last wavefront -- and its three copies must come
back with identical bits: lane- or wavefront-dependent indexing that a tolerance would hide."""
import numpy as np
import pytest

import closed_shapes_common as cs
import gpu_harness as gh
from gpu_harness import BLOCK_TRIALS, LATENCY, STRICT, TOL, TOL_MODES

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SHAPE = -1, -2
LEFT_OUT = {}                                                # (case, method, annealing, trial, family) -> err deviations on a trial the gates leave out
WORST = gh.Worst()                                           # family -> stream -> worst relative deviation from the oracles so far


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    WORST.report('closed shapes')
    print('closed shapes: trials left out of the gates (the CPU oracles disagree there):', {k: list(v) for k, v in cs.EXCLUDED.items()})
    for key, devs in LEFT_OUT.items():
        print('closed shapes: left out', key, {k: f'{v:.1e}' for k, v in devs.items()})


def _matches_c(out, case, method, anneal, family):
    """status and k_done on every trial, the streams the launch wrote and the statistics on the kept ones, against oracle/c."""
    key = (case, method, anneal)
    gh.assert_matches_c(out, cs.c_reference(*key), cs.kept_trials(key), WORST, family, key)


def _matches_block(out, case, method, anneal, family, trials=BLOCK_TRIALS):
    """The same against oracle/rmckf_block (numpy pinv) on a few kept trials; f too where the launch wrote it."""
    key = (case, method, anneal)
    trials = [t for t in trials if t < len(out['status']) and t in cs.kept_trials(key)]
    gh.assert_matches_block(out, lambda t: cs.block_reference(*key, t), trials, WORST, family, key)


def _report_left_out(out, case, method, anneal, family):
    """The trials the gates leave out (the two CPU oracles disagree there): status and k_done are held as everywhere; how far the kernel's err
    stream is from either oracle goes into the printed summary, next to how far the oracles are from each other."""
    ref = cs.c_reference(case, method, anneal)
    for t in cs.EXCLUDED.get((case, method, anneal), ()):
        blk = cs.block_reference(case, method, anneal, t)
        k = blk['k_done']
        LEFT_OUT[(case, method, anneal, t, family)] = {'kernel - oracle/c': cs.rel(out['err'][t, :k], ref['err'][t, :k]), 'kernel - numpy': cs.rel(out['err'][t, :k], blk['err']),
                                                       'oracle/c - numpy': cs.rel(ref['err'][t, :k], blk['err'])}


ESTIMATORS = [(method, anneal) for method in cs.METHODS for anneal in (False, True)]


# ---------------------------------------------------------------------------------------------- a. (6,6) on the DH plant
@pytest.mark.parametrize('method,anneal', ESTIMATORS)
@pytest.mark.parametrize('case', ['dh66', 'dh66_x0'])
def test_dh66_every_lane_mapping_matches_the_oracles(uvs, case, method, anneal):
    """Three image points, analytic initial guess (dh66) and a supplied X0 (dh66_x0).  lanes_per_filter 0 and 2: closed_loop_tuned_kernel<6, 6, 2>
    (three rows per lane, one block in registers and two in LDS, MCKF as whole trials); 1 and -1: the generic (6,6,1) template; -2: the generic
    (6,6,2) one.  0 and 2 are one kernel, 1 and -1 likewise: the same bits."""
    outs = {}
    for lanes in (0, 2, 1, -1, -2):
        family = f'(6,6) DH {"tuned" if lanes in (0, 2) else "generic L" + str(abs(lanes))}'
        out = outs[lanes] = gh.launch(uvs, case, method, anneal, lanes)
        assert out['lanes'] == (abs(lanes) or 2) and out['segments'] == 1
        _matches_c(out, case, method, anneal, family)
        gh.assert_twins(out, (case, method, anneal, lanes))
        if lanes in (0, -1, -2):
            _report_left_out(out, case, method, anneal, family)
    _matches_block(outs[0], case, method, anneal, '(6,6) DH tuned')
    _matches_block(outs[-1], case, method, anneal, '(6,6) DH generic L1')
    _matches_block(outs[-2], case, method, anneal, '(6,6) DH generic L2')
    gh.assert_same_launch(outs[0], outs[2], (case, method, anneal, '0 = 2'))
    gh.assert_same_launch(outs[1], outs[-1], (case, method, anneal, '1 = -1'))


@pytest.mark.parametrize('method', cs.METHODS)
def test_dh66_batches_of_1_and_33_are_slices_of_the_batch_of_70(uvs, method):
    """T = 1 (one filter in the only wavefront) and T = 33 (at two lanes one full wavefront plus one trial), once per kernel family: the tuned
    kernel, the two generic templates and the careful pass alone.  A trial does not depend on its batch: the bits of the first T trials of the
    T = 70 launch (which the oracles hold)."""
    for lanes, reserved in ((0, 0), (-1, 0), (-2, 0), (0, STRICT)):
        whole = gh.launch(uvs, 'dh66', method, True, lanes, reserved)
        for T in (1, 33):
            part = gh.launch(uvs, 'dh66', method, True, lanes, reserved, T=T)
            assert not np.isnan(part['stats']).any()
            gh.assert_same_launch(whole, part, (method, lanes, reserved, T))
            _matches_c(part, 'dh66', method, True, f'(6,6) DH T = {T}')


@pytest.mark.parametrize('method', cs.METHODS)
def test_dh66_without_the_x_stream(uvs, method):
    """want without 'x': the XOUT = false instantiations.  err, q and the statistics inside the gates, and the bits of the launch that logs X."""
    for lanes in (0, -2):
        out = gh.launch(uvs, 'dh66', method, True, lanes, want=('err', 'q'))
        assert out['x'] is None
        _matches_c(out, 'dh66', method, True, '(6,6) DH no X stream')
        gh.assert_twins(out, (method, lanes))
        gh.assert_same_launch(gh.launch(uvs, 'dh66', method, True, lanes), out, (method, lanes, 'XOUT'))


@pytest.mark.parametrize('method', cs.METHODS)
@pytest.mark.parametrize('lanes', [0, -2])
def test_dh66_all_five_streams_and_the_final_state(uvs, method, lanes):
    """f = plant + noise (the numpy oracle's), dq = the finite difference of q, x_final = the last X row bit for bit, p_final symmetric and the
    numpy oracle's P (1e-10, the gate of test_replay_other_shapes_match_block_oracle)."""
    case, anneal = 'dh66', True
    inp = cs.inputs(case)
    out = gh.launch(uvs, case, method, anneal, lanes, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
    family = '(6,6) DH five streams'
    _matches_c(out, case, method, anneal, family)
    gh.assert_twins(out, (method, lanes))
    gh.assert_same_launch(gh.launch(uvs, case, method, anneal, lanes), out, (method, lanes, 'three streams = five'), keys=('x', 'err', 'q', 'stats', 'status', 'k_done'))
    trials = cs.sampled(case)[::7]
    _matches_block(out, case, method, anneal, family, trials)
    assert not out['status'].any()
    assert gh.same_bits(out['f'] - inp['desired'], out['err'])                               # one subtraction
    # q[k + 1] = q[k] + dq[k] dt: the difference quotient returns dq[k] up to the cancellation, 2 eps max|q| / dt = 2e-14 absolute
    quotient = (out['q'][:, 1:] - out['q'][:, :-1]) / cs.DT
    d = float((gh.per_trial_rel(out['dq'][:, :-1], quotient)).max())
    WORST.note(family, 'dq (difference of q)', d)
    assert d <= TOL and np.abs(out['dq']).max() > 1e-3
    assert gh.same_bits(out['x_final'], out['x'][:, -1])
    P = out['p_final'].reshape(cs.T, inp['m'], inp['n'], inp['n'])
    assert np.abs(P - P.transpose(0, 1, 3, 2)).max() <= 1e-14 * np.abs(P).max()
    for t in trials:
        d = cs.rel(P[t], cs.block_reference(case, method, anneal, t)['P_final'])
        WORST.note(family, 'p_final (numpy)', d)
        assert d <= 1e-10, (d, t)


@pytest.mark.parametrize('method', cs.METHODS)
def test_dh66_record_layouts_give_the_same_bits(uvs, method):
    """Streams as [step][trial][component] (noise too) and X as per-trial records: other strides, the same bits as the trial-fastest default."""
    for lanes in (0, -1):
        ref = gh.launch(uvs, 'dh66', method, True, lanes)
        gh.assert_same_launch(ref, gh.launch(uvs, 'dh66', method, True, lanes, layout='ktc'), (method, lanes, 'ktc'))
        gh.assert_same_launch(ref, gh.launch(uvs, 'dh66', method, True, lanes, x_layout='tkc'), (method, lanes, 'x tkc'))


@pytest.mark.parametrize('anneal', [False, True])
def test_dh66_mckf_in_four_segments_is_bit_identical_to_whole_trials(uvs, anneal):
    """fp.reserved = 4 << 8 with K = 60 >= 32: the two-lane MCKF kernel runs every trial as four work items whose state crosses through the
    workspace.  The same bits as whole trials, and no work item fell back to recomputing its trial."""
    for case in ('dh66', 'dh66_x0'):
        whole = gh.launch(uvs, case, 'MCKF', anneal, 0, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
        assert whole['segments'] == 1 and whole['workspace'] == 0 and whole['fallbacks'] is None
        for lanes in (0, 2):
            cut = gh.launch(uvs, case, 'MCKF', anneal, lanes, reserved=4 << 8, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
            assert cut['segments'] == 4 and cut['workspace'] > 0 and cut['fallbacks'] == 0
            ok = np.flatnonzero(whole['status'] == 0)
            gh.assert_same_launch(whole, cut, (case, anneal, lanes, 'segments'), keys=('x', 'err', 'q', 'f', 'dq', 'status', 'k_done'))
            gh.assert_same_launch(whole, cut, (case, anneal, lanes, 'segments, final'), keys=('stats', 'x_final', 'p_final'), trials=ok)
            _matches_c(cut, case, 'MCKF', anneal, '(6,6) DH MCKF in 4 segments')
        for T in (1, 33):                                                                   # one chunk; one full chunk and one of a single trial
            part = gh.launch(uvs, case, 'MCKF', anneal, 0, reserved=4 << 8, T=T)
            assert part['segments'] == 4 and part['fallbacks'] == 0
            gh.assert_same_launch(gh.launch(uvs, case, 'MCKF', anneal, 0), part, (case, anneal, T, 'segments, slice'))


def _assert_strict(uvs, case, method, anneal, family, lanes=0):
    """UVS_OPT_STRICT_PINV at `lanes` (RMCKF on a tuned kernel: certified first pass; otherwise the careful kernel alone): inside the oracle
    gates, within 1e-9 of the default mode on the kept trials, and -- where the careful kernel is the only pass -- the bits of the same
    request through the generic lane mapping, which plans the same careful kernel."""
    fast, strict = gh.launch(uvs, case, method, anneal, lanes), gh.launch(uvs, case, method, anneal, lanes, STRICT)
    assert strict['lanes'] == fast['lanes'] and strict['segments'] == 1
    _matches_c(strict, case, method, anneal, family)
    _matches_block(strict, case, method, anneal, family)
    gh.assert_twins(strict, (case, method, anneal, 'strict'))
    assert np.array_equal(strict['status'], fast['status']) and np.array_equal(strict['k_done'], fast['k_done'])
    kept = cs.kept_trials((case, method, anneal))
    for key in ('err', 'q'):
        assert cs.rel(gh.live(strict, key)[kept], gh.live(fast, key)[kept]) <= TOL_MODES, (key, case, method, anneal)
    m, n = cs.inputs(case)['m'], cs.inputs(case)['n']
    generic = -max(abs(lanes), {(6, 6): 2, (2, 6): 1, (8, 6): 2}[(m, n)])
    careful = gh.launch(uvs, case, method, anneal, generic, STRICT)
    if method == 'GMCKF' and (m, n) != (2, 6):
        # The certified first pass is the default mode's arithmetic plus a certificate: on trials it does not mark it writes the default
        # mode's bits (test_strict_pinv_audit_at_full_size), which the careful kernel alone -- another solve -- does not.  So equal bits on the
        # kept trials say that the plan did take the certified tuned pass and not kCarefulOnly.
        gh.assert_same_launch(fast, strict, (case, method, anneal, lanes, 'certified pass = default bits'), trials=kept)
        assert not gh.same_bits(gh.live(careful, 'x')[kept], gh.live(strict, 'x')[kept]), (case, anneal, lanes, 'the careful pass alone would have other bits')
        for key in ('err', 'q'):
            assert cs.rel(gh.live(strict, key)[kept], gh.live(careful, key)[kept]) <= TOL_MODES, (key, case, method, anneal)
    else:
        gh.assert_same_launch(careful, strict, (case, method, anneal, 'careful alone'))


@pytest.mark.parametrize('method,anneal', ESTIMATORS)
def test_dh66_strict_pinv(uvs, method, anneal):
    """RMCKF: the certified pass of closed_loop_tuned_kernel<6, 6, 2>; KF, IMCC-KF and MCKF: the careful (6,6,2) kernel alone."""
    _assert_strict(uvs, 'dh66', method, anneal, '(6,6) DH strict pinv')


# ---------------------------------------------------------------------------------------------- b. (2,6) on the DH plant
@pytest.mark.parametrize('method,anneal', ESTIMATORS)
def test_dh26_matches_the_oracles(uvs, method, anneal):
    """One image point, m < n: the control law is the minimum-norm branch of pinv.  lanes_per_filter 0, 1 and -1 are all the generic (2,6,1)
    kernel (the same bits); UVS_OPT_STRICT_PINV runs the careful (2,6,1) pass alone."""
    case = 'dh26'
    outs = {}
    for lanes in (0, 1, -1):
        out = outs[lanes] = gh.launch(uvs, case, method, anneal, lanes)
        assert out['lanes'] == 1 and out['segments'] == 1
        _matches_c(out, case, method, anneal, '(2,6) DH generic')
        gh.assert_twins(out, (case, method, anneal, lanes))
    _matches_block(outs[0], case, method, anneal, '(2,6) DH generic')
    gh.assert_same_launch(outs[0], outs[1], (method, anneal, '0 = 1'))
    gh.assert_same_launch(outs[0], outs[-1], (method, anneal, '0 = -1'))
    _assert_strict(uvs, case, method, anneal, '(2,6) DH strict pinv')
    if anneal:
        for reserved in (0, STRICT):
            for T in (1, 33):
                part = gh.launch(uvs, case, method, anneal, 0, reserved, T=T)
                gh.assert_same_launch(gh.launch(uvs, case, method, anneal, 0, reserved), part, (method, reserved, T))


# ---------------------------------------------------------------------------------------------- c. the linear plant at (8,6) and (6,6)
LINEAR_LANES = {'lin86': (0, 1, 2, 4, -2, -4), 'lin66': (0, 2, -2)}


@pytest.mark.parametrize('method,anneal', ESTIMATORS)
@pytest.mark.parametrize('case', ['lin86', 'lin66'])
def test_linear_plant_every_lane_mapping_matches_the_oracles(uvs, case, method, anneal):
    """f = f0 + J (q - q0) inside the tuned kernels: closed_loop_tuned_kernel<8, 6, {1, 2, 4}, ..., UVS_PLANT_LINEAR> and <6, 6, 2, ...>, whose
    rows index lin_f0 and lin_jacobian by row = r * RS + rb (MCKF has tuned kernels on two lanes only: 1 and 4 are generic for it); negative
    lanes: the generic templates on the same plant.  No four-lane small-batch mapping here: 0 is the two-lane kernel."""
    outs = {}
    for lanes in LINEAR_LANES[case]:
        tuned = lanes >= 0 and (method != 'MCKF' or lanes in (0, 2))
        family = f'{"(8,6)" if case == "lin86" else "(6,6)"} linear {"tuned" if tuned else "generic"} L{abs(lanes) or 2}'
        out = outs[lanes] = gh.launch(uvs, case, method, anneal, lanes)
        assert out['lanes'] == (abs(lanes) or 2) and out['segments'] == 1 and out['workspace'] == 0
        _matches_c(out, case, method, anneal, family)
        gh.assert_twins(out, (case, method, anneal, lanes))
        if lanes in (0, 1, 4, -2):
            _matches_block(out, case, method, anneal, family)
    gh.assert_same_launch(outs[0], outs[2], (case, method, anneal, '0 = 2'))


@pytest.mark.parametrize('method', cs.METHODS)
def test_linear_plant_batches_of_1_and_33_are_slices_of_the_batch_of_70(uvs, method):
    for case, lanes in (('lin86', 0), ('lin86', 1), ('lin86', 4), ('lin86', -4), ('lin66', 0), ('lin66', -2)):
        whole = gh.launch(uvs, case, method, True, lanes)
        for T in (1, 33):
            part = gh.launch(uvs, case, method, True, lanes, T=T)
            gh.assert_same_launch(whole, part, (case, method, lanes, T))
            _matches_c(part, case, method, True, f'linear T = {T}')


@pytest.mark.parametrize('method,anneal', ESTIMATORS)
def test_linear_plant_latency_option(uvs, method, anneal):
    """UVS_OPT_LATENCY at lanes_per_filter 0: the four-lane linear kernel for KF, IMCC-KF and RMCKF -- the bits of lanes_per_filter 4 --, MCKF
    stays on two lanes.  At (6,6) the option selects nothing."""
    out = gh.launch(uvs, 'lin86', method, anneal, 0, LATENCY)
    assert out['lanes'] == (2 if method == 'MCKF' else 4)
    _matches_c(out, 'lin86', method, anneal, '(8,6) linear UVS_OPT_LATENCY')
    gh.assert_twins(out, (method, anneal, 'latency'))
    gh.assert_same_launch(gh.launch(uvs, 'lin86', method, anneal, 2 if method == 'MCKF' else 4), out, (method, anneal, 'latency = forced lanes'))
    small = gh.launch(uvs, 'lin66', method, anneal, 0, LATENCY)
    assert small['lanes'] == 2
    gh.assert_same_launch(gh.launch(uvs, 'lin66', method, anneal, 0), small, (method, anneal, 'latency at (6,6)'))


@pytest.mark.parametrize('method,anneal', ESTIMATORS)
@pytest.mark.parametrize('case', ['lin86', 'lin66'])
def test_linear_plant_strict_pinv(uvs, case, method, anneal):
    """RMCKF: certified pass of the tuned linear kernels; KF, IMCC-KF and MCKF: kCarefulOnly (their certifying instantiations are DH-only)."""
    _assert_strict(uvs, case, method, anneal, f'{"(8,6)" if case == "lin86" else "(6,6)"} linear strict pinv')
    if case == 'lin86' and method == 'GMCKF':
        _assert_strict(uvs, case, method, anneal, '(8,6) linear strict pinv', lanes=4)
        _assert_strict(uvs, case, method, anneal, '(8,6) linear strict pinv', lanes=1)


@pytest.mark.parametrize('case', ['lin86', 'lin66'])
def test_linear_plant_refuses_the_analytic_initial_guess(uvs, case):
    inp = cs.inputs(case)
    fp = gh.params(uvs, case, 'GMCKF', False, guess=True)
    with pytest.raises(uvs._lib.UvsError) as exc:
        uvs.engine.closed_loop(fp, gh.plant(uvs, case).to_struct(), gh.cuda(inp['q0']), gh.cuda(inp['noise'].transpose(1, 2, 0)), gh.cuda(inp['x0']))
    assert exc.value.code == ERR_ARG and len(uvs.lib().uvs_last_error()) > 0


@pytest.mark.parametrize('anneal', [False, True])
@pytest.mark.parametrize('case', ['lin86', 'lin66'])
def test_linear_plant_mckf_ignores_a_forced_segment_count(uvs, case, anneal):
    """The linear-plant instantiations compile the hand-over code out (SEG), so a forced segment count must not reach them: the query says
    whole trials, no workspace is asked for, the launch runs whole trials on the two-lane kernel -- the bits of the unforced launch."""
    for lanes in (0, 2):
        cut = gh.launch(uvs, case, 'MCKF', anneal, lanes, reserved=4 << 8)
        assert cut['segments'] == 1 and cut['workspace'] == 0 and cut['fallbacks'] is None and cut['lanes'] == 2
        _matches_c(cut, case, 'MCKF', anneal, 'linear MCKF, segments forced')
        gh.assert_same_launch(gh.launch(uvs, case, 'MCKF', anneal, 2), cut, (case, anneal, lanes, 'forced segments'))


# ---------------------------------------------------------------------------------------------- d. a rank-deficient Jacobian among healthy neighbours
RANKDEF_K, SICK = 12, 40                                     # at two lanes per filter trial 40 sits mid-wavefront (32..63)


@pytest.mark.parametrize('lanes', [0, -2])
@pytest.mark.parametrize('case', ['dh66_x0', 'lin86'])
def test_a_rank_deficient_x0_among_healthy_neighbours(uvs, case, lanes):
    """One trial starts from an X0 with two identical columns (sigma_min / sigma_max under numpy's 1e-15 cutoff; h = 0 keeps it exact on the
    first step), its 69 neighbours are healthy.  Short horizon (K = 12), RMCKF with annealing (sigma_0 = 107.5: the weights of the first step,
    whose innovation is the whole feature vector when X0 is supplied, are 0.5 and not 1e-63, so the first command is a command), as
    test_wide_shape_closed_loop_on_a_kahan_like_jacobian: the sick trial follows the numpy oracle within 1e-6, healthy trials within 1e-8; its
    first command is numpy's truncated minimum-norm one (gate of test_single_step_bank_uses_pinv_semantics); the healthy trials keep the bits of a launch in which that trial is healthy too."""
    from oracle import rmckf_block
    inp = cs.inputs(case)
    m, n = inp['m'], inp['n']
    x0 = inp['x0'].copy()
    x = x0[SICK].reshape(m, n)
    x[:, 5] = x[:, 4]
    sv = np.linalg.svd(x, compute_uv=False)
    assert sv[-1] <= 1e-16 * sv[0] and sv[-2] > 1e-4 * sv[0], 'the input: rank n - 1, a decade under the cutoff'
    want = ('x', 'err', 'q', 'dq')
    mixed = gh.launch(uvs, case, 'GMCKF', True, lanes, want=want, steps=RANKDEF_K, x0=x0)
    healthy = gh.launch(uvs, case, 'GMCKF', True, lanes, want=want, steps=RANKDEF_K)
    assert not mixed['status'].any() and np.all(mixed['k_done'] == RANKDEF_K)
    others = [t for t in range(cs.T) if t != SICK]
    gh.assert_same_launch(healthy, mixed, (case, lanes, 'neighbours'), trials=others)
    gh.assert_twins(mixed, (case, lanes, 'rank-deficient batch'))
    for t in (0, SICK - 1, SICK, SICK + 1, 47, cs.T - 1):
        ref = rmckf_block.run_closed_loop(inp['features'], inp['q0'][t], inp['desired'], inp['noise'][t, :RANKDEF_K], cs.DT, cs.DT * (RANKDEF_K + 0.5),
                                          cs.GAIN, x0[t], method='GMCKF', kernel_bw=cs.BW, annealing=True, initial_guess=False)
        assert ref['status'] == 0 and ref['k_done'] == RANKDEF_K
        tol = 1e-6 if t == SICK else TOL
        for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
            d = cs.rel(mixed[key][t], ref[rk])
            WORST.note('rank-deficient X0', key + (' (sick)' if t == SICK else ' (healthy)'), d)
            assert d <= tol, (key, d, t, case, lanes)
    filt = rmckf_block.BlockFilter(m, n, x0[SICK], 'GMCKF', cs.BW, True, RANKDEF_K)
    f_first = inp['features'](inp['q0'][SICK]) + inp['noise'][SICK, 0]
    kappa = filt.step(f_first, np.zeros(n), 0)                                              # a supplied X0: the first f_old is 0
    assert gh.same_bits(filt.X, x)
    first = rmckf_block.control_law(filt.X, f_first - inp['desired'], kappa, cs.GAIN)
    assert np.abs(first).max() > 1e-3                                                       # a command of a size the gate means something for
    assert np.abs(mixed['dq'][SICK, 0] - first).max() <= 1e-8 * max(1e-3, np.abs(first).max())


# ---------------------------------------------------------------------------------------------- e. tuned replay at (6,6)
REPLAY_T, REPLAY_K, REPLAY_TWINS = 35, 40, (1, 17, 34)       # two lanes per filter: trial 34 rides in the second wavefront
_REPLAY = {}


def _replay_case():
    """The streams of test_replay_other_shapes_match_block_oracle at (6,6), K = 40, T = 35, trial 1 in three places."""
    if 'case' not in _REPLAY:
        f, dq, x0, des = gh.random_replay_case(6, 6, REPLAY_K, REPLAY_T, 1006)
        for a in (f, dq, x0):
            a[list(REPLAY_TWINS[1:])] = a[REPLAY_TWINS[0]]
        _REPLAY['case'] = (f, dq, x0, des)
    return _REPLAY['case']


def _replay_reference(method, t, fpi_threshold=cs.FPI_THRESHOLD):
    from oracle import rmckf_block
    if (method, t, fpi_threshold) not in _REPLAY:
        f, dq, x0, des = _replay_case()
        _REPLAY[(method, t, fpi_threshold)] = rmckf_block.run_replay(f[t], dq[t], x0[t], des, 0.2, method, 7.5, True, 300, fpi_threshold)
    return _REPLAY[(method, t, fpi_threshold)]


def _tuned_replay(uvs, method, lanes, want, layout='kct', T=REPLAY_T, fpi_threshold=cs.FPI_THRESHOLD):
    """gh.replay on the first T trials; numpy arrays in [trial][step][component] order."""
    f, dq, x0, des = _replay_case()
    fp = uvs.engine.make_params(6, 6, method, 7.5, True, 0.05, 15, 0.2, des, False, lanes, REPLAY_K, fpi_threshold, 1000)
    return gh.replay(uvs, fp, f[:T], dq[:T], x0[:T], want, layout)


REPLAY_KEYS = ('x', 'err', 'kappa', 'dqcmd', 'status', 'k_done', 'x_final', 'p_final')


@pytest.mark.parametrize('method', cs.METHODS)
def test_tuned_replay_at_66_matches_the_block_oracle(uvs, method):
    """replay_tuned_kernel<6, 6, ...> (lanes_per_filter 0 and 2) with X and the command wanted, with the estimator alone (cmd = false: the
    four-lane row kernels decline (6,6)) and with err alone; MCKF with a fixed-point loop that iterates.  Per trial against
    rmckf_block.run_replay at the gates of test_replay_other_shapes_match_block_oracle (X 1e-10, command 1e-8, kappa 1e-9, final P 1e-10);
    [step][trial][component] streams carry the same bits, batches of 1 and 33 those of the first trials of the 35; lanes_per_filter -2, the
    generic template, is held to the same gates."""
    f, dq, x0, des = _replay_case()
    refs = [_replay_reference(method, t) for t in range(REPLAY_T)]
    if method == 'MCKF':
        assert max(r['fpi_iterations'].max() for r in refs) >= 3
    full, alone = ('x', 'err', 'kappa', 'dqcmd'), ('x', 'err', 'kappa')
    outs = {}
    for lanes in (0, 2, -2):
        for want in (full, alone, ('err',)):
            out = outs[(lanes, want)] = _tuned_replay(uvs, method, lanes, want)
            tag = (method, lanes, want)
            assert not out['status'].any() and np.all(out['k_done'] == REPLAY_K), tag
            assert [k for k in full if out[k] is not None] == list(want), tag
            assert gh.same_bits(out['err'], f[:, 1:] - des), tag
            for key in REPLAY_KEYS:
                if out[key] is not None:
                    for t in REPLAY_TWINS[1:]:
                        assert gh.same_bits(out[key][t], out[key][REPLAY_TWINS[0]]), (key, t) + tag
            gh.assert_replay(out, refs, WORST, '(6,6) tuned replay', tag)
            if 'x' in want:
                assert gh.same_bits(out['x_final'], out['x'][:, -1]), tag
    for want in (full, alone, ('err',)):
        for key in REPLAY_KEYS:
            if outs[(0, want)][key] is not None:
                assert gh.same_bits(outs[(0, want)][key], outs[(2, want)][key]), (key, method, want, '0 = 2')
    for lanes in (0, 2):
        for want in (full, alone):
            records = _tuned_replay(uvs, method, lanes, want, layout='ktc')
            for key in REPLAY_KEYS:
                if records[key] is not None:
                    assert gh.same_bits(records[key], outs[(lanes, want)][key]), (key, method, lanes, want, 'ktc')
    for want in (full, alone):                                                              # T = 1 and T = 33: slices of the batch of 35
        for T in (1, 33):
            part = _tuned_replay(uvs, method, 0, want, T=T)
            for key in REPLAY_KEYS:
                if part[key] is not None:
                    assert gh.same_bits(part[key], outs[(0, want)][key][:T]), (key, method, want, T)
    if method == 'MCKF':
        # With fpi_threshold 1e-4 every trial needs more than the first fixed-point pass, so the careful second pass re-runs it and what the
        # tuned kernel stored is overwritten.  At the reference's 0.1 the first pass is the whole story (the oracle: two iterations, the second
        # only confirms): here the tuned kernel's own stores are what comes back.
        loose = [_replay_reference(method, t, 0.1) for t in range(REPLAY_T)]
        assert max(r['fpi_iterations'].max() for r in loose) == 2
        for lanes in (0, 2):
            for want in (full, alone):
                out = _tuned_replay(uvs, method, lanes, want, fpi_threshold=0.1)
                assert not out['status'].any() and np.all(out['k_done'] == REPLAY_K)
                gh.assert_replay(out, loose, WORST, '(6,6) tuned replay', (method, lanes, want, 'fpi_threshold 0.1'), skip=('x_final',))
