"""The plain-C oracle (oracle/c/rmckf_oracle.c) against the reference fixtures and the numpy oracle."""
import numpy as np
import pytest

import closed_shapes_common as shapes
import estimator_params_common as params
from conftest import golden_names, load_golden, rel_err
from oracle import c_oracle

CLOSED = golden_names('closed_')
FPI = golden_names('fpi_')
CHAOTIC = {'closed_gmckf_mix_anneal_hold'}


@pytest.mark.parametrize('name', CLOSED)
def test_c_oracle_reproduces_reference(name):
    g = load_golden(name)
    meta, p = g['meta'], g['meta']['params']
    out = c_oracle.closed_loop_batch(g['q_start'][None], g['noise'][None], g['desired'], meta['method'], p['kernel_bw'], p['annealing'],
                                     meta['dt'], meta['t_max'], meta['gain'], want_x=True, fpi_threshold=p['fpi_threshold'], fpi_epoch_max=p['fpi_epoch_max'])
    assert out['status'][0] == int(g['status']) and out['k_done'][0] == len(g['t'])
    horizon = 40 if name in CHAOTIC else len(g['t'])
    assert rel_err(out['err'][0, :horizon], g['err'][:horizon]) <= 1e-9
    assert rel_err(out['q'][0, :horizon], g['q'][:horizon]) <= 1e-9
    steps = g['X_steps'][g['X_steps'] < horizon]
    assert rel_err(out['X'][0, steps], g['X'][:len(steps)]) <= 1e-9
    if name not in CHAOTIC:
        from oracle.rmckf_dense import trial_stats
        assert rel_err(out['stats'][0], trial_stats(g['err'], g['t'])) <= 1e-9


def test_c_oracle_fails_on_non_finite_measurement():
    g = load_golden('closed_gmckf_a1p5')
    noise = g['noise'][None, :40].copy()
    noise[0, 11, 2] = np.inf
    out = c_oracle.closed_loop_batch(g['q_start'][None], noise, g['desired'])
    assert out['status'][0] == 1 and out['k_done'][0] == 11


@pytest.mark.parametrize('name', FPI)
def test_c_oracle_reproduces_reference_fpi(name):
    """MCKF with a live fixed-point iteration (oracle/gen_golden_fpi.py): trajectories, passes per step, status and the FAILing step."""
    g = load_golden(name)
    meta, p = g['meta'], g['meta']['params']
    out = c_oracle.closed_loop_batch(g['q_start'][None], g['noise_full'][None], g['desired'], 'MCKF', p['kernel_bw'], p['annealing'],
                                     meta['dt'], meta['t_max'], meta['gain'], want_x=True, fpi_threshold=p['fpi_threshold'], fpi_epoch_max=p['fpi_epoch_max'])
    k = len(g['t'])
    assert out['status'][0] == int(g['status']) and out['k_done'][0] == k
    assert np.array_equal(out['fpi'][0, :len(g['fpi_epochs'])], g['fpi_epochs'])
    # cap4: deviations sit at 4e-11 by step 255 and grow 100-fold across an ill-conditioned stretch (cond 577, steps 274-280) -- 6e-9 at the end
    tol = 1e-7 if name == 'fpi_mckf_a1p2_cap4' else 1e-9
    assert rel_err(out['err'][0, :k], g['err']) <= tol and rel_err(out['q'][0, :k], g['q']) <= tol
    assert rel_err(out['X'][0, g['X_steps']], g['X']) <= tol


@pytest.mark.parametrize('name', CLOSED + FPI)
def test_c_oracle_replay_reproduces_reference(name):
    """Open-loop replay in plain C (uvs_oracle_replay): the reference's recorded f / regressor streams in, its per-step X and commands out."""
    g = load_golden(name)
    meta, p = g['meta'], g['meta']['params']
    k = len(g['t'])
    f_seq = np.vstack([g['f_init'][None], g['f']])
    out = c_oracle.replay_batch(f_seq[None], g['dq_prev'][None], g['X'][0][None], g['desired'], meta['method'], p['kernel_bw'], p['annealing'],
                                int(meta['t_max'] / meta['dt']), meta['gain'], p['fpi_threshold'], p['fpi_epoch_max'])
    assert out['status'][0] == 0 and out['k_done'][0] == k
    assert rel_err(out['X'][0, g['X_steps']], g['X']) <= 1e-10
    assert rel_err(out['dq_cmd'][0, :-1], g['dq_prev'][1:]) <= 1e-8
    if 'fpi_epochs' in g:
        assert np.array_equal(out['fpi'][0], g['fpi_epochs'][:k])


# ---------------------------------------------------------------------------------------------- the shapes the reference cannot run
@pytest.mark.parametrize('case,method,anneal', shapes.configurations())
def test_c_oracle_agrees_with_the_block_oracle_at_the_other_shapes(case, method, anneal):
    """Closed loop at (6,6) and (2,6) on the DH plant (3 points / 1 point; (6,6) also from a supplied X0) and at (8,6) and (6,6) on the
    linear plant: oracle/c (batch speed) against oracle/rmckf_block (numpy pinv, the authority) on the trials shapes.sampled(case), every
    estimator, annealing off and on, MCKF with fpi_threshold 1e-4 (its fixed-point loop iterates).  Gate 1e-11 on X, q and err, status and
    k_done exact.  A trial may miss it -- closed-loop sensitivity of the square (6,6) estimate -- only if shapes.EXCLUDED lists it (the list
    has a decade of margin, so it may also name trials that pass here); the GPU parity module leaves the listed trials out, and no
    configuration lists more than 10 % of its sampled trials."""
    agreement = shapes.oracle_agreement(case, method, anneal)
    apart = tuple(sorted(t for t, d in agreement.items() if not d <= shapes.AGREE_TOL))
    listed = tuple(shapes.EXCLUDED.get((case, method, anneal), ()))
    close = [d for t, d in agreement.items() if t not in apart]
    print(f'{case} {method} annealing {anneal}: {len(close)} trials agree to {max(close):.1e}; left out', {t: f'{agreement[t]:.1e}' for t in listed})
    assert set(apart) <= set(listed), {t: agreement[t] for t in apart if t not in listed}
    assert len(listed) <= shapes.MAX_EXCLUDED_FRACTION * len(agreement)
    assert not set(listed) & set(shapes.TWINS)                          # the bit-identity trials stay in the comparison
    ref = shapes.c_reference(case, method, anneal)
    if method == 'MCKF':
        assert ref['fpi'].max() >= 3                                    # the fixed-point loop does iterate
    if shapes.CASES[case][2] == 'linear':
        assert not ref['status'].any() and np.all(ref['k_done'] == shapes.inputs(case)['K'])


# ---------------------------------------------------------------------------------------------- reg and anneal_span off their defaults
@pytest.mark.parametrize('case,name,method', params.configurations())
def test_oracles_agree_at_other_reg_and_anneal_span(case, name, method):
    """The closed loops above (and 'dh86', the (8,6) DH plant) at the parameter sets of tests/estimator_params_common.py: oracle/c against
    oracle/rmckf_block at AGREE_TOL on the kept trials, params.EXCLUDED under the 10 % cap and clear of the twins, nothing FAILs -- and the
    teeth: oracle/c run with the DEFAULT reg and anneal_span is at least 100 GPU gates (1e-8) away on the worst kept trial, so a kernel
    that used a literal 1e-6 or 100 in place of the field cannot pass tests/test_gpu_estimator_params.py."""
    anneal, reg, span = params.estimator(name, method)
    assert (reg, span) != (params.REG, params.ANNEAL_SPAN) and (anneal or span == params.ANNEAL_SPAN)
    agreement = shapes.oracle_agreement(case, **params.run(name, method))
    apart = tuple(sorted(t for t, d in agreement.items() if not d <= shapes.AGREE_TOL))
    listed = tuple(params.EXCLUDED.get((case, name, method), ()))
    close = [d for t, d in agreement.items() if t not in apart]
    bite = params.teeth(case, name, method)
    print(f'{case} {name} {method}: {len(close)} trials agree to {max(close):.1e}; left out', {t: f'{agreement[t]:.1e}' for t in listed},
          f'; the default-valued run is {bite:.1e} away')
    assert set(apart) <= set(listed), {t: agreement[t] for t in apart if t not in listed}
    assert len(listed) <= shapes.MAX_EXCLUDED_FRACTION * len(agreement)
    assert not set(listed) & set(shapes.TWINS)
    ref = shapes.c_reference(case, **params.run(name, method))
    assert not ref['status'].any() and np.all(ref['k_done'] == shapes.inputs(case)['K'])
    if method == 'MCKF':
        assert ref['fpi'].max() >= 2                                    # the fixed-point loop iterates at these bandwidths too
    assert bite >= params.TEETH * params.GATE, bite


@pytest.mark.parametrize('name,method', params.WIDE_CONFIGS)
def test_oracles_agree_at_other_reg_and_anneal_span_on_the_wide_shape(name, method):
    """(32,7) on the linear plant (the inputs of test_closed_loop_stress_plant, T = 4, K = 80): every trial at AGREE_TOL, and the teeth."""
    agreement = shapes.oracle_agreement('wide', **params.run(name, method))
    bite = params.teeth('wide', name, method)
    print(f'(32,7) {name} {method}: agree to {max(agreement.values()):.1e}; the default-valued run is {bite:.1e} away')
    assert max(agreement.values()) <= shapes.AGREE_TOL, agreement
    ref = shapes.c_reference('wide', **params.run(name, method))
    assert not ref['status'].any() and np.all(ref['k_done'] == shapes.inputs('wide')['K'])
    assert bite >= params.TEETH * params.GATE, bite


@pytest.mark.parametrize('name,method', [('R3', 'GMCKF'), ('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A25', 'MCKF'), ('A400', 'GMCKF'), ('A400', 'IMCCKF')])
def test_dense_oracle_agrees_with_the_block_oracle_at_other_reg_and_anneal_span(name, method):
    """oracle/rmckf_dense -- the reference's own arithmetic: reg * eye(m) added to Cy, dense mn x mn covariance -- against the block form on
    the streams (f, and dq as the difference quotient of q) of three 'dh86' closed-loop trials at the set's values.  Gates: those
    test_oracle_golden.py holds the block form to against the reference's fixtures, which the dense form reproduces -- X 1e-11 and
    command 1e-9 (test_block_replay_matches_reference), X 1e-10 and command 1e-8 for MCKF (test_block_replay_matches_reference_fpi)."""
    from oracle import rmckf_block, rmckf_dense
    inp = shapes.inputs('dh86')
    anneal, reg, span = params.estimator(name, method)
    for t in (0, 28, 56):
        run = shapes.block_reference('dh86', t=t, **params.run(name, method))
        f_seq = np.vstack([inp['features'](inp['q0'][t])[None], run['f']])
        dq_seq = np.vstack([np.zeros((1, 6)), np.diff(run['q'], axis=0) / shapes.DT])
        kw = dict(method=method, kernel_bw=inp['bw'], annealing=anneal, k_max=inp['K'], fpi_threshold=shapes.FPI_THRESHOLD, reg=reg, anneal_span=span)
        a = rmckf_dense.run_replay(f_seq, dq_seq, inp['x0'][t], inp['desired'], shapes.GAIN, **kw)
        b = rmckf_block.run_replay(f_seq, dq_seq, inp['x0'][t], inp['desired'], shapes.GAIN, **kw)
        tol_x, tol_cmd = (1e-10, 1e-8) if method == 'MCKF' else (1e-11, 1e-9)
        print(f'dense - block, dh86 {name} {method} trial {t}: X {rel_err(b["X"], a["X"]):.1e}, command {rel_err(b["dq_cmd"], a["dq_cmd"]):.1e}')
        assert rel_err(b['X'], a['X']) <= tol_x and rel_err(b['kappa'], a['kappa']) <= tol_x and rel_err(b['dq_cmd'], a['dq_cmd']) <= tol_cmd
        assert np.abs(b['X'] - run['X']).max() <= 1e-6 * np.abs(run['X']).max()        # the streams are the closed loop's: the replay follows it


@pytest.mark.parametrize('method', sorted(params.GRID_CELLS))
def test_the_oracle_alone_is_calm_on_the_per_trial_grid_cells(method):
    """The cells tests/test_gpu_estimator_params.py holds the per-trial reg / fpi_threshold to (the reference configuration, alpha = 1.5,
    32 trials per cell, host noise): at least 95 % of the trials are reproduced by oracle/c from a start moved by 1e-14 -- measured 124 of
    128 for RMCKF, 64 of 64 for MCKF -- and nothing FAILs."""
    import json
    import os
    import uvs_amd
    import sweep_common
    from conftest import ROOT
    raw = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
    raw['estimator']['method'] = method
    raw['estimator']['estimator_params']['annealing'] = False
    cfg = uvs_amd.batch.load_config(raw)
    plan = uvs_amd.batch.plan_trials(cfg, [1.5], params.GRID_E)
    noise = sweep_common.host_noise(uvs_amd, cfg, plan)
    calm_total = 0
    for cell in params.GRID_CELLS[method]:
        a, calm = params.grid_oracle(cfg, plan.q_start, noise, cell)
        print(f'{method} {cell}: calm {int(calm.sum())}/{params.GRID_E}, FAIL {int(a["status"].sum())}')
        assert not a['status'].any()
        calm_total += int(calm.sum())
    assert calm_total >= params.GRID_MIN_CALM * params.GRID_E * len(params.GRID_CELLS[method]), calm_total
