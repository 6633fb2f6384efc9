"""CPU-only: the oracle of the pixel closed loops itself (oracle/pixel_loop.py) and the cases the GPU suite runs it on
(tests/pixel_loop_common.py; the kernels' side is tests/test_gpu_pixel_loop_oracle.py).

  - the tie: with the sensor swapped for the ideal projection and no occluders, pixel_loop.run has the BITS of
    rmckf_block.run_closed_loop -- the oracle every other closed-loop suite is held to -- for the four estimators, with and without
    annealing, at (8,6) and (2,6);
  - the loop's bookkeeping: the rows that exist, pixels, held and the statistics, on a trial that FAILs after a hold;
  - the PRECONDITIONS of pixel_loop_common, for every trial of every case, none excluded;
  - the TEETH: every applicable misreading of the loop's text moves q or dq by at least 100 gates (1e-6); the table is printed when the
    module finishes (pytest -s) and kept in profiles/pixel_loop_oracle.txt;
  - the hold variants of the wide bar are what their names say."""
import numpy as np
import pytest

import pixel_loop_common as pl

TABLE = {}


def teardown_module(module):
    print('\nteeth: distance in q or dq of each misreading from the unmutated oracle run (smallest over the trials of the case)')
    for name, row in TABLE.items():
        print(f'  {name:32s}', '  '.join(f'{mut} {d:.1e}' for mut, d in row.items()))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('n_points', [4, 1])
@pytest.mark.parametrize('annealing', [False, True])
@pytest.mark.parametrize('method', pl.METHODS)
def test_with_the_ideal_sensor_it_is_run_closed_loop(method, annealing, n_points):
    from oracle import pixel_loop, rmckf_block, rmckf_dense
    import uvs_amd
    m, K = 2 * n_points, 25
    plant = pl.plant_of(n_points)
    rng = np.random.default_rng(5 + n_points)
    for initial_guess in (True, False):
        q0 = pl.jittered(11 + n_points)
        noise = rng.standard_normal((K, m)) * 0.5
        robot = uvs_amd.SyntheticRobot(plant, pl.DT)
        robot.start(q0)
        x0 = uvs_amd.plant.analytic_guess(robot, plant.features(q0), (256, 256), m, 6) * (1.0 if initial_guess else 1.01)
        est = dict(method=method, kernel_bw=7.5, annealing=annealing, fpi_threshold=1e-4, fpi_epoch_max=1000, reg=1e-3, anneal_span=40.0)
        want = rmckf_block.run_closed_loop(plant.features, q0, pl.DESIRED[:m], noise, pl.DT, pl.DT * (K + 0.5), 0.3, x0, initial_guess=initial_guess,
                                           **est)
        got = pixel_loop.run(plant, q0, pl.DESIRED[:m], noise, pl.DT, K, 0.3, k_max=K, initial_guess=initial_guess,
                             x0=None if initial_guess else x0, sensor=pixel_loop.ideal, **est)
        assert want['k_done'] == K == got['k_done'] and want['status'] == 0 == got['status']
        assert same_bits(got['x0'], x0), 'the analytic guess at the step-0 detection'
        for key in ('err', 'q'):
            assert same_bits(got[key], want[key]), (key, initial_guess)
        assert np.array_equal(got['fpi_iterations'], want['fpi_iterations'])
        assert same_bits(got['stats'], rmckf_dense.trial_stats(want['err'], want['t']))


def test_bookkeeping_of_a_trial_that_fails_after_a_hold():
    """c_GMCKF_86_wide_shorter, trial 1: the bar covers red for three steps and the hold is two."""
    name = 'c_GMCKF_86_wide_shorter'
    c, a = pl.CASES[name], pl.oracle_trial('c_GMCKF_86_wide_shorter', 1)
    k = a['k_done']
    assert a['status'] == 1 and 0 < k < c.K
    assert len(a['q']) == len(a['f']) == len(a['counts']) == k + 1 and len(a['dq']) == len(a['err']) == len(a['kappa']) == k
    assert np.array_equal(a['pixels'], a['counts'].min(axis=0)) and a['counts'][k].min() == 0
    assert np.all(np.isfinite(a['f'][:k])) and np.any(np.isnan(a['f'][k])) and np.all(np.isfinite(a['err']))
    red = a['held'][0]
    assert red == [k - 2, k - 1] and all(a['counts'][j, 0] == 0 for j in red + [k]), 'held for two steps, lost at the third'
    noise = pl.noise_of(c, 1)
    for j in red:                                                    # a held pair is the row before, bit for bit: no noise of its own step
        assert same_bits(a['f'][j, :2], a['f'][j - 1, :2]) and np.all(noise[j, :2] != 0.0)
    t = np.cumsum(np.full(k, pl.DT))
    assert np.allclose(a['stats'][0], np.linalg.norm(np.sum(a['err'] ** 2, axis=0)), rtol=1e-14)
    assert np.allclose(a['stats'][2], np.linalg.norm(t @ np.abs(a['err'])), rtol=1e-12)


def longest_run(steps):
    best = run = 0
    for i, k in enumerate(steps):
        run = run + 1 if i and k == steps[i - 1] + 1 else 1
        best = max(best, run)
    return best


@pytest.mark.parametrize('tag', ['GMCKF_86', 'IMCCKF_66'])
def test_the_hold_variants_are_what_their_names_say(tag):
    n_points = pl.CASES[f'c_{tag}_wide_longer'].n_points
    loss, holds = pl.LONGEST_LOSS[n_points], pl.HOLDS[n_points]
    runs = {name: [pl.oracle_trial(f'c_{tag}_wide_{name}', i) for i in range(2)] for name in holds}
    longest = max(longest_run(h) for a in runs['longer'] for h in a['held'])
    assert longest == loss and holds['longer'] > loss == holds['equal'] == holds['shorter'] + 1
    for name in ('longer', 'equal'):
        assert [a['status'] for a in runs[name]] == [0, 0] and all(a['pixels'].max() == 0 for a in runs[name]), 'every disc is lost at some step'
    for a, b in zip(runs['longer'], runs['equal']):
        assert a['held'] == b['held'] and same_bits(a['q'], b['q'])
    failed = [a for a in runs['shorter'] if a['status'] == 1]
    assert failed, 'the hold runs out on the trial with the longest loss'
    for a in failed:
        k = a['k_done']
        assert any(h[-holds['shorter']:] == list(range(k - holds['shorter'], k)) for h in a['held'] if h), 'FAIL at the step the hold runs out'


def test_the_scenarios_do_what_they_are_for():
    assert all(len(c.trials) <= 8 for c in pl.CASES.values())
    bar = pl.oracle_trial('c_GMCKF_86_bar', 0)
    clear = pl.oracle_trial('a_GMCKF_86_plain', 0)
    assert bar['pixels'].min() > 0 and np.all(bar['pixels'] < clear['pixels']), 'partial occlusion of every disc, no loss'
    held = pl.oracle_trial('c_GMCKF_86_distractor_held', 0)
    assert held['held'][0] == [] and held['pixels'][0] > 0 and all(held['held'][1:]), 'the distractor keeps red from being lost'
    for method in ('GMCKF', 'MCKF'):
        a, b = pl.oracle_trial(f'c_{method}_86_leaves_hold0', 0), pl.oracle_trial(f'c_{method}_86_leaves_hold2', 0)
        assert a['status'] == 1 == b['status'] and a['pixels'].min() == 0 and not any(a['held']) and any(len(h) == 2 for h in b['held'])
    fpi = [pl.oracle_trial('d_MCKF_86_grid', i)['fpi_iterations'].sum() for i in range(8)]
    assert len(set(fpi)) >= 3, 'the thresholds of the grid change how often the fixed point iterates'
    a = pl.oracle_trial('b_GMCKF_86_x0', 0)
    assert not a['f0'].any() and a['kappa'][0].max() < 1e-6, 'f_old of step 0 is zeros: the first innovation is the whole feature vector'


@pytest.mark.parametrize('name', list(pl.CASES))
def test_preconditions_of_every_trial(name):
    for i in range(len(pl.CASES[name].trials)):
        p = pl.preconditions(name, i)
        assert not p['problems'], (name, i, p)


@pytest.mark.parametrize('name', list(pl.CASES))
def test_teeth(name):
    c = pl.CASES[name]
    TABLE[name] = row = pl.teeth(name)
    assert {'regressor_halved', 'regressor_stale'} <= set(row)
    assert ('anneal_k_plus_1' in row) == (c.annealing and c.method != 'KF') and ('kappa_dropped' in row) == (c.method == 'GMCKF')
    assert ('step0_unoccluded' in row) == any(tr.occluders is not None for tr in c.trials)
    if c.hold and c.noise_px:
        assert 'held_pair_new_noise' in row
    for mut, d in row.items():
        if (name, mut) in pl.NO_TEETH:
            assert c.n_points == 1, 'only a (2,6) entry may go without teeth'
            continue
        assert d >= pl.TEETH_MIN, (name, mut, d)
