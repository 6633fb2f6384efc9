"""MCKF with a LIVE fixed-point iteration on the HIP kernels (experiment.py:194-250): second and later passes inside the tuned two-lane
closed-loop kernel (undo of the optimistic commit, Cholesky per block, X-stream overwrite, epoch cap, Cy = 0 skips) and the
subnormal-weight path that ends a trial with FAIL.  Fixtures tests/golden/fpi_*.npz are runs of the unmodified reference
(oracle/gen_golden_fpi.py); the batch tests compare with the block / C oracle, which test_oracle_golden.py / test_oracle_c.py pin to the
same fixtures (trajectories AND passes per step)."""
import numpy as np
import pytest

from conftest import golden_names, load_golden, rel_err, scene_desired

pytestmark = pytest.mark.gpu

FPI = golden_names('fpi_')
# cap4: two correct fp64 evaluations (numpy dense vs plain C) already differ by 6e-9 at the end of this trial (test_oracle_c.py)
TOL = {'fpi_mckf_a1p2_cap4': 1e-6}


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    return uvs_amd


def _cuda(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _fp(uvs, g, lanes=0, steps=None):
    meta, p = g['meta'], g['meta']['params']
    return uvs.engine.make_params(8, 6, 'MCKF', p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], meta['gain'], g['desired'], True, lanes, steps,
                                  p['fpi_threshold'], p['fpi_epoch_max'])


# lanes 0 / 2: tuned two-lane kernel, every pass in-kernel; 4 / 1: tuned first pass + careful second pass; negative / 8: generic template
@pytest.mark.parametrize('lanes', [0, 2, 4, 1, -2, -4, 8])
@pytest.mark.parametrize('name', FPI)
def test_closed_loop_matches_reference_fpi(uvs, name, lanes):
    g = load_golden(name)
    k = len(g['t'])
    plant = uvs.SyntheticPlant.ur10(scene_desired(g))
    T = 3                                                                     # the same trial three times: lanes must agree bitwise
    out = uvs.engine.closed_loop(_fp(uvs, g, lanes), plant.to_struct(), _cuda(np.tile(g['q_start'], (T, 1))),
                                 _cuda(np.repeat(g['noise_full'][:, :, None], T, axis=2)), want=('x', 'err', 'q', 'f', 'dq'))
    assert out['status'].cpu().tolist() == [int(g['status'])] * T and out['k_done'].cpu().tolist() == [k] * T
    tol = TOL.get(name, 1e-8)
    err, q, X, f, dq = (out[key].cpu().numpy()[:k] for key in ('err', 'q', 'x', 'f', 'dq'))
    for a in (err, q, X):
        assert np.array_equal(a[:, :, 0], a[:, :, 1]) and np.array_equal(a[:, :, 0], a[:, :, 2])
    assert rel_err(err[:, :, 0], g['err']) <= tol and rel_err(q[:, :, 0], g['q']) <= tol and rel_err(f[:, :, 0], g['f']) <= tol
    assert rel_err(X[g['X_steps'], :, 0], g['X']) <= tol
    assert rel_err(dq[:k - 1, :, 0], g['dq_prev'][1:]) <= 10 * tol
    if int(g['status']) == 0:
        from oracle.rmckf_dense import trial_stats
        assert rel_err(out['stats'].cpu().numpy()[0], trial_stats(g['err'], g['t'])) <= tol


@pytest.mark.parametrize('lanes', [0, 2, 4, -2])
@pytest.mark.parametrize('name', FPI)
def test_replay_matches_reference_fpi(uvs, name, lanes):
    """The reference's recorded f / dq streams: per-step X of every pass count, final P; a FAILed trial is replayed up to its last logged step."""
    g = load_golden(name)
    k = len(g['t'])
    f_seq = np.vstack([g['f_init'][None], g['f']])
    out = uvs.engine.replay(_fp(uvs, g, lanes, steps=k), _cuda(f_seq[:, :, None]), _cuda(g['dq_prev'][:, :, None]), _cuda(g['X'][0][None]), final_state=True)
    assert int(out['status'][0]) == 0 and int(out['k_done'][0]) == k
    assert rel_err(out['x'].cpu().numpy()[g['X_steps'], :, 0], g['X']) <= 1e-9
    assert rel_err(out['dqcmd'].cpu().numpy()[:-1, :, 0], g['dq_prev'][1:]) <= 1e-7
    if int(g['P_steps'][-1]) == k - 1:
        assert rel_err(out['p_final'].cpu().numpy()[0].reshape(8, 6, 6), g['P_blocks'][-1]) <= 1e-9


def _mixed_batch(rng, T, K):
    """Trials of very different temper in one batch, so that a wavefront holds filters that stop after one pass next to filters that
    iterate, skip or FAIL: per-trial noise scale from 0 (never iterates) to heavy-tailed (Cy = 0 and subnormal weights)."""
    scale = rng.choice([0.0, 0.3, 1.0, 3.0, 10.0], size=T)
    noise = rng.standard_t(1.2, size=(T, K, 8)) * scale[:, None, None]
    q0 = np.tile([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0], (T, 1))
    q0[:, :3] += rng.uniform(-0.15, 0.15, (T, 3))
    return q0, noise


@pytest.mark.parametrize('thr,cap', [(1e-3, 1000), (1e-4, 3), (0.1, 1000), (1e-2, 1)])
@pytest.mark.parametrize('lanes', [0, 4, -2])
def test_ragged_mixed_batch_matches_c_oracle(uvs, lanes, thr, cap):
    """150 trials (4 full wavefronts of 32 + 22; at 4 lanes 9 + 6): only some lanes of a wavefront take the `__any(more)` branch, the
    X-stream overwrite and the skip / FAIL exits.  Passes per step are the C oracle's (pinned to the reference's own counts)."""
    from oracle import c_oracle
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 150, 90
    q0, noise = _mixed_batch(np.random.default_rng(77), T, K)
    ref = c_oracle.closed_loop_batch(q0, noise, desired, method='MCKF', kernel_bw=10.0, annealing=False, dt=0.05, t_max=15.0, gain=0.2, steps=K, want_x=True,
                                     fpi_threshold=thr, fpi_epoch_max=cap)
    fpi = ref['fpi']
    live = [fpi[t, :ref['k_done'][t]] for t in range(T)]
    if cap > 1 and thr < 0.1:                                                 # steps at which some filters of a wavefront iterate and others do not
        alive = np.arange(K)[None, :] < ref['k_done'][:32, None]
        multi, n_alive = ((fpi[:32] >= 2) & alive).sum(axis=0), alive.sum(axis=0)
        assert int(((multi > 0) & (multi < n_alive)).sum()) >= 20
    if cap > 1:
        assert 3 <= int((ref['status'] == 1).sum()) <= T // 2                 # subnormal weights: some trials FAIL
    else:
        assert int((ref['status'] == 1).sum()) == 0                           # one pass allowed = epoch cap reached = every correction skipped
    assert sum(int((v == 0).any()) for v in live) >= 5                        # Cy = 0: skipped corrections
    fp = uvs.engine.make_params(8, 6, 'MCKF', 10.0, False, 0.05, 15.0, 0.2, desired, True, lanes, K, thr, cap)
    out = uvs.engine.closed_loop(fp, uvs.SyntheticPlant.ur10(desired).to_struct(), _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('x', 'err', 'q'))
    assert np.array_equal(out['status'].cpu().numpy(), ref['status']) and np.array_equal(out['k_done'].cpu().numpy(), ref['k_done'])
    dev = np.zeros(T)
    for t in range(T):
        kd = int(ref['k_done'][t])
        for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
            if kd:
                dev[t] = max(dev[t], rel_err(out[key][:kd, :, t].cpu().numpy(), ref[rk][t, :kd]))
    # Heavy-tailed noise at scale 10: a few trials amplify rounding without bound -- the numpy block oracle and oracle/c
    # themselves end 2.4 apart on trial 134 of the (0.1, 1000) batch and 7.6e-7 on trial 80 of the (1e-4, 3) one.  Such trials are found
    # by running the oracle again from starts moved by 1e-14 and are held to status / k_done only; everybody else is held tight.
    ref2 = c_oracle.closed_loop_batch(q0 * (1.0 + 1e-14), noise, desired, method='MCKF', kernel_bw=10.0, annealing=False, dt=0.05, t_max=15.0, gain=0.2, steps=K,
                                      want_x=True, fpi_threshold=thr, fpi_epoch_max=cap)
    sens = np.array([max([rel_err(ref2[rk][t, :ref['k_done'][t]], ref[rk][t, :ref['k_done'][t]]) for rk in ('err', 'q', 'X')]) if ref['k_done'][t] else 0.0
                     for t in range(T)])
    calm = sens <= 1e-11
    assert int((~calm).sum()) <= 6 and dev[calm].max() <= 1e-8, (int((~calm).sum()), dev[calm].max(), np.argmax(np.where(calm, dev, 0)))
    ok = (ref['status'] == 0) & calm
    assert rel_err(out['stats'].cpu().numpy()[ok], ref['stats'][ok]) <= 1e-7


def test_iterating_trials_do_not_disturb_their_wavefront(uvs):
    """Bit-exactness across batch composition: a trial's streams do not depend on whether its wavefront neighbours iterate."""
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 64, 60
    q0, noise = _mixed_batch(np.random.default_rng(5), T, K)
    fp = uvs.engine.make_params(8, 6, 'MCKF', 10.0, False, 0.05, 15.0, 0.2, desired, True, 0, K, 1e-3, 1000)
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    full = uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('x', 'err', 'q'))
    for t in (0, 7, 31, 40, 63):
        one = uvs.engine.closed_loop(fp, plant, _cuda(q0[t:t + 1]), _cuda(noise[t:t + 1].transpose(1, 2, 0)), want=('x', 'err', 'q'))
        kd = int(one['k_done'][0])
        assert kd == int(full['k_done'][t]) and int(one['status'][0]) == int(full['status'][t])
        for key in ('x', 'err', 'q'):
            assert np.array_equal(one[key][:kd, :, 0].cpu().numpy(), full[key][:kd, :, t].cpu().numpy()), (t, key)


def test_monte_carlo_batch_matches_c_oracle_mckf(uvs):
    """2 048 trials of the reference's SHIPPED configuration (config.json: MCKF, sigma 10, threshold 0.1, alpha-stable noise) at the first cell
    of its sweep, alpha = 1.0, seeds 123456 + t, jittered starts: status (~7 % FAIL through a subnormal weight), the FAILing step, and the
    trajectories up to it against oracle/c.  Trial 0 is fixture fpi_default_a1p0_seed0 without jitter -- here with: another trajectory."""
    from oracle import c_oracle
    import bench
    cfg = bench.config2()
    cfg['experiments']['epoch'] = 2048
    cfg['estimator']['method'] = 'MCKF'
    cfg['noise']['noise_params']['alpha'] = 1.0
    plan = uvs.batch.plan_trials(cfg, cells=[1.0])
    K = 299
    noise = np.zeros((len(plan), K, 8))
    uvs.batch.trial_noise(cfg, plan, 0, len(plan), K, noise)
    desired = cfg['experiments']['desired_f']
    ref = c_oracle.closed_loop_batch(plan.q_start, noise, desired, method='MCKF')
    n_fail = int((ref['status'] == 1).sum())
    assert 60 <= n_fail <= 500, n_fail                                      # 16 % of these 2 048 (jittered starts): not an exotic path
    # MCKF under Cauchy noise is chaotic for part of the trials: the oracle run again from starts moved by 1e-14 ends
    # elsewhere -- other FAIL steps included -- for ~15 % of them.  Those are excluded; the calm ones are held to exact status / k_done.
    ref2 = c_oracle.closed_loop_batch(plan.q_start * (1.0 + 1e-14), noise, desired, method='MCKF')

    def deviation(a_err, a_kd, b):
        dev = np.zeros(len(plan))
        for t in range(len(plan)):
            kd = int(min(a_kd[t], b['k_done'][t]))
            if kd:
                dev[t] = np.abs(a_err[t, :kd] - b['err'][t, :kd]).max() / np.abs(b['err'][t, :kd]).max()
        return dev
    calm = (deviation(ref2['err'], ref2['k_done'], ref) <= 1e-11) & (ref2['status'] == ref['status']) & (ref2['k_done'] == ref['k_done'])
    assert int(calm.sum()) >= 1500 and 40 <= int((ref['status'][calm] == 1).sum())
    for lanes in (0, 4):
        fp = uvs.engine.make_params(8, 6, 'MCKF', 10, False, 0.05, 15, 0.2, desired, True, lanes)
        out = uvs.engine.closed_loop(fp, uvs.SyntheticPlant.ur10().to_struct(), _cuda(plan.q_start), _cuda(noise.transpose(1, 2, 0)), want=('err', 'q'))
        status, k_done = out['status'].cpu().numpy(), out['k_done'].cpu().numpy()
        assert np.array_equal(status[calm], ref['status'][calm]) and np.array_equal(k_done[calm], ref['k_done'][calm])
        dev = deviation(out['err'].cpu().numpy().transpose(2, 0, 1), k_done, ref)
        agree = int(((status == ref['status']) & (k_done == ref['k_done'])).sum())
        print(f'MCKF alpha = 1.0, 2048 trials vs C oracle (lanes {lanes}): {n_fail} FAIL in the oracle, {int(calm.sum())} calm trials; deviation of the calm ones: '
              f'median {np.median(dev[calm]):.2e}, max {dev[calm].max():.2e}; status and k_done agree on {agree} of all 2048')
        assert dev[calm].max() <= 1e-8 and agree >= 1900
        ok = calm & (ref['status'] == 0)
        sdev = np.abs(out['stats'].cpu().numpy()[ok] - ref['stats'][ok]) / ref['stats'][ok]
        assert sdev.max() <= 1e-8


@pytest.mark.parametrize('route', ['device_plant', 'external_robot'])
@pytest.mark.parametrize('name', ['fpi_mckf_a1p5_thr1em6', 'fpi_default_a1p0_seed0', 'fpi_mckf_a1p2_cap4'])
def test_experiment_api_drop_in_fpi(uvs, name, route):
    """Experiment(...).run() with the reference's call signature on runs whose fixed-point iteration iterates, skips or ends in FAIL:
    the 9-tuple of the reference, logs trimmed to the FAILing step (experiment.py:345-352).  Both routes: whole trial in one kernel, and
    the Python loop around a robot the package knows nothing about with one estimator step per call (uvs_rmckf_step_f64)."""
    from oracle.plant_ref import PinholeUR10
    g = load_golden(name)
    meta = g['meta']
    prof = uvs.NoiseProfiler(num_features=8, noise_type=uvs.NoiseType.ALPHA_STABLE, seed=meta['seed'], noise_hold=False, noise_hold_cnt=10,
                             noise_params=meta['noise_params'])
    robot = uvs.SyntheticRobot(dt=meta['dt']) if route == 'device_plant' else PinholeUR10(meta['dt'])
    ex = uvs.Experiment(q_start=g['q_start'], desired_f=g['desired'], noise_prof=prof, t_s=meta['dt'], t_max=meta['t_max'], ibvs_gain=meta['gain'],
                        robot=robot, method=uvs.Method.MCKF, method_params=meta['params'])
    status, t, err, q, f, fd, cam, noise, bw = ex.run()
    k = len(g['t'])
    assert status.value == int(g['status']) and len(t) == k == len(err) == len(q) == len(f) == len(fd) == len(cam) == len(noise) == len(bw)
    assert np.array_equal(t, g['t']) and np.array_equal(noise, g['noise'])
    tol = TOL.get(name, 1e-8)
    for got, ref in ((err, g['err']), (q, g['q']), (f, g['f'])):
        assert rel_err(got, ref) <= tol
    assert np.array_equal(bw, g['sigma_log'])


@pytest.mark.parametrize('lanes', [0, 4, -2])
def test_infinite_sample_is_a_skipped_correction_for_mckf(uvs, lanes):
    """An infinite measurement: Cy = exp(-inf) = 0, inv(Cy) raises and MCKF keeps only the prediction of that step (experiment.py:225-236) -- the
    state survives (found by tools/fuzz_replay.py: the kernels formed 0 * inf in the state update).  The trial still ends one step later,
    when the infinite error has gone through the control law into the joints; KF / IMCC-KF / RMCKF lose X at the step itself.  Both as the
    reference's restatements do (oracle/c here; the dense numpy port agrees)."""
    from oracle import c_oracle
    g = load_golden('closed_mckf_a1p5')
    meta = g['meta']
    K = 40
    noise = np.repeat(g['noise'][:K, :, None], 3, axis=2).copy()
    noise[11, 2, 1] = np.inf                                                  # trial 1 only
    plant = uvs.SyntheticPlant.ur10(scene_desired(g))
    for method, k_fail in (('MCKF', 12), ('GMCKF', 11), ('KF', 11)):
        ref = c_oracle.closed_loop_batch(np.tile(g['q_start'], (3, 1)), noise.transpose(2, 0, 1), g['desired'], method, steps=K)
        assert ref['status'].tolist() == [0, 1, 0] and ref['k_done'].tolist() == [K, k_fail, K]
        fp = uvs.engine.make_params(8, 6, method, 10, False, meta['dt'], meta['t_max'], meta['gain'], g['desired'], True, lanes, K)
        out = uvs.engine.closed_loop(fp, plant.to_struct(), _cuda(np.tile(g['q_start'], (3, 1))), _cuda(noise), want=('x', 'err'))
        assert out['status'].cpu().tolist() == [0, 1, 0] and out['k_done'].cpu().tolist() == [K, k_fail, K], method
        X = out['x'].cpu().numpy()
        assert np.array_equal(X[:, :, 0], X[:, :, 2]) and rel_err(X[:11, :, 1], X[:11, :, 0]) <= 1e-12
        if method == 'MCKF':
            assert np.all(np.isfinite(X[11, :, 1])) and rel_err(X[11, :, 1], X[10, :, 1]) <= 1e-15    # skipped correction: X unchanged


# ---------------------------------------------------------------------------------------------- small batches: four lanes per filter, two-lane bits
def _same_bits(torch, a, b, K, keys=('x', 'err', 'q')):
    assert torch.equal(a['status'], b['status']) and torch.equal(a['k_done'], b['k_done'])
    live = torch.arange(K, device='cuda')[:, None, None] < a['k_done'][None, None, :]
    for key in keys:
        assert torch.equal(torch.where(live, a[key], 0.0).view(torch.int64), torch.where(live, b[key], 0.0).view(torch.int64)), key
    ok = a['status'] == 0
    assert torch.equal(a['stats'][ok].view(torch.int64), b['stats'][ok].view(torch.int64))


@pytest.mark.parametrize('name', FPI)
def test_small_batch_mapping_keeps_the_two_lane_bits_on_reference_fixtures(uvs, name):
    """MCKF batches that do not fill the chip run on four lanes per filter (the EMU2 mapping, every fixed-point pass in-kernel) and
    return the two-lane kernel's bits -- on the reference's own runs that iterate, skip and FAIL."""
    import ctypes as C
    import torch
    g = load_golden(name)
    k = len(g['t'])
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    T = 70
    q0, nz = _cuda(np.tile(g['q_start'], (T, 1))), _cuda(np.repeat(g['noise_full'][:, :, None], T, axis=2))
    fp0, fp2 = _fp(uvs, g, 0), _fp(uvs, g, 2)
    assert uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp0), C.byref(plant), T) == 4 and uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp2), C.byref(plant), T) == 2
    a = uvs.engine.closed_loop(fp2, plant, q0, nz, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
    b = uvs.engine.closed_loop(fp0, plant, q0, nz, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
    _same_bits(torch, a, b, a['x'].shape[0], ('x', 'err', 'q', 'f', 'dq'))
    assert b['status'].cpu().tolist() == [int(g['status'])] * T and b['k_done'].cpu().tolist() == [k] * T
    if int(g['status']) == 0:
        for key in ('x_final', 'p_final'):
            assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), key


@pytest.mark.parametrize('thr,cap', [(1e-3, 1000), (1e-4, 3), (0.1, 1000), (1e-2, 1), (1e-6, 40)])
def test_small_batch_mapping_keeps_the_two_lane_bits_on_mixed_batches(uvs, thr, cap):
    """150 trials of mixed temper (16 per wavefront on four lanes: several filters of a wavefront iterate at the same step, more than one round of
    eight slots included at the tight thresholds), iterating up to 40 passes: status, k_done, X / err / q and the statistics bit for bit."""
    import torch
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 150, 90
    q0, noise = _mixed_batch(np.random.default_rng(77), T, K)
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    outs = []
    for lanes in (2, 0):
        fp = uvs.engine.make_params(8, 6, 'MCKF', 10.0, False, 0.05, 15.0, 0.2, desired, True, lanes, K, thr, cap)
        outs.append(uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('x', 'err', 'q')))
    _same_bits(torch, outs[0], outs[1], K)


# ---------------------------------------------------------------------------------------------- segmented trials (uvs_rmckf_closed_loop_ws_f64)
def _seg_fp(uvs, base, segments):
    fp = type(base).from_buffer_copy(base)
    fp.reserved = segments << 8
    return fp


@pytest.mark.parametrize('segments', [2, 3, 8, 16])
@pytest.mark.parametrize('name', FPI)
def test_segmented_trials_equal_whole_trials_on_reference_fixtures(uvs, name, segments):
    """A trial cut into work items whose state crosses HBM is the same arithmetic: status, k_done and every stream bit for
    bit, on the reference's own MCKF runs that iterate, skip and FAIL -- and still within the fixture's gate."""
    import torch
    g = load_golden(name)
    k = len(g['t'])
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    T = 70                                                                    # three wavefronts, the last one ragged
    q0, nz = _cuda(np.tile(g['q_start'], (T, 1))), _cuda(np.repeat(g['noise_full'][:, :, None], T, axis=2))
    base = _fp(uvs, g)
    whole = uvs.engine.closed_loop(_seg_fp(uvs, base, 1), plant, q0, nz, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
    assert uvs.engine.workspace(_seg_fp(uvs, base, 1), plant, T, 'cuda') == (None, 0)
    fp = _seg_fp(uvs, base, segments)
    ptr, nbytes = uvs.engine.workspace(fp, plant, T, 'cuda')
    assert ptr is not None and nbytes >= 3 * 64 * 8 * 100
    cut = uvs.engine.closed_loop(fp, plant, q0, nz, want=('x', 'err', 'q', 'f', 'dq'), final_state=True)
    assert torch.equal(whole['status'], cut['status']) and torch.equal(whole['k_done'], cut['k_done'])
    assert cut['status'].cpu().tolist() == [int(g['status'])] * T and cut['k_done'].cpu().tolist() == [k] * T
    for key in ('x', 'err', 'q', 'f', 'dq'):
        assert torch.equal(whole[key][:k].view(torch.int64), cut[key][:k].view(torch.int64)), key
    assert torch.equal(whole['stats'].view(torch.int64), cut['stats'].view(torch.int64))
    if int(g['status']) == 0:
        for key in ('x_final', 'p_final'):
            assert torch.equal(whole[key].view(torch.int64), cut[key].view(torch.int64)), key
    assert rel_err(cut['err'].cpu().numpy()[:k, :, 0], g['err']) <= TOL.get(name, 1e-8)


@pytest.mark.parametrize('thr,cap,segments', [(1e-3, 1000, 4), (1e-4, 3, 7), (0.1, 1000, 2)])
def test_segmented_mixed_batch_is_bit_identical(uvs, thr, cap, segments):
    """150 trials of mixed temper (iterating, skipping, FAILing at different steps -- also inside a segment and right at its edges):
    the segmented launch reproduces the whole-trial launch bit for bit, rows at and after k_done excepted (unspecified)."""
    import torch
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 150, 90
    q0, noise = _mixed_batch(np.random.default_rng(77), T, K)
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    outs = []
    for n in (1, segments):
        fp = uvs.engine.make_params(8, 6, 'MCKF', 10.0, False, 0.05, 15.0, 0.2, desired, True, 0, K, thr, cap)
        fp.reserved = n << 8
        outs.append(uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('x', 'err', 'q')))
    a, b = outs
    assert torch.equal(a['status'], b['status']) and torch.equal(a['k_done'], b['k_done']) and int((a['status'] == 1).sum()) >= (3 if cap > 1 else 0)
    live = torch.arange(K, device='cuda')[:, None, None] < a['k_done'][None, None, :]
    for key in ('x', 'err', 'q'):
        assert torch.equal(torch.where(live, a[key], 0.0).view(torch.int64), torch.where(live, b[key], 0.0).view(torch.int64)), key
    ok = a['status'] == 0
    assert torch.equal(a['stats'][ok].view(torch.int64), b['stats'][ok].view(torch.int64))


@pytest.mark.parametrize('method,segments', [('MCKF', 4), ('GMCKF', 3), ('GMCKF', 9), ('MCKF', 16)])
def test_lost_hand_over_falls_back_to_recomputation(uvs, method, segments):
    """The hand-over relies on in-order workgroup dispatch; if a predecessor's counter never arrives, a later segment recomputes the trial from
    step 0 after its spin budget (~65 ms, csrc/rmckf_device.hpp kSegSpinMax) -- never a hang.  UVS_OPT_DIAG_DROP_SEG_FLAG withholds every chunk's
    first counter: the launch must still finish promptly and reproduce the whole-trial launch bit for bit -- also when many items of a chunk fall
    back at once (9 / 16 segments: round 4's fallback let them race for the chunk's state slot, found by tools/fuzz_long.py)."""
    import time
    import torch
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 150, (90 if segments < 10 else 140)
    q0, noise = _mixed_batch(np.random.default_rng(78), T, K)
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    outs = []
    for n, drop in ((1, 0), (segments, 0), (segments, 4)):
        fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True, 2, K, 1e-3, 1000)
        fp.reserved = (n << 8) | drop
        assert uvs.lib().uvs_rmckf_closed_loop_segments(fp, plant, T) == n
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs.append(uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('x', 'err', 'q')))
        torch.cuda.synchronize()
        outs[-1]['wall'] = time.perf_counter() - t0
        outs[-1]['fallbacks'] = uvs.engine.hand_over_fallbacks(fp, plant, T)
        named = uvs.engine.hand_over_fallbacks(fp, plant, T, device=torch.device('cuda'))    # 'cuda' is the workspace of the current 'cuda:N'
        assert named == outs[-1]['fallbacks'] and (n == 1 or isinstance(named, int)), (named, outs[-1]['fallbacks'])
    a, b, c = outs
    # the launch counts the items that fell back (uvs_rmckf_closed_loop_fallback_offset): none on a healthy launch, every later segment of every
    # chunk when the first counter is withheld (an item that fell back hands nothing over, so its successors fall back too)
    chunks = (2 * T + 63) // 64
    assert a['fallbacks'] is None and b['fallbacks'] == 0 and c['fallbacks'] == chunks * (segments - 1), (a['fallbacks'], b['fallbacks'], c['fallbacks'])
    assert c['wall'] > 0.03, 'the diagnostic bit did not take the fallback (a hand-over that waits out its budget lasts > 30 ms)'
    assert c['wall'] < 2.0, 'fallback after the spin budget must come within a watchdog\'s patience'
    live = torch.arange(K, device='cuda')[:, None, None] < a['k_done'][None, None, :]
    for other in (b, c):
        assert torch.equal(a['status'], other['status']) and torch.equal(a['k_done'], other['k_done'])
        for key in ('x', 'err', 'q'):
            assert torch.equal(torch.where(live, a[key], 0.0).view(torch.int64), torch.where(live, other[key], 0.0).view(torch.int64)), key
        ok = a['status'] == 0
        assert torch.equal(a['stats'][ok].view(torch.int64), other['stats'][ok].view(torch.int64))


def test_workspace_too_small_or_absent_runs_whole_trials(uvs):
    """The workspace is an offer: NULL or too small simply runs unsegmented (same bits); a misaligned pointer is an argument error."""
    import ctypes as C
    import torch
    import bench
    desired = bench.config2()['experiments']['desired_f']
    T, K = 64, 40
    q0, noise = _mixed_batch(np.random.default_rng(3), T, K)
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    fp = uvs.engine.make_params(8, 6, 'MCKF', 10.0, False, 0.05, 15.0, 0.2, desired, True, 0, K, 1e-3, 1000)
    fp.reserved = 4 << 8
    need = int(uvs.lib().uvs_rmckf_closed_loop_workspace_bytes(C.byref(fp), C.byref(plant), T))
    assert need > 0
    ref = uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise.transpose(1, 2, 0)), want=('err',))
    qd, nd = _cuda(q0), _cuda(noise.transpose(1, 2, 0))
    NV = uvs._lib.NULL_VIEW
    flat = lambda t: uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))          # noqa: E731
    buf = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    for ws, nbytes, want_rc in ((None, 0, 0), (buf.data_ptr(), need - 1, 0), (buf.data_ptr() + 4, need, -1), (buf.data_ptr() + 8, need, 0)):
        err = uvs.engine.alloc_stream(T, K, 8)
        stats, status, k_done = torch.zeros((T, 3), dtype=torch.float64, device='cuda'), torch.zeros(T, dtype=torch.int32, device='cuda'), torch.zeros(T, dtype=torch.int32, device='cuda')
        rc = uvs.lib().uvs_rmckf_closed_loop_ws_f64(C.byref(fp), C.byref(plant), T, flat(qd), uvs.engine.stream_view(nd), NV, NV, uvs.engine.stream_view(err), NV, NV, NV,
                                                    stats.data_ptr(), status.data_ptr(), k_done.data_ptr(), NV, NV, ws, nbytes, None)
        torch.cuda.synchronize()
        assert rc == want_rc
        if rc == 0:
            assert torch.equal(k_done, ref['k_done']) and torch.equal(status, ref['status'])
            live = torch.arange(K, device='cuda')[:, None, None] < k_done[None, None, :]
            assert torch.equal(torch.where(live, err, 0.0).view(torch.int64), torch.where(live, ref['err'], 0.0).view(torch.int64))
