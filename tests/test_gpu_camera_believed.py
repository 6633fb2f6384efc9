"""The calibrated IBVS baseline on a per-trial believed model, on the device (uvs_camera_believed_step_f64, uvs_camera_believed_loop_f64,
uvs_camera_believed_guess_f64; the ``believed=`` / ``believed_index=`` arguments of engine.camera_analytical_step, camera_guess and
camera_closed_loop) against the calibrated kernels, against numpy (tests/camera_believed_ref.py) and against itself.

Gates, those of tests/test_gpu_camera_analytical.py.  With the true model as the believed one: the bits of the calibrated kernels (the same
device function on the same operands, -ffp-contract=off).  J against numpy: 1e-10 of max |J|.  err: the bits of f - desired.  dq against
numpy's pinv: 1e-8 of max |dq|, under cond(J) <= 100 of the numpy matrices compared against (asserted; measured on the CPU with the wrong
models below: at most 90 at four and three points, about 1.3 at one).  One launch against K x (camera features on the true camera, believed
step): every specified value bit for bit.  The analytic guess: 1e-10 of max |X0|.  Against the numpy loop through pixels: 1e-8 relative, with
exact status, k_done and masks."""
import ctypes

import numpy as np
import pytest

import camera_believed_ref as ref
import camera_common as cc
from conftest import rel_err as rel
from test_gpu_camera_analytical import (DESIRED, DT, G, GAIN, Q_BLIND, Q_HOST_ROUTE, SMALL, assert_same_bits, bits, dev, jittered, params, plant_of,
                                        uvs)  # noqa: F401  (uvs: the module fixture)

pytestmark = pytest.mark.gpu

JOINT_OFFSETS = (0.03, -0.02, 0.04, -0.03, 0.02, 0.1)
COMBINATION = 6                                                      # its place in wrong_plants
FIVE = (0, 2, 4, 5, COMBINATION)                                     # one of each kind


def wrong_plants(uvs, plant):
    mis = uvs.plant.miscalibrated
    return [mis(plant, focal_scale=0.8), mis(plant, focal_scale=1.25), mis(plant, point_offset=(0.0, 0.0, -0.3)), mis(plant, point_offset=(0.0, 0.0, 0.2)),
            mis(plant, joint_offset=JOINT_OFFSETS), mis(plant, link_scale=1.05),
            mis(plant, focal_scale=1.2, point_offset=(0.05, -0.05, -0.2), joint_offset=JOINT_OFFSETS, link_scale=0.97)]


def mixed(T, n_models, seed=0):
    """An index that uses every model and puts different ones next to each other, inside one workgroup and one control wavefront."""
    index = (np.arange(T) * 3 + seed) % n_models
    return index.astype(np.int32)


def loop(uvs, fp, plant, q0, noise, fused, **kw):
    return uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=fused, **kw)


# ------------------------------------------------------------------------------------------------------------- 1: the true model
def true_forms(uvs, plant, T):
    """The true model as the believed one: one struct, T copies, and through an index into an array that holds wrong ones too."""
    wrong = wrong_plants(uvs, plant)
    return (('one struct', dict(believed=uvs.engine.believed_models(plant))),
            ('T copies', dict(believed=uvs.engine.believed_models([plant] * T))),
            ('an index', dict(believed=uvs.engine.believed_models([wrong[0], plant, wrong[COMBINATION]]), believed_index=np.ones(T, np.int32))))


@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_true_model_step_and_guess_have_the_calibrated_bits(uvs, n_points, strict):
    import torch
    T, m = 33, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, 1, m, strict)
    q = dev(jittered(T, 1000 + T))
    f0 = uvs.engine.camera_features(plant, q)
    f = f0 + dev(np.random.default_rng(n_points).standard_normal((T, m)) * 0.5)
    j = torch.full((T, m * 6), 7.0, dtype=torch.float64, device='cuda')
    dq, err, status = uvs.engine.camera_analytical_step(plant, q, f, fp, j=j)
    x0 = uvs.engine.camera_guess(plant, q, f0)
    assert status.tolist() == [0] * T
    for name, kw in true_forms(uvs, plant, T):
        j2 = torch.full((T, m * 6), 7.0, dtype=torch.float64, device='cuda')
        dq2, err2, status2 = uvs.engine.camera_analytical_step(plant, q, f, fp, j=j2, **kw)
        assert status2.tolist() == [0] * T, name
        for got, want, what in ((dq2, dq, 'dq'), (err2, err, 'err'), (j2, j, 'J')):
            assert np.array_equal(bits(got), bits(want)), (name, what)
        dq3, err3, _ = uvs.engine.camera_analytical_step(plant, q, f, fp, **kw)         # without j_out: the same bits
        assert np.array_equal(bits(dq3), bits(dq)) and np.array_equal(bits(err3), bits(err)), name
        assert np.array_equal(bits(uvs.engine.camera_guess(plant, q, f0, **kw)), bits(x0)), (name, 'guess')


@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('variant', ['', 'no noise', 'strict'])
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_true_model_loops_have_the_calibrated_bits(uvs, n_points, variant, T):
    import torch
    K, m = 12, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, K, m, variant == 'strict')
    q0 = dev(np.concatenate([Q_HOST_ROUTE, jittered(T - 2, 7)]))
    noise = None if variant == 'no noise' else dev(np.random.default_rng(100 + n_points).standard_normal((K, T, m)) * 0.5)
    calibrated = {fused: loop(uvs, fp, plant, q0, noise, fused) for fused in (True, False)}
    assert calibrated[True]['k_done'].tolist() == [K] * T, 'the comparison would be vacuous'
    for name, kw in true_forms(uvs, plant, T):
        for fused in (True, False):
            got = loop(uvs, fp, plant, q0, noise, fused, **kw)
            torch.cuda.synchronize()
            assert set(got) == set(calibrated[fused])
            assert_same_bits(got, calibrated[fused], K, (n_points, variant, T, name, fused))


# ------------------------------------------------------------------------------------------------------------- 2: the step against numpy
@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_step_against_numpy_on_wrong_models(uvs, n_points, strict):
    import torch
    T, m = 33, 2 * n_points
    plant = plant_of(uvs, n_points)
    models = wrong_plants(uvs, plant)
    index = mixed(T, len(models))
    fp = params(uvs, 1, m, strict)
    q_host = jittered(T, 1000 + T)
    q = dev(q_host)
    f = uvs.engine.camera_features(plant, q) + dev(np.random.default_rng(n_points).standard_normal((T, m)) * 0.5)   # detected on the TRUE camera
    j = torch.full((T, m * 6), 7.0, dtype=torch.float64, device='cuda')
    dq, err, status = uvs.engine.camera_analytical_step(plant, q, f, fp, j=j, believed=models, believed_index=index)
    torch.cuda.synchronize()
    f_host = f.cpu().numpy()
    assert status.tolist() == [0] * T
    assert np.array_equal(bits(err), bits(f_host - DESIRED[:m])), 'err is not f - desired'
    robots = [uvs.SyntheticRobot(model, DT) for model in models]
    worst_j, worst_dq, conds = 0.0, 0.0, []
    for t in range(T):
        J, _, want = ref.step(models[index[t]], robots[index[t]], q_host[t], f_host[t], DESIRED, GAIN)
        conds.append(np.linalg.cond(J))
        worst_j = max(worst_j, float(np.abs(j[t].cpu().numpy().reshape(m, 6) - J).max() / np.abs(J).max()))
        worst_dq = max(worst_dq, float(np.abs(dq[t].cpu().numpy() - want).max() / np.abs(want).max()))
    print(f'believed step, {n_points} points, strict={strict}: worst |dJ| / max |J| {worst_j:.3e}, worst |ddq| / max |dq| {worst_dq:.3e}, '
          f'cond(J) {min(conds):.1f} .. {max(conds):.1f}')
    assert max(conds) <= 100.0, 'the precondition of the 1e-8 gate'
    assert worst_j < 1e-10
    assert worst_dq < 1e-8
    # the wrong models are wrong: the calibrated step commands something else from the same frame
    dq_true, _, _ = uvs.engine.camera_analytical_step(plant, q, f, fp)
    assert float((dq_true - dq).abs().max() / dq_true.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------- 3: one launch = stepwise
@pytest.mark.parametrize('n_points,T', [(4, 1), (4, G - 1), (4, G), (4, G + 1), (4, 17), (4, SMALL), (4, SMALL + 1), (4, SMALL + G - 1), (4, SMALL + G),
                                        (3, G + 1), (3, SMALL + 1), (1, 65), (1, SMALL + 2)])
def test_one_launch_is_the_stepwise_loop_on_wrong_models(uvs, n_points, T):
    """Models mixed through an index over one, a few and many workgroups; the batch sizes of the calibrated test around every boundary."""
    import torch
    K, m = 12, 2 * n_points
    plant = plant_of(uvs, n_points)
    believed = uvs.engine.believed_models(wrong_plants(uvs, plant))
    index = dev(mixed(T, believed.shape[0], seed=T))                 # a device index: passed on as it is
    fp = params(uvs, K, m)
    q0 = dev(jittered(T, 1000 + T))
    noise = dev(np.random.default_rng(T).standard_normal((K, T, m)) * 0.5)
    kw = dict(believed=believed, believed_index=index)
    fused, stepwise = (loop(uvs, fp, plant, q0, noise, f, **kw) for f in (True, False))
    torch.cuda.synchronize()
    assert stepwise['k_done'].tolist() == [K] * T and fused['k_done'].tolist() == [K] * T, 'the comparison would be vacuous'
    assert_same_bits(fused, stepwise, K, (n_points, T))
    calibrated = loop(uvs, fp, plant, q0, noise, True)
    assert not np.array_equal(bits(fused['dq'][0]), bits(calibrated['dq'][0])), 'the wrong models changed nothing'
    if T in (G + 1, SMALL + G - 1):                                  # optional logs, and a single step, in both forms of the kernel
        bare = loop(uvs, fp, plant, q0, noise, True, want=(), **kw)
        assert set(bare) == {'stats', 'status', 'k_done', 'pixels'}
        assert_same_bits(bare, fused, K, 'want=()')
        some = loop(uvs, fp, plant, q0, noise, True, want=('err', 'dq'), **kw)
        assert set(some) == {'err', 'dq', 'stats', 'status', 'k_done', 'pixels'}
        assert_same_bits(some, fused, K, "want=('err', 'dq')")
        fp1 = params(uvs, 1, m)
        one, one_stepwise = (loop(uvs, fp1, plant, q0, noise[:1].contiguous(), f, **kw) for f in (True, False))
        assert one['k_done'].tolist() == [1] * T
        assert_same_bits(one, one_stepwise, 1, 'K = 1')
        assert np.array_equal(bits(one['dq'][0]), bits(fused['dq'][0]))


# ------------------------------------------------------------------------------------------------------------- 4: a trial's model is its own
def test_a_trials_model_is_its_own(uvs):
    K, T = 12, SMALL + 3
    plant = plant_of(uvs, 4)
    wrong = wrong_plants(uvs, plant)
    models = [wrong[i] for i in FIVE]
    index = mixed(T, len(models))
    fp = params(uvs, K)
    q0 = dev(jittered(T, 77))
    noise = dev(np.random.default_rng(77).standard_normal((K, T, 8)) * 0.5)
    mix = loop(uvs, fp, plant, q0, noise, True, believed=models, believed_index=index)
    assert mix['k_done'].tolist() == [K] * T
    for i, model in enumerate(models):
        uniform = loop(uvs, fp, plant, q0, noise, True, believed=model)                  # n_believed = 1
        trials = [t for t in range(T) if index[t] == i]
        assert len(trials) >= T // len(models)
        assert_same_bits(mix, uniform, K, ('mixed against uniform', i), trials=trials)
        copies = loop(uvs, fp, plant, q0, noise, True, believed=[model] * T)             # n_believed = T, no index
        assert_same_bits(copies, uniform, K, ('T copies against one struct', i))
        others = [t for t in range(T) if index[t] != i]
        assert not np.array_equal(bits(mix['dq'][0])[others], bits(uniform['dq'][0])[others]), 'the models do not differ'


# ------------------------------------------------------------------------------------------------------------- 5: failing trials
@pytest.mark.parametrize('T,blind,poisoned', [(18, (5,), (17,)), (SMALL + G + 2, (G - 1, SMALL + G + 1), (5,)), (SMALL + G + 2, (5,), (G - 1, SMALL + G + 1))])
def test_a_failing_trial_stops_alone(uvs, T, blind, poisoned):
    """The failing cases and positions of tests/test_gpu_camera_analytical.py, with the models mixed over the batch."""
    import torch
    K = 12
    plant = plant_of(uvs, 4)
    believed = uvs.engine.believed_models(wrong_plants(uvs, plant))
    index = mixed(T, believed.shape[0])
    fp = params(uvs, K)
    q_host = jittered(T, 300 + T)
    q_host[list(blind)] = Q_BLIND
    noise_host = np.random.default_rng(T).standard_normal((K, T, 8)) * 0.3
    for t in poisoned:
        noise_host[5, t, 3] = np.nan
    q0, noise = dev(q_host), dev(noise_host)
    fused, stepwise = (loop(uvs, fp, plant, q0, noise, f, believed=believed, believed_index=index) for f in (True, False))
    torch.cuda.synchronize()
    assert_same_bits(fused, stepwise, K, ('failing', T))
    k_done, status = fused['k_done'].tolist(), fused['status'].tolist()
    for t in blind:
        assert status[t] == 1 and k_done[t] == 0
        assert bool(torch.isnan(fused['f'][0, t]).all()) and fused['pixels'][t].tolist() == [0, 0, 0, 0]
    for t in poisoned:
        assert status[t] == 1 and k_done[t] == 5
        f_last = fused['f'][5, t]
        assert bool(torch.isnan(f_last[3])) and int(torch.isnan(f_last).sum()) == 1 and fused['pixels'][t].min().item() >= 50
    failing = set(blind) | set(poisoned)
    others = [t for t in range(T) if t not in failing]
    assert all(k_done[t] == K and status[t] == 0 for t in others)
    without = loop(uvs, fp, plant, q0[others].contiguous(), noise[:, others].contiguous(), True, believed=believed, believed_index=index[others])
    assert_same_bits(fused, without, K, ('without the failing trials', T), trials=others, want_trials=list(range(len(others))))
    assert bool(torch.isfinite(fused['stats']).all())


@pytest.mark.parametrize('T,outside', [(18, (5, 17)), (SMALL + G + 2, (G - 1, 5, SMALL + G + 1))])
def test_an_index_that_names_no_model_fails_its_trial_alone(uvs, T, outside):
    """Index values -1 and n_believed, on the device, through the C entry points (the Python layer would refuse them on the host): FAIL with
    k_done = 0 in the loop, status FAIL in the step, nothing else of theirs written, every other trial as in a launch without them."""
    import torch
    K, m, SENTINEL = 12, 8, 7.0
    plant = plant_of(uvs, 4)
    cam = plant.to_camera()
    believed = uvs.engine.believed_models(wrong_plants(uvs, plant))
    n_believed = believed.shape[0]
    index_host = mixed(T, n_believed)
    for i, t in enumerate(outside):
        index_host[t] = -1 if i % 2 == 0 else n_believed
    index = dev(index_host)
    others = [t for t in range(T) if t not in outside]
    fp = params(uvs, K)
    q0 = dev(jittered(T, 500 + T))
    noise = dev(np.random.default_rng(T).standard_normal((K, T, m)) * 0.3)
    lib = uvs._vision.lib()
    f64 = dict(dtype=torch.float64, device='cuda')
    log = {key: torch.full((K, T, comp), SENTINEL, **f64) for key, comp in (('q', 6), ('f', m), ('dq', 6), ('err', m))}
    status, k_done = (torch.full((T,), 7, dtype=torch.int32, device='cuda') for _ in range(2))
    stats = torch.full((T, 3), SENTINEL, **f64)
    pixels = torch.full((T, 4), 7, dtype=torch.int32, device='cuda')
    uvs._vision.check(lib.uvs_camera_believed_loop_f64(ctypes.byref(fp), ctypes.byref(cam), T, believed.data_ptr(), n_believed, index.data_ptr(),
                                                       q0.data_ptr(), noise.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(), log['dq'].data_ptr(),
                                                       log['err'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
                                                       pixels.data_ptr(), None))
    torch.cuda.synchronize()
    for t in outside:
        assert status[t].item() == 1 and k_done[t].item() == 0, t
        assert all(bool((log[key][:, t] == SENTINEL).all()) for key in log), (t, 'a log row was written')
        assert bool((stats[t] == SENTINEL).all()) and pixels[t].tolist() == [7] * 4, t
    got = dict(log, status=status, k_done=k_done, stats=stats, pixels=pixels)
    without = loop(uvs, fp, plant, q0[others].contiguous(), noise[:, others].contiguous(), True, believed=believed, believed_index=index_host[others])
    assert without['k_done'].tolist() == [K] * len(others)
    assert_same_bits(got, without, K, ('without the trials that have no model', T), trials=others, want_trials=list(range(len(others))))
    # the step
    q, f = log['q'][3].contiguous(), log['f'][3].contiguous()
    q[list(outside)], f[list(outside)] = q[others[0]].clone(), f[others[0]].clone()      # ordinary operands: their log rows are sentinels
    dq, err, j = (torch.full((T, comp), SENTINEL, **f64) for comp in (6, m, m * 6))
    step_status = torch.full((T,), 7, dtype=torch.int32, device='cuda')
    fp1 = params(uvs, 1)
    uvs._vision.check(lib.uvs_camera_believed_step_f64(ctypes.byref(fp1), T, believed.data_ptr(), n_believed, index.data_ptr(), q.data_ptr(), f.data_ptr(),
                                                       dq.data_ptr(), err.data_ptr(), j.data_ptr(), step_status.data_ptr(), None))
    torch.cuda.synchronize()
    assert step_status.tolist() == [int(t in outside) for t in range(T)]
    for t in outside:
        assert bool((dq[t] == SENTINEL).all()) and bool((err[t] == SENTINEL).all()) and bool((j[t] == SENTINEL).all()), t
    j2 = torch.full((len(others), m * 6), SENTINEL, **f64)
    dq2, err2, status2 = uvs.engine.camera_analytical_step(plant, q[others].contiguous(), f[others].contiguous(), fp1, j=j2, believed=believed,
                                                           believed_index=index_host[others])
    assert status2.tolist() == [0] * len(others)
    assert np.array_equal(bits(dq)[others], bits(dq2)) and np.array_equal(bits(err)[others], bits(err2)) and np.array_equal(bits(j)[others], bits(j2))
    assert np.array_equal(bits(dq)[others], bits(log['dq'][3])[others]), 'the step of the loop'
    # the guess writes nothing for them either
    x0 = torch.full((T, m * 6), SENTINEL, **f64)
    uvs._vision.check(lib.uvs_camera_believed_guess_f64(T, 4, believed.data_ptr(), n_believed, index.data_ptr(), q.data_ptr(), f.data_ptr(), x0.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool((x0[list(outside)] == SENTINEL).all()) and not bool((x0[others] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------- 6: the guess
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_guess_on_wrong_models_against_numpy(uvs, n_points):
    T, m = 33, 2 * n_points
    plant = plant_of(uvs, n_points)
    models = wrong_plants(uvs, plant)
    index = mixed(T, len(models))
    q_host = jittered(T, 1000 + T)
    q = dev(q_host)
    f0 = uvs.engine.camera_features(plant, q)                        # what the true camera shows
    x0 = uvs.engine.camera_guess(plant, q, f0, believed=models, believed_index=index).cpu().numpy()
    f_host = f0.cpu().numpy()
    worst = 0.0
    for t in range(T):
        robot = uvs.SyntheticRobot(models[index[t]], DT)
        robot.start(q_host[t])
        want = uvs.plant.analytic_guess(robot, f_host[t], (uvs.plant.RESOLUTION,) * 2, m, 6)
        worst = max(worst, float(np.abs(x0[t] - want).max() / np.abs(want).max()))
    print(f'believed guess, {n_points} points: worst |dX0| / max |X0| {worst:.3e}')
    assert worst < 1e-10
    calibrated = uvs.engine.camera_guess(plant, q, f0).cpu().numpy()
    assert float(np.abs(calibrated - x0).max() / np.abs(calibrated).max()) > 1e-3, 'the wrong models changed nothing'


@pytest.mark.parametrize('fused', [True, False])
def test_an_estimator_starts_from_the_believed_guess(uvs, fused):
    K, T = 12, 5
    plant = plant_of(uvs, 4)
    believed = uvs.engine.believed_models(wrong_plants(uvs, plant))
    index = mixed(T, believed.shape[0])
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, DT, DT * (K + 0.5), GAIN, DESIRED)
    assert fp.steps == K and fp.initial_guess
    q0 = dev(jittered(T, 9))
    noise = dev(np.random.default_rng(9).standard_normal((K, T, 8)) * 0.3)
    x0 = uvs.engine.camera_guess(plant, q0, uvs.engine.camera_features(plant, q0), believed=believed, believed_index=index)
    got = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=fused, guess='device', believed=believed, believed_index=index)
    want = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=fused, x0=x0)
    assert got['k_done'].tolist() == [K] * T and set(got) == set(want)
    for key in got:
        a, b = got[key].cpu().numpy(), want[key].cpu().numpy()
        assert np.array_equal(a.view(np.int64 if a.dtype == np.float64 else a.dtype), b.view(np.int64 if b.dtype == np.float64 else b.dtype)), key
    calibrated = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=fused, guess='device')
    assert not np.array_equal(bits(calibrated['dq'][1]), bits(got['dq'][1])), 'the wrong start changed nothing'


# ------------------------------------------------------------------------------------------------------------- 7: the numpy loop through pixels
def test_one_launch_against_the_numpy_loop_through_pixels(uvs):
    """Each trial of one launch on the combination model against tests/camera_believed_ref.run: numpy rasteriser and detector on the true plant,
    analytic_guess as J and numpy's pinv on the believed one."""
    import torch
    T, K = 2, 20
    plant = uvs.SyntheticPlant.ur10()
    combination = wrong_plants(uvs, plant)[COMBINATION]
    noise = np.random.default_rng(20).standard_normal((K, T, 8)) * 0.3
    out = loop(uvs, params(uvs, K), plant, dev(Q_HOST_ROUTE), dev(noise), True, believed=combination)
    pix_d = torch.zeros((K * T, 4), dtype=torch.int32, device='cuda')
    uvs.engine.camera_features(plant, out['q'].reshape(K * T, 6), pixels=pix_d)
    pixels = pix_d.cpu().numpy().reshape(K, T, 4)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0]
    for t in range(T):
        want = ref.run(plant, combination, Q_HOST_ROUTE[t], noise[:, t], DESIRED, DT, GAIN, K)
        assert want['status'] == 0 and want['k_done'] == K
        # the preconditions under which a 1e-10 px projection difference cannot flip a pixel, on the numpy trajectory
        discs = want['discs']
        lo, hi = discs[:, :, :2] - discs[:, :, 2:], discs[:, :, :2] + discs[:, :, 2:]
        assert lo.min() > 0.0 and hi.max() < 255.0, 'a disc touches the edge of the frame'
        assert want['masks'].min() >= 50
        assert cc.closest_to_rim(discs) > 1e-6, "a pixel's d^2 comes within 1e-6 of r^2"
        assert max(np.linalg.cond(J.reshape(8, 6)) for J in want['j']) <= 100.0
        for name in ('err', 'f', 'q', 'dq'):
            got = out[name][:, t].cpu().numpy()
            print(f'trial {t} {name}: rel {rel(got, want[name]):.3e}')
            assert rel(got, want[name]) < 1e-8, (t, name)
        assert np.array_equal(pixels[:, t], want['masks']), 'mask sizes differ at some step'
        assert np.array_equal(out['pixels'][t].cpu().numpy(), want['masks'].min(axis=0))
        print(f'trial {t} stats: rel {rel(out["stats"][t].cpu().numpy(), want["stats"]):.3e}')
