"""The calibrated IBVS baseline through pixels on the device (uvs_camera_analytical_step_f64, uvs_camera_analytical_loop_f64;
engine.camera_analytical_step, engine.camera_closed_loop with fp.method == ANALYTICAL) against numpy (tests/camera_analytical_ref.py) and
against itself: the one launch against the stepwise loop.

Gates.  J against numpy: 1e-10 of max |J|, the project's gate for Jacobians.  err: the bits of f - desired.  dq against numpy's pinv: 1e-8
of max |dq|, the project's closed-loop gate (cond(J) at these poses is 23-39 at four points, 26-34 at three, 1.2 at one).  One launch
against K x (camera features, analytical step): every specified row of every log (q, f for k <= k_done; dq, err for k < k_done), stats,
status, k_done and pixels, bit for bit -- both kernels form every value through the same device functions in the same order, compiled with
-ffp-contract=off.  Against the numpy loop through pixels: 1e-8 relative, with exact status, k_done and masks."""
import os

import numpy as np
import pytest

import camera_analytical_ref as ref
import camera_common as cc
from conftest import rel_err as rel

pytestmark = pytest.mark.gpu

DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
DT, GAIN = 0.05, 0.2
# the poses of tests/test_gpu_camera.py, chosen there on the CPU with the numpy oracle through pixels
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
# Under the calibrated law the estimator tests' leaving pose stays in view for all 12 steps.  This one sees no disc at all: joint 4 of
# Q_HOST_ROUTE[0] turned by 0.9 rad; every mask is empty at step 0 (checked on the CPU restatement below).
Q_BLIND = Q_HOST_ROUTE[0] + np.array([0.0, 0.0, 0.0, 0.0, 0.9, 0.0])
LOGS = ('err', 'q', 'f', 'dq')
G, SMALL = 4, 256                                                    # trials per workgroup of the four-trial form; the last one-trial batch


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    uvs_amd.lib()
    uvs_amd._vision.lib()
    return uvs_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """int64 view of an fp64 tensor / array on the host: equality of bits, NaN payloads included."""
    a = t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64)


def params(uvs, K, m=8, strict=False):
    fp = uvs.engine.make_params(m, 6, 'ANALYTICAL', 10.0, False, DT, DT * (K + 0.5), GAIN, DESIRED[:m])
    assert fp.steps == K and fp.method == 1
    if strict:
        fp.reserved = uvs._lib.UVS_OPT_STRICT_PINV
    return fp


def plant_of(uvs, n_points):
    return uvs.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))


def jittered(T, seed):
    """T start poses: Q_HOST_ROUTE[0] plus a seeded jitter of +-0.05 rad."""
    return Q_HOST_ROUTE[0] + np.random.default_rng(seed).uniform(-0.05, 0.05, (T, 6))


def assert_same_bits(got, want, K, where, trials=None, want_trials=None):
    """Every specified value of ``got`` equals that of ``want`` bit for bit; ``trials`` / ``want_trials`` pair up the trials to compare."""
    import torch
    T = got['status'].shape[0]
    trials = list(range(T)) if trials is None else trials
    want_trials = trials if want_trials is None else want_trials
    k_done = got['k_done'].cpu().numpy()
    assert np.array_equal(k_done[trials], want['k_done'].cpu().numpy()[want_trials]), (where, 'k_done')
    assert torch.equal(got['status'].cpu()[trials], want['status'].cpu()[want_trials]), (where, 'status')
    assert torch.equal(got['pixels'].cpu()[trials], want['pixels'].cpu()[want_trials]), (where, 'pixels')
    assert np.array_equal(bits(got['stats'])[trials], bits(want['stats'])[want_trials]), (where, 'stats')
    for key in LOGS:
        if key not in got:
            continue
        a, b = bits(got[key]), bits(want[key])
        assert a.shape[0] == K and a.shape[2] == b.shape[2], (where, key)
        for t, tw in zip(trials, want_trials):
            rows = min(K, k_done[t] + 1) if key in ('q', 'f') else k_done[t]
            assert np.array_equal(a[:rows, t], b[:rows, tw]), (where, key, t)


def both_routes(uvs, fp, plant, q0, noise):
    fused = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True)
    stepwise = uvs.engine.camera_closed_loop(fp, plant, q0, noise)
    return fused, stepwise


# ------------------------------------------------------------------------------------------------------------- 1: the step against numpy
@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_step_against_numpy(uvs, n_points, strict):
    import torch
    T, m = 33, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, 1, m, strict)
    q_host = jittered(T, 1000 + T)
    q = dev(q_host)
    f = uvs.engine.camera_features(plant, q) + dev(np.random.default_rng(n_points).standard_normal((T, m)) * 0.5)
    j = torch.full((T, m * 6), 7.0, dtype=torch.float64, device='cuda')
    dq, err, status = uvs.engine.camera_analytical_step(plant, q, f, fp, j=j)
    torch.cuda.synchronize()
    f_host = f.cpu().numpy()
    assert status.tolist() == [0] * T
    assert np.array_equal(bits(err), bits(f_host - DESIRED[:m])), 'err is not f - desired'
    robot = uvs.SyntheticRobot(plant, DT)
    worst_j, worst_dq, conds = 0.0, 0.0, []
    for t in range(T):
        J, _, want = ref.step(plant, robot, q_host[t], f_host[t], DESIRED, GAIN)
        conds.append(np.linalg.cond(J))
        worst_j = max(worst_j, float(np.abs(j[t].cpu().numpy().reshape(m, 6) - J).max() / np.abs(J).max()))
        worst_dq = max(worst_dq, float(np.abs(dq[t].cpu().numpy() - want).max() / np.abs(want).max()))
    print(f'analytical step, {n_points} points, strict={strict}: worst |dJ| / max |J| {worst_j:.3e}, worst |ddq| / max |dq| {worst_dq:.3e}, '
          f'cond(J) {min(conds):.1f} .. {max(conds):.1f}')
    assert worst_j < 1e-10
    assert worst_dq < 1e-8
    # without j_out: the same bits
    dq2, err2, status2 = uvs.engine.camera_analytical_step(plant, q, f, fp)
    assert np.array_equal(bits(dq2), bits(dq)) and np.array_equal(bits(err2), bits(err)) and status2.tolist() == [0] * T
    # a NaN feature pair: that trial FAILs, its err and J are still written, and its neighbours keep their bits
    for victim in (0, 16, T - 1):
        f_nan = f.clone()
        f_nan[victim, m - 2:] = float('nan')
        j_nan = torch.full((T, m * 6), 7.0, dtype=torch.float64, device='cuda')
        dq_nan, err_nan, status_nan = uvs.engine.camera_analytical_step(plant, q, f_nan, fp, j=j_nan)
        others = [t for t in range(T) if t != victim]
        assert status_nan.tolist() == [int(t == victim) for t in range(T)]
        assert np.array_equal(bits(dq_nan)[others], bits(dq)[others]) and np.array_equal(bits(err_nan)[others], bits(err)[others])
        assert np.array_equal(bits(j_nan)[others], bits(j)[others])
        assert bool(torch.isnan(err_nan[victim, m - 2:]).all()) and bool(torch.isnan(j_nan[victim]).any()) and not bool((j_nan[victim] == 7.0).any())
        assert np.array_equal(bits(err_nan)[victim, :m - 2], bits(err)[victim, :m - 2])


# ------------------------------------------------------------------------------------------------------------- 2: one launch = stepwise
@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('variant', ['', 'no noise', 'strict'])
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_one_launch_is_the_stepwise_loop(uvs, n_points, variant, T):
    import torch
    K, m = 12, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, K, m, variant == 'strict')
    q0 = dev(np.concatenate([Q_HOST_ROUTE, jittered(T - 2, 7)]))
    noise = None if variant == 'no noise' else dev(np.random.default_rng(100 + n_points).standard_normal((K, T, m)) * 0.5)
    fused, stepwise = both_routes(uvs, fp, plant, q0, noise)
    torch.cuda.synchronize()
    assert stepwise['k_done'].tolist() == [K] * T and fused['k_done'].tolist() == [K] * T, 'the comparison would be vacuous'
    assert all(bool(torch.isfinite(stepwise[key]).all()) and bool(torch.isfinite(fused[key]).all()) for key in LOGS + ('stats',))
    assert set(fused) == set(stepwise) == set(LOGS) | {'stats', 'status', 'k_done', 'pixels'}
    for key, comp in (('err', m), ('q', 6), ('f', m), ('dq', 6)):
        assert tuple(fused[key].shape) == (K, T, comp) and fused[key].is_contiguous()
    assert_same_bits(fused, stepwise, K, (n_points, variant, T))
    assert float(fused['dq'].abs().max()) > 0.0 and not torch.equal(fused['q'][0], fused['q'][K - 1]), 'the arm did not move'


# ------------------------------------------------------------------------------------------------------------- 3: batch boundaries
@pytest.mark.parametrize('n_points,T', [(4, 1), (4, G - 1), (4, G), (4, G + 1), (4, 17), (4, SMALL), (4, SMALL + 1), (4, SMALL + G - 1),
                                        (4, SMALL + G), (1, 65), (1, SMALL + 2)])
def test_batch_sizes_around_every_boundary(uvs, n_points, T):
    """One, a few and many workgroups; batch sizes at which the step kernel gets padding lanes and a second wavefront; the last batch of the
    one-trial form and the first of the four-trial form, whose last workgroup then has three, one or no padding wavefronts."""
    K, m = 6, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, K, m)
    q0 = dev(jittered(T, 1000 + T))
    noise = dev(np.random.default_rng(T).standard_normal((K, T, m)) * 0.5)
    fused, stepwise = both_routes(uvs, fp, plant, q0, noise)
    assert stepwise['k_done'].tolist() == [K] * T
    assert_same_bits(fused, stepwise, K, (n_points, T))


# ------------------------------------------------------------------------------------------------------------- 4: a failing neighbour
@pytest.mark.parametrize('T,blind,poisoned', [(18, (5,), (17,)), (SMALL + G + 2, (G - 1, SMALL + G + 1), (5,)), (SMALL + G + 2, (5,), (G - 1, SMALL + G + 1))])
def test_a_failing_trial_stops_alone(uvs, T, blind, poisoned):
    """Trials that FAIL next to trials that run on, in the same workgroup and the same control wavefront -- in the four-trial form at the last
    index of the first workgroup, inside the second, and as the last trial next to padding.  ``blind`` trials start where no disc is in view:
    four NaN pairs, FAIL at step 0.  ``poisoned`` trials get a NaN in one component of their noise row of step 5: FAIL at step 5."""
    import torch
    K = 12
    plant = plant_of(uvs, 4)
    fp = params(uvs, K)
    q_host = jittered(T, 300 + T)
    q_host[list(blind)] = Q_BLIND
    noise_host = np.random.default_rng(T).standard_normal((K, T, 8)) * 0.3
    for t in poisoned:
        noise_host[5, t, 3] = np.nan
    q0, noise = dev(q_host), dev(noise_host)
    fused, stepwise = both_routes(uvs, fp, plant, q0, noise)
    torch.cuda.synchronize()
    assert_same_bits(fused, stepwise, K, ('failing', T))
    k_done, status = fused['k_done'].tolist(), fused['status'].tolist()
    for t in blind:
        assert status[t] == 1 and k_done[t] == 0 and stepwise['k_done'][t].item() == 0
        assert bool(torch.isnan(fused['f'][0, t]).all()) and fused['pixels'][t].tolist() == [0, 0, 0, 0]
    for t in poisoned:
        assert status[t] == 1 and k_done[t] == 5 and stepwise['k_done'][t].item() == 5
        f_last = fused['f'][5, t]
        assert bool(torch.isnan(f_last[3])) and int(torch.isnan(f_last).sum()) == 1 and fused['pixels'][t].min().item() >= 50
    failing = set(blind) | set(poisoned)
    others = [t for t in range(T) if t not in failing]
    assert all(k_done[t] == K and status[t] == 0 for t in others)
    without = uvs.engine.camera_closed_loop(fp, plant, q0[others].contiguous(), noise[:, others].contiguous(), fused=True)
    assert_same_bits(fused, without, K, ('without the failing trials', T), trials=others, want_trials=list(range(len(others))))
    assert bool(torch.isfinite(fused['stats']).all()) and bool(torch.isfinite(stepwise['stats']).all())


# ------------------------------------------------------------------------------------------------------------- 5: optional outputs
@pytest.mark.parametrize('T', [5, SMALL + 5])
def test_logs_are_optional_and_one_step_works(uvs, T):
    import torch
    K = 12
    plant = plant_of(uvs, 4)
    fp = params(uvs, K)
    q_host = jittered(T, 44)
    q_host[2] = Q_BLIND
    q0 = dev(q_host)
    noise = dev(np.random.default_rng(4).standard_normal((K, T, 8)) * 0.1)
    full = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True)
    bare = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True, want=())
    assert set(bare) == {'stats', 'status', 'k_done', 'pixels'} and full['status'].tolist()[2] == 1
    assert_same_bits(bare, full, K, 'want=()')
    some = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True, want=('err', 'dq'))
    assert set(some) == {'err', 'dq', 'stats', 'status', 'k_done', 'pixels'}
    assert_same_bits(some, full, K, "want=('err', 'dq')")
    assert set(uvs.engine.camera_closed_loop(fp, plant, q0, noise, want=('q',))) == {'q', 'stats', 'status', 'k_done', 'pixels'}
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True, want=('kappa',))
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True, guess='device')
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=torch.zeros((T, 48), dtype=torch.float64, device='cuda'))
    one, stepwise = both_routes(uvs, params(uvs, 1), plant, q0, noise[:1].contiguous())
    torch.cuda.synchronize()
    assert_same_bits(one, stepwise, 1, 'K = 1')
    assert one['k_done'].tolist() == [int(t != 2) for t in range(T)]


# ------------------------------------------------------------------------------------------------------------- 6: the numpy loop through pixels
def test_one_launch_against_the_numpy_loop_through_pixels(uvs):
    """Each trial of one launch against tests/camera_analytical_ref.run: numpy rasteriser, numpy detector, analytic_guess as J, numpy's pinv."""
    import torch
    T, K = 2, 20
    plant = uvs.SyntheticPlant.ur10()
    noise = np.random.default_rng(20).standard_normal((K, T, 8)) * 0.3
    out = uvs.engine.camera_closed_loop(params(uvs, K), plant, dev(Q_HOST_ROUTE), dev(noise), fused=True)
    pix_d = torch.zeros((K * T, 4), dtype=torch.int32, device='cuda')
    uvs.engine.camera_features(plant, out['q'].reshape(K * T, 6), pixels=pix_d)
    pixels = pix_d.cpu().numpy().reshape(K, T, 4)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0]
    for t in range(T):
        want = ref.run(plant, Q_HOST_ROUTE[t], noise[:, t], DESIRED, DT, GAIN, K)
        assert want['status'] == 0 and want['k_done'] == K
        # the preconditions under which a 1e-10 px projection difference cannot flip a pixel, on the numpy trajectory
        discs = want['discs']
        lo, hi = discs[:, :, :2] - discs[:, :, 2:], discs[:, :, :2] + discs[:, :, 2:]
        assert lo.min() > 0.0 and hi.max() < 255.0, 'a disc touches the edge of the frame'
        assert want['masks'].min() >= 50
        assert cc.closest_to_rim(discs) > 1e-6, "a pixel's d^2 comes within 1e-6 of r^2"
        for name in ('err', 'f', 'q'):
            got = out[name][:, t].cpu().numpy()
            print(f'trial {t} {name}: rel {rel(got, want[name]):.3e}')
            assert rel(got, want[name]) < 1e-8, (t, name)
        assert np.array_equal(pixels[:, t], want['masks']), 'mask sizes differ at some step'
        assert np.array_equal(out['pixels'][t].cpu().numpy(), want['masks'].min(axis=0))
        print(f'trial {t} stats: rel {rel(out["stats"][t].cpu().numpy(), want["stats"]):.3e}')
