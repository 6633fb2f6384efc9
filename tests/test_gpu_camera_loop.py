"""The pixel closed loop as one launch (uvs_camera_closed_loop_f64; engine.camera_closed_loop(fused=True)) and the device guess
(uvs_camera_guess_f64; engine.camera_guess) against what the repository already has: the two-launch loop of camera_closed_loop(fused=False)
fed the same x0, and the host route of Experiment.

Gates.  One launch against two launches per step: every specified row of every log (q, f for k <= k_done; dq, err, kappa for k < k_done),
stats, status, k_done and pixels, bit for bit -- both libraries compile with -ffp-contract=off and the kernel forms every sum in the order
of the kernels it replaces.  Device guess against plant.analytic_guess: 1e-10 relative to the largest entry of X0, the project's gate for
Jacobian estimates.  Against the host route: 1e-8 relative, the project's closed-loop gate, with exact status, k_done and masks."""
import os

import numpy as np
import pytest

import camera_common as cc
from conftest import load_golden, rel_err as rel

pytestmark = pytest.mark.gpu

DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
DT = 0.05
# the poses of tests/test_gpu_camera.py, chosen there on the CPU with the numpy oracle through pixels
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
Q_LEAVES = np.array([-0.47915568, -0.55367504, 2.20583478, -0.05228325, -1.09351535, 0.40221985])     # all four discs out of view at step 6
LOGS = cc.LOGS
# The loop kernel has two forms: up to SMALL trials one trial per workgroup (four wavefronts share its colours), beyond that G trials per
# workgroup (one wavefront each).  Both forms must give the two-launch loop's bits, so the cases below come at batch sizes on both sides.
G, SMALL = 4, 256


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


bits = cc.bits


def params(uvs, method, K, initial_guess=True, m=8, annealing=False):
    return uvs.engine.make_params(m, 6, method, 10.0, annealing, DT, DT * (K + 0.5), 0.2, DESIRED[:m], initial_guess)


def plant_of(uvs, n_points):
    return uvs.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))


def jittered(T, seed):
    """T start poses: Q_HOST_ROUTE[0] plus a seeded jitter of +-0.05 rad."""
    return Q_HOST_ROUTE[0] + np.random.default_rng(seed).uniform(-0.05, 0.05, (T, 6))


def device_x0(uvs, plant, q0):
    return uvs.engine.camera_guess(plant, q0, uvs.engine.camera_features(plant, q0))


assert_same_bits = cc.assert_same_bits                            # shared with tests/test_gpu_camera_scenes.py


def both_routes(uvs, fp, plant, q0, noise, x0):
    fused = uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0, fused=True)
    oracle = uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0)
    return fused, oracle


# ------------------------------------------------------------------------------------------------------------- 1: shapes and methods
CASES = [(method, n_points, '') for method in ('GMCKF', 'KF', 'IMCCKF') for n_points in (4, 3, 1)]
CASES += [('MCKF', 4, ''), ('MCKF', 1, ''), ('GMCKF', 4, 'strict'), ('GMCKF', 4, 'annealing'), ('GMCKF', 4, 'no noise'), ('GMCKF', 3, 'no guess')]


@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('method,n_points,variant', CASES)
def test_one_launch_is_the_two_launch_loop(uvs, method, n_points, variant, T):
    import torch
    K, m = 12, 2 * n_points
    rng = np.random.default_rng(100 + n_points)
    plant = plant_of(uvs, n_points)
    fp = params(uvs, method, K, initial_guess=variant != 'no guess', m=m, annealing=variant == 'annealing')
    assert fp.steps == K
    if variant == 'strict':
        fp.reserved = uvs._lib.UVS_OPT_STRICT_PINV
    q0 = dev(np.concatenate([Q_HOST_ROUTE, jittered(T - 2, 7)]))
    noise = None if variant == 'no noise' else dev(rng.standard_normal((K, T, m)) * 0.5)
    x0 = device_x0(uvs, plant, q0)
    fused, oracle = both_routes(uvs, fp, plant, q0, noise, x0)
    torch.cuda.synchronize()
    assert oracle['k_done'].tolist() == [K] * T and bool(torch.isfinite(oracle['err']).all()), 'the comparison would be vacuous'
    for key, comp in (('err', m), ('q', 6), ('f', m), ('dq', 6), ('kappa', m)):
        assert tuple(fused[key].shape) == (K, T, comp) and fused[key].is_contiguous()
    assert_same_bits(fused, oracle, K, (method, n_points, variant))
    if variant == 'no guess':                                        # f_old of the first step is zeros
        assert np.array_equal(bits(fused['f'][0]), bits(uvs.engine.camera_features(plant, q0, noise=noise[0])))


def test_mckf_is_refused_where_it_is_not_built(uvs):
    plant = plant_of(uvs, 3)
    q0 = dev(Q_HOST_ROUTE)
    with pytest.raises(uvs.UvsError) as exc:
        uvs.engine.camera_closed_loop(params(uvs, 'MCKF', 4, m=6), plant, q0, x0=device_x0(uvs, plant, q0), fused=True)
    assert exc.value.code == -4


# ------------------------------------------------------------------------------------------------------------- 2: lane-group boundaries
@pytest.mark.parametrize('n_points,T', [(4, 1), (4, G - 1), (4, G), (4, G + 1), (4, 17), (4, 33), (3, 33), (3, 65), (1, 33), (1, 65),
                                        (4, SMALL), (4, SMALL + 1), (4, SMALL + G - 1), (4, SMALL + G), (3, SMALL + 1), (1, SMALL + 2)])
def test_batch_sizes_around_every_boundary(uvs, n_points, T):
    """One, a few and many workgroups; the batch sizes at which the two-launch loop's step kernel gets padding lanes and a second wavefront at
    4, 2 and 1 lanes per filter; the last batch of the one-trial form and the first of the four-trial form, whose last workgroup then has
    three, one or no padding wavefronts."""
    K, m = 6, 2 * n_points
    plant = plant_of(uvs, n_points)
    fp = params(uvs, 'GMCKF', K, m=m)
    q0 = dev(jittered(T, 1000 + T))
    noise = dev(np.random.default_rng(T).standard_normal((K, T, m)) * 0.5)
    fused, oracle = both_routes(uvs, fp, plant, q0, noise, device_x0(uvs, plant, q0))
    assert oracle['k_done'].tolist() == [K] * T
    assert_same_bits(fused, oracle, K, (n_points, T))


# ------------------------------------------------------------------------------------------------------------- 3: a failing neighbour
@pytest.mark.parametrize('T,leaving', [(18, (5, 17)), (G + 2, (G - 1,)), (SMALL + G + 2, (G - 1, 5, SMALL + G))])
def test_a_failing_trial_stops_alone(uvs, T, leaving):
    """Trials that leave the frame FAIL (the existing path: NaN features, non-finite X) next to trials that run on, in the same workgroup
    and the same estimator wavefront (the third case: the four-trial form, failing at the last index of the first workgroup, in the second
    one, and next to a padding wavefront in the last); the launch returns, and every other trial has the bits it has in a launch without them."""
    import torch
    K = 12
    plant = plant_of(uvs, 4)
    fp = params(uvs, 'GMCKF', K)
    q_host = jittered(T, 300 + T)
    q_host[list(leaving)] = Q_LEAVES
    q0 = dev(q_host)
    x0 = device_x0(uvs, plant, q0)
    fused, oracle = both_routes(uvs, fp, plant, q0, None, x0)
    torch.cuda.synchronize()
    assert_same_bits(fused, oracle, K, ('failing', T))
    k_done = fused['k_done'].tolist()
    for t in leaving:
        assert fused['status'][t].item() == 1 and 0 < k_done[t] < K and k_done[t] == oracle['k_done'][t].item()
        f_last = fused['f'][k_done[t], t].cpu().numpy().reshape(4, 2)
        assert any(np.all(np.isnan(pair)) for pair in f_last), 'no NaN pair at k_done'
        assert fused['pixels'][t].min().item() == 0
    others = [t for t in range(T) if t not in leaving]
    assert all(k_done[t] == K and fused['status'][t].item() == 0 for t in others)
    without = uvs.engine.camera_closed_loop(fp, plant, q0[others].contiguous(), x0=x0[others].contiguous(), fused=True)
    assert_same_bits(fused, without, K, ('without the failing trials', T), trials=others, want_trials=list(range(len(others))))
    assert bool(torch.isfinite(fused['stats']).all())


# ------------------------------------------------------------------------------------------------------------- 4: optional outputs
@pytest.mark.parametrize('T', [5, SMALL + 5])
def test_logs_are_optional_and_one_step_works(uvs, T):
    import torch
    K = 12
    plant = plant_of(uvs, 4)
    fp = params(uvs, 'GMCKF', K)
    q_host = jittered(T, 44)
    q_host[2] = Q_LEAVES
    q0 = dev(q_host)
    noise_host = np.random.default_rng(4).standard_normal((K, T, 8)) * 0.1
    noise_host[:, 2] = 0.0                                           # Q_LEAVES was found without noise: that trial shall FAIL at every T
    noise = dev(noise_host)
    x0 = device_x0(uvs, plant, q0)
    full = uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0, fused=True)
    bare = uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0, fused=True, want=())
    assert set(bare) == {'stats', 'status', 'k_done', 'pixels'} and full['status'].tolist()[2] == 1
    assert_same_bits(bare, full, K, 'want=()')
    some = uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0, fused=True, want=('err', 'dq'))
    assert set(some) == {'err', 'dq', 'stats', 'status', 'k_done', 'pixels'}
    assert_same_bits(some, full, K, "want=('err', 'dq')")
    assert set(uvs.engine.camera_closed_loop(fp, plant, q0, noise, x0=x0, want=('q',))) == {'q', 'stats', 'status', 'k_done', 'pixels'}
    fp1 = params(uvs, 'GMCKF', 1)
    assert fp1.steps == 1
    one, oracle = both_routes(uvs, fp1, plant, q0, noise[:1].contiguous(), x0)
    torch.cuda.synchronize()
    assert_same_bits(one, oracle, 1, 'K = 1')


# ------------------------------------------------------------------------------------------------------------- 5: device guess
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_device_guess(uvs, n_points):
    T, K, m = 33, 6, 2 * n_points
    plant = plant_of(uvs, n_points)
    q_host = jittered(T, 1000 + T)
    q0 = dev(q_host)
    f0 = uvs.engine.camera_features(plant, q0)
    got = uvs.engine.camera_guess(plant, q0, f0).cpu().numpy()
    assert got.shape == (T, m * 6)
    f_host = f0.cpu().numpy()
    robot = uvs.SyntheticRobot(plant, DT)
    worst = 0.0
    for t in range(T):
        robot.start(q_host[t])
        want = uvs.plant.analytic_guess(robot, f_host[t], (256, 256), m, 6)
        worst = max(worst, float(np.abs(got[t] - want).max() / np.abs(want).max()))
    print(f'device guess, {n_points} points: worst |diff| / max |X0| over {T} trials {worst:.3e}')
    assert worst < 1e-10
    fp = params(uvs, 'GMCKF', K, m=m)
    noise = dev(np.random.default_rng(n_points).standard_normal((K, T, m)) * 0.5)
    fused = uvs.engine.camera_closed_loop(fp, plant, q0, noise, fused=True, guess='device')
    loop = uvs.engine.camera_closed_loop(fp, plant, q0, noise, guess='device')
    assert loop['k_done'].tolist() == [K] * T
    assert_same_bits(fused, loop, K, ('guess on the device', n_points))


# ------------------------------------------------------------------------------------------------------------- 6: the host route
class Replay:
    """A noise profile that hands out the rows of a recorded sequence (the duck-type of NoiseProfiler.getNoise)."""

    def __init__(self, rows):
        self.rows, self.i = rows, 0

    def getNoise(self):
        self.i += 1
        return self.rows[self.i - 1].copy()


def test_one_launch_against_the_host_route(uvs):
    """Each trial of one fused launch, guess included, against Experiment(robot=CameraRobot, perception='host').run(): numpy rasteriser, numpy
    detector, the Python loop of the external-robot route."""
    import torch
    T, K = 2, 20
    rng = np.random.default_rng(20)
    plant = uvs.SyntheticPlant.ur10()
    noise = rng.standard_normal((K, T, 8)) * 0.3
    fp = params(uvs, 'GMCKF', K)
    g = load_golden('closed_gmckf_a1p5')
    assert fp.steps == K and g['meta']['params']['kernel_bw'] == 10
    out = uvs.engine.camera_closed_loop(fp, plant, dev(Q_HOST_ROUTE), dev(noise), fused=True, guess='device')
    pix_d = torch.zeros((K * T, 4), dtype=torch.int32, device='cuda')
    uvs.engine.camera_features(plant, out['q'].reshape(K * T, 6), pixels=pix_d)
    pixels = pix_d.cpu().numpy().reshape(K, T, 4)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0]
    for t in range(T):
        ex = uvs.Experiment(Q_HOST_ROUTE[t], DESIRED, Replay(noise[:, t]), DT, DT * (K + 0.5), 0.2, uvs.CameraRobot(plant, dt=DT),
                            uvs.Method.GMCKF, **g['meta']['params'], perception='host')
        status, t_log, err, q_log, f_log = ex.run()[:5]
        assert status == uvs.ExperimentStatus.SUCCESS and len(t_log) == K
        # the preconditions under which a 1e-10 px projection difference cannot flip a pixel, on the host trajectory
        discs = np.stack([plant.discs(q) for q in q_log])
        lo, hi = discs[:, :, :2] - discs[:, :, 2:], discs[:, :, :2] + discs[:, :, 2:]
        assert lo.min() > 0.0 and hi.max() < 255.0, 'a disc touches the edge of the frame'
        masks = np.stack([cc.host_counts(uvs.plant.render_discs(d)) for d in discs])
        assert masks.min() >= 50
        assert cc.closest_to_rim(discs) > 1e-6, "a pixel's d^2 comes within 1e-6 of r^2"
        for name, dev_log, host_log in (('err', out['err'], err), ('q', out['q'], q_log), ('f', out['f'], f_log)):
            got = dev_log[:, t].cpu().numpy()
            print(f'trial {t} {name}: rel {rel(got, host_log):.3e}')
            assert rel(got, host_log) < 1e-8, (t, name)
        assert np.array_equal(pixels[:, t], masks), 'mask sizes differ at some step'
        assert np.array_equal(out['pixels'][t].cpu().numpy(), masks.min(axis=0))
