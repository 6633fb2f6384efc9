"""The pixel closed loop with per-trial estimator parameters (uvs_camera_closed_loop_grid_f64; engine.camera_closed_loop(trial_params=...)):
a hyperparameter grid over the same starts and noise in one launch.

The oracle is the uniform one-launch loop, camera_closed_loop(fused=True), which tests/test_gpu_camera_loop.py holds to the two-launch
loop: trial t of a grid launch must have the BITS of trial source[t] of the uniform launch that runs t's values over the same inputs -- every
specified log row, stats, status, k_done and pixels (camera_common.assert_same_bits).  The two kernels are one text compiled twice, both
with -ffp-contract=off, so nothing looser is due.  Batch sizes come on both sides of 256 output trials, where the kernel changes from one
trial per workgroup to four, and are chosen so that a workgroup of four mixes grid cells.

What each test catches was tried on the kernel with one-line mutations."""
import ctypes
import os

import numpy as np
import pytest

import camera_common as cc

pytestmark = pytest.mark.gpu

DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
DT, K = 0.05, 12
# the start poses and the noise scale of tests/test_gpu_camera_loop.py
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
Q_LEAVES = np.array([-0.47915568, -0.55367504, 2.20583478, -0.05228325, -1.09351535, 0.40221985])     # all four discs out of view at step 6
NOISE_PX = 0.5
G, SMALL = 4, 256                                                    # trials per workgroup beyond SMALL output trials; one up to it
SCALARS = ('kernel_bw', 'gain', 'reg', 'fpi_threshold')
BANDWIDTHS, GAINS = (2.0, 5.0, 10.0, 20.0), (0.1, 0.2, 0.4)
LEAVING_BW = (10.0, 12.0, 15.0, 20.0)                                # test 7: bandwidths at which Q_LEAVES leaves the frame within K steps

bits, assert_same_bits = cc.bits, cc.assert_same_bits


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


def params(uvs, method, m=8, annealing=False, strict=False):
    fp = uvs.engine.make_params(m, 6, method, 10.0, annealing, DT, DT * (K + 0.5), 0.2, DESIRED[:m], True)
    assert fp.steps == K
    if strict:
        fp.reserved = uvs._lib.UVS_OPT_STRICT_PINV
    return fp


def plant_of(uvs, n_points):
    return uvs.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))


def jittered(T, seed):
    """T start poses: Q_HOST_ROUTE[0] plus a seeded jitter of +-0.05 rad."""
    return Q_HOST_ROUTE[0] + np.random.default_rng(seed).uniform(-0.05, 0.05, (T, 6))


class Inputs:
    """n_in input trials on the device: start poses, noise and the device's initial guess."""

    def __init__(self, uvs, n_points, q_host, seed=None):
        self.plant, self.m, self.n_in = plant_of(uvs, n_points), 2 * n_points, len(q_host)
        self.q0 = dev(q_host)
        self.noise = None if seed is None else dev(np.random.default_rng(seed).standard_normal((K, self.n_in, self.m)) * NOISE_PX)
        self.x0 = uvs.engine.camera_guess(self.plant, self.q0, uvs.engine.camera_features(self.plant, self.q0))

    def only(self, trials):
        """The same inputs, cut down to ``trials``."""
        other = object.__new__(Inputs)
        other.plant, other.m, other.n_in = self.plant, self.m, len(trials)
        other.q0, other.x0 = self.q0[trials].contiguous(), self.x0[trials].contiguous()
        other.noise = None if self.noise is None else self.noise[:, trials].contiguous()
        return other


def uniform(uvs, fp, inp, **values):
    """The oracle: the uniform one-launch loop over all of ``inp`` with ``values`` written into a copy of fp."""
    one = type(fp).from_buffer_copy(fp)
    for key, value in values.items():
        if key == 'desired':
            for i, v in enumerate(value):
                one.desired[i] = v
        else:
            setattr(one, key, value)
    return uvs.engine.camera_closed_loop(one, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=True)


def grid(uvs, fp, inp, host):
    """One grid launch over ``inp``; ``host``: key -> numpy array, one row per output trial."""
    tp = {key: dev(np.asarray(value, np.int32 if key == 'source' else np.float64)) for key, value in host.items()}
    return uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=True, trial_params=tp)


def check_grid(uvs, fp, inp, host, where):
    """Every trial of the grid launch against its uniform launch.  Returns (the grid's outputs, {cell values: (oracle outputs, its trials)})."""
    import torch
    got = grid(uvs, fp, inp, host)
    T = got['status'].shape[0]
    source = np.asarray(host['source']) if 'source' in host else np.arange(T)
    assert T == len(source)
    for key, comp in (('err', inp.m), ('q', 6), ('f', inp.m), ('dq', 6), ('kappa', inp.m)):
        assert tuple(got[key].shape) == (K, T, comp) and got[key].is_contiguous()
    assert tuple(got['stats'].shape) == (T, 3) and tuple(got['pixels'].shape) == (T, inp.m // 2)
    cells = {}
    for t in range(T):
        cell = tuple((key, tuple(np.atleast_1d(host[key][t]).tolist())) for key in SCALARS + ('desired',) if key in host)
        cells.setdefault(cell, []).append(t)
    oracles = {}
    for cell, trials in cells.items():
        values = {key: (value if key == 'desired' else value[0]) for key, value in cell}
        want = uniform(uvs, fp, inp, **values)
        torch.cuda.synchronize()
        assert_same_bits(got, want, K, (where, cell), trials=trials, want_trials=source[trials].tolist())
        oracles[cell] = (want, trials)
    return got, oracles


def bandwidth_gain_grid(E):
    """kernel_bw x gain over E input trials, source = t % E: cell c holds the output trials [c E, (c + 1) E)."""
    cells = [(bw, gain) for bw in BANDWIDTHS for gain in GAINS]
    T = len(cells) * E
    return dict(kernel_bw=np.repeat([c[0] for c in cells], E), gain=np.repeat([c[1] for c in cells], E), source=np.arange(T) % E)


def all_complete(oracles):
    return all(want['k_done'].tolist() == [K] * want['k_done'].shape[0] for want, _ in oracles.values())


def cells_differ(oracles, key='err'):
    seen = {bits(want[key]).tobytes() for want, _ in oracles.values()}
    return len(seen) >= 2


# ------------------------------------------------------------------------------------------------------------- 1: bandwidth x gain
CASES = [(method, n_points) for method in ('GMCKF', 'KF', 'IMCCKF') for n_points in (4, 3, 1)] + [('MCKF', 4), ('MCKF', 1)]


@pytest.mark.parametrize('E', [1, 22])                               # T = 12: one trial per workgroup; T = 264: four, and 22 % 4 != 0 mixes cells
@pytest.mark.parametrize('method,n_points', CASES)
def test_a_grid_has_the_bits_of_its_uniform_launches(uvs, method, n_points, E):
    fp = params(uvs, method, 2 * n_points)
    inp = Inputs(uvs, n_points, jittered(E, 7), seed=100 + n_points)
    host = bandwidth_gain_grid(E)
    assert (len(host['source']) > SMALL) == (E == 22)
    got, oracles = check_grid(uvs, fp, inp, host, (method, n_points, E))
    assert len(oracles) == 12 and all_complete(oracles), 'the comparison would be vacuous: a cell did not run its 12 steps'
    assert cells_differ(oracles), 'the comparison would be vacuous: every cell has the same errors'
    assert got['status'].tolist() == [0] * len(host['source'])


# ------------------------------------------------------------------------------------------------------------- 2: reg, fpi_threshold
@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('method,key,values', [('GMCKF', 'reg', (1e-6, 1e-3, 1e-1)), ('MCKF', 'fpi_threshold', (1e-1, 1e-4, 1e-8))])
def test_regulariser_and_fixed_point_threshold_per_trial(uvs, method, key, values, T):
    """Output trials 3 i, 3 i + 1, 3 i + 2 run the three values on input trial i (the last input of T = 259 has one value only)."""
    fp = params(uvs, method)
    E = (T + 2) // 3
    inp = Inputs(uvs, 4, jittered(E, 21), seed=5)
    host = {key: np.array(values)[np.arange(T) % 3], 'source': np.arange(T) // 3}
    got, oracles = check_grid(uvs, fp, inp, host, (method, key, T))
    assert len(oracles) == 3 and all_complete(oracles)
    # Every value gives other results on the same inputs (MCKF: the iteration counts moved).  Read off the commands: the detector quantises,
    # so joints that differ in their last digits can show the same features, and with them the same errors, for all 12 steps.
    assert len({bits(want['dq']).tobytes() for want, _ in oracles.values()}) == 3, f'{key} does not reach the estimator'


# ------------------------------------------------------------------------------------------------------------- 3: desired
@pytest.mark.parametrize('T', [6, SMALL + 6])
def test_desired_features_per_trial(uvs, T):
    """Two targets alternate from trial to trial; no source: trial t reads input trial t."""
    fp = params(uvs, 'GMCKF')
    inp = Inputs(uvs, 4, jittered(T, 31), seed=6)
    shifted = DESIRED + np.array([3., -2., 3., -2., 3., -2., 3., -2.])
    host = {'desired': np.where((np.arange(T) % 2 == 0)[:, None], DESIRED, shifted)}
    got, oracles = check_grid(uvs, fp, inp, host, ('desired', T))
    assert len(oracles) == 2 and all_complete(oracles) and cells_differ(oracles)
    assert sorted(len(trials) for _, trials in oracles.values()) == [T // 2, T // 2]


# ------------------------------------------------------------------------------------------------------------- 4: launch-wide variants
@pytest.mark.parametrize('E', [1, 22])
@pytest.mark.parametrize('variant', ['annealing', 'strict'])
def test_annealing_and_strict_pinv_stay_launch_wide(uvs, variant, E):
    fp = params(uvs, 'GMCKF', annealing=variant == 'annealing', strict=variant == 'strict')
    inp = Inputs(uvs, 4, jittered(E, 8), seed=9)
    got, oracles = check_grid(uvs, fp, inp, bandwidth_gain_grid(E), (variant, E))
    assert len(oracles) == 12 and all_complete(oracles) and cells_differ(oracles)
    if variant == 'annealing':                                       # sigma_k = the trial's sigma_0 + the launch's span: other weights than without
        plain = grid(uvs, params(uvs, 'GMCKF'), inp, bandwidth_gain_grid(E))
        assert not np.array_equal(bits(plain['kappa']), bits(got['kappa'])), 'annealing changed nothing'


# ------------------------------------------------------------------------------------------------------------- 5: NULL members
@pytest.mark.parametrize('T', [1, G, G + 1, SMALL, SMALL + 1, SMALL + G])
def test_null_members_are_the_uniform_call(uvs, T):
    import torch
    fp = params(uvs, 'GMCKF')
    inp = Inputs(uvs, 4, jittered(T, 1000 + T), seed=T)
    want = uniform(uvs, fp, inp)
    assert want['k_done'].tolist() == [K] * T
    for tp in ({}, {'source': dev(np.arange(T, dtype=np.int32))}, {'source': np.arange(T)}, {'gain': None, 'desired': None}):
        got = uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=True, trial_params=tp)
        torch.cuda.synchronize()
        assert got['status'].shape[0] == T
        assert_same_bits(got, want, K, (T, sorted(tp)))


# ------------------------------------------------------------------------------------------------------------- 6: source, on every input
@pytest.mark.parametrize('T', [9, SMALL + 5])
def test_a_permutation_source_permutes_the_outputs(uvs, T):
    """Distinct start poses, noise rows and guesses: f[0] needs q_start and the noise row of the source trial, the first err its x0 and f0."""
    fp = params(uvs, 'GMCKF')
    inp = Inputs(uvs, 4, jittered(T, 77), seed=78)
    perm = np.random.default_rng(T).permutation(T)
    assert not np.array_equal(perm, np.arange(T))
    want = uniform(uvs, fp, inp)
    assert want['k_done'].tolist() == [K] * T
    assert len({bits(want['f'][0, t]).tobytes() for t in range(T)}) == T and len({bits(want['err'][0, t]).tobytes() for t in range(T)}) == T
    got = grid(uvs, fp, inp, {'source': perm})
    assert_same_bits(got, want, K, ('permutation', T), trials=list(range(T)), want_trials=perm.tolist())
    # the device guess and f0 are computed over the inputs, not given: the same bits again
    guessed = uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, fused=True, guess='device', trial_params={'source': perm})
    assert_same_bits(guessed, want, K, ('permutation, device guess', T), trials=list(range(T)), want_trials=perm.tolist())


# ------------------------------------------------------------------------------------------------------------- 7: a failing neighbour
@pytest.mark.parametrize('E,leaving', [(5, 3), (66, 41)])            # 4 cells: T = 20, and T = 264 with 66 % 4 != 0
def test_a_failing_source_trial_fails_in_every_cell_alone(uvs, E, leaving):
    """At gain 0.2 the discs of Q_LEAVES are out of view at step 6 for sigma_0 = 10, 12 and 15 and at step 7 for 20 (found with the uniform
    kernel; smaller bandwidths keep them in view for 12 steps): the copies FAIL at their own cells' steps."""
    fp = params(uvs, 'GMCKF')
    q_host = jittered(E, 300 + E)
    q_host[leaving] = Q_LEAVES
    inp = Inputs(uvs, 4, q_host)                                     # Q_LEAVES was found without noise
    T = 4 * E
    host = dict(kernel_bw=np.repeat(LEAVING_BW, E), source=np.arange(T) % E)
    got, oracles = check_grid(uvs, fp, inp, host, ('failing', E))
    k_done, status = got['k_done'].tolist(), got['status'].tolist()
    assert len(oracles) == 4
    assert len({want['k_done'][leaving].item() for want, _ in oracles.values()}) >= 2, 'every cell fails at the same step'
    for want, trials in oracles.values():
        assert want['status'][leaving].item() == 1 and 0 < want['k_done'][leaving].item() < K, 'the oracle does not FAIL there'
        for t in trials:
            if t % E == leaving:
                assert status[t] == 1 and k_done[t] == want['k_done'][leaving].item() and got['pixels'][t].min().item() == 0
            else:
                assert status[t] == 0 and k_done[t] == K
    others_in = [e for e in range(E) if e != leaving]
    host_without = dict(kernel_bw=np.repeat(LEAVING_BW, E - 1), source=np.arange(4 * (E - 1)) % (E - 1))
    without = grid(uvs, fp, inp.only(others_in), host_without)
    others = [t for t in range(T) if t % E != leaving]
    assert_same_bits(got, without, K, ('without the failing trial', E), trials=others, want_trials=list(range(len(others))))


# ------------------------------------------------------------------------------------------------------------- 8: an index that names no trial
@pytest.mark.parametrize('T,outside', [(18, (0, 5, 17)), (SMALL + 6, (3, 4, SMALL, SMALL + 5))])
def test_an_index_that_names_no_trial_fails_its_trial_alone(uvs, T, outside):
    """source values -1 and n_in, on the device, through the C entry point (the Python layer refuses them on the host): status FAIL and
    k_done = 0, nothing else of theirs written, and every other trial as in a launch without them."""
    import torch
    m, SENTINEL, E = 8, 7.0, 6
    fp = params(uvs, 'GMCKF')
    inp = Inputs(uvs, 4, jittered(E, 500 + T), seed=T)
    cam = inp.plant.to_camera()
    source_host = (np.arange(T) % E).astype(np.int32)
    for i, t in enumerate(outside):
        source_host[t] = -1 if i % 2 == 0 else E
    bw_host = np.array(BANDWIDTHS)[np.arange(T) % 4]
    source, bw = dev(source_host), dev(bw_host)
    others = [t for t in range(T) if t not in outside]
    f64 = dict(dtype=torch.float64, device='cuda')
    log = {key: torch.full((K, T, comp), SENTINEL, **f64) for key, comp in (('q', 6), ('f', m), ('dq', 6), ('err', m), ('kappa', m))}
    status, k_done = (torch.full((T,), 7, dtype=torch.int32, device='cuda') for _ in range(2))
    stats = torch.full((T, 3), SENTINEL, **f64)
    pixels = torch.full((T, 4), 7, dtype=torch.int32, device='cuda')
    f0 = uvs.engine.camera_features(inp.plant, inp.q0)
    tp = uvs._vision.CameraTrialParams(bw.data_ptr(), None, None, None, None, source.data_ptr(), E)
    uvs._vision.check(uvs._vision.lib().uvs_camera_closed_loop_grid_f64(
        ctypes.byref(fp), ctypes.byref(cam), T, ctypes.byref(tp), inp.q0.data_ptr(), inp.noise.data_ptr(), inp.x0.data_ptr(), f0.data_ptr(),
        log['q'].data_ptr(), log['f'].data_ptr(), log['dq'].data_ptr(), log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(),
        k_done.data_ptr(), stats.data_ptr(), pixels.data_ptr(), None))
    torch.cuda.synchronize()
    for t in outside:
        assert status[t].item() == 1 and k_done[t].item() == 0, t
        assert all(bool((log[key][:, t] == SENTINEL).all()) for key in log), (t, 'a log row was written')
        assert bool((stats[t] == SENTINEL).all()) and pixels[t].tolist() == [7] * 4, t
    got = dict(log, status=status, k_done=k_done, stats=stats, pixels=pixels)
    without = grid(uvs, fp, inp, dict(kernel_bw=bw_host[others], source=source_host[others]))
    assert without['k_done'].tolist() == [K] * len(others)
    assert_same_bits(got, without, K, ('without the trials that name no input', T), trials=others, want_trials=list(range(len(others))))
