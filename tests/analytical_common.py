"""Inputs shared by tests/test_analytical_host.py (their preconditions, on the CPU) and tests/test_gpu_analytical.py (the kernel against the
restatement tests/analytical_ref.py on them): the calibrated baseline off the fixture path.

T = 70 trials -- one full wavefront and a ragged one of six lanes -- of K = 40 steps from Q_START with the first three joints jittered,
noise 0.5 x t(3).  Two cases on these base inputs:

'tilted'  a general DH / pinhole plant: every parameter group of the UR10 table (alpha, d, a, theta_offset) and of the camera (focal, center)
          moved, the discs where plant_ref places them for the UR10.  Every trial succeeds and is well conditioned, so the project's gates
          apply.  'tilted_placed' is the same plant with the discs placed for IT (they project onto DESIRED_F from Q_GOAL again).
'mixed'   the UR10 plant with outliers that make single trials of a wavefront leave the first pass between healthy neighbours: 1e13 on one
          feature at step HIT_STEP of the trials HIT (J drops to numerical rank 2 there: the careful pass's truncated solve), a NaN (trial
          20: the first pass FAILs it), an inf (41: suspect in the first pass, FAILed by the careful pass) and 1e13 followed by an inf (64).
Amplitudes of 3e7 - 3e8 ("suspect but full rank") are left out on purpose: two numpy solvers already disagree by 1e-9 - 1.3e-8 on the
command there and q moves by up to 9e-8 under a 1e-14 shift of q0, so no gate of this project can be derived for them."""
import functools

import numpy as np

T, K, DT, GAIN = 70, 40, 0.05, 0.2
SEED = 5
HIT, HIT_STEP, HIT_FEATURE, HIT_VALUE = (5, 37, 63, 66), 17, 2, 1e13      # a mid lane, the second half, the last lane of wavefront 0, the ragged tail
# trial -> ((step, feature, value), ...) and the step at which the trial FAILs
EXTRA = {20: ((9, 4, np.nan),), 41: ((23, 3, np.inf),), 64: ((5, 2, 1e13), (30, 3, np.inf))}
FAIL_AT = {20: 9, 41: 23, 64: 30}
UNTOUCHED = tuple(t for t in range(T) if t not in HIT and t not in EXTRA)
PLANT_GROUPS = ('alpha', 'd', 'a', 'theta_offset', 'focal', 'center')
WATCH = 2.0 ** 34                                                         # the first pass's |R_cc| spread watch (rmckf_lstsq.hpp)


def ur10_values():
    import analytical_ref
    return analytical_ref.plant_values(None)


@functools.lru_cache(maxsize=None)
def tilted_values(placed=False):
    """The tilted plant as analytical_ref.plant_values' dict: the UR10 table and camera with every group moved, and the default discs --
    or, `placed`, discs put where they project onto DESIRED_F from Q_GOAL on THIS plant (plant_ref.place_discs' recipe)."""
    import analytical_ref
    from oracle import plant_ref
    pv = ur10_values()
    i = np.arange(6)
    pv['alpha'] = pv['alpha'] + np.array([0.02, -0.03, 0.015, -0.01, 0.025, 0.02])
    pv['d'] = pv['d'] + 0.01 * (i + 1)
    pv['a'] = pv['a'] + 0.005 * (6 - i)
    pv['theta_offset'] = pv['theta_offset'] + 0.03 * (-1.0) ** i
    pv['focal'] = pv['focal'] * 1.1
    pv['center'] = 120.0
    if placed:
        cam = analytical_ref.fkine_all_batch(plant_ref.Q_GOAL[None], pv)[5][0]
        depth = cam[2, 3]
        rays = np.array([[(u - pv['center']) / pv['focal'] * depth, (v - pv['center']) / pv['focal'] * depth, depth]
                         for u, v in plant_ref.DESIRED_F.reshape(-1, 2)])
        pv['points'] = cam[:3, 3] + rays @ cam[:3, :3].T
    for v in pv.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pv


def device_plant(uvs, values):
    """uvs_amd.SyntheticPlant of a plant_values dict."""
    return uvs.SyntheticPlant(theta_offset=values['theta_offset'].copy(), d=values['d'].copy(), a=values['a'].copy(), alpha=values['alpha'].copy(),
                              points=values['points'].copy(), focal=values['focal'], center=values['center'])


@functools.lru_cache(maxsize=None)
def base_inputs():
    """dict(desired (8,), q0 (T, 6), noise (T, K, 8)): read-only, shared by every test of a session."""
    from oracle import plant_ref
    rng = np.random.default_rng(SEED)
    q0 = np.tile(plant_ref.Q_START, (T, 1))
    q0[:, :3] += rng.uniform(-0.15, 0.15, (T, 3))
    noise = 0.5 * rng.standard_t(3, (T, K, 8))
    desired = plant_ref.DESIRED_F.copy()
    for a in (desired, q0, noise):
        a.setflags(write=False)
    return dict(desired=desired, q0=q0, noise=noise)


@functools.lru_cache(maxsize=None)
def mixed_noise():
    noise = base_inputs()['noise'].copy()
    for t in HIT:
        noise[t, HIT_STEP, HIT_FEATURE] = HIT_VALUE
    for t, hits in EXTRA.items():
        for step, feature, value in hits:
            noise[t, step, feature] = value
    noise.setflags(write=False)
    return noise


def plant_of(case):
    """plant_values dict of a case; None: the UR10 plant ('mixed', 'base')."""
    return {'tilted': tilted_values, 'tilted_placed': lambda: tilted_values(True)}.get(case, lambda: None)()


def restate(plant=None, noise=None, q0=None, steps=K, logs=('err', 'q', 'f', 'dq', 'j')):
    """The restatement on the base inputs (noise: None = the base noise; pass an array for another one), `steps` steps, make_params' clock."""
    import analytical_ref
    inp = base_inputs()
    noise = inp['noise'] if noise is None else noise
    return analytical_ref.run(inp['q0'] if q0 is None else q0, noise[:, :steps], inp['desired'], DT, 15.0, GAIN, steps=steps, logs=logs, plant=plant)


@functools.lru_cache(maxsize=None)
def reference(case, steps=K):
    """The restatement's run of 'tilted', 'tilted_placed', 'mixed' or 'base' (the UR10 plant, the base noise without any outlier).  Read-only."""
    ref = restate(plant_of(case), mixed_noise() if case == 'mixed' else None, steps=steps)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def rdiag_spread(J):
    """max / min of |R_cc| of the Householder QR of (..., 8, 6) matrices: what the first pass's watch looks at."""
    r = np.abs(np.diagonal(np.linalg.qr(J)[1], axis1=-2, axis2=-1))
    return r.max(axis=-1) / r.min(axis=-1)


def plain_qr_solve(J, y):
    """min |J x - y| by QR and back substitution, no truncation: what a solver without numpy's cutoff returns."""
    Q, R = np.linalg.qr(J)
    return np.linalg.solve(R, Q.T @ y)
