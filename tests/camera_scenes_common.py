"""What tests/test_camera_scenes_host.py (CPU) and tests/test_gpu_camera_scene_batch.py (GPU) share: the SCENE SET of the scene-per-trial
pixel loops (include/uvs_vision.h, "A SCENE PER TRIAL"; engine.camera_scenes) -- six variants of SyntheticPlant.ur10() chosen so that every
field the sensor side reads differs somewhere: theta_offset (camera roll), d and a (link scale), points, focal, center and radius -- with the
starts, the noise and the rectangles the loops run on, and the per-trial oracle runs.

The loop's settings are those of tests/pixel_loop_common.py (dt 0.05, gain 0.2, noise 0.3 px, its desired features and start poses);
K = 16 steps.  The six step-0 frames are pairwise different, and on every oracle trajectory every disc stays inside the frame with a mask
of at least pixel_loop_common.MASK_MIN pixels (asserted on the CPU)."""
import functools

import numpy as np

import camera_hold_common as hc
import camera_occluders_common as oc
import camera_painted_common as pc
import pixel_loop_common as pl

K = 16
N_SCENES = 6
RADII = (0.024, 0.018, 0.030, 0.024, 0.024, 0.024)
CENTER_OF = {3: 120.0}                                               # scene -> principal point; the others keep 128
NAMES = ('nominal', 'focal 0.9', 'focal 1.1', 'points moved, centre 120', 'camera roll 0.05', 'links 1.03')
SIZES = (3, 259)                                                     # one trial per workgroup; four, the last with a padding wavefront
ORACLE = (('GMCKF', 4), ('KF', 4), ('MCKF', 1))                      # (8,6), (8,6), (2,6): one oracle trial per scene each


def plants(uvs, n_points=4):
    """The six scenes as plants; the nominal one first."""
    nominal = uvs.SyntheticPlant.ur10(desired_f=tuple(pl.DESIRED[:2 * n_points]))
    mis = uvs.plant.miscalibrated
    out = [nominal, mis(nominal, focal_scale=0.9), mis(nominal, focal_scale=1.1), mis(nominal, point_offset=(0.02, -0.01, 0.03)),
           mis(nominal, joint_offset=[0.0, 0.0, 0.0, 0.0, 0.0, 0.05]), mis(nominal, link_scale=1.03)]
    for scene, center in CENTER_OF.items():
        out[scene].center = center
    return out


def structs(uvs, n_points=4):
    """The six uvs_camera structs, radii included: what engine.camera_scenes packs."""
    return [plant.to_camera(radius) for plant, radius in zip(plants(uvs, n_points), RADII)]


def starts(T, seed=0):
    """T start poses: the two of the host-route tests, then seeded jitters of 0.03 rad around the first."""
    rng = np.random.default_rng(seed)
    q = np.concatenate([pl.Q_HOST_ROUTE, pl.Q_HOST_ROUTE[0] + rng.uniform(-0.03, 0.03, (max(T - 2, 0), 6))])
    return np.ascontiguousarray(q[:T])


def noise(T, n_points=4, seed=1, steps=K):
    return np.random.default_rng(seed).standard_normal((steps, T, 2 * n_points)) * pl.NOISE_PX


def mixed_index(T, shuffled=False):
    """Scene of output trial t: t % 6, or a seeded shuffle of that whose last trial -- the one a padding wavefront shadows -- is not on
    scene 0."""
    idx = (np.arange(T) % N_SCENES).astype(np.int32)
    if not shuffled:
        return idx
    idx = np.random.default_rng(T).permutation(idx).astype(np.int32)
    if idx[-1] == 0:
        other = int(np.flatnonzero(idx != 0)[0])
        idx[-1], idx[other] = idx[other], 0
    return idx


def rectangles(scenario, n_points=4):
    """(occluder rows, paints or None, hold) of a scenario: 'plain', 'occluded' (the sweeping bar and a half cover), 'held' (the wide bar
    with hold = K), 'painted' (the still distractor of the first disc's colour, and a half cover)."""
    if scenario == 'plain':
        return None, None, 0
    if scenario == 'occluded':
        return pl.bar_rows(n_points), None, 0
    if scenario == 'held':
        return pl.wide_rows(n_points), None, K
    if scenario == 'painted':
        rows, paints = pl.distractor_rows(n_points, False)
        return rows, paints, 0
    raise KeyError(scenario)


SCENARIOS = ('plain', 'occluded', 'held', 'painted')
assert hc and oc and pc                                              # the suites the rectangles come from


def oracle_start(scene):
    """The start of the oracle trial on `scene`: the first host-route pose, jittered by a seed of the scene's own (chosen on the CPU so
    that every trial is calm: test_camera_scenes_host.py)."""
    return pl.jittered(ORACLE_SEEDS[scene], pl.Q_HOST_ROUTE[0], 0.03)


ORACLE_SEEDS = (11, 12, 13, 14, 15, 16)


def oracle_noise(scene, n_points):
    return np.random.default_rng(200 + scene).standard_normal((K, 2 * n_points)) * pl.NOISE_PX


@functools.lru_cache(maxsize=None)
def oracle_trial(method, n_points, scene, nudged=False):
    """oracle.pixel_loop.run on the scene's own plant and radius, from oracle_start(scene) (nudged: times 1 + 1e-14)."""
    import uvs_amd
    from oracle import pixel_loop
    plant = plants(uvs_amd, n_points)[scene]
    q = oracle_start(scene) * ((1.0 + pl.CALM_NUDGE) if nudged else 1.0)
    out = pixel_loop.run(plant, q, pl.DESIRED[:2 * n_points], oracle_noise(scene, n_points), pl.DT, K, pl.GAIN, method, pl.BW, False, K,
                         pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN, initial_guess=True, radius=RADII[scene])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
