"""What tests/test_camera_moving_host.py (CPU) and tests/test_gpu_camera_moving.py (GPU) share: the MOTIONS of the moving-target pixel loops
(include/uvs_vision.h, "MOVING TARGETS"; plant.target_at states the rule; engine.*(target_motion=, motion_window=)) -- the two the oracle is
run on, a per-trial mix for batches -- with the sizes, the scene set of camera_scenes_common.py, and the oracle's runs through its
``sensor=`` hook: pixel_loop.detect(target_at(plant, v, k, window), q, k, radius).

The loop's settings are those of tests/pixel_loop_common.py (DT, GAIN, BW, NOISE_PX, DESIRED; ONE_DISC for (2,6)); K = 16 steps; the start
is pl.jittered(11, pl.Q_HOST_ROUTE[0], 0.03), the noise seed 5, the radius 0.024.  In the oracle's motions every disc moves with velocity
(v, -v/2, 0): 'drift' v = 0.002 m/step in the window (0, 16), 'window' v = 0.004 m/step in (4, 10).  The preconditions of
pixel_loop_common (status 0 over 16 steps, every disc inside the frame with a mask of at least MASK_MIN pixels, no pixel within RIM_MIN
of a rim, calm under the (1 + 1e-14) nudge) and the teeth ("the motion is ignored" at least TEETH_MIN away in q or dq) are asserted on
the CPU by test_camera_moving_host.py for every oracle trial."""
import functools

import numpy as np

import camera_scenes_common as sc
import pixel_loop_common as pl

K = 16
SIZES = sc.SIZES                                                     # (3, 259): one trial per workgroup; four, the last with a padding wavefront
RADIUS = 0.024
START_SEED, NOISE_SEED = 11, 5
MOTIONS = {'drift': (0.002, (0, 16)), 'window': (0.004, (4, 10))}    # name -> (v in metres per step, (k_on, k_off))
ORACLE = (('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1))       # (8,6), (8,6), (6,6), (2,6)
STILL_WINDOW = (0, 0)


def velocity(v, n_points):
    """Every disc with the world velocity (v, -v/2, 0)."""
    return np.tile(np.array([v, -v / 2, 0.0]), (n_points, 1))


def motion(name, n_points):
    """(velocity (n_points, 3), window) of one of MOTIONS."""
    v, window = MOTIONS[name]
    return velocity(v, n_points), window


def mixed(T, n_points):
    """(velocity (T, n_points, 3), window (T, 2)) of a batch: trial t % 4 is still / 'drift' / 'window' with a velocity of its own per disc
    / a NaN velocity whose k_on = K, which must behave as still.  The last trial of T = 259 (258 % 4 == 2), which a padding wavefront
    shadows, moves; so does the last of T = 3."""
    vel = np.zeros((T, n_points, 3))
    win = np.zeros((T, 2), np.int64)
    per_disc = np.array([1.0, 0.5, -1.0, 0.75])[:n_points, None]
    for t in range(T):
        kind = t % 4
        if kind == 0:
            win[t] = STILL_WINDOW
        elif kind == 1:
            vel[t], win[t] = motion('drift', n_points)
        elif kind == 2:
            vel[t], win[t] = velocity(MOTIONS['window'][0], n_points) * per_disc, MOTIONS['window'][1]
        else:
            vel[t], win[t] = np.nan, (K, 2 ** 31 - 1)
    return vel, win


def still(T, n_points, nan=False):
    """A batch in which s(k) == 0 at every step k < K: zero velocities in an empty window, or NaN velocities whose k_on = K."""
    vel = np.full((T, n_points, 3), np.nan if nan else 0.0)
    win = np.tile(np.array([K, 2 ** 31 - 1] if nan else STILL_WINDOW, np.int64), (T, 1))
    return vel, win


def moved_plants(uvs, plant, vel, win, k):
    """The host-moved plants of a batch at step k: plant.target_at per trial (`plant`: one plant, or one per trial)."""
    plants = plant if isinstance(plant, (list, tuple)) else [plant] * len(vel)
    return [uvs.plant.target_at(p, v, k, tuple(int(x) for x in w)) for p, v, w in zip(plants, vel, win)]


# ------------------------------------------------------------------------------------------------------------- the oracle's runs
def oracle_settings(n_points):
    one = n_points == 1
    return dict(gain=pl.ONE_DISC['gain'] if one else pl.GAIN, kernel_bw=pl.ONE_DISC['kernel_bw'] if one else pl.BW,
                noise_px=pl.ONE_DISC['noise_px'] if one else pl.NOISE_PX)


def oracle_start():
    return pl.jittered(START_SEED, pl.Q_HOST_ROUTE[0], 0.03)


def oracle_noise(n_points):
    return np.random.default_rng(NOISE_SEED).standard_normal((K, 2 * n_points)) * oracle_settings(n_points)['noise_px']


@functools.lru_cache(maxsize=None)
def oracle_trial(method, n_points, name, nudged=False, rows=None, hold=0):
    """oracle.pixel_loop.run through its sensor= hook on the motion `name` (None: the still trial, the same code path); nudged: from the
    start times 1 + 1e-14; rows: occluder rows (a tuple of tuples) with `hold`.  Read-only, shared by every test of a session."""
    import uvs_amd
    from oracle import pixel_loop
    plant, cfg = pl.plant_of(n_points), oracle_settings(n_points)
    vel, window = motion(name, n_points) if name is not None else (np.zeros((n_points, 3)), STILL_WINDOW)
    occ = None if rows is None else np.array(rows, np.int64)

    def sensor(p, q, k):
        return pixel_loop.detect(uvs_amd.plant.target_at(p, vel, k, window), q, k, RADIUS, occ)

    q = oracle_start() * ((1.0 + pl.CALM_NUDGE) if nudged else 1.0)
    out = pixel_loop.run(plant, q, pl.DESIRED[:2 * n_points], oracle_noise(n_points), pl.DT, K, cfg['gain'], method, cfg['kernel_bw'], False, K,
                         pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN, initial_guess=True, radius=RADIUS, occluders=occ, hold=hold,
                         sensor=sensor)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
