"""What tests/test_camera_latency_host.py (CPU) and tests/test_gpu_camera_latency.py (GPU) share: the LATENCIES of the delayed pixel loops
(include/uvs_vision.h, "CAMERA LATENCY"; plant.delayed_step states the rule; engine.camera_closed_loop(latency=)) -- the ones the oracle
is run on, a per-trial mix for batches -- with the sizes and the oracle's runs through its ``sensor=`` hook: a closure that caches
pixel_loop.detect per step and returns the entry of step delayed_step(k, d).

The loop's settings are those of tests/camera_moving_common.py (and so of pixel_loop_common.py: DT, GAIN, BW, NOISE_PX, DESIRED; ONE_DISC
for (2,6)); K = 16 steps, the same start, noise seed and radius.  The oracle's latencies are 1, 2 and 3 control periods at the suite's own
gains: a latency of three periods at gain * dt = 0.01 per step (0.03 for one disc) leaves the loop far from its stability margin, so the
oracle alone meets pixel_loop_common's preconditions (status 0 over 16 steps, every reported frame's discs inside the frame with masks of
at least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the (1 + 1e-14) nudge); test_camera_latency_host.py asserts them
for every oracle trial, with the teeth: "latency ignored", "off by one" (d - 1 and d + 1) and "noise of step kk instead of k" each at
least TEETH_MIN away in q or dq."""
import functools

import numpy as np

import camera_moving_common as mc
import pixel_loop_common as pl

K = mc.K
SIZES = mc.SIZES                                                     # (3, 259): one trial per workgroup; four, the last with a padding wavefront
RADIUS = mc.RADIUS
MAX_LATENCY = 8
MIX = (0, 1, 2, 3, 8)                                                # the latencies of a mixed batch
ORACLE_LATENCIES = (1, 2, 3)
ORACLE = mc.ORACLE                                                   # (8,6), (8,6), (6,6), (2,6)
MISREADINGS = ('ignored', 'one less', 'one more', 'noise of kk')


def mixed(T):
    """(T,) latencies of a batch: trial t has MIX[(t + 1) % 5], so that trial 0 has 1, the last trial of T = 3 (index 2) has 3 and the
    last of T = 259 (index 258, 259 % 5 == 4), which the padding wavefront shadows, has 8 while trial 0 has not."""
    return np.array([MIX[(t + 1) % len(MIX)] for t in range(T)], np.int64)


def uniform(T, d):
    return np.full(T, d, np.int64)


# ------------------------------------------------------------------------------------------------------------- the oracle's runs
def delayed_sensor(d, rows=None, vel=None, window=None, noise=None, noise_of_kk=False):
    """The rule as a stateful ``sensor=`` of oracle.pixel_loop.run: detect the frame of step k (occluder rows and target motion at k), keep
    it, hand back the one of step delayed_step(k, d).  noise_of_kk (with `noise`, the (K, m) rows the run adds): the misreading that adds
    step kk's noise, made by handing back the detection plus noise[kk] minus noise[k]."""
    import uvs_amd
    from oracle import pixel_loop
    kept = {}

    def sensor(p, q, k):
        at = p if vel is None else uvs_amd.plant.target_at(p, vel, k, window)
        kept[k] = pixel_loop.detect(at, q, k, RADIUS, rows)
        kk = uvs_amd.plant.delayed_step(k, d)
        f, counts, discs = kept[kk]
        if noise_of_kk:
            f = f + noise[kk] - noise[k]
        return f, counts, discs
    return sensor


@functools.lru_cache(maxsize=None)
def oracle_trial(method, n_points, d, nudged=False, misreading=None, rows=None, hold=0, motion=None, steps=K):
    """oracle.pixel_loop.run through the delayed sensor at latency d (0: the same code path, nothing delayed); nudged: from the start times
    1 + 1e-14; misreading: None or one of MISREADINGS; rows: occluder rows (a tuple of tuples) with `hold`; motion: None or a name of
    camera_moving_common.MOTIONS.  Read-only, shared by every test of a session."""
    from oracle import pixel_loop
    plant, cfg = pl.plant_of(n_points), mc.oracle_settings(n_points)
    noise = mc.oracle_noise(n_points)[:steps]
    occ = None if rows is None else np.array(rows, np.int64)
    vel, window = (None, None) if motion is None else mc.motion(motion, n_points)
    used = {None: d, 'ignored': 0, 'one less': d - 1, 'one more': d + 1, 'noise of kk': d}[misreading]
    sensor = delayed_sensor(used, occ, vel, window, noise, misreading == 'noise of kk')
    q = mc.oracle_start() * ((1.0 + pl.CALM_NUDGE) if nudged else 1.0)
    out = pixel_loop.run(plant, q, pl.DESIRED[:2 * n_points], noise, pl.DT, steps, cfg['gain'], method, cfg['kernel_bw'], False, steps,
                         pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN, initial_guess=True, radius=RADIUS, occluders=occ, hold=hold,
                         sensor=sensor)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
