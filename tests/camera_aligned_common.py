"""What tests/test_camera_aligned_host.py (CPU) and tests/test_gpu_camera_aligned.py (GPU) share: the (latency, ASSUMED latency) pairs of the
aligned pixel loops (include/uvs_vision.h, "ASSUMED LATENCY"; plant.aligned_regressor_step and plant.delayed_step state the rule;
engine.camera_closed_loop(assumed_latency=)) -- a per-trial mix for batches, the pairs the CPU restatements are run on -- with the sizes and
two numpy restatements of one trial for ANY assumed latency a:

  estimator_trial   the oracle's loop (oracle/pixel_loop.py) over rmckf_block.BlockFilter and rmckf_block.control_law through
                    camera_latency_common.delayed_sensor, with the regressor of step k the command of step k - 1 - a, or zeros.  The
                    untouched oracle contains a = 0 (mutation=None) and a = 1 (mutation='regressor_stale'); the host file compares bit for bit.
  law_trial         the calibrated law over camera_analytical_ref.step at the joints q_{max(k - a, 0)} on the reported row of step k.

The settings are those of tests/camera_latency_common.py (and so of camera_moving_common.py and pixel_loop_common.py); K = 16, the same
start, noise seed and radius.  `variant` names one misreading of the rule (MISREADINGS): the host file measures how far each moves q or dq."""
import functools

import numpy as np

import camera_latency_common as lc
import camera_moving_common as mc
import pixel_loop_common as pl

K = lc.K
SIZES = lc.SIZES                                                     # (3, 259): one trial per workgroup; four, the last with a padding wavefront
RADIUS = lc.RADIUS
MAX_LATENCY = lc.MAX_LATENCY
LATENCIES = (0, 1, 3, 8)                                             # d of a mixed batch
ASSUMED = (0, 1, 2, 3, 8)                                            # a of a mixed batch
PAIRS = tuple((d, a) for a in ASSUMED for d in LATENCIES)            # the 20 (d, a) pairs
LAST = (3, 8)                                                        # the pair of the last trial of T = 259 alone: the padding wavefront shadows it
CYCLE = tuple(p for p in PAIRS if p != LAST)                         # 19 pairs, walked with stride 7
ORACLE = lc.ORACLE                                                   # (8,6), (8,6), (6,6), (2,6)
ORACLE_ASSUMED = (1, 2, 3)                                           # estimator trials at a = d
LAW_ASSUMED = (1, 2, 3, 8)                                           # law trials at a = d
MISREADINGS = ('ignored', 'one less', 'one more', 'clamped')         # 'clamped': the regressor clamped to dq_0 instead of zero (estimators)
# (what, n_points, a, misreading) -> measured distance: an "off by one" misreading that falls under TEETH_MIN, as pixel_loop_common.NO_TEETH
# lists its own.  The host file asserts that every entry is still under TEETH_MIN and that nothing else is.
NO_TEETH = {}


def mixed(T):
    """(d, a), two (T,) arrays: trial t has CYCLE[(7 t + 3) % 19] -- trial 0 has (8, 0), the trials of T = 3 have a = 0, 2 and 8 -- and the
    last trial of T = 259 has LAST = (3, 8), which no other trial has."""
    pairs = [CYCLE[(7 * t + 3) % len(CYCLE)] for t in range(T)]
    if T > 3:
        pairs[-1] = LAST
    d, a = np.array(pairs, np.int64).T
    return d.copy(), a.copy()


def regressor_step(k, a, variant=None):
    """The step whose command is the regressor at step k, or -1 for zeros: the rule, or one misreading of it."""
    import uvs_amd
    if variant == 'ignored':
        return k - 1
    if variant == 'one less':
        a = a - 1
    if variant == 'one more':
        a = a + 1
    kr = uvs_amd.plant.aligned_regressor_step(k, a) if variant is None else max(k - 1 - a, -1)
    if variant == 'clamped' and k >= 1:
        kr = max(kr, 0)
    return kr


def law_step(k, a, variant=None):
    """The step whose joints the law is handed at step k: the rule, or one misreading of it."""
    import uvs_amd
    used = {None: a, 'ignored': 0, 'one less': a - 1, 'one more': a + 1}[variant]
    return uvs_amd.plant.delayed_step(k, used) if variant is None else max(k - max(used, 0), 0)


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def estimator_trial(method, n_points, d, a, nudged=False, variant=None, steps=K):
    """oracle.pixel_loop.run's loop without occluders and hold, on the detections of camera_latency_common.delayed_sensor(d), with the
    regressor of regressor_step(k, a, variant).  The same keys as the oracle's dict.  Read-only, shared by every test of a session."""
    import uvs_amd
    from oracle import rmckf_block, rmckf_dense
    plant, cfg = pl.plant_of(n_points), mc.oracle_settings(n_points)
    noise = mc.oracle_noise(n_points)[:steps]
    desired = np.asarray(pl.DESIRED[:2 * n_points], float)
    m, n = 2 * n_points, 6
    sensor = lc.delayed_sensor(d)
    q = mc.oracle_start() * ((1.0 + pl.CALM_NUDGE) if nudged else 1.0)
    f0 = sensor(plant, q, 0)[0]
    robot = uvs_amd.plant.SyntheticRobot(plant, pl.DT)
    robot.start(q)
    x0 = uvs_amd.plant.analytic_guess(robot, f0, (uvs_amd.plant.RESOLUTION, uvs_amd.plant.RESOLUTION), m, n)
    filt = rmckf_block.BlockFilter(m, n, x0, method, cfg['kernel_bw'], False, steps, pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN)
    log = {key: [] for key in ('q', 'f', 'dq', 'err', 'kappa', 'discs', 'counts', 'fpi_iterations')}
    f_prev, dq = None, np.zeros(n)
    t, ts, status, k_done = pl.DT, [], 0, steps
    for k in range(steps):
        if k:
            q = q + dq * pl.DT                                       # the command integrated into the joints stays dq_{k-1}
        clean, counts, discs = sensor(plant, q, k)
        f = clean + noise[k]
        f_old = f0 if f_prev is None else f_prev
        kr = regressor_step(k, a, variant)
        h = log['dq'][kr] if kr >= 0 else np.zeros(n)
        with np.errstate(all='ignore'):
            kappa = filt.step(f - f_old, h, k)
        err = f - desired
        log['q'].append(q.copy()); log['f'].append(f.copy()); log['discs'].append(discs); log['counts'].append(counts)
        if not np.all(np.isfinite(filt.X)):
            status, k_done = 1, k
            break
        dq = rmckf_block.control_law(filt.X, err, kappa, cfg['gain'])
        log['dq'].append(dq.copy()); log['err'].append(err); log['kappa'].append(np.array(kappa, float))
        log['fpi_iterations'].append(filt.fpi_iterations)
        ts.append(t)
        t += pl.DT
        f_prev = f
    widths = dict(q=n, f=m, dq=n, err=m, kappa=m, discs=(n_points, 3), counts=n_points)
    out = {key: np.array(rows).reshape((len(rows),) + tuple(np.atleast_1d(widths[key]))) if key != 'fpi_iterations' else np.array(rows, int)
           for key, rows in log.items()}
    out.update(status=status, k_done=k_done, pixels=out['counts'].min(axis=0), held=[[] for _ in range(n_points)],
               x0=np.asarray(x0, float).reshape(m * n), f0=f0, stats=rmckf_dense.trial_stats(out['err'], np.array(ts)) if k_done else np.zeros(3))
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def law_trial(n_points, d, a, nudged=False, variant=None, steps=K):
    """The calibrated law through pixels at latency d, told a: camera_analytical_ref.step at the joints of step law_step(k, a, variant) on the
    reported row of step k (the detection of step max(k - d, 0) plus step k's noise).  q, f (k_done + 1 rows, at most K), dq, err (k_done
    rows), discs, counts, status, k_done, pixels, stats.  Read-only, shared."""
    import uvs_amd
    import camera_analytical_ref as ref
    plant, cfg = pl.plant_of(n_points), mc.oracle_settings(n_points)
    noise = mc.oracle_noise(n_points)[:steps]
    m = 2 * n_points
    sensor = lc.delayed_sensor(d)
    robot = uvs_amd.SyntheticRobot(plant, pl.DT)
    q = mc.oracle_start() * ((1.0 + pl.CALM_NUDGE) if nudged else 1.0)
    log = {key: [] for key in ('q', 'f', 'dq', 'err', 'discs', 'counts')}
    acc = np.zeros((3, m))
    t, status, k_done = 0.0 + pl.DT, 0, steps
    for k in range(steps):
        clean, counts, discs = sensor(plant, q, k)
        f = clean + noise[k]
        log['q'].append(q.copy()); log['f'].append(f.copy()); log['discs'].append(discs); log['counts'].append(counts)
        _, err, dq = ref.step(plant, robot, log['q'][law_step(k, a, variant)], f, pl.DESIRED, cfg['gain'])
        if dq is None:
            status, k_done = 1, k
            break
        log['dq'].append(dq); log['err'].append(err)
        acc += np.stack([err * err, np.abs(err), t * np.abs(err)])
        q = q + dq * pl.DT                                           # the joint integration stays current
        t += pl.DT
    widths = dict(q=6, f=m, dq=6, err=m, discs=(n_points, 3), counts=n_points)
    out = {key: np.array(rows).reshape((len(rows),) + tuple(np.atleast_1d(widths[key]))) for key, rows in log.items()}
    out.update(status=status, k_done=k_done, pixels=out['counts'].min(axis=0), stats=np.sqrt((acc ** 2).sum(axis=1)))
    return _frozen(out)
