"""What tests/test_camera_predicted_host.py (CPU) and tests/test_gpu_camera_predicted.py (GPU) share: the (latency, assumed latency, prediction
HORIZON) triples of the predicted pixel loops (include/uvs_vision.h, "FEATURE PREDICTION"; plant.prediction_steps states the steps;
engine.camera_closed_loop(predict=)) -- a per-trial mix for batches, the triples the CPU restatements are run on -- with the sizes and two
numpy restatements of one trial for ANY horizon p:

  estimator_trial   camera_aligned_common.estimator_trial's loop with the law's error formed after the update as (f + X_k s) - desired,
                    s = cmd_{k-1} + ... + cmd_{max(k-p, 0)} summed newest first from zeros.  z, the f log, kappa and the regressor are the
                    aligned loop's.  p = 0 is that loop bit for bit (the host file compares).
  law_trial         camera_aligned_common.law_trial's loop with the law handed f + (h(q_k) - h(q_{max(k-p, 0)})), h = plant.discs(q)[:, :2]
                    of the law's model (here the calibrated one), the difference first.

The settings are those of tests/camera_aligned_common.py (and so of camera_latency_common.py, camera_moving_common.py and
pixel_loop_common.py); K = 16, the same start, noise seed and radius.  `variant` names one misreading of the rule (MISREADINGS): the host
file measures how far each moves q or dq."""
import functools

import numpy as np

import camera_aligned_common as ac
import camera_latency_common as lc
import camera_moving_common as mc
import pixel_loop_common as pl

K = ac.K
SIZES = ac.SIZES                                                     # (3, 259): one trial per workgroup; four, the last with a padding wavefront
RADIUS = ac.RADIUS
MAX_LATENCY = ac.MAX_LATENCY
LATENCIES = (0, 1, 3, 8)                                             # d of a mixed batch
ASSUMED = (0, 3)                                                     # a of a mixed batch
HORIZONS = (0, 1, 2, 3, 8)                                           # p of a mixed batch
TRIPLES = tuple((d, a, p) for p in HORIZONS for a in ASSUMED for d in LATENCIES)   # the 40 (d, a, p) triples
LAST = (3, 3, 8)                                                     # the triple of the last trial of T = 259 alone: the padding wavefront shadows it
CYCLE = tuple(t for t in TRIPLES if t != LAST)                       # 39 triples, walked with stride 7
ORACLE = ac.ORACLE                                                   # (8,6), (8,6), (6,6), (2,6)
ORACLE_HORIZONS = (1, 2, 3)                                          # estimator trials at d = p, a in {0, d}
LAW_HORIZONS = (1, 2, 3, 8)                                          # law trials at d = p, a = 0
# 'clamped': a missing term (k - i < 0) taken as dq_0 instead of zero -- at p = 1 that IS the rule (step 0 has no term, step 1's is dq_0), so
# it applies for p >= 2 alone; 'pre-update X': X_{k-1}, the matrix before step k's update, in place of X_k (estimators alone).
MISREADINGS = ('ignored', 'one less', 'one more', 'clamped', 'pre-update X')
LAW_MISREADINGS = ('ignored', 'one less', 'one more')
# (what, ..., misreading) -> measured distance: an "off by one" misreading that falls under TEETH_MIN, as pixel_loop_common.NO_TEETH lists
# its own.  The host file asserts that every entry is still under TEETH_MIN and that nothing else is.
NO_TEETH = {}


def applicable(p, estimator=True):
    """The misreadings that are not the rule itself at horizon p."""
    names = MISREADINGS if estimator else LAW_MISREADINGS
    return tuple(name for name in names if not (name == 'clamped' and p < 2))


def mixed(T):
    """(d, a, p), three (T,) arrays: trial t has CYCLE[(7 t + 5) % 39] -- the trials of T = 3 have (1, 3, 0), (0, 3, 1) and (8, 0, 2), three
    different horizons -- and the last trial of T = 259 has LAST = (3, 3, 8), which no other trial has."""
    triples = [CYCLE[(7 * t + 5) % len(CYCLE)] for t in range(T)]
    if T > 3:
        triples[-1] = LAST
    d, a, p = np.array(triples, np.int64).T
    return d.copy(), a.copy(), p.copy()


def summed_steps(k, p, variant=None):
    """The steps whose commands are summed at step k, newest first (a zero vector is left out): the rule, or one misreading of it."""
    import uvs_amd
    if variant in (None, 'pre-update X'):
        return uvs_amd.plant.prediction_steps(k, p)
    if variant == 'ignored':
        return []
    if variant == 'one less':
        p = p - 1
    if variant == 'one more':
        p = p + 1
    p = min(max(p, 0), MAX_LATENCY + 1)                              # a misreading may look nine steps back
    steps = [k - i for i in range(1, p + 1)]
    if variant == 'clamped':
        return [max(s, 0) for s in steps] if k >= 1 else []
    return [s for s in steps if s >= 0]


def shown_step(k, p, variant=None):
    """The step whose joints the law's prediction starts from at step k: the rule, or one misreading of it."""
    import uvs_amd
    used = {None: p, 'ignored': 0, 'one less': p - 1, 'one more': p + 1}[variant]
    return uvs_amd.plant.delayed_step(k, p) if variant is None else max(k - max(used, 0), 0)


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def estimator_trial(method, n_points, d, a, p, nudged=False, variant=None, steps=K):
    """camera_aligned_common.estimator_trial(method, n_points, d, a) whose control law sees err = (f + X_k s) - desired, s the sum of the
    commands of summed_steps(k, p, variant).  The same keys.  Read-only, shared by every test of a session."""
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
        kr = ac.regressor_step(k, a)
        h = log['dq'][kr] if kr >= 0 else np.zeros(n)
        x_before = np.array(filt.X, float).reshape(m, n)
        with np.errstate(all='ignore'):
            kappa = filt.step(f - f_old, h, k)                       # z and kappa come from the reported row
        s = np.zeros(n)
        for i in summed_steps(k, p, variant):                        # newest first
            s = s + log['dq'][i]
        x_used = x_before if variant == 'pre-update X' else np.asarray(filt.X, float).reshape(m, n)
        with np.errstate(all='ignore'):
            err = (f + x_used @ s) - desired
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
def law_trial(n_points, d, a, p, nudged=False, variant=None, steps=K):
    """camera_aligned_common.law_trial(n_points, d, a) whose law is handed f + (h(q_k) - h(q_j)), j = shown_step(k, p, variant),
    h = plant.discs(q)[:, :2] of the law's own model (the calibrated one; its points do not move).  The f log stays the reported row.
    Read-only, shared."""
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
    model = lambda joints: plant.discs(joints, RADIUS)[:, :2].reshape(m)   # noqa: E731
    for k in range(steps):
        clean, counts, discs = sensor(plant, q, k)
        f = clean + noise[k]
        log['q'].append(q.copy()); log['f'].append(f.copy()); log['discs'].append(discs); log['counts'].append(counts)
        moved = model(log['q'][k]) - model(log['q'][shown_step(k, p, variant)])
        _, err, dq = ref.step(plant, robot, log['q'][ac.law_step(k, a)], f + moved, pl.DESIRED, cfg['gain'])
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
