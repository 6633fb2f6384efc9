"""What tests/test_camera_score_host.py (CPU) and tests/test_gpu_camera_score.py (GPU) share: the X log of the one-launch estimator loop,
the true image Jacobian and the score of an X stream against it (include/uvs_vision.h, "THE ESTIMATE AS A LOG" and "THE TRUE IMAGE
JACOBIAN"; plant.projection_jacobian, plant.jacobian_score; engine.camera_jacobian, engine.camera_jacobian_score).

  logged_trial       camera_predicted_common.estimator_trial's loop, restated, which additionally records X_k after filt.step: key 'x',
                     (k_done, m n).  Every other key is that function's bit for bit (the host file compares), so it is the oracle's loop
                     and nothing else.
  poses              seeded joint vectors: the goal pose +- SPREAD rad.
  misread_jacobian   plant.projection_jacobian with ONE named misreading of the rule; the host file measures how far each lies from it.
  numpy_jacobians    the rule for a (K, T, 6) or (T, 6) array of joints over per-trial plants, motions and a first step.

The sizes are those of the other pixel suites: T = 3 (one trial per workgroup), T = 259 (four per workgroup, the last workgroup with
padding wavefronts), K = 16."""
import functools

import numpy as np

import camera_aligned_common as ac
import camera_common as cc
import camera_latency_common as lc
import camera_moving_common as mc
import camera_predicted_common as pc
import pixel_loop_common as pl

K = pc.K
SIZES = pc.SIZES
RADIUS = pc.RADIUS
ORACLE = pc.ORACLE
SPREAD = 0.15                                                        # rad around the goal pose
FD_STEP = 1e-5                                                       # central differences of plant.features
FD_BOUND = 1e-7                                                      # relative Frobenius: measured 1.6e-10; truncation stays O(h^2)
MISREAD_MIN = 1e-3                                                   # every named misreading lies at least this far from the rule
X_BOUND = 1e-10                                                      # the X log against the CPU restatement, relative
J_BOUND = 1e-10                                                      # a device Jacobian record against the rule, relative to |J|_F
SUM_BOUND = 1e-10                                                    # the six sums against plant.jacobian_score
MISREADINGS = ('uncentred pixels', 'distance for depth', 'no w x term', 'sign of v', 'analytic_guess')


def poses(n, seed=0, spread=SPREAD):
    return cc.Q_GOAL + np.random.default_rng(seed).uniform(-spread, spread, (n, 6))


def central_differences(plant, q, h=FD_STEP):
    eye = np.eye(6)
    return np.stack([(plant.features(q + h * eye[j]) - plant.features(q - h * eye[j])) / (2 * h) for j in range(6)], axis=1)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def misread_jacobian(uvs, plant, q, name):
    """plant.projection_jacobian(plant, q) under one misreading of its rule."""
    P = uvs.plant
    Ts = plant.fkine_all(q)
    R, c = Ts[-1][:3, :3], Ts[-1][:3, 3]
    Jg = plant.jacobian(Ts)
    m = 2 * plant.n_points
    if name == 'analytic_guess':                                     # the reference's initial guess itself: all three quirks
        robot = P.SyntheticRobot(plant, pl.DT)
        robot.start(q)
        return P.analytic_guess(robot, plant.features(q), (P.RESOLUTION, P.RESOLUTION), m, 6).reshape(m, 6)
    if name in ('uncentred pixels', 'distance for depth'):           # the interaction row on the camera-frame twist, one quirk at a time
        twist = np.kron(np.eye(2), R.T) @ Jg
        f = plant.features(q)
        out = np.empty((m, 6))
        for i, w in enumerate(plant.points):
            p = R.T @ (w - c)
            u, v = (f[2 * i], f[2 * i + 1]) if name == 'uncentred pixels' else (f[2 * i] - plant.center, f[2 * i + 1] - plant.center)
            z = np.linalg.norm(w - c) if name == 'distance for depth' else p[2]
            F = plant.focal
            out[2 * i] = np.array([-F / z, 0.0, u / z, u * v / F, -(F * F + u * u) / F, v]) @ twist
            out[2 * i + 1] = np.array([0.0, -F / z, v / z, (F * F + v * v) / F, -u * v / F, -u]) @ twist
        return out
    out = np.empty((m, 6))
    for i, w in enumerate(plant.points):
        p = R.T @ (w - c)
        for j in range(6):
            turn = np.zeros(3) if name == 'no w x term' else np.cross(Jg[3:, j], w - c)
            lin = -Jg[:3, j] if name == 'sign of v' else Jg[:3, j]
            dp = -R.T @ (turn + lin)
            out[2 * i, j] = plant.focal * (dp[0] / p[2] - p[0] * dp[2] / p[2] ** 2)
            out[2 * i + 1, j] = plant.focal * (dp[1] / p[2] - p[1] * dp[2] / p[2] ** 2)
    return out


def numpy_jacobians(uvs, plants, q, velocity=None, window=None, k0=0):
    """plant.projection_jacobian for q (T, 6) or (K, T, 6): trial t on plants[t], its points where step k0 + r of (velocity[t], window[t])
    has taken them (None: nothing moves).  (..., m, 6)."""
    q = np.asarray(q, float)
    rows = q.reshape((-1,) + q.shape[-2:])
    out = np.empty(rows.shape[:2] + (2 * plants[0].n_points, 6))
    for r in range(rows.shape[0]):
        for t in range(rows.shape[1]):
            points = None
            if velocity is not None:
                points = uvs.plant.target_at(plants[t], velocity[t], k0 + r, tuple(int(w) for w in window[t])).points
            out[r, t] = uvs.plant.projection_jacobian(plants[t], rows[r, t], points)
    return out.reshape(q.shape[:-1] + out.shape[-2:])


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def logged_trial(method, n_points, d=0, a=0, p=0, steps=K):
    """camera_predicted_common.estimator_trial(method, n_points, d, a, p) restated, with the key 'x': row k = X_k, the matrix after
    filt.step of step k, (m n,) row-major -- recorded for the steps whose err, kappa and dq rows are.  Read-only, shared."""
    import uvs_amd
    from oracle import rmckf_block, rmckf_dense
    plant, cfg = pl.plant_of(n_points), mc.oracle_settings(n_points)
    noise = mc.oracle_noise(n_points)[:steps]
    desired = np.asarray(pl.DESIRED[:2 * n_points], float)
    m, n = 2 * n_points, 6
    sensor = lc.delayed_sensor(d)
    q = mc.oracle_start()
    f0 = sensor(plant, q, 0)[0]
    robot = uvs_amd.plant.SyntheticRobot(plant, pl.DT)
    robot.start(q)
    x0 = uvs_amd.plant.analytic_guess(robot, f0, (uvs_amd.plant.RESOLUTION, uvs_amd.plant.RESOLUTION), m, n)
    filt = rmckf_block.BlockFilter(m, n, x0, method, cfg['kernel_bw'], False, steps, pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN)
    log = {key: [] for key in ('q', 'f', 'dq', 'err', 'kappa', 'discs', 'counts', 'fpi_iterations', 'x')}
    f_prev, dq = None, np.zeros(n)
    t, ts, status, k_done = pl.DT, [], 0, steps
    for k in range(steps):
        if k:
            q = q + dq * pl.DT
        clean, counts, discs = sensor(plant, q, k)
        f = clean + noise[k]
        f_old = f0 if f_prev is None else f_prev
        kr = ac.regressor_step(k, a)
        h = log['dq'][kr] if kr >= 0 else np.zeros(n)
        with np.errstate(all='ignore'):
            kappa = filt.step(f - f_old, h, k)
        x_k = np.array(filt.X, float).reshape(m * n)                 # X_k: what this step's law and prediction read
        s = np.zeros(n)
        for i in pc.summed_steps(k, p):
            s = s + log['dq'][i]
        with np.errstate(all='ignore'):
            err = (f + x_k.reshape(m, n) @ s) - desired
        log['q'].append(q.copy()); log['f'].append(f.copy()); log['discs'].append(discs); log['counts'].append(counts)
        if not np.all(np.isfinite(filt.X)):
            status, k_done = 1, k
            break
        dq = rmckf_block.control_law(filt.X, err, kappa, cfg['gain'])
        log['dq'].append(dq.copy()); log['err'].append(err); log['kappa'].append(np.array(kappa, float)); log['x'].append(x_k)
        log['fpi_iterations'].append(filt.fpi_iterations)
        ts.append(t)
        t += pl.DT
        f_prev = f
    widths = dict(q=n, f=m, dq=n, err=m, kappa=m, discs=(n_points, 3), counts=n_points, x=m * n)
    out = {key: np.array(rows).reshape((len(rows),) + tuple(np.atleast_1d(widths[key]))) if key != 'fpi_iterations' else np.array(rows, int)
           for key, rows in log.items()}
    out.update(status=status, k_done=k_done, pixels=out['counts'].min(axis=0), held=[[] for _ in range(n_points)],
               x0=np.asarray(x0, float).reshape(m * n), f0=f0, stats=rmckf_dense.trial_stats(out['err'], np.array(ts)) if k_done else np.zeros(3))
    return _frozen(out)
