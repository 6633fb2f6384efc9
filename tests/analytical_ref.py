"""Vectorised numpy restatement of the calibrated IBVS baseline (Method.ANALYTICAL, experiment.py:145-162 and :300-320) over a batch of
trials, on the plant of oracle/plant_ref.py or on any DH / pinhole plant handed over (``plant=``): the checker of
uvs_analytical_closed_loop_f64.  Per step: f = project(q) + noise; J_image from the noisy raw-pixel u, v and the
Euclidean camera-disc distance; J_feature = J_image kron(I2, R^T) J_robot; pinv raises on a non-finite J_feature (FAIL, k_done = k); dq = -gain pinv(J_feature) (f - desired); q += dq dt.  np.linalg.pinv on stacks follows numpy's cutoff."""
import numpy as np

from oracle import plant_ref


def _dh_batch(theta, d, a, alpha):
    """plant_ref.dh_link for a vector of angles: Rz(theta) Tz(d) Rx(alpha) Tx(a), (B, 4, 4)."""
    B = theta.shape[0]
    c, s = np.cos(theta), np.sin(theta)
    ca, sa = np.cos(alpha), np.sin(alpha)
    rz = np.zeros((B, 4, 4))
    rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = c, -s, s, c
    rz[:, 2, 2], rz[:, 2, 3], rz[:, 3, 3] = 1.0, d, 1.0
    rx = np.array([[1.0, 0.0, 0.0, a], [0.0, ca, -sa, 0.0], [0.0, sa, ca, 0.0], [0.0, 0.0, 0.0, 1.0]])
    return rz @ rx


PLANT_KEYS = ('theta_offset', 'd', 'a', 'alpha', 'focal', 'center', 'points')


def plant_values(plant=None):
    """dict of PLANT_KEYS from a plant description -- a uvs_amd.SyntheticPlant or a dict with any of those keys; what is missing (None:
    everything) is the UR10 / pinhole plant of oracle/plant_ref.py with its discs."""
    table = np.array(plant_ref.DH_TABLE)
    out = dict(theta_offset=table[:, 0], d=table[:, 1], a=table[:, 2], alpha=table[:, 3], focal=plant_ref.FOCAL, center=plant_ref.CENTER, points=None)
    if plant is not None:
        unknown = set(plant) - set(PLANT_KEYS) if isinstance(plant, dict) else ()
        assert not unknown, unknown
        for key in PLANT_KEYS:
            value = plant.get(key) if isinstance(plant, dict) else getattr(plant, key)
            if value is not None:
                out[key] = value
    if out['points'] is None:
        out['points'] = plant_ref.place_discs()
    return {k: float(v) if k in ('focal', 'center') else np.array(v, float) for k, v in out.items()}


def fkine_all_batch(q, plant=None):
    """plant_ref.fkine_all for (B, 6) joints, on the DH table of ``plant`` (plant_values): list of six (B, 4, 4) cumulative transforms."""
    pv = plant_values(plant)
    out, T = [], None
    for i, (off, d, a, alpha) in enumerate(zip(pv['theta_offset'], pv['d'], pv['a'], pv['alpha'])):
        link = _dh_batch(q[:, i] + off, d, a, alpha)
        T = link if i == 0 else T @ link
        out.append(T)
    return out


def geometric_jacobian_batch(Ts):
    """plant_ref.geometric_jacobian for (B, 4, 4) transforms: (B, 6, 6)."""
    B = Ts[0].shape[0]
    p_e = Ts[5][:, :3, 3]
    J = np.zeros((B, 6, 6))
    z_prev, p_prev = np.tile([0.0, 0.0, 1.0], (B, 1)), np.zeros((B, 3))
    for i in range(6):
        J[:, :3, i] = np.cross(z_prev, p_e - p_prev)
        J[:, 3:, i] = z_prev
        z_prev, p_prev = Ts[i][:, :3, 2], Ts[i][:, :3, 3]
    return J


def run(q_start, noise=None, desired=plant_ref.DESIRED_F, dt=0.05, t_max=15.0, gain=0.2, points=None, steps=None,
        logs=('err', 'q', 'f', 'dq', 'j'), plant=None):
    """q_start (B, 6); noise (B, K, 8) or None; ``plant``: a plant description (plant_values; None: oracle/plant_ref.py's), whose discs
    ``points`` replaces when given.  Returns dict of the per-step streams named in ``logs`` (B, K, .) -- rows at and after
    k_done are zero -- plus status (B,), k_done (B,), stats (B, 3) = ||ISE||, ||IAE||, ||ITAE|| over the features, and t (K,).
    ``logs=()`` keeps only the statistics (full-size batches: the J stream of 65 536 trials is 7.5 GB)."""
    q = np.array(q_start, float).reshape(-1, 6).copy()
    B = q.shape[0]
    pv = plant_values(plant)
    discs = pv['points'] if points is None else np.asarray(points, float)
    P = len(discs)
    m = 2 * P
    desired = np.asarray(desired, float)
    ts, t = [], dt                                               # the loop clock (engine.loop_clock)
    while t < t_max:
        ts.append(t)
        t += dt
    K = len(ts) if steps is None else int(steps)
    ts = np.array(ts[:K])
    logs = {k: np.zeros((B, K, c)) for k, c in (('err', m), ('q', 6), ('f', m), ('dq', 6), ('j', m * 6)) if k in logs}
    acc = np.zeros((B, 3, m))                                    # per-feature sums of e^2, |e|, t |e| over the logged steps
    status, k_done = np.zeros(B, np.int32), np.full(B, K, np.int32)
    alive = np.ones(B, bool)
    F, center = pv['focal'], pv['center']
    for k in range(K):
        Ts = fkine_all_batch(q, pv)
        R, pos = Ts[5][:, :3, :3], Ts[5][:, :3, 3]
        f = np.zeros((B, m))
        Z = np.zeros((B, P))
        for i, d in enumerate(discs):
            pc = np.einsum('bji,bj->bi', R, d - pos)             # R^T (d - t)
            f[:, 2 * i] = center + F * pc[:, 0] / pc[:, 2]
            f[:, 2 * i + 1] = center + F * pc[:, 1] / pc[:, 2]
            Z[:, i] = np.linalg.norm(pos - d, axis=1)
        if noise is not None:
            f = f + noise[:, k, :m]
        Ji = np.zeros((B, m, 6))
        for i in range(P):
            u, v, z = f[:, 2 * i], f[:, 2 * i + 1], Z[:, i]
            Ji[:, 2 * i, 0] = -F / z
            Ji[:, 2 * i + 1, 1] = -F / z
            Ji[:, 2 * i, 2] = u / z
            Ji[:, 2 * i + 1, 2] = v / z
            Ji[:, 2 * i, 3] = u * v / F
            Ji[:, 2 * i + 1, 3] = (F ** 2 + v ** 2) / F
            Ji[:, 2 * i, 4] = -(F ** 2 + u ** 2) / F
            Ji[:, 2 * i + 1, 4] = -u * v / F
            Ji[:, 2 * i, 5] = v
            Ji[:, 2 * i + 1, 5] = -u
        kronRT = np.zeros((B, 6, 6))
        kronRT[:, :3, :3] = np.transpose(R, (0, 2, 1))
        kronRT[:, 3:, 3:] = np.transpose(R, (0, 2, 1))
        with np.errstate(all='ignore'):
            J = Ji @ kronRT @ geometric_jacobian_batch(Ts)
        err = f - desired
        bad = alive & ~np.isfinite(J).reshape(B, -1).all(axis=1)  # pinv raises (experiment.py:313-316)
        status[bad], k_done[bad] = 1, k
        alive &= ~bad
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        dq = np.zeros((B, 6))
        dq[idx] = (-gain * np.linalg.pinv(J[idx]) @ err[idx][:, :, None])[:, :, 0]
        for key, val in (('err', err), ('q', q), ('f', f), ('dq', dq), ('j', J.reshape(B, -1))):
            if key in logs:
                logs[key][idx, k] = val[idx]
        ae = np.abs(err[idx])
        acc[idx, 0] += err[idx] * err[idx]
        acc[idx, 1] += ae
        acc[idx, 2] += ts[k] * ae
        q[idx] = q[idx] + dq[idx] * dt
    return dict(logs, status=status, k_done=k_done, t=ts, stats=np.sqrt((acc ** 2).sum(axis=2)))
