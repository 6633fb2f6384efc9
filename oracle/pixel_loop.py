"""Oracle (test infrastructure): the PIXEL closed loop on the CPU, one trial at a time.

The loop of include/uvs_vision.h (the text at uvs_camera_closed_loop_f64 and at uvs_camera_closed_loop_held_f64) restated from parts that are
each held to the reference on their own: ``plant.SyntheticPlant.discs`` (the projection), ``plant.render_discs`` (the pixel rule, occluders and
paints included), the host detector of ``utils.py`` (bit for bit to the reference's outputs, tests/test_detect.py), ``plant.hold_features``,
``plant.analytic_guess``, ``rmckf_block.BlockFilter`` / ``control_law`` and ``rmckf_dense.trial_stats``.  Step k:

    q_k = q_{k-1} + dq_{k-1} * dt                         (q_0 = q_start)
    f_k = detector(frame of plant.discs(q_k) behind the occluders at step k) + noise_k, then the hold rule on the integer mask counts
    z   = f_k - f_{k-1}                                   (f_{-1}: the noise-free step-0 detection with initial_guess, else zeros)
    BlockFilter.step(z, dq_{k-1}, k)                      (a zero regressor at k = 0);   err = f_k - desired
    a non-finite X: status FAIL, k_done = k, the trial stops;   otherwise dq_k = control_law(X, err, kappa, gain)

Rows q[k], f[k] exist for k <= k_done, rows dq[k], err[k], kappa[k] for k < k_done.  No torch and no library handle is imported: the loop
runs on any machine.  ``mutation`` names one deliberate misreading of that text (MUTATIONS): the suites measure how far each one moves the
joints, so that a kernel or a glue that made the same mistake could not pass their gates."""
import numpy as np

from . import rmckf_block, rmckf_dense

MUTATIONS = ('anneal_k_plus_1',        # sigma_k evaluated at k + 1
             'f_old_noise_free',       # z = f_k - (f_{k-1} without its noise)
             'regressor_halved',       # the regressor is dq_{k-1} / 2
             'regressor_stale',        # the regressor is dq_{k-2}
             'kappa_dropped',          # the command is -gain pinv(X) err
             'held_pair_new_noise',    # a held pair is given step k's noise on top
             'f0_unoccluded',          # f_{-1} comes from the step-0 frame without the occluders (it meets a zero regressor: only kappa sees it)
             'step0_unoccluded')       # f_{-1} and the guess made from it both come from that frame
_DETECTORS = {1: 'detectGreenCircle', 3: 'detectRGBCircles', 4: 'detect4Circles'}
_THRESHOLD = 250                                                     # utils.py:15


def mask_counts(frame, n_points):
    """Mask sizes per feature pair of an n_points-colour camera, by the reference's integer thresholds (utils.py:15-24, :130-144)."""
    r, g, b = (np.asarray(frame)[..., ch].astype(int) for ch in range(3))
    lo, hi = (lambda x: x < _THRESHOLD), (lambda x: x > _THRESHOLD)
    masks = (hi(r) & lo(g) & lo(b), lo(r) & hi(g) & lo(b), lo(r) & lo(g) & hi(b), hi(r) & lo(g) & hi(b))
    four = np.array([int(mk.sum()) for mk in masks])
    return four[1:2] if n_points == 1 else four[:n_points]


def detect(plant, q, k, radius=None, occluders=None, occluder_colours=None):
    """(f, counts, discs): the host detector's features (NaN pairs for empty masks), the mask sizes and the discs of the frame at joints q
    behind the occluders at step k."""
    from uvs_amd import plant as plant_mod, utils
    n_points = plant.n_points
    discs = plant.discs(q, plant_mod.DISC_RADIUS if radius is None else radius)
    frame = plant_mod.render_discs(discs, n_points, occluders=occluders, k=k, occluder_colours=occluder_colours)
    with np.errstate(invalid='ignore', divide='ignore'):             # an empty mask divides 0 by 0, like the reference
        f = np.asarray(getattr(utils, _DETECTORS[n_points])(frame), float)
    return f, mask_counts(frame, n_points), discs


def ideal(plant, q, k):
    """The sensor swapped for the ideal projection: what ties this loop to rmckf_block.run_closed_loop."""
    return plant.features(q), np.full(plant.n_points, 1 << 16), np.zeros((plant.n_points, 3))


def run(plant, q_start, desired, noise, dt, K, gain, method, kernel_bw, annealing, k_max, fpi_threshold, fpi_epoch_max, reg, anneal_span,
        initial_guess=True, x0=None, radius=None, occluders=None, occluder_colours=None, hold=0, sensor=None, mutation=None):
    """One trial of K steps.  ``noise`` (K, m) or None; ``occluders`` (n_occ, 8) integer rows or None, ``occluder_colours`` (n_occ,) or None;
    ``sensor``: None (pixels) or a callable (plant, q, k) -> (f, counts, discs), e.g. ``ideal``; ``mutation``: None or one of MUTATIONS.
    Returns a dict: q, f (k_done + 1 rows, at most K), dq, err, kappa (k_done rows), status, k_done, pixels (n_points,), held (per disc, the
    list of steps), stats (3,), fpi_iterations (per step), discs and counts (per step, for the preconditions of the suites), x0, f0."""
    from uvs_amd import plant as plant_mod
    assert mutation is None or mutation in MUTATIONS, mutation
    desired = np.asarray(desired, float)
    m, n, npts = len(desired), len(q_start), plant.n_points
    assert m == 2 * npts

    def see(q, k, occ=occluders):
        if sensor is not None:
            return sensor(plant, q, k)
        return detect(plant, q, k, radius, occ, occluder_colours if occ is not None else None)

    q = np.array(q_start, float)
    f0 = np.zeros(m)
    if initial_guess:
        f0 = see(q, 0, None if mutation == 'step0_unoccluded' else occluders)[0]
        if x0 is None:
            robot = plant_mod.SyntheticRobot(plant, dt)
            robot.start(q)
            x0 = plant_mod.analytic_guess(robot, f0, (plant_mod.RESOLUTION, plant_mod.RESOLUTION), m, n)
        if mutation == 'f0_unoccluded':
            f0 = see(q, 0, None)[0]
    assert x0 is not None, 'x0 is needed without initial_guess'
    filt = rmckf_block.BlockFilter(m, n, x0, method, kernel_bw, annealing, k_max, fpi_threshold, fpi_epoch_max, reg, anneal_span)
    log = {key: [] for key in ('q', 'f', 'dq', 'err', 'kappa', 'discs', 'counts', 'fpi_iterations')}
    held = [[] for _ in range(npts)]
    miss = np.zeros((1, npts), np.int64)
    f_prev, clean_prev = None, f0                                    # the reported row of step k - 1; the same row without its noise
    dq, dq_before = np.zeros(n), np.zeros(n)
    t, ts, status, k_done = dt, [], 0, K
    for k in range(K):
        if k:
            q = q + dq * dt
        clean, counts, discs = see(q, k)
        f = clean + (noise[k] if noise is not None else 0.0)
        f, miss, held_now = plant_mod.hold_features(f[None], None if f_prev is None else f_prev[None], counts[None], miss, hold)
        f, held_now = f[0], held_now[0].astype(bool)
        pairs = np.repeat(held_now, 2)
        clean = np.where(pairs, clean_prev, clean)
        if mutation == 'held_pair_new_noise' and noise is not None:
            f = np.where(pairs, f + noise[k], f)
        for j in np.flatnonzero(held_now):
            held[j].append(k)
        f_old = f0 if f_prev is None else (clean_prev if mutation == 'f_old_noise_free' else f_prev)
        h = {'regressor_halved': 0.5 * dq, 'regressor_stale': dq_before}.get(mutation, dq)
        with np.errstate(all='ignore'):
            kappa = filt.step(f - f_old, h, k + 1 if mutation == 'anneal_k_plus_1' else k)
        err = f - desired
        log['q'].append(q.copy()); log['f'].append(f.copy()); log['discs'].append(discs); log['counts'].append(counts)
        if not np.all(np.isfinite(filt.X)):
            status, k_done = 1, k
            break
        dq_before, dq = dq, rmckf_block.control_law(filt.X, err, np.ones(m) if mutation == 'kappa_dropped' else kappa, gain)
        log['dq'].append(dq.copy()); log['err'].append(err); log['kappa'].append(np.array(kappa, float))
        log['fpi_iterations'].append(filt.fpi_iterations)
        ts.append(t)
        t += dt
        f_prev, clean_prev = f, clean
    widths = dict(q=n, f=m, dq=n, err=m, kappa=m, discs=(npts, 3), counts=npts, fpi_iterations=())
    out = {key: np.array(rows).reshape((len(rows),) + tuple(np.atleast_1d(widths[key]))) if key != 'fpi_iterations' else np.array(rows, int)
           for key, rows in log.items()}
    out.update(status=status, k_done=k_done, pixels=out['counts'].min(axis=0), held=held, x0=np.asarray(x0, float).reshape(m * n), f0=f0,
               stats=rmckf_dense.trial_stats(out['err'], np.array(ts)) if k_done else np.zeros(3))
    return out
