"""Cases shared by tests/test_pixel_loop_oracle.py (CPU) and tests/test_gpu_pixel_loop_oracle.py (GPU): the pixel closed loops
(engine.camera_closed_loop, stepwise and as one launch) against oracle/pixel_loop.py, the loop of include/uvs_vision.h restated on the CPU.

A CASE is a tuple of at most eight distinct TRIALS that share what one launch shares -- shape, estimator, annealing, initial_guess, the
strict option, hold, K -- and may differ in everything a launch takes per trial: the start, the noise, the occluders and their paints, and
(in the grid cases, which the one launch runs through trial_params) kernel_bw, gain, reg, fpi_threshold and desired.  A batch of T output
trials is tiled from them: output trial t is trial t % E of the case.  The oracle runs each distinct trial once per session (lru_cache).

The plant is SyntheticPlant.ur10(desired_f=DESIRED[:m]), dt 0.05, gain 0.2, K = 20 steps, noise 0.3 px: the settings of the four
host-route tests.  The (2,6) loop hardly moves from the starts of the larger shapes (one disc: two features for six joints), and a
misreading then moves q by 1e-10 or less; its cases start 0.1 rad further out, with 1 px of noise and gain 0.6 (ONE_DISC; at kernel_bw 2
IMCC-KF weighs every step to nothing there, so the bandwidth stays 10).

PRECONDITIONS (test_pixel_loop_oracle.py asserts them for every trial of every case): on the oracle's trajectory no pixel comes within
1e-6 of a rim; the trial is calm (re-run from q_start (1 + 1e-14): the same status, k_done, masks, holds and fixed-point iteration counts,
logs within 1e-10); and, where the scenario is not about clipping, the discs stay inside the frame with masks of at least 50 pixels
(behind an occluder, whose business is to clip a mask, the discs still stay inside the frame and the mask sizes are compared exactly).
TEETH: oracle_trial(..., mutation=) runs one misreading of the loop's text; every applicable one sits at least 100 gates from the
unmutated run in q or dq (TEETH_MIN); the (2,6) entries that do not are listed in NO_TEETH with their measured distances."""
import collections
import functools

import numpy as np

import camera_common as cc
import camera_hold_common as hc
import camera_occluders_common as oc
import camera_painted_common as pc

DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
DT, GAIN, K, NOISE_PX = 0.05, 0.2, 20, 0.3
REG, ANNEAL_SPAN, BW = 0.001 ** 2, 100.0, 10.0
FPI_THRESHOLD, FPI_EPOCH_MAX = 1e-4, 1000                            # MCKF iterates at 1e-4 (closed_shapes_common.py)
METHODS = ('GMCKF', 'KF', 'IMCCKF', 'MCKF')
# the start poses of the host-route tests, and the one from which the loop swings all four discs out of view
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
Q_LEAVES = np.array([-0.47915568, -0.55367504, 2.20583478, -0.05228325, -1.09351535, 0.40221985])
GATE = 1e-8                                                          # err, q, f, stats (gpu_harness.TOL)
GATE_DQ = 1e-7                                                       # the command (gpu_harness.STEP_GATES)
GATE_KAPPA = 1e-8
TEETH_MIN = 100 * GATE                                               # 1e-6: in q or dq
CALM_NUDGE, CALM_TOL, RIM_MIN, MASK_MIN = 1e-14, 1e-10, 1e-6, 50
# (2,6): a start further from the target, more noise, a higher gain
ONE_DISC = dict(kernel_bw=BW, gain=0.6, noise_px=1.0)
Q_ONE_DISC = Q_HOST_ROUTE[0] + np.array([0.10, -0.08, 0.09, 0.07, -0.10, 0.08])

Trial = collections.namedtuple('Trial', 'q_start seed kernel_bw gain reg fpi_threshold desired occluders paints x0_seed')
Case = collections.namedtuple('Case', 'name n_points method annealing initial_guess strict noise_px hold K trials clipping guess grid anneal_span')


def jittered(seed, base=Q_HOST_ROUTE[0], spread=0.05):
    return base + np.random.default_rng(seed).uniform(-spread, spread, 6)


def trial(n_points, q_start, seed, kernel_bw=BW, gain=GAIN, reg=REG, fpi_threshold=FPI_THRESHOLD, desired=None, occluders=None, paints=None,
          x0_seed=None):
    desired = DESIRED[:2 * n_points] if desired is None else desired
    occluders = None if occluders is None else tuple(tuple(int(v) for v in row) for row in occluders)
    paints = None if paints is None else tuple(int(p) for p in paints)
    return Trial(tuple(float(v) for v in q_start), seed, float(kernel_bw), float(gain), float(reg), float(fpi_threshold),
                 tuple(float(v) for v in desired), occluders, paints, x0_seed)


def case(name, n_points, method, annealing=False, trials=None, initial_guess=True, strict=False, noise_px=NOISE_PX, hold=0, steps=K,
         clipping=False, guess='host', grid=False, anneal_span=ANNEAL_SPAN, **per_trial):
    if trials is None:
        starts = START_SEEDS.get(name, DEFAULT_STARTS[n_points])
        trials = tuple(trial(n_points, start_pose(n_points, s), 100 + i, **{**(ONE_DISC_TRIAL if n_points == 1 else {}), **per_trial})
                       for i, s in enumerate(starts))
    if n_points == 1 and noise_px == NOISE_PX:
        noise_px = ONE_DISC['noise_px']
    return Case(name, n_points, method, annealing, initial_guess, strict, noise_px, hold, steps, tuple(trials), clipping, guess, grid, anneal_span)


ONE_DISC_TRIAL = dict(kernel_bw=ONE_DISC['kernel_bw'], gain=ONE_DISC['gain'])
# start s: 'h0' / 'h1' the host-route poses, an integer a seeded jitter around the first (around Q_ONE_DISC for one disc)
DEFAULT_STARTS = {4: ('h0', 'h1'), 3: ('h0', 'h1'), 1: (0, 1)}
# a case whose default starts missed a precondition would get others here, chosen on the CPU: none does
START_SEEDS = {}


def start_pose(n_points, s):
    if s == 'h0' or s == 'h1':
        return Q_HOST_ROUTE[int(s[1])]
    return jittered(s, Q_ONE_DISC if n_points == 1 else Q_HOST_ROUTE[0])


# ------------------------------------------------------------------------------------------------------------- the scenes of the scenarios
def pair_of(n_points):
    return 0 if n_points == 1 else 1


def bar_rows(n_points):
    """The sweeping bar of the occluder suite and the still half cover of the disc the servo brings to its place: partial occlusion."""
    return [oc.sweeping_bar(), oc.half_cover(DESIRED[:2 * n_points], pair_of(n_points))]


def wide_rows(n_points):
    """The hold suite's bar, wider than a disc, which empties each mask for a few steps; the half cover makes the step-0 frame differ."""
    return [hc.wide_bar(), oc.half_cover(DESIRED[:2 * n_points], pair_of(n_points))]


def distractor_rows(n_points, with_bar):
    """The painted suite's still distractor, painted the first disc's colour; with_bar: behind the wide bar, where the other discs are lost
    and held while the first one's mask never empties (its distractor stays visible)."""
    rows, paints = pc.still_distractor(0)
    if with_bar:
        return [hc.wide_bar()] + rows, [pc.OPAQUE] + paints
    return rows + [oc.half_cover(DESIRED[:2 * n_points], pair_of(n_points))], paints + [pc.OPAQUE]


# ------------------------------------------------------------------------------------------------------------- the cases
def _cases():
    out = []
    shapes = {4: '86', 3: '66', 1: '26'}
    for method in METHODS:                                           # a. estimators x shapes x annealing
        for n_points in (4, 3, 1):
            for annealing in (False, True):
                out.append(case(f'a_{method}_{shapes[n_points]}_{"anneal" if annealing else "plain"}', n_points, method, annealing))
    for method, n_points in (('GMCKF', 4), ('KF', 3)):               # b. variants
        tag = f'{method}_{shapes[n_points]}'
        out.append(case(f'b_{tag}_x0', n_points, method, initial_guess=False, x0_seed=7))
        out.append(case(f'b_{tag}_strict', n_points, method, strict=True))
        out.append(case(f'b_{tag}_noiseless', n_points, method, noise_px=0.0))
    for method, n_points in (('GMCKF', 4), ('IMCCKF', 3)):           # c. scenarios
        tag = f'{method}_{shapes[n_points]}'
        out.append(case(f'c_{tag}_bar', n_points, method, occluders=bar_rows(n_points)))
        for name, hold in HOLDS[n_points].items():
            out.append(case(f'c_{tag}_wide_{name}', n_points, method, hold=hold, occluders=wide_rows(n_points)))
    for method, n_points in (('GMCKF', 4), ('IMCCKF', 3)):           # (KF at (6,6) follows the distractor out of the frame)
        tag = f'{method}_{shapes[n_points]}'
        rows, paints = distractor_rows(n_points, False)
        out.append(case(f'c_{tag}_distractor', n_points, method, occluders=rows, paints=paints))
        rows, paints = distractor_rows(n_points, True)
        out.append(case(f'c_{tag}_distractor_held', n_points, method, hold=HOLDS[n_points]['longer'], occluders=rows, paints=paints))
    # Leaving the frame: from Q_LEAVES, found without noise.  No start around it makes a (6,6) loop leave within K steps, so the other
    # estimator is MCKF at (8,6).  With a hold the trial is calm only from some starts: seeded jitters of 0.02 rad, chosen on the CPU.
    for method, jitter in (('GMCKF', 3), ('MCKF', 4)):
        for hold in (0, 2):
            leaving = Q_LEAVES if hold == 0 else jittered(jitter, Q_LEAVES, 0.02)
            trials = (trial(4, leaving, 100), trial(4, Q_HOST_ROUTE[0], 101))
            out.append(case(f'c_{method}_86_leaves_hold{hold}', 4, method, trials=trials, hold=hold, noise_px=0.0, clipping=True))
    # d. per-trial parameters: eight cells, the half fraction of 2^4 (every pair of parameters meets in all four combinations), on two starts
    shifted = DESIRED + np.array([3., -2., 3., -2., 3., -2., 3., -2.])
    cells = [(bw, gain, reg, des) for bw in (5.0, 20.0) for gain in (0.1, 0.3) for reg in (REG, 0.25) for des in (0, 1)
             if ((bw > 5) + (gain > 0.1) + (reg > REG) + des) % 2 == 0]
    for name, rows in (('d_GMCKF_86_grid', None), ('d_GMCKF_86_grid_bar', bar_rows(4))):
        trials = tuple(trial(4, Q_HOST_ROUTE[c % 2], 100 + c % 2, bw, gain, reg, desired=shifted if des else DESIRED,
                             occluders=None if rows is None else [rows[0], rows[1] if c % 4 < 2 else oc.NEVER])
                       for c, (bw, gain, reg, des) in enumerate(cells))
        out.append(case(name, 4, 'GMCKF', trials=trials, grid=True))
    trials = tuple(trial(4, Q_HOST_ROUTE[c % 2], 100 + c % 2, fpi_threshold=thr) for c, thr in enumerate((0.1, 0.1, 1e-4, 1e-4, 1e-2, 1e-2, 1e-6, 1e-6)))
    out.append(case('d_MCKF_86_grid', 4, 'MCKF', trials=trials, grid=True))
    for method, n_points in (('GMCKF', 4), ('KF', 3)):               # e. the device's initial guess
        out.append(case(f'e_{method}_{shapes[n_points]}_device_guess', n_points, method, guess='device'))
    return collections.OrderedDict((c.name, c) for c in out)


# hold variants of the wide bar: the longest loss of any disc over the trials of the case was measured on the CPU with hold = K
# (test_pixel_loop_oracle.py asserts it): 'equal' is that length, 'shorter' one less -- the trial FAILs at the step the hold runs out.
LONGEST_LOSS = {4: 3, 3: 3}
HOLDS = {n: {'longer': loss + 3, 'equal': loss, 'shorter': loss - 1} for n, loss in LONGEST_LOSS.items()}
CASES = _cases()
# (case, mutation) -> measured distance, for (2,6) entries that could not be brought to TEETH_MIN (nothing is claimed for them): none is left
NO_TEETH = {}


# ------------------------------------------------------------------------------------------------------------- the oracle's runs
def plant_of(n_points):
    import uvs_amd
    return uvs_amd.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))


def noise_of(c, i):
    """(K, m) noise of trial i of case c, or None."""
    if c.noise_px == 0.0:
        return None
    return np.random.default_rng(c.trials[i].seed).standard_normal((c.K, 2 * c.n_points)) * c.noise_px


def given_x0(c, i):
    """The supplied X0 of a case without initial_guess: the analytic guess at the start, every entry off by a relative sigma of 1 %."""
    tr = c.trials[i]
    if tr.x0_seed is None:
        return None
    from oracle import pixel_loop
    import uvs_amd
    plant, m = plant_of(c.n_points), 2 * c.n_points
    robot = uvs_amd.SyntheticRobot(plant, DT)
    robot.start(np.array(tr.q_start))
    x0 = uvs_amd.plant.analytic_guess(robot, pixel_loop.detect(plant, np.array(tr.q_start), 0)[0], (256, 256), m, 6)
    return x0 * (1 + 0.01 * np.random.default_rng(tr.x0_seed + i).standard_normal(x0.shape))


@functools.lru_cache(maxsize=None)
def oracle_trial(name, i, mutation=None, nudged=False):
    """oracle.pixel_loop.run on trial i of the case; nudged: from q_start (1 + 1e-14).  Read-only, shared by every test of a session."""
    from oracle import pixel_loop
    c = CASES[name]
    tr = c.trials[i]
    q = np.array(tr.q_start) * ((1.0 + CALM_NUDGE) if nudged else 1.0)
    out = pixel_loop.run(plant_of(c.n_points), q, np.array(tr.desired), noise_of(c, i), DT, c.K, tr.gain, c.method, tr.kernel_bw, c.annealing, c.K,
                         tr.fpi_threshold, FPI_EPOCH_MAX, tr.reg, c.anneal_span, initial_guess=c.initial_guess, x0=given_x0(c, i),
                         occluders=None if tr.occluders is None else np.array(tr.occluders, np.int64),
                         occluder_colours=None if tr.paints is None else np.array(tr.paints, np.int64), hold=c.hold, mutation=mutation)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def applicable(c, i=0):
    """The mutations that apply to trial i of the case: annealing, a kappa (GMCKF), occluders, noise, a hold that happens."""
    tr = c.trials[i]
    muts = ['regressor_halved', 'regressor_stale']
    if c.noise_px:
        muts.append('f_old_noise_free')
    if c.annealing and c.method != 'KF':
        muts.append('anneal_k_plus_1')
    if c.method == 'GMCKF':
        muts.append('kappa_dropped')
    if tr.occluders is not None and c.initial_guess:
        muts.append('step0_unoccluded')
        if c.method == 'GMCKF':                                      # f_{-1} meets a zero regressor: X cannot see it, kappa does
            muts.append('f0_unoccluded')
    if c.hold and c.noise_px and any(oracle_trial(c.name, i)['held']):
        muts.append('held_pair_new_noise')
    return muts


def distance(a, b):
    """How far run b is from run a in q and dq, relative, over the rows both have; inf when status or k_done differ."""
    if a['status'] != b['status'] or a['k_done'] != b['k_done']:
        return np.inf
    worst = 0.0
    for key in ('q', 'dq'):
        rows = min(len(a[key]), len(b[key]))
        if rows:
            worst = max(worst, float(np.abs(a[key][:rows] - b[key][:rows]).max() / np.abs(a[key][:rows]).max()))
    return worst


def teeth(name):
    """{mutation: the smallest distance over the trials of the case to which it applies}."""
    c = CASES[name]
    out = {}
    for i in range(len(c.trials)):
        for mut in applicable(c, i):
            d = distance(oracle_trial(name, i), oracle_trial(name, i, mut))
            out[mut] = min(out.get(mut, np.inf), d)
    return out


def preconditions(name, i):
    """dict(rim, calm, inside, mask_min, problems): what PRECONDITIONS asks of trial i, measured; problems is the list of those it misses."""
    c = CASES[name]
    a, b = oracle_trial(name, i), oracle_trial(name, i, None, True)
    rim = cc.closest_to_rim(a['discs'])
    same = (a['status'] == b['status'] and a['k_done'] == b['k_done'] and np.array_equal(a['counts'], b['counts']) and a['held'] == b['held']
            and np.array_equal(a['fpi_iterations'], b['fpi_iterations']))
    drift = 0.0
    if same:
        for key in ('q', 'f', 'dq', 'err', 'kappa'):
            if len(a[key]):
                with np.errstate(invalid='ignore'):
                    d = np.abs(a[key] - b[key]) / np.nanmax(np.abs(a[key]))
                assert np.array_equal(np.isnan(a[key]), np.isnan(b[key]))
                drift = max(drift, float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
    discs = a['discs']
    inside = bool((discs[:, :, :2] - discs[:, :, 2:]).min() > 0.0 and (discs[:, :, :2] + discs[:, :, 2:]).max() < 255.0 and discs[:, :, 2].min() > 0)
    problems = []
    if not rim > RIM_MIN:
        problems.append(f'rim {rim:.1e}')
    if not same or drift > CALM_TOL:
        problems.append(f'not calm (same {same}, drift {drift:.1e})')
    if not c.clipping and not inside:
        problems.append('a disc touches the edge of the frame')
    occluded = c.trials[i].occluders is not None
    if not c.clipping and not occluded and a['counts'].min() < MASK_MIN:
        problems.append(f'a mask of {a["counts"].min()} pixels')
    return dict(rim=rim, same=same, drift=drift, inside=inside, mask_min=int(a['counts'].min()), problems=problems)
