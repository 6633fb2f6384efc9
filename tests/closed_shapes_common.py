"""Inputs and CPU references shared by tests/test_oracle_c.py (the two oracles agree) and the GPU suites tests/test_gpu_closed_shapes.py and
tests/test_gpu_estimator_params.py (the kernels agree with them): closed loops at (6,6), (2,6) and (8,6) on the DH / pinhole plant and at
(8,6), (6,6) and (32,7) on the linear plant.

T = 70 trials of K = 60 steps: at two lanes per filter two full wavefronts plus six trials.  q0 = goal + jitter, noise 0.5 x t(2.5)
(at scale 3 the two CPU oracles themselves drift apart by 4e-3 on one (6,6) KF trial in ten: closed-loop sensitivity, kept out of the
parity cases), kernel_bw 7.5, MCKF with fpi_threshold 1e-4 so that the fixed-point loop iterates, t_max = dt (K + 0.5) on both oracles
so that their annealing horizons are the same k_max = K.  Trials TWINS carry the inputs of trial 1: one trial in the first, a middle
and the last wavefront of every lane mapping.  'wide', the (32,7) plant, has T = 4, K = 80, kernel_bw 10 and no twins: every case
carries its T, K, bw, t_max and twins in inputs(case).

oracle/c runs every trial (batch speed); oracle/rmckf_block (numpy pinv, the authority) runs the trials sampled(case).  A sampled trial on
which the two disagree by more than AGREE_TOL is closed-loop sensitivity, not a kernel matter: EXCLUDED lists those (with a decade of
margin), per configuration; test_oracle_c.py holds every trial that is not listed to AGREE_TOL and the list to the 10 % cap, the GPU
modules leave the listed trials out of their gates and print how far the kernels are from either oracle there."""
import functools

import numpy as np

from conftest import rel_err as rel                              # noqa: F401  (cs.rel: one definition for the suite)

T, K, DT, GAIN, BW, FPI_THRESHOLD = 70, 60, 0.05, 0.2, 7.5, 1e-4       # T, K, BW: of every case but 'wide'; comparisons read inputs(case)
REG, ANNEAL_SPAN = 0.001 ** 2, 100.0                             # the estimators' defaults (engine.make_params, experiment.py:280 and :271)
NOISE_SCALE = 0.5
X0_SPREAD = {'dh': 0.01, 'linear': 0.1}                          # a supplied X0: the plant's Jacobian, every entry off by this relative sigma
TWINS = (1, 35, 69)
AGREE_TOL = 1e-11
MAX_EXCLUDED_FRACTION = 0.10                                     # of a configuration's sampled trials
METHODS = ('GMCKF', 'KF', 'IMCCKF', 'MCKF')
# name -> (m, n, plant kind, analytic initial guess)
CASES = {'dh66': (6, 6, 'dh', True), 'dh66_x0': (6, 6, 'dh', False), 'dh26': (2, 6, 'dh', True),
         'lin86': (8, 6, 'linear', False), 'lin66': (6, 6, 'linear', False)}
SEEDS = {'dh66': 6601, 'dh66_x0': 6602, 'dh26': 2601, 'lin86': 8601, 'lin66': 6603, 'dh86': 8602, 'wide': 5}
# Further inputs that are no parity case of their own (not part of configurations()): tests/estimator_params_common.py runs them, and the
# cases above, at other values of reg and anneal_span.  'wide': the inputs of test_gpu_parity.py::test_closed_loop_stress_plant at T = 4,
# K = 80 (its generator: LinearPlant.random(32, 7, seed=2), noise 0.5 x t(3), one perturbed Jacobian as the X0 of every trial).
PARAM_CASES = {'dh86': (8, 6, 'dh', True), 'wide': (32, 7, 'linear', False)}
# (case, method, annealing) -> the sampled trials left out of the parity comparison: every one on which oracle/c and oracle/rmckf_block were
# measured more than 1e-12 apart -- a decade under AGREE_TOL, so that another libm or BLAS does not carry a kept trial past the gate (the
# kept ones: <= 8.9e-13, most <= 1e-13).  Measured: dh66 RMCKF 28: 1.7, 30: 8.3e-12, 63: 1.0e-10; dh66_x0 RMCKF 17: 1.3, 30: 0.99 (annealed
# 2.0e-12), KF 30: 3.3e-12, annealed MCKF 30: 1.7e-12.
EXCLUDED = {('dh66', 'GMCKF', False): (28, 30, 63), ('dh66_x0', 'GMCKF', False): (17, 30), ('dh66_x0', 'GMCKF', True): (30,),
            ('dh66_x0', 'KF', False): (30,), ('dh66_x0', 'KF', True): (30,), ('dh66_x0', 'MCKF', True): (30,)}


def sampled(case):
    """Trials of `case` that oracle/rmckf_block runs next to oracle/c.  Three points give a square interaction matrix, and a closed loop
    around a square estimate that passes near a singular one amplifies rounding (RMCKF without annealing: a few trials in 70 leave the other
    oracle by more than 1e-11, some by O(1)): every trial there, so that every such trial is known; one in seven elsewhere (<= 1e-12);
    all four of 'wide'."""
    trials = range(inputs(case)['T'])
    return tuple(trials if case in ('dh66', 'dh66_x0', 'wide') else trials[::7])


def configurations():
    return [(case, method, anneal) for case in CASES for method in METHODS for anneal in (False, True)]


def linear_plant_arrays(m, n, seed):
    """(J, f0, q0) of LinearPlant.random(m, n, seed)."""
    import uvs_amd
    plant = uvs_amd.LinearPlant.random(m, n, seed=seed)
    return plant.J, plant.f0, plant.q0


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(m, n, kind, guess, T, K, bw, t_max, twins, desired, q0 (T, n), noise (T, K, m), x0 (T, m n) -- what the estimator starts from on
    either route --, features: q -> noise-free f, discs | lin = (J, f0, lin_q0)).  Read-only: shared by every test of a session."""
    from oracle import plant_ref, rmckf_dense
    m, n, kind, guess = CASES[case] if case in CASES else PARAM_CASES[case]
    wide = case == 'wide'
    nT, nK, bw, twins = (4, 80, 10.0, ()) if wide else (T, K, BW, TWINS)
    rng = np.random.default_rng(SEEDS[case])
    d = dict(m=m, n=n, kind=kind, guess=guess, T=nT, K=nK, bw=bw, t_max=DT * (nK + 0.5), twins=twins)
    if kind == 'dh':
        desired = plant_ref.DESIRED_F[:m].copy()
        discs = plant_ref.place_discs(desired)
        q0 = plant_ref.Q_GOAL + 0.05 * rng.standard_normal((nT, n))
        d.update(discs=discs, features=lambda q: plant_ref.project(plant_ref.fkine_all(q)[5], discs))
    else:
        J, f0, lin_q0 = linear_plant_arrays(m, n, 2 if wide else SEEDS[case])
        q_goal = lin_q0 + rng.uniform(-0.3, 0.3, n)
        desired = f0 + J @ (q_goal - lin_q0)
        q0 = q_goal + rng.uniform(-0.15, 0.15, (nT, n))
        d.update(lin=(J, f0, lin_q0), features=lambda q: f0 + J @ (np.asarray(q, float) - lin_q0))
    noise = NOISE_SCALE * rng.standard_t(3 if wide else 2.5, size=(nT, nK, m))
    for a in (q0, noise):
        a[list(twins[1:])] = a[list(twins[:1])]
    x0 = np.zeros((nT, m * n))
    for t in range(nT):
        if kind == 'dh':                                              # the analytic guess at q0 -- as it is, or perturbed (X0_SPREAD) and handed over
            robot = plant_ref.PinholeUR10(DT, discs)
            robot.start(q0[t])
            x0[t] = rmckf_dense.analytic_initial_guess(robot, robot.features(), m, n).ravel()
        else:
            x0[t] = J.ravel()
    if wide:                                                          # one perturbation, the same for every trial
        x0 *= (1 + X0_SPREAD[kind] * rng.normal(size=J.shape)).ravel()
    elif not guess:
        x0 *= 1 + X0_SPREAD[kind] * rng.standard_normal(x0.shape)
        x0[list(twins[1:])] = x0[twins[0]]
    d.update(desired=desired, q0=q0, noise=noise, x0=x0)
    for a in (desired, q0, noise, x0):
        a.setflags(write=False)
    return d


def c_plant(inp):
    from oracle import c_oracle
    if inp['kind'] == 'linear':
        return c_oracle.linear_plant(*inp['lin'])
    pl = c_oracle.ur10_plant()
    pl.n_points = inp['m'] // 2
    for i, w in enumerate(inp['discs']):
        for c in range(3):
            pl.points[i][c] = w[c]
    return pl


def c_reference(case, method, anneal, reg=REG, anneal_span=ANNEAL_SPAN):
    """oracle/c on every trial: err (T, K, m), q (T, K, n), X (T, K, m n), stats (T, 3), status, k_done, fpi (T, K)."""
    return _c_reference(case, method, bool(anneal), float(reg), float(anneal_span))


@functools.lru_cache(maxsize=None)
def _c_reference(case, method, anneal, reg, anneal_span):
    from oracle import c_oracle
    inp = inputs(case)
    return c_oracle.closed_loop_batch(inp['q0'], inp['noise'], inp['desired'], method=method, kernel_bw=inp['bw'], annealing=anneal, dt=DT,
                                      t_max=inp['t_max'], gain=GAIN, steps=inp['K'], want_x=True, plant=c_plant(inp), fpi_threshold=FPI_THRESHOLD,
                                      x0=None if inp['guess'] else inp['x0'], reg=reg, anneal_span=anneal_span)


def block_reference(case, method, anneal, t, reg=REG, anneal_span=ANNEAL_SPAN):
    """oracle/rmckf_block on trial t: run_closed_loop's dict plus stats (3,) and f (K, m), the noisy features of every step."""
    return _block_reference(case, method, bool(anneal), int(t), float(reg), float(anneal_span))


@functools.lru_cache(maxsize=None)
def _block_reference(case, method, anneal, t, reg, anneal_span):
    from oracle import rmckf_block, rmckf_dense
    inp = inputs(case)
    ref = rmckf_block.run_closed_loop(inp['features'], inp['q0'][t], inp['desired'], inp['noise'][t], DT, inp['t_max'], GAIN, inp['x0'][t],
                                      method=method, kernel_bw=inp['bw'], annealing=anneal, initial_guess=inp['guess'],
                                      fpi_threshold=FPI_THRESHOLD, reg=reg, anneal_span=anneal_span)
    ref['stats'] = rmckf_dense.trial_stats(ref['err'], ref['t'])
    ref['f'] = ref['err'] + inp['desired']
    return ref


def oracle_agreement(case, method, anneal, reg=REG, anneal_span=ANNEAL_SPAN):
    """{sampled trial: worst relative difference of X, q and err between the two oracles (inf when status or k_done differ)}."""
    c = c_reference(case, method, anneal, reg, anneal_span)
    out = {}
    for t in sampled(case):
        b = block_reference(case, method, anneal, t, reg, anneal_span)
        if b['status'] != c['status'][t] or b['k_done'] != c['k_done'][t]:
            out[t] = np.inf
            continue
        k = b['k_done']
        out[t] = max(rel(c['X'][t, :k], b['X']), rel(c['q'][t, :k], b['q']), rel(c['err'][t, :k], b['err'])) if k else 0.0
    return out


def kept_trials(key, excluded=EXCLUDED):
    """Trials the parity tests compare: every trial of the case key[0] but those the table `excluded` lists for the configuration `key`."""
    gone = set(excluded.get(key, ()))
    return [t for t in range(inputs(key[0])['T']) if t not in gone]
