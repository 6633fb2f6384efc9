"""Parameter sets shared by tests/test_oracle_c.py and tests/test_gpu_estimator_params.py: the closed loops of tests/closed_shapes_common.py
(its cases plus 'dh86', the (8,6) DH plant from the analytic guess, and 'wide', the (32,7) linear plant of
test_gpu_parity.py::test_closed_loop_stress_plant) with uvs_filter_params.reg and .anneal_span moved off the one value every other test
leaves them at (engine.REG = 1e-6, engine.ANNEAL_SPAN = 100).

    R3    RMCKF, annealing off, reg 1e-3        A25   annealing on, anneal_span 25  (RMCKF: reg 0.25; IMCC-KF, MCKF: reg ignored)
    R25   RMCKF, annealing off, reg 0.25        A400  annealing on, anneal_span 400 (likewise)

The references are the two CPU oracles run with these values (cs.c_reference on every trial, cs.block_reference on cs.sampled(case));
test_oracle_c.py holds them to cs.AGREE_TOL of each other on the kept trials, the list EXCLUDED to the 10 % cap, and -- the teeth -- the
oracle run with the DEFAULT reg and anneal_span at least 100 gates away from the one with the set's values on the worst kept trial, so that
a kernel that read a literal instead of the field could not pass.  R25 sits at the cap on the (6,6) DH cases and is not run there."""
import numpy as np

import closed_shapes_common as cs

REG, ANNEAL_SPAN = cs.REG, cs.ANNEAL_SPAN                        # the defaults (engine.make_params, experiment.py:280 and :271)
GATE = 1e-8                                                      # the closed loop's GPU gate (gpu_harness.TOL)
TEETH = 100.0                                                    # the default-valued oracle misses GATE by at least this factor
SETS = {'R3': (False, 1e-3, ANNEAL_SPAN), 'R25': (False, 0.25, ANNEAL_SPAN), 'A25': (True, 0.25, 25.0), 'A400': (True, 0.25, 400.0)}
SET_METHODS = {'R3': ('GMCKF',), 'R25': ('GMCKF',), 'A25': ('GMCKF', 'IMCCKF', 'MCKF'), 'A400': ('GMCKF', 'IMCCKF', 'MCKF')}
CASE_SETS = {'dh86': ('R3', 'R25', 'A25', 'A400'), 'lin86': ('R3', 'R25', 'A25', 'A400'), 'lin66': ('R3', 'R25', 'A25', 'A400'),
             'dh26': ('R3', 'R25', 'A25', 'A400'), 'dh66': ('R3', 'A25', 'A400'), 'dh66_x0': ('R3', 'A25', 'A400')}
# (case, set, method) -> sampled trials left out of the comparisons: those on which oracle/c and oracle/rmckf_block were measured more than
# 1e-12 apart (a decade under cs.AGREE_TOL, as cs.EXCLUDED keeps it; the kept ones: <= 8.7e-13 at (6,6) on the DH plant, <= 4.1e-14 elsewhere).
# Every one is an RMCKF trial of a square (6,6) estimate.  Measured: lin66 R3 63: 1.1e-12; dh66 R3 28: 1.0, 30: 2.3e-12, 63: 4.8e-9, A400 30:
# 1.9e-12, 60: 3.0e-12; dh66_x0 R3 17: 3.8e-5, 30: 1.6e-11, 43: 1.2e-12, A25 54: 1.5e-12, A400 30: 3.8e-8.  No trial FAILs on any set.
EXCLUDED = {('lin66', 'R3', 'GMCKF'): (63,), ('dh66', 'R3', 'GMCKF'): (28, 30, 63), ('dh66', 'A400', 'GMCKF'): (30, 60),
            ('dh66_x0', 'R3', 'GMCKF'): (17, 30, 43), ('dh66_x0', 'A25', 'GMCKF'): (54,), ('dh66_x0', 'A400', 'GMCKF'): (30,)}


def estimator(name, method):
    """(annealing, reg, anneal_span) of parameter set `name` for `method`; only RMCKF reads reg, so the others keep the default there."""
    anneal, reg, span = SETS[name]
    return anneal, (reg if method == 'GMCKF' else REG), span


def configurations():
    return [(case, name, method) for case, names in CASE_SETS.items() for name in names for method in SET_METHODS[name]]


WIDE_CONFIGS = [('R25', 'GMCKF'), ('A25', 'GMCKF'), ('A25', 'IMCCKF'), ('A400', 'GMCKF'), ('A400', 'IMCCKF')]     # case 'wide': no MCKF on the wide kernel


def run(name, method, default=False):
    """The estimator of set `name` as keywords of cs.c_reference, cs.block_reference and cs.oracle_agreement -- or, default=True, the same
    estimator with reg and anneal_span left at the defaults."""
    anneal, reg, span = estimator(name, method)
    return dict(method=method, anneal=anneal, reg=REG if default else reg, anneal_span=ANNEAL_SPAN if default else span)


def _distance(a, b, kept):
    """Worst over the trials `kept` of the per-trial relative distance of err, q, X and stats between two oracle/c runs (rows at and after
    k_done zeroed; inf where status or k_done differ): what the GPU gates would see if a kernel computed b where a is expected."""
    worst = 0.0
    for t in kept:
        if a['status'][t] != b['status'][t] or a['k_done'][t] != b['k_done'][t]:
            return np.inf
        k = a['k_done'][t]
        if k:
            worst = max(worst, cs.rel(b['err'][t, :k], a['err'][t, :k]), cs.rel(b['q'][t, :k], a['q'][t, :k]), cs.rel(b['X'][t, :k], a['X'][t, :k]))
    return worst


def teeth(case, name, method):
    """How far the default-valued oracle run is from the set's on the worst kept trial, relative -- in units of nothing; compare with GATE."""
    return _distance(cs.c_reference(case, **run(name, method)), cs.c_reference(case, **run(name, method, True)),
                     cs.kept_trials((case, name, method), EXCLUDED))


# ---------------------------------------------------------------------------------------------- per-trial reg / fpi_threshold against oracle/c
GRID_E = 32                                                      # trials per grid cell
GRID_CELLS = {'GMCKF': [dict(reg=r, kernel_bw=b) for r in (1e-3, 0.25) for b in (5.0, 20.0)],
              'MCKF': [dict(fpi_threshold=thr) for thr in (0.1, 1e-4)]}
GRID_MIN_CALM = 0.95


def grid_oracle(cfg, q_start, noise, cell):
    """oracle/c on one grid cell -- the configuration `cfg` (batch.load_config) with the values of `cell` in place of its own -- and which trials
    are calm by the rule of test_grid_against_the_oracle: status, k_done and the statistics (1e-9) reproduced from a start moved by 1e-14."""
    from oracle import c_oracle
    ex, p = cfg['experiments'], cfg['estimator']['estimator_params']
    kw = dict(method=cfg['estimator']['method'], kernel_bw=p['kernel_bw'], annealing=p['annealing'], dt=ex['dt'], t_max=ex['t_max'], gain=ex['ibvs_gain'],
              fpi_threshold=p['fpi_threshold'], fpi_epoch_max=p['fpi_epoch_max'])
    kw.update(cell)
    a = c_oracle.closed_loop_batch(q_start, noise, ex['desired_f'], **kw)
    moved = c_oracle.closed_loop_batch(q_start * (1.0 + 1e-14), noise, ex['desired_f'], **kw)
    calm = (a['status'] == moved['status']) & (a['k_done'] == moved['k_done']) & \
           (np.abs(a['stats'] - moved['stats']).max(axis=1) / np.abs(a['stats']).max(axis=1) <= 1e-9)
    return a, calm
