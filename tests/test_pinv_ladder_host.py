"""The pinv ladder on the CPU (pinv_ladder_common.py): the committed case list has the properties the GPU suite relies on, numpy's own pinv
stays within C <= 8 of the perturbation bound (otherwise the bound is the wrong yardstick), and the two oracles the other suites trust --
rmckf_block.control_law (numpy) and oracle/c's pinv_apply (one-sided Jacobi) -- are held to the exact reference at the kernels' gate."""
import functools

import numpy as np
import pytest

import pinv_ladder_common as pl
from oracle import c_oracle, rmckf_block

GAIN = 0.25                                                  # a power of two: dq / -gain is exact


@functools.lru_cache(maxsize=None)
def references(m, n):
    """Per case of the shape: the exact solution for the case's own y."""
    return tuple(pl.spectrum(m, n, i).solve(c['y']) for i, c in enumerate(pl.cases(m, n)))


def _assert_within_gate(m, n, solve, what):
    worst, failed = 0.0, []
    for i, (c, ref) in enumerate(zip(pl.cases(m, n), references(m, n))):
        got = solve(i, c)
        r = pl.ratio(ref, got)
        worst = max(worst, r)
        if not pl.passes(ref, got):
            failed.append((c['cls'], c['name'], r))
        if c['name'] == 'zero':
            assert not np.any(got), (what, 'J = 0 must give a command of exactly zero')
    print(f'{what} ({m}, {n}): worst error / bound {worst:.2f} (gate {pl.G:.1f})')
    assert not failed, (what, (m, n), failed)


@pytest.mark.parametrize('m,n', pl.SHAPES)
def test_case_list_is_finite_covers_every_class_and_stays_out_of_the_cutoff_band(m, n):
    cases = pl.cases(m, n)
    sides = {}
    for i, c in enumerate(cases):
        J, sp = c['J'], pl.spectrum(m, n, i)
        assert J.shape == (m, n) and c['y'].shape == (m,) and np.all(np.isfinite(J)) and np.all(np.isfinite(c['y'])), c['name']
        nz = np.abs(J[J != 0])
        assert nz.size == 0 or (nz.min() >= 1e-100 and nz.max() <= 1e100), c['name']
        assert not sp.in_band, (c['cls'], c['name'], sp.ratios.tolist())
        sides.setdefault(c['cls'], set()).add(sp.side)
    classes = [k for k in pl.CLASSES if k != 'kahan' or m >= n]
    assert list(sides) == classes
    for k in classes:
        assert 'kept' in sides[k], k
        assert ('dropped' in sides[k]) == (k in pl.HAS_DROPPED), k
    again = pl.cases.__wrapped__(m, n)                                                   # seeded: the same list every time
    assert all(np.array_equal(a['J'], b['J']) and np.array_equal(a['y'], b['y']) for a, b in zip(cases, again))
    kept = [pl.spectrum(m, n, i).kappa for i, c in enumerate(cases) if c['cls'] == 'ladder']
    assert min(kept) < 10 and max(kept) > 9e12                                           # the ladder spans the range


def test_numpy_pinv_stays_within_the_recorded_multiple_of_the_bound():
    C = 0.0
    for m, n in pl.SHAPES:
        for c, ref in zip(pl.cases(m, n), references(m, n)):
            C = max(C, pl.ratio(ref, np.linalg.pinv(c['J']) @ c['y']))
    print(f'numpy pinv over {sum(len(pl.cases(m, n)) for m, n in pl.SHAPES)} cases: C = {C:.3f} (recorded {pl.C_NUMPY}, G = {pl.G:.1f})')
    assert C <= 8 and C <= pl.C_NUMPY and pl.G == 16 * pl.C_NUMPY


@pytest.mark.parametrize('m,n', pl.SHAPES)
def test_numpy_oracle_control_law_is_within_the_gate(m, n):
    _assert_within_gate(m, n, lambda i, c: rmckf_block.control_law(c['J'], c['y'], np.ones(m), GAIN) / -GAIN, 'rmckf_block.control_law')


@pytest.mark.parametrize('m,n', pl.SHAPES)
def test_c_oracle_control_law_is_within_the_gate(m, n):
    """Step 0 of a K = 1 replay with method KF: H = 0 leaves X at x0 and kappa at 1, so the command is -gain pinv(x0) (f_1 - desired)."""
    cases = pl.cases(m, n)
    T = len(cases)
    f = np.zeros((T, 2, m))
    f[:, 1] = [c['y'] for c in cases]                                                    # desired = 0: err = f_1 = y, the same bits
    x0 = np.stack([c['J'].ravel() for c in cases])
    out = c_oracle.replay_batch(f, np.zeros((T, 1, n)), x0, np.zeros(m), method='KF', gain=GAIN)
    assert not out['status'].any() and np.all(out['k_done'] == 1)
    assert np.array_equal(out['X'][:, 0], x0) and np.all(out['kappa'] == 1.0)
    _assert_within_gate(m, n, lambda i, c: out['dq_cmd'][i, 0] / -GAIN, 'oracle/c pinv_apply')
