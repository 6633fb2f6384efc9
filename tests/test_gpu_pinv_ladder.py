"""The control law of every device route -- dq = -gain pinv(J) (kappa o err) with numpy's pinv semantics -- held to the exact multiprecision
reference of pinv_ladder_common.py over the whole condition range, at a gate that is a perturbation bound (G bound, see there), in the default
mode (watches + careful pass) and under UVS_OPT_STRICT_PINV (certificate / careful kernels).

Every solve runs at H = 0 -- `first` = 1 on the step route, step 0 of a K = 1 replay or closed loop -- so the estimator leaves X at the x0 it was
given and the solve sees exactly the case's J.  All cases of a shape are the filters of ONE launch (ragged blocks for free); the right-hand
side of the reference is what the kernel itself logged: err, times kappa_out where the route gives it, times the per-row oracle's kappa on the
closed loop.  Asserted per launch: X read back is bit-identical to x0, status 0 and k_done 1 everywhere (no mark leaks), nothing of the poison
the outputs were filled with is left, dq / -gain within the gate for every case, and J = 0 gives a command of exactly zero.
Worst error / bound per route and class: pytest -s."""
import ctypes as C

import numpy as np
import pytest

import gpu_harness as gh
import pinv_ladder_common as pl
from conftest import load_golden
from gpu_harness import LATENCY, STRICT

pytestmark = pytest.mark.gpu

GAIN = 0.25                                                  # a power of two: dq / -gain is exact
BW = 100.0                                                   # RMCKF bandwidth: kappa of order 0.1 .. 1 at the innovations used here
MODES = [pytest.param(0, id='default'), pytest.param(STRICT, id='strict')]
REPLAY_ROUTES = [(8, 6, 0), (8, 6, 1), (8, 6, 2), (8, 6, 4), (8, 6, -2), (6, 6, 0), (6, 6, 1), (6, 6, 2), (2, 6, 1),
                 (32, 7, 0), (32, 7, 8), (32, 7, 16), (32, 7, 32)]
# (m, n, lanes, option bits, estimator): the DH plant at (8,6), the linear plant at (32,7); KF throughout, RMCKF on the default lanes
CLOSED_ROUTES = [(8, 6, 0, 0, 'KF'), (8, 6, 0, 0, 'GMCKF'), (8, 6, 2, 0, 'KF'), (8, 6, 0, LATENCY, 'KF'),
                 (32, 7, 0, 0, 'KF'), (32, 7, 0, 0, 'GMCKF'), (32, 7, 16, 0, 'KF')]
WORST = gh.Worst()                                           # route -> class -> worst error / bound


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    WORST.report('pinv ladder: worst error / bound (gate %.1f)' % pl.G)


def _inputs(m, n, seed):
    """x0 (T, m n): the cases' J; desired (m,); f (T, m) = desired + y; f_old (T, m): a few pixels off f."""
    cases = pl.cases(m, n)
    rng = np.random.default_rng([seed, m, n])
    desired = 128 + 10 * rng.standard_normal(m)
    f = desired + np.stack([c['y'] for c in cases])
    return np.stack([c['J'].ravel() for c in cases]), desired, f, f - 5 * rng.standard_normal(f.shape)


# What the default mode does NOT deliver (found by this suite; include/uvs_rmckf.h, UVS_OPT_STRICT_PINV, says so): shape, estimator -> cases.
# A Kahan-like Jacobian below numpy's cutoff whose right-hand side avoids the small direction up to rounding: the spread of the factor is
# ordinary, and the plain solution grows only by what ROUNDING puts into that direction (1e5, not 2^34), so no watch fires and the plain
# command is returned -- 6e16 to 1e19 bounds from numpy's truncated one.  With kappa != 1 (RMCKF) the product kappa o err excites the
# direction and the growth watch fires.  Held by test_default_mode_on_a_kahan_jacobian_whose_rhs_avoids_the_small_direction (xfail, strict);
# UVS_OPT_STRICT_PINV is held to every case.
DEFAULT_MODE_MISSES = {(6, 6, 'KF'): ('c1000_perp', 'c3000_perp')}


def _judge(m, n, method, route, mode, x0, X_back, status, k_done, y, dq, normal_equations=False):
    """One launch against the reference (module docstring).  y (T, m): the right-hand sides the kernel solved for.  Returns the cases that
    miss the gate, those of DEFAULT_MODE_MISSES (default mode) apart: (failed, known)."""
    tag = ('%s %s' % (route, method), 'strict' if mode & STRICT else 'default')
    for X in X_back:
        assert np.array_equal(X, x0), tag + ('the state changed at H = 0',)
    assert not status.any() and (k_done is None or np.all(k_done == 1)), tag + (status.tolist(),)
    assert np.all(np.isfinite(y)), tag
    apart = () if mode & STRICT else DEFAULT_MODE_MISSES.get((m, n, method), ())
    worst, failed, known = {}, [], []
    for i, c in enumerate(pl.cases(m, n)):
        ref = pl.spectrum(m, n, i).solve(y[i])
        got = dq[i] / -GAIN
        r = pl.ratio(ref, got)
        if not pl.passes(ref, got, normal_equations and not mode & STRICT):
            (known if c['name'] in apart else failed).append(tag + (c['cls'], c['name'], 'error / bound %.3g' % r, 'kappa %.1e' % ref['kappa'], pl.spectrum(m, n, i).side))
        if c['name'] == 'zero':
            assert not np.any(dq[i]), tag + ('J = 0 must give a command of exactly zero', dq[i].tolist())
        if c['name'] not in apart:
            worst[c['cls']] = max(worst.get(c['cls'], 0.0), r)
            WORST.note('%s, %s' % tag, c['cls'], r)
    print('pinv ladder, %s, %s: worst error / bound' % tag, {k: '%.2g' % v for k, v in worst.items()}, *(['set apart:', known] if known else []))
    return failed, known


# ---------------------------------------------------------------------------------------------- uvs_rmckf_step_f64
def _step(uvs, fp, x0, f, f_old):
    T, n = len(x0), fp.n
    bank = uvs.engine.FilterBank(fp, T, np.ascontiguousarray(x0))
    for buf in (bank.dq, bank.err, bank.kappa):
        buf.fill_(float('nan'))
    bank.status.fill_(gh.POISON_INT)
    assert bank.first
    dq, err, kappa, status = (o.cpu().numpy().copy() for o in bank.step(gh.cuda(f), gh.cuda(f_old), gh.cuda(np.zeros((T, n))), 0))
    assert not (np.isnan(dq).any() or np.isnan(err).any() or np.isnan(kappa).any() or (status == gh.POISON_INT).any()), 'not stored'
    return dict(X=bank.X.cpu().numpy(), dq=dq, err=err, kappa=kappa, status=status)


def _step_route(uvs, m, n, lanes, mode, method):
    x0, desired, f, f_old = _inputs(m, n, 1)
    fp = uvs.engine.make_params(m, n, method, BW, False, 0.05, 15.0, GAIN, desired, False, lanes, 0)
    fp.reserved = mode
    out = _step(uvs, fp, x0, f, f_old)
    assert gh.same_bits(out['err'], f - desired)
    if method == 'KF':
        assert np.all(out['kappa'] == 1.0)
    # the header: a filter's command never depends on its neighbours -- the same batch in reversed order, the same bits per case
    rev = _step(uvs, fp, x0[::-1], f[::-1], f_old[::-1])
    for key in ('dq', 'kappa', 'status', 'X'):
        assert gh.same_bits(rev[key][::-1], out[key]), (key, 'depends on the order of the batch', m, n, lanes, method, mode)
    return _judge(m, n, method, 'step (%d,%d) lanes %d' % (m, n, lanes), mode, x0, [out['X']], out['status'], None, out['err'] * out['kappa'], out['dq'])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('m,n,lanes', gh.SHAPES)
def test_step_route_solves_the_ladder(uvs, m, n, lanes, mode):
    failed = sum((_step_route(uvs, m, n, lanes, mode, method)[0] for method in ('KF', 'GMCKF')), [])
    assert not failed, failed


# ---------------------------------------------------------------------------------------------- uvs_rmckf_replay_f64
def _replay_route(uvs, m, n, lanes, mode, method):
    x0, desired, f1, f0 = _inputs(m, n, 2)
    T = len(x0)
    fp = uvs.engine.make_params(m, n, method, BW, False, 0.05, 15.0, GAIN, desired, False, lanes, 1)
    fp.reserved = mode
    out = gh.replay(uvs, fp, np.stack([f0, f1], axis=1), np.zeros((T, 1, n)), x0, ('x', 'err', 'kappa', 'dqcmd'))      # poisoned outputs
    assert gh.same_bits(out['err'][:, 0], f1 - desired)
    if method == 'KF':
        assert np.all(out['kappa'] == 1.0)
    # lanes 0 at (8,6): the control wavefronts solve by the normal equations
    return _judge(m, n, method, 'replay (%d,%d) lanes %d' % (m, n, lanes), mode, x0, [out['x'][:, 0], out['x_final']], out['status'], out['k_done'],
                  out['err'][:, 0] * out['kappa'][:, 0], out['dqcmd'][:, 0], normal_equations=(m, n, lanes) == (8, 6, 0))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('m,n,lanes', REPLAY_ROUTES)
def test_replay_solves_the_ladder(uvs, m, n, lanes, mode):
    failed = sum((_replay_route(uvs, m, n, lanes, mode, method)[0] for method in ('KF', 'GMCKF')), [])
    assert not failed, failed


@pytest.mark.xfail(strict=True, raises=AssertionError, reason='default mode, (6,6), KF: no watch sees a Kahan-like Jacobian below the cutoff when only rounding excites its small '
                   'direction; measured on an MI355X: 6e16 (c = 1000) to 1e19 (c = 3000) bounds from the truncated command, every (6,6) route')
@pytest.mark.parametrize('route,lanes', [('step', 1), ('step', 2), ('replay', 0), ('replay', 1), ('replay', 2)])
def test_default_mode_on_a_kahan_jacobian_whose_rhs_avoids_the_small_direction(uvs, route, lanes):
    """The cases DEFAULT_MODE_MISSES sets apart, held to the same gate: fails as long as the default mode returns the plain command there."""
    _, known = (_step_route if route == 'step' else _replay_route)(uvs, 6, 6, lanes, 0, 'KF')
    assert not known, known


# ---------------------------------------------------------------------------------------------- uvs_rmckf_closed_loop_ws_f64
def _closed_loop(uvs, fp, ps, q0, noise, x0):
    """K = 1 closed loop with x0 supplied into poisoned outputs; numpy arrays [trial][component] of step 0."""
    import torch
    T, m, n = len(x0), fp.m, fp.n
    comps = {'x': m * n, 'err': m, 'q': n, 'f': m, 'dq': n}
    dev = {k: gh.poisoned(T, 1, comps[k]) for k in gh.STREAMS}
    dev.update(gh.poisoned_trials(T, final=(m, n)))
    q0_dev, x0_dev, noise_dev = gh.cuda(q0), gh.cuda(x0), gh.cuda(noise.T[None])              # noise: [step][component][trial]
    flat = lambda t: uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))                 # noqa: E731
    view = uvs.engine.stream_view
    rc = uvs.engine.launch_closed_loop(fp, ps, T, flat(q0_dev), view(noise_dev), flat(x0_dev), *(view(dev[k]) for k in gh.STREAMS),
                                       dev['stats'].data_ptr(), dev['status'].data_ptr(), dev['k_done'].data_ptr(), flat(dev['x_final']), flat(dev['p_final']))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    out = {k: np.ascontiguousarray(uvs.engine.as_tkc(dev[k]).cpu().numpy())[:, 0] for k in gh.STREAMS}
    out.update({k: dev[k].cpu().numpy() for k in ('stats', 'status', 'k_done', 'x_final', 'p_final')})
    for k, v in out.items():
        assert not (np.isnan(v).any() if v.dtype.kind == 'f' else (v == gh.POISON_INT).any()), (k, 'not stored')
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('m,n,lanes,opts,method', CLOSED_ROUTES)
def test_closed_loop_solves_the_ladder(uvs, m, n, lanes, opts, method, mode):
    from oracle import rmckf_block
    x0, desired, f, _ = _inputs(m, n, 3)
    T = len(x0)
    if (m, n) == (8, 6):
        g = load_golden('closed_gmckf_a1p5')
        plant, q_start = uvs.SyntheticPlant.ur10(g['desired']), np.asarray(g['q_start'], float)
    else:
        plant = uvs.LinearPlant.random(m, n, seed=2)
        q_start = plant.q0 + 0.1
    noise = f - plant.features(q_start)                                                      # so that f_plant + noise = desired + y up to rounding
    fp = uvs.engine.make_params(m, n, method, BW, False, 0.05, 15.0, GAIN, desired, False, lanes, 1)
    fp.reserved = mode | opts
    ps = plant.to_struct()
    if (m, n, lanes) == (8, 6, 0):
        # the small-batch kernels, four lanes per filter: EMU2 by default, the plain one under UVS_OPT_LATENCY; EMU2 carries no certificate, so
        # strict mode alone stays on the certifying two-lane kernel
        assert int(uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp), C.byref(ps), T)) == (2 if mode & STRICT and not opts & LATENCY else 4)
    out = _closed_loop(uvs, fp, ps, np.tile(q_start, (T, 1)), noise, x0)
    assert np.array_equal(out['q'], np.tile(q_start, (T, 1)))
    assert np.abs(out['err'] - (f - desired)).max() <= 1e-9                                   # the plant's rounding, nothing else
    assert gh.same_bits(out['err'], out['f'] - desired)
    # the per-row oracle's kappa of step 0: f_old = 0 when x0 is supplied, H = 0
    kappa = np.stack([rmckf_block.BlockFilter(m, n, x0[t], method, BW).step(out['f'][t], np.zeros(n), 0) for t in range(T)])
    if method == 'KF':
        assert np.all(kappa == 1.0)
    failed, _ = _judge(m, n, method, 'closed loop (%d,%d) lanes %d opts %d' % (m, n, lanes, opts), mode, x0, [out['x'], out['x_final']], out['status'],
                       out['k_done'], out['err'] * kappa, out['dq'], normal_equations=(m, n) == (32, 7))
    assert not failed, failed
