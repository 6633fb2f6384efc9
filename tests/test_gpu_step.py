"""The batched single-step route (uvs_rmckf_step_f64: engine.FilterBank.step / step_host, step_kernel<M, N, L, 0>) against the per-row numpy
oracle (oracle/rmckf_block: BlockFilter.step, control_law = numpy.linalg.pinv, run_replay) -- every instantiated (m, n, L), every estimator,
batches of more than one filter in ragged launches.  What only this kernel does is what is held here: the trial / sub-row index arithmetic
of each L, the symmetric-packed load and the full store of P, the `first` flag, the bandwidth of a caller-supplied k, the padding lanes'
clamp to trial T - 1, the per-filter choice between the plain and the careful command after a wavefront-wide vote, the non-finite flag
gathered into the group's first lane, and the pinned-host operands of step_host.

Inputs follow tools/fuzz_step.py: J ~ N(0, 50^2), X0 = J, f_old = 128 + 20 N(0, 1), f = f_old + 0.05 J dq + scale * t_2 noise, commands
clipped to +-5, desired = 128 + 10 N(0, 1), fixed seeds.  Gates: X 1e-10, P 1e-9, command 1e-7 (tools/fuzz_step.py), kappa 1e-9
(test_replay_other_shapes_match_block_oracle); the oracle's own sensitivity to one ulp of its inputs on this recipe is X 4e-15, P 1e-15,
command 2.5e-12."""
import zlib

import numpy as np
import pytest

import gpu_harness as gh
from conftest import load_golden, rel_err as rel
from gpu_harness import DEFAULT_LANES, K_MAX, SHAPES, TOL_DQ, TOL_KAPPA, TOL_P, TOL_X

pytestmark = pytest.mark.gpu

LANE_CASES = SHAPES + [(m, n, 0) for m, n in DEFAULT_LANES] + [(8, 6, -8), (6, 6, -1), (2, 6, -1), (32, 7, -32)]
METHODS = ['GMCKF', 'KF', 'IMCCKF', 'MCKF']
RANKDEF = 'rankdef_gmckf_zero_and_scaled_col'
WORST = gh.Worst()                                           # 'module': worst deviation per key over the per-step parity cases run so far


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    return uvs_amd


def _np(t):
    return t.cpu().numpy().copy()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------------------------------------- 1. per-step parity
def _parity_run(uvs, rng, m, n, lanes, method, k0, scale, thr, cap, route, steps=6):
    """One bank of T = 64 // L + 3 filters (two blocks, the second ragged) stepped `steps` times from k0 (gh.step_recipe at a kernel_bw drawn
    from {1, 10, 50}, annealed); every step compared with the oracle started from the same state, then both sides continue from the ORACLE's
    state and command.  The deviations go to WORST[route] and WORST['module']; returns how many filters FAILed, on both sides."""
    bw = float(rng.choice([1.0, 10.0, 50.0]))
    head, *recipe = gh.step_recipe(rng, m, n, lanes, method, k0, scale, bw, True, steps, fpi_threshold=thr, fpi_epoch_max=cap)
    fp = uvs.engine.make_params(m, n, method, bw, True, 0.05, 15.0, head['gain'], head['desired'], False, lanes, 0, thr, cap)
    assert fp.k_max == K_MAX
    bank = uvs.engine.FilterBank(fp, head['T'], head['x0'])
    for s, st in enumerate(recipe):
        gh.assert_step(bank, st, head['desired'], WORST, (route, 'module'), (m, n, lanes, method, head['T'], bw, thr, cap, scale), fresh=s == 0)
    return sum(int((~st['finite']).sum()) for st in recipe)


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('m,n,lanes', LANE_CASES)
def test_every_step_matches_the_block_oracle(uvs, m, n, lanes, method):
    """Annealed bandwidth (kernel_bw from {1, 10, 50}) at k = 0.. and k = 290.. of 300, noise scales 1, 30 and 400 (zero and subnormal
    correntropy weights; at the narrow bandwidths of k = 290), MCKF at (threshold, cap) = (0.1, 1000) and (1e-2, 3)."""
    rng = np.random.default_rng(_seed(m, n, lanes, method))
    route, fails = (m, n, lanes, method), 0
    for thr, cap in ([(0.1, 1000), (1e-2, 3)] if method == 'MCKF' else [(0.1, 1000)]):
        for k0, scale in ((0, 1.0), (290, 1.0), (0, 30.0), (290, 30.0), (290, 400.0)):
            fails += _parity_run(uvs, rng, m, n, lanes, method, k0, scale, thr, cap, route)
    fmt = lambda w: {k: f'{v:.1e}' for k, v in w.items()}                                   # noqa: E731
    print(f'step parity ({m},{n}) lanes {lanes} {method}: worst relative deviations {fmt(WORST[route])}, {fails} FAILs on both sides; module so far {fmt(WORST["module"])}')


# ---------------------------------------------------------------------------------------------- 2. chained run, no resynchronisation
@pytest.mark.parametrize('method', ['GMCKF', 'KF', 'IMCCKF'])
@pytest.mark.parametrize('m,n,lanes', [(8, 6, 4), (6, 6, 2), (2, 6, 1), (32, 7, 16)])
def test_forty_chained_steps_match_run_replay(uvs, m, n, lanes, method):
    """X and P make the HBM round trip 40 times with nothing copied back from the oracle: the gates of
    test_replay_other_shapes_match_block_oracle on the streams of its generator."""
    from oracle import rmckf_block
    K, T = 40, 5
    f, dq, x0, des = gh.random_replay_case(m, n, K, T, 1000 + m)
    fp = uvs.engine.make_params(m, n, method, 7.5, True, 0.05, 15, 0.2, des, False, lanes, 0)
    bank = uvs.engine.FilterBank(fp, T, x0)
    X, cmd, kap = [], [], []
    for k in range(K):
        out = bank.step(gh.cuda(f[:, k + 1]), gh.cuda(f[:, k]), gh.cuda(dq[:, k]), k)
        assert not _np(out[3]).any()
        X.append(_np(bank.X)); cmd.append(_np(out[0])); kap.append(_np(out[2]))
    X, cmd, kap, P = np.array(X), np.array(cmd), np.array(kap), _np(bank.P).reshape(T, m, n, n)
    worst = {'X': 0.0, 'dq': 0.0, 'kappa': 0.0, 'P': 0.0}
    for t in range(T):
        ref = rmckf_block.run_replay(f[t], dq[t], x0[t], des, 0.2, method, 7.5, True, K_MAX)
        d = {'X': max(rel(X[k, t], ref['X'][k]) for k in range(K)), 'dq': rel(cmd[:, t], ref['dq_cmd']),
             'kappa': rel(kap[:, t], ref['kappa']), 'P': rel(P[t], ref['P_final'])}
        for key, tol in (('X', 1e-10), ('dq', 1e-8), ('kappa', 1e-9), ('P', 1e-10)):
            worst[key] = max(worst[key], d[key])
            assert d[key] <= tol, (key, d[key], t)
    print(f'chained steps ({m},{n}) lanes {lanes} {method}: worst', {k: f'{v:.1e}' for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------- 3. neighbours do not matter
def _streams(rng, m, n, T, S):
    """S steps of inputs for T healthy filters, fixed beforehand so that every run of them reads the same bits."""
    J = rng.standard_normal((T, m, n)) * 50
    dq = np.clip(rng.standard_normal((S, T, n)), -5, 5)
    f_old, f = np.zeros((S, T, m)), np.zeros((S, T, m))
    prev = 128 + 20 * rng.standard_normal((T, m))
    for s in range(S):
        f_old[s] = prev
        f[s] = prev + np.einsum('tmn,tn->tm', J, dq[s]) * 0.05 + rng.standard_t(2.0, size=(T, m))
        prev = f[s]
    return dict(x0=J.reshape(T, m * n).copy(), f=f, f_old=f_old, dq=dq)


def _run(uvs, fp, inp, sel=None, k0=0):
    """Step a fresh bank over the input streams (of the filters `sel` only, if given); per-step copies of everything the kernel writes."""
    sel = slice(None) if sel is None else sel
    x0 = inp['x0'][sel]
    bank = uvs.engine.FilterBank(fp, len(x0), x0)
    keys = ('X', 'P', 'dq', 'err', 'kappa', 'status')
    rec = {key: [] for key in keys}
    for s in range(len(inp['f'])):
        out = bank.step(gh.cuda(inp['f'][s][sel]), gh.cuda(inp['f_old'][s][sel]), gh.cuda(inp['dq'][s][sel]), k0 + s)
        for key, v in zip(keys, (bank.X, bank.P) + tuple(out)):
            rec[key].append(_np(v))
    return {key: np.array(v) for key, v in rec.items()}                                     # [step][filter]...


def _assert_singletons_equal(uvs, fp, inp, batch, T):
    for t in range(T):
        one = _run(uvs, fp, inp, [t])
        for key in batch:
            assert gh.same_bits(batch[key][:, t], one[key][:, 0]), (key, t)


def _oracle_chain(fp_args, inp, t, method='GMCKF'):
    """The oracle on filter t of the streams: per step (X, P, command, kappa)."""
    from oracle import rmckf_block
    m, n, bw, anneal, gain, desired = fp_args
    filt = rmckf_block.BlockFilter(m, n, inp['x0'][t], method, bw, anneal, K_MAX)
    out = []
    for s in range(len(inp['f'])):
        kappa = filt.step(inp['f'][s, t] - inp['f_old'][s, t], inp['dq'][s, t], s)
        out.append((filt.X.copy(), filt.P.copy(), rmckf_block.control_law(filt.X, inp['f'][s, t] - desired, kappa, gain), kappa))
    return out


def _neighbour_case(shape):
    """(fp arguments, healthy streams, streams with three rank-deficient filters, their slots, their reference commands [step][slot])."""
    S = 3
    if shape == (8, 6):
        g = load_golden(RANKDEF)
        m, n, lanes, T = 8, 6, 0, 19
        p = g['meta']['params']
        args = (m, n, float(p['kernel_bw']), bool(p['annealing']), float(g['meta']['gain']), np.asarray(g['desired'], float))
        sick = [0, 7, T - 1]                                                                # 7: mid-wavefront (16 filters ride in one)
    else:
        m, n, lanes, T = 32, 7, 32, 5
        rng0 = np.random.default_rng(3207)
        args = (m, n, 10.0, False, 0.2, 128 + 10 * rng0.standard_normal(m))
        sick = [0, 3, T - 1]                                                                # 3: the second filter of the second wavefront
    healthy = _streams(np.random.default_rng(_seed('neighbours', shape)), m, n, T, S)
    mixed = {key: v.copy() for key, v in healthy.items()}
    ref_cmd = np.full((S, len(sick), n), np.nan)
    for i, t in enumerate(sick):
        if shape == (8, 6):                                                                 # the reference's own trial from its rank-deficient X0
            f_seq = np.vstack([g['f_init'][None], g['f']])
            mixed['x0'][t] = g['X'][0]
            for s in range(S):
                mixed['f'][s, t], mixed['f_old'][s, t], mixed['dq'][s, t] = f_seq[s + 1], f_seq[s], g['dq_prev'][s]
                ref_cmd[s, i] = g['dq_prev'][s + 1]
        else:                                                                               # an exactly zero column; h = 0 keeps it exact on the first step
            x = mixed['x0'][t].reshape(m, n)
            x[:, (2 * i + 1) % n] = 0.0
            ref_cmd[0, i] = _oracle_chain(args, mixed, t)[0][2]
            sv = np.linalg.svd(x, compute_uv=False)
            assert sv[-1] <= 1e-16 * sv[0] and sv[-2] > 1e-3 * sv[0]                       # the input: rank n - 1, a decade under numpy's cutoff
    return args, lanes, T, healthy, mixed, sick, ref_cmd


def _fp_of(uvs, args, lanes, strict=False):
    m, n, bw, anneal, gain, desired = args
    fp = uvs.engine.make_params(m, n, 'GMCKF', bw, anneal, 0.05, 15.0, gain, desired, False, lanes, 0)
    fp.reserved = 1 if strict else 0                                                        # UVS_OPT_STRICT_PINV
    return fp


def _assert_sick_commands(out, sick, ref_cmd):
    for i, t in enumerate(sick):
        for s in range(len(ref_cmd)):
            ref = ref_cmd[s, i]
            if np.all(np.isfinite(ref)):                                                    # gate of test_single_step_bank_uses_pinv_semantics
                assert np.abs(out['dq'][s, t] - ref).max() <= 1e-8 * max(1e-3, np.abs(ref).max()), (s, t)


@pytest.mark.parametrize('shape', [(8, 6), (32, 7)])
def test_a_filter_does_not_depend_on_its_neighbours(uvs, shape):
    """(8,6) default lanes with T = 19 and (32,7) on 32 lanes with T = 5, three steps from `first`.  (a) every filter of a batch has the bits
    of a T = 1 bank fed that filter alone; (b) with rank-deficient filters in slots 0, mid-wavefront and T - 1 (their watch sends the whole
    wavefront through the careful solve) the healthy filters keep the bits they have in an all-healthy batch and the sick ones return
    numpy's truncated command; (c) under UVS_OPT_STRICT_PINV the state, err, kappa and status keep the default mode's bits and every
    command is the oracle's."""
    args, lanes, T, healthy, mixed, sick, ref_cmd = _neighbour_case(shape)
    keep = [t for t in range(T) if t not in sick]
    fp = _fp_of(uvs, args, lanes)
    out_h, out_m = _run(uvs, fp, healthy), _run(uvs, fp, mixed)
    assert not out_h['status'].any() and not out_m['status'].any()
    _assert_singletons_equal(uvs, fp, healthy, out_h, T)                                   # (a)
    _assert_singletons_equal(uvs, fp, mixed, out_m, T)
    for key in out_m:                                                                       # (b)
        assert gh.same_bits(out_m[key][:, keep], out_h[key][:, keep]), key
    _assert_sick_commands(out_m, sick, ref_cmd)
    oracle = {t: _oracle_chain(args, healthy, t) for t in range(T)}
    worst = {'default': 0.0, 'strict': 0.0}
    strict = _fp_of(uvs, args, lanes, strict=True)
    for inp, out, who in ((healthy, out_h, range(T)), (mixed, out_m, keep)):               # (c)
        out_s = _run(uvs, strict, inp)
        for key in ('X', 'P', 'err', 'kappa', 'status'):
            assert gh.same_bits(out_s[key], out[key]), key
        for t in who:
            for s, (X, P, cmd, kappa) in enumerate(oracle[t]):
                assert rel(out['X'][s, t], X.ravel()) <= TOL_X and rel(out['P'][s, t].reshape(P.shape), P) <= TOL_P, (s, t)
                for mode, o in (('default', out), ('strict', out_s)):
                    worst[mode] = max(worst[mode], rel(o['dq'][s, t], cmd))
                    assert rel(o['dq'][s, t], cmd) <= TOL_DQ, (mode, s, t)
        if inp is mixed:
            _assert_sick_commands(out_s, sick, ref_cmd)
    print(f'neighbours {shape}: worst command deviation of the healthy filters', {k: f'{v:.1e}' for k, v in worst.items()})


def test_duplicated_column_is_numpys_truncated_command_in_a_batch(uvs):
    """A further deficient state, built from a duplicated column (the recipe of tools/fuzz_step.py), in the last slot of a ragged (6,6)
    batch: its first command -- h = 0 keeps the deficiency exact -- is numpy's.  The input is checked first: the oracle's sigma_min / sigma_max
    must sit a decade under numpy's 1e-15 cutoff."""
    m, n, T = 6, 6, 35                                                                      # two lanes per filter: 32 filters per wavefront
    inp = _streams(np.random.default_rng(66), m, n, T, 1)
    x = inp['x0'][T - 1].reshape(m, n)
    x[:, 5] = x[:, 4] * 2.0
    sv = np.linalg.svd(x, compute_uv=False)
    assert sv[-1] / sv[0] <= 1e-16, 'pick another seed: this duplicate is not below the cutoff'
    args = (m, n, 10.0, False, 0.2, 128 + 10 * np.random.default_rng(67).standard_normal(m))
    out = _run(uvs, _fp_of(uvs, args, 0), inp)
    for t in (0, 17, T - 1):
        ref = _oracle_chain(args, inp, t)[0][2]
        assert np.abs(out['dq'][0, t] - ref).max() <= 1e-8 * max(1e-3, np.abs(ref).max()), t


# ---------------------------------------------------------------------------------------------- 4. failure semantics in a batch
@pytest.mark.parametrize('method', ['GMCKF', 'KF'])
@pytest.mark.parametrize('lanes', [4, 8])
def test_a_nan_sample_fails_its_filter_alone(uvs, lanes, method):
    """NaN in the last feature of one filter of T = 19 on the second step: that row belongs to the LAST lane of the filter's group, the
    status is written by the first.  Only that filter FAILs; every other filter has the bits of the batch without the NaN."""
    m, n, T, hit = 8, 6, 19, 7
    inp = _streams(np.random.default_rng(_seed('nan', lanes, method)), m, n, T, 2)
    bad = {key: v.copy() for key, v in inp.items()}
    bad['f'][1, hit, m - 1] = np.nan
    fp = uvs.engine.make_params(m, n, method, 10.0, True, 0.05, 15.0, 0.2, 128 + 10 * np.random.default_rng(4).standard_normal(m), False, lanes, 0)
    a, b = _run(uvs, fp, inp), _run(uvs, fp, bad)
    assert not a['status'].any() and not b['status'][0].any()
    assert b['status'][1].tolist() == [int(t == hit) for t in range(T)]
    others = [t for t in range(T) if t != hit]
    for key in a:
        assert gh.same_bits(a[key][:, others], b[key][:, others]), key
        assert gh.same_bits(a[key][0], b[key][0]), key


@pytest.mark.parametrize('lanes', [4, 8])
def test_an_infinite_sample_skips_the_mckf_correction(uvs, lanes):
    """+inf in the same place under MCKF: the weight of that row is 0, inv(Cy) raises in the reference and the whole correction is skipped --
    X unchanged, P = P + I, status SUCCESS -- for that filter alone.  State and status against the oracle at the per-step gates (that
    step's command is not compared: numpy's is non-finite)."""
    m, n, T, hit = 8, 6, 19, 7
    inp = _streams(np.random.default_rng(_seed('inf', lanes)), m, n, T, 2)
    inp['f'][1, hit, m - 1] = np.inf
    desired = 128 + 10 * np.random.default_rng(5).standard_normal(m)
    fp = uvs.engine.make_params(m, n, 'MCKF', 10.0, True, 0.05, 15.0, 0.2, desired, False, lanes, 0)
    out = _run(uvs, fp, inp)
    assert not out['status'].any()
    assert gh.same_bits(out['X'][1, hit], out['X'][0, hit])                                   # skipped: the state of the step before
    assert gh.same_bits(out['P'][1, hit], out['P'][0, hit] + np.tile(np.eye(n), (m, 1, 1)).reshape(out['P'][0, hit].shape))
    for t in range(T):
        ref = _oracle_chain((m, n, 10.0, True, 0.2, desired), inp, t, 'MCKF')
        for s, (X, P, cmd, kappa) in enumerate(ref):
            assert np.all(np.isfinite(X))
            assert rel(out['X'][s, t], X.ravel()) <= TOL_X and rel(out['P'][s, t].reshape(P.shape), P) <= TOL_P, (s, t)
            if not (s == 1 and t == hit):
                assert rel(out['dq'][s, t], cmd) <= TOL_DQ and rel(out['kappa'][s, t], kappa) <= TOL_KAPPA, (s, t)


# ---------------------------------------------------------------------------------------------- 5. step_host at T > 1
@pytest.mark.parametrize('method', ['GMCKF', 'MCKF'])
@pytest.mark.parametrize('T', [19, 64])
def test_step_host_is_the_same_kernel_on_pinned_operands(uvs, T, method):
    """Six calls: step_host (operands in pinned host memory) returns the bits of bank.step on device tensors given the same inputs, with
    dq_prev passed explicitly and with dq_prev = None (the double-buffer chaining) alike; the views call k returned still hold call k's
    values after call k + 1."""
    m, n, S = 8, 6, 6
    inp = _streams(np.random.default_rng(_seed('host', T, method)), m, n, T, S)
    desired = 128 + 10 * np.random.default_rng(6).standard_normal(m)
    mk = lambda: uvs.engine.FilterBank(uvs.engine.make_params(m, n, method, 10.0, True, 0.05, 15.0, 0.2, desired, False, 0, 0), T, inp['x0'])   # noqa: E731
    dev, explicit, chained = mk(), mk(), mk()
    prev = np.zeros((T, n))
    held = None
    for k in range(S):
        f, f_old = inp['f'][k], inp['f_old'][k]
        ref = [_np(o) for o in dev.step(gh.cuda(f), gh.cuda(f_old), gh.cuda(prev), k)]
        views_e = explicit.step_host(f, f_old, k, dq_prev=prev)
        views_c = chained.step_host(f, f_old, k)
        for name, r, e, c in zip(('dq', 'err', 'kappa', 'status'), ref, views_e, views_c):
            assert gh.same_bits(r, e) and gh.same_bits(r, c), (name, k)
        if held is not None:                                                                # call k - 1's views after call k
            for views in held[:2]:
                for name, view, then in zip(('dq', 'err', 'kappa', 'status'), views, held[2]):
                    assert gh.same_bits(view, then), (name, k)
        held = (views_e, views_c, ref)
        prev = ref[0]                                                                       # the explicit regressor is the previous return
    for bank in (explicit, chained):
        assert gh.same_bits(_np(bank.X), _np(dev.X)) and gh.same_bits(_np(bank.P), _np(dev.P))
    assert not ref[3].any()


# ---------------------------------------------------------------------------------------------- 6. return codes
def test_a_lane_count_that_is_not_instantiated_is_refused(uvs):
    fp = uvs.engine.make_params(8, 6, 'GMCKF', desired=np.zeros(8), lanes=16, steps=0)
    bank = uvs.engine.FilterBank(fp, 3, np.ones((3, 48)))
    z = gh.cuda(np.zeros((3, 8)))
    with pytest.raises(uvs._lib.UvsError) as exc:
        bank.step(z, z, gh.cuda(np.zeros((3, 6))), 0)
    assert exc.value.code == -2                                                             # UVS_ERR_SHAPE
    assert len(uvs.lib().uvs_last_error()) > 0
    assert gh.same_bits(_np(bank.X), np.ones((3, 48)))                                        # nothing ran
