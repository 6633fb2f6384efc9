"""The single-precision replay (uvs_rmckf_replay_f32; SURVEY.md 8d "fp32 variant: report measured error, do not gate at 1e-5 closed-loop").

A MEASURED lower-precision variant, never the parity path: the reference's recorded f / dq streams (float32-rounded) go through the fp32
estimator-only kernel and the per-step Jacobian estimates are compared with the reference's own fp64 X.  The test PRINTS the error of
every fixture (pytest -s shows the table; it also lands in the assertion message on failure) and bounds it at the contract's 1e-5 -- open
loop only: there is no closed-loop fp32 path and no claim for one.

Below those, the gates (tests/replay_f32_common.py has the inputs, the figure E and the reasoning): the kernel against a plain float32
restatement of the same formulas, E_kernel <= 2 E_f32 per case; every one of the twelve instantiations (3 estimators x X wanted x err
wanted) and the optional status / k_done; row 0 of dq never read; pitched and [trial][step][component] views; and what a FAILed trial
leaves of itself and of its neighbours.  Every launch there goes through the C ABI with views built by hand, into buffers preset to a
sentinel."""
import ctypes as C

import numpy as np
import pytest

import replay_f32_common as rc
from conftest import golden_names, load_golden, rel_err
from gpu_harness import POISON_INT, same_bits

pytestmark = pytest.mark.gpu

CLOSED_F32 = [n for n in golden_names('closed_') if '_mckf_' not in n]        # KF, IMCC-KF, GMCKF runs of the unmodified reference


GATE_ROWS = []                                               # (case, layout, E_kernel, E_f32): printed when the module finishes (pytest -s)


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    if GATE_ROWS:
        print('\nfp32 replay against the float32 restatement (E: worst trial, relative to max |X64|; gate: E_kernel <= 2 E_f32):')
        for case, layout, ek, ef in GATE_ROWS:
            print(f'  {rc.case_id(case):44s} {layout}  E_kernel {ek:.2e}  E_f32 {ef:.2e}  ratio {ek / ef:.2f}')


def _run(uvs, g, T=35, layout='kct'):
    import torch
    meta, p = g['meta'], g['meta']['params']
    K = len(g['t'])
    fp = uvs.engine.make_params(8, 6, meta['method'], p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], meta['gain'], g['desired'], False, 0, K)
    f_seq = np.vstack([g['f_init'][None], g['f']])
    dims = {'kct': lambda a: np.repeat(a[:, :, None], T, axis=2), 'ktc': lambda a: np.repeat(a[:, None, :], T, axis=1)}[layout]
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')      # noqa: E731
    return uvs.engine.replay_f32(fp, cu(dims(f_seq)), cu(dims(g['dq_prev'])), cu(np.tile(g['X'][0], (T, 1))), layout=layout), K


def test_fp32_replay_error_against_the_reference_is_measured_and_bounded(uvs, capsys):
    rows = []
    for name in CLOSED_F32:
        g = load_golden(name)
        out, K = _run(uvs, g)
        X = out['x'].cpu().numpy().astype(np.float64)
        assert np.array_equal(X[:, :, 0], X[:, :, 34])                         # ragged batch (35 trials = 32 + 3): every copy the same bits
        assert out['status'].cpu().tolist() == [0] * 35 and out['k_done'].cpu().tolist() == [K] * 35
        ex = rel_err(X[g['X_steps'], :, 0], g['X'])
        per_step = np.abs(X[g['X_steps'], :, 0] - g['X']).max(axis=1) / np.abs(g['X']).max()
        ee = rel_err(out['err'].cpu().numpy()[:, :, 0].astype(np.float64), g['err'])
        rows.append((name, ex, float(per_step[:10].max()), ee))
    table = '\n'.join(f'{n:34s} X rel err {a:.2e} (first 10 steps {b:.2e})   err stream {c:.2e}' for n, a, b, c in rows)
    with capsys.disabled():
        print('\nfp32 replay vs the reference (fp64), open loop, per-step X over all 299 steps:\n' + table)
    worst = max(r[1] for r in rows)
    assert len(rows) >= 14 and worst <= 1e-5, table                           # the contract's 1e-5, open loop; SURVEY probe: 6e-7
    assert max(r[3] for r in rows) <= 1e-6                                    # err = f - f*: one fp32 rounding of the inputs


def test_fp32_replay_layouts_and_error_returns(uvs):
    """Per-trial records ([step][trial][component]) give the same bits as the trial-fastest layout; MCKF and other shapes are refused."""
    import ctypes as C
    g = load_golden('closed_gmckf_a1p5')
    a, K = _run(uvs, g, layout='kct')
    b, _ = _run(uvs, g, layout='ktc')
    assert np.array_equal(a['x'].cpu().numpy()[:, :, 3], b['x'].cpu().numpy()[:, 3, :]) and np.array_equal(a['err'].cpu().numpy()[:, :, 3], b['err'].cpu().numpy()[:, 3, :])
    # distinct trials in full and ragged wavefronts (36 = 32 + 4, 100 = 3 x 32 + 4): the two layouts agree bit for bit, a misplaced lane would show
    import torch
    meta, p = g['meta'], g['meta']['params']
    for T in (36, 100, 4):
        rng = np.random.default_rng(T)
        f_seq = np.vstack([g['f_init'][None], g['f']])[:41]
        f = f_seq[:, :, None] + rng.normal(size=(41, 8, T))
        dq = g['dq_prev'][:40, :, None] * (1 + 0.1 * rng.normal(size=(1, 1, T)))
        x0 = np.tile(g['X'][0], (T, 1)) * (1 + 0.01 * rng.normal(size=(T, 1)))
        fp = uvs.engine.make_params(8, 6, 'GMCKF', p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], meta['gain'], g['desired'], False, 0, 40)
        cu = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device='cuda')      # noqa: E731
        wide = uvs.engine.replay_f32(fp, cu(f), cu(dq), cu(x0), layout='kct')          # (trial-fastest)
        narrow = uvs.engine.replay_f32(fp, cu(f.transpose(0, 2, 1)), cu(dq.transpose(0, 2, 1)), cu(x0), layout='ktc')
        assert torch.equal(wide['x'], narrow['x'].permute(0, 2, 1)) and torch.equal(wide['err'], narrow['err'].permute(0, 2, 1)), T
        assert len({wide['x'][5, 7, t].item() for t in range(T)}) == T
    V = uvs._lib.NULL_VIEW
    fp = uvs.engine.make_params(8, 6, 'MCKF', desired=np.zeros(8), steps=3)
    one = uvs._lib.View(1, 0, 0, 0)
    assert uvs.lib().uvs_rmckf_replay_f32(C.byref(fp), 4, one, one, one, V, V, None, None, None) == -4
    fp = uvs.engine.make_params(6, 6, 'GMCKF', desired=np.zeros(6), steps=3)
    assert uvs.lib().uvs_rmckf_replay_f32(C.byref(fp), 4, one, one, one, V, V, None, None, None) == -2
    fp = uvs.engine.make_params(8, 6, 'GMCKF', desired=np.zeros(8), steps=3)
    assert uvs.lib().uvs_rmckf_replay_f32(C.byref(fp), 4, V, one, one, V, V, None, None, None) == -1


def test_fp32_replay_fails_a_trial_on_a_non_finite_state(uvs):
    import torch
    g = load_golden('closed_kf_a1p5')
    meta, p = g['meta'], g['meta']['params']
    K, T = 40, 64
    fp = uvs.engine.make_params(8, 6, 'KF', p['kernel_bw'], False, meta['dt'], meta['t_max'], meta['gain'], g['desired'], False, 0, K)
    f = np.repeat(np.vstack([g['f_init'][None], g['f']])[:K + 1, :, None], T, axis=2).astype(np.float32)
    f[17, 3, 5] = np.inf                                                      # an infinite feature reaches trial 5 at step 16
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')      # noqa: E731
    out = uvs.engine.replay_f32(fp, cu(f), cu(np.repeat(g['dq_prev'][:K, :, None], T, axis=2)), cu(np.tile(g['X'][0], (T, 1))))
    st, kd = out['status'].cpu().numpy(), out['k_done'].cpu().numpy()
    assert st[5] == 1 and kd[5] == 16 and st.sum() == 1 and (np.delete(kd, 5) == K).all()


# ---------------------------------------------------------------------------------------------- the gates (tests/replay_f32_common.py)
SENTINEL = -777.25                                           # what every buffer holds before a launch: finite, so that padding compares equal
ESTIMATORS = ['closed_kf_a1p5', 'closed_imcckf_sigma30_anneal', 'closed_gmckf_a1p5_anneal']       # one case per estimator, the annealed ones where there are
T35 = rc.T_RAGGED


def _window(T, K, comp, layout):
    """(whole, window): a device buffer full of SENTINEL and its logical [trial][step][component] window.  'pitched': trial-fastest rows
    pitched at T + 5 with one more step row than the stream has."""
    import torch
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device='cuda')      # noqa: E731
    if layout == 'kct':
        whole = full(K, comp, T)
        return whole, whole.permute(2, 0, 1)
    if layout == 'ktc':
        whole = full(K, T, comp)
        return whole, whole.permute(1, 0, 2)
    if layout == 'tkc':
        whole = full(T, K, comp)
        return whole, whole
    assert layout == 'pitched'
    whole = full(K + 1, comp, T + 5)
    return whole, whole[:K, :, :T].permute(2, 0, 1)


def _params(uvs, inp, K):
    fp = uvs.engine.make_params(8, 6, inp['method'], inp['kernel_bw'], inp['annealing'], inp['dt'], inp['t_max'], inp['gain'], inp['desired64'], False, 0, K)
    assert fp.k_max == inp['k_max'] and fp.steps == K
    return fp


def _launch(uvs, fp, f, dq, x0, want=('x', 'err'), layout='kct', status=True, k_done=True):
    """uvs_rmckf_replay_f32 through the C ABI on float32 streams f (T, K + 1, 8), dq (T, K, 6), x0 (T, 48), every stream -- in and out -- a
    hand-built view of a SENTINEL-filled buffer in `layout`; status / k_done NULL on request.  numpy arrays in [trial][step][component] order
    (None: not requested).  Whatever lies outside a window must still hold SENTINEL afterwards, and -- where status and k_done are returned --
    every live row of a requested stream must have been stored."""
    import torch
    T, K = x0.shape[0], fp.steps
    assert f.shape == (T, K + 1, 8) and dq.shape == (T, K, 6) and x0.shape == (T, 48) and f.dtype == dq.dtype == x0.dtype == np.float32
    view = lambda w: uvs._lib.NULL_VIEW if w is None else uvs._lib.View(w.data_ptr(), w.stride(0), w.stride(1), w.stride(2))      # noqa: E731
    ins = []
    for a in (f, dq):
        whole, win = _window(T, a.shape[1], a.shape[2], layout)
        win.copy_(torch.from_numpy(np.array(a)))
        ins.append((whole, win, whole.clone()))
    x0_dev = torch.from_numpy(np.array(x0)).cuda()
    outs = {key: _window(T, K, comp, layout) if key in want else (None, None) for key, comp in (('x', 48), ('err', 8))}
    ints = {key: torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda') if asked else None for key, asked in (('status', status), ('k_done', k_done))}
    code = uvs.lib().uvs_rmckf_replay_f32(C.byref(fp), T, view(ins[0][1]), view(ins[1][1]), uvs._lib.View(x0_dev.data_ptr(), x0_dev.stride(0), 0, x0_dev.stride(1)),
                                          view(outs['x'][1]), view(outs['err'][1]), *(None if ints[k] is None else ints[k].data_ptr() for k in ('status', 'k_done')),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(code)
    torch.cuda.synchronize()
    got = {key: None if win is None else np.array(win.cpu().numpy()) for key, (whole, win) in outs.items()}
    got.update({key: None if t is None else t.cpu().numpy() for key, t in ints.items()})
    for whole, win, before in ins:                                            # the inputs, padding included, are read-only
        assert torch.equal(whole.view(torch.int32), before.view(torch.int32))
    for key, (whole, win) in outs.items():
        if whole is not None:
            win.fill_(SENTINEL)
            assert bool((whole == SENTINEL).all()), (key, layout, 'a store outside the view')
    if status and k_done:
        assert set(got['status'].tolist()) <= {0, 1} and got['k_done'].min() >= 0 and got['k_done'].max() <= K
        live = np.arange(K)[None, :, None] < got['k_done'][:, None, None]
        for key in ('x', 'err'):
            if got[key] is not None:
                assert not (got[key] == SENTINEL)[np.broadcast_to(live, got[key].shape)].any(), (key, layout, 'a live row was not stored')
    return got


def _short(name, K, T=T35):
    """The first K steps of the K = 40 inputs of the case: (inp, f, dq, x0)."""
    inp = rc.inputs(name, T, rc.K_SHORT)
    return inp, inp['f'][:, :K + 1], inp['dq'][:, :K], inp['x0']


def _same_streams(a, b, keys=('x', 'err', 'status', 'k_done')):
    return all(a[k] is None or b[k] is None or same_bits(a[k], b[k]) for k in keys)


@pytest.mark.parametrize('case', rc.GPU_CASES, ids=rc.case_id)
def test_fp32_replay_is_within_twice_the_float32_restatement(uvs, case, capsys):
    """E_kernel(case) <= 2 E_f32(case), E_f32 from oracle/rmckf_block_f32 on the same inputs -- never from the kernel -- and the contract's
    1e-5 as well; both physical layouts.  The inputs carry a non-zero dq row 0.  Measured ratios: DESIGN.md, next to the kernel's entry."""
    name, T, K = case
    inp = rc.inputs(*case)
    ref32, e_f32 = rc.restatement(*case)
    assert e_f32 <= rc.E_F32_MAX
    fp = _params(uvs, inp, K)
    outs = {}
    for layout in ('kct', 'ktc'):
        out = outs[layout] = _launch(uvs, fp, inp['f'], inp['dq'], inp['x0'], layout=layout)
        e_kernel = rc.figure(out['x'], *case)
        GATE_ROWS.append((case, layout, e_kernel, e_f32))
        with capsys.disabled():
            print(f'\n  {rc.case_id(case):44s} {layout}  E_kernel {e_kernel:.2e}  E_f32 {e_f32:.2e}  ratio {e_kernel / e_f32:.2f}', end='')
        assert not out['status'].any() and (out['k_done'] == K).all(), (case, layout)
        assert e_kernel <= rc.MARGIN * e_f32 and e_kernel <= rc.CONTRACT, (case, layout, e_kernel, e_f32)
        assert same_bits(out['err'], ref32['err']), (case, layout)           # err = f - f*: one float32 subtraction, the restatement's bits
    assert _same_streams(outs['kct'], outs['ktc']), case


@pytest.mark.parametrize('name', ESTIMATORS)
def test_fp32_replay_every_instantiation_writes_the_same_bits(uvs, name):
    """3 estimators x (X wanted) x (err wanted): twelve kernels.  A requested stream has the bits of the both-streams launch, status and k_done
    are the same in all four; and either of them, or both, may be NULL."""
    K = 12
    inp, f, dq, x0 = _short(name, K)
    fp = _params(uvs, inp, K)
    both = _launch(uvs, fp, f, dq, x0)
    assert not both['status'].any() and (both['k_done'] == K).all()
    assert len({both['x'][t, 5, 7] for t in range(T35)}) == T35               # distinct trials
    for want in (('x',), ('err',), ()):
        out = _launch(uvs, fp, f, dq, x0, want=want)
        assert [k for k in ('x', 'err') if out[k] is not None] == list(want)
        assert _same_streams(out, both), (name, want)
    for status, k_done in ((False, True), (True, False), (False, False)):
        out = _launch(uvs, fp, f, dq, x0, status=status, k_done=k_done)
        assert (out['status'] is None) == (not status) and (out['k_done'] is None) == (not k_done)
        assert _same_streams(out, both), (name, status, k_done)


@pytest.mark.parametrize('name', ESTIMATORS)
def test_fp32_replay_ignores_row_0_of_dq(uvs, name):
    """H = 0 on the first step (experiment.py:183-185): zeros, other finite values or NaN in row 0 of dq -- the same bits everywhere, no FAIL."""
    K = 12
    inp, f, dq, x0 = _short(name, K)
    fp = _params(uvs, inp, K)
    assert np.abs(dq[:, 0]).min() > 0
    outs = []
    for row0 in (0.0, dq[:, 0], 1e3 * dq[:, 0], np.nan):
        dq_in = np.array(dq)
        dq_in[:, 0] = row0
        outs.append(_launch(uvs, fp, f, dq_in, x0))
        assert not outs[-1]['status'].any() and (outs[-1]['k_done'] == K).all(), name
        assert _same_streams(outs[-1], outs[0]), name


@pytest.mark.parametrize('name', ESTIMATORS)
def test_fp32_replay_takes_any_strides(uvs, name):
    """"Any other strides work": trial-fastest rows pitched at T + 5 with a spare step row, and [trial][step][component], inputs and outputs
    alike, against the dense trial-fastest launch; _launch checks that the padding keeps its sentinel."""
    K = 12
    inp, f, dq, x0 = _short(name, K)
    fp = _params(uvs, inp, K)
    dense = _launch(uvs, fp, f, dq, x0)
    for layout in ('pitched', 'tkc'):
        for want in (('x', 'err'), ('x',)):
            assert _same_streams(_launch(uvs, fp, f, dq, x0, want=want, layout=layout), dense), (name, layout, want)


# what goes non-finite -> {trial: the step it FAILs at}.  35 trials = 32 + 3: trial 34 is the one the 29 padding lanes of the second
# wavefront shadow; with 32, 33 and 34 all failed that wavefront leaves its step loop early.
FAILURES = {'trial 5 at step 16': {5: 16}, 'the last trial at step 3': {34: 3}, 'the whole second wavefront at step 3': {32: 3, 33: 3, 34: 3},
            'x0 of trial 0': {0: 0}}


@pytest.mark.parametrize('where', list(FAILURES))
def test_fp32_replay_failed_trials_leave_everything_else_alone(uvs, where):
    """status and k_done exact; every other trial, and the failed trial's rows before k_done, carry the bits of the clean launch."""
    K = rc.K_SHORT
    for name in ESTIMATORS:
        inp, f, dq, x0 = _short(name, K)
        fp = _params(uvs, inp, K)
        clean = _launch(uvs, fp, f, dq, x0)
        assert not clean['status'].any() and (clean['k_done'] == K).all()
        f_bad, x0_bad = np.array(f), np.array(x0)
        for t, k in FAILURES[where].items():
            if where.startswith('x0'):
                x0_bad[t, 7] = np.nan
            else:
                f_bad[t, k + 1, 3] = np.inf                                   # the features of step k
        out = _launch(uvs, fp, f_bad, dq, x0_bad)
        status, k_done = np.zeros(T35, np.int32), np.full(T35, K, np.int32)
        for t, k in FAILURES[where].items():
            status[t], k_done[t] = 1, k
        assert np.array_equal(out['status'], status) and np.array_equal(out['k_done'], k_done), (name, where, out['status'].tolist(), out['k_done'].tolist())
        for t in range(T35):
            for key in ('x', 'err'):
                assert same_bits(out[key][t, :k_done[t]], clean[key][t, :k_done[t]]), (name, where, key, t)


@pytest.mark.parametrize('name', ESTIMATORS)
def test_fp32_replay_of_a_single_step(uvs, name):
    """K = 1: no prefetch inside the loop, and H = 0 -- the gain is exactly 0 in any arithmetic, so the one row of X is x0 and the
    restatement's bits."""
    from oracle import rmckf_block_f32
    inp, f, dq, x0 = _short(name, 1)
    out = _launch(uvs, _params(uvs, inp, 1), f, dq, x0)
    ref = rmckf_block_f32.run_replay(f, dq, x0, inp['desired'], inp['method'], inp['kernel_bw'], inp['annealing'], inp['k_max'])
    assert not out['status'].any() and (out['k_done'] == 1).all()
    assert same_bits(ref['X'][:, 0], x0) and same_bits(out['x'], ref['X']) and same_bits(out['err'], ref['err']), name
