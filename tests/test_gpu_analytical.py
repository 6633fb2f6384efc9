"""GPU tests of the calibrated IBVS baseline (Method.ANALYTICAL, uvs_analytical_closed_loop_f64 / engine.analytical_closed_loop /
batch with "method": "ANALYTICAL") against the reference's own runs and the numpy restatement (tests/analytical_ref.py).  Need an MI355X."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import analytical_common as ac
import gpu_harness as gh
from conftest import ROOT, golden_names, load_golden, rel_err
from gpu_harness import STRICT, TOL

pytestmark = pytest.mark.gpu
FIXTURES = golden_names('analytical_')
GATE = {'analytical_mix_hold': 1e-3}          # intrinsic sensitivity of that trajectory: tests/test_analytical_host.py
TOL_J = 1e-10                                 # the J stream (test_fixture_through_c_abi)
WORST = gh.Worst()                            # route -> quantity -> worst relative deviation from the restatement so far


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    WORST.report('calibrated baseline')


def _cfg(method='ANALYTICAL', epoch=100):
    cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
    cfg['estimator']['method'] = method
    cfg['experiments']['epoch'] = epoch
    return cfg


def _fixture_noise(g, K):
    noise = np.zeros((K, 8))
    noise[:len(g['noise'])] = g['noise']
    if g['meta']['profile'] == 'InfAt':
        noise[40, 3] = np.inf
    return noise


@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_through_c_abi(uvs, name, strict):
    import torch
    g = load_golden(name)
    meta = g['meta']
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', t_s=meta['dt'], t_max=meta['t_max'], gain=meta['gain'], desired=g['desired'])
    fp.reserved = 1 if strict else 0
    K = fp.steps
    T = 3                                                                    # the trial replicated: padding lanes of one wavefront
    q0 = torch.as_tensor(np.tile(g['q_start'], (T, 1)), device='cuda')
    noise = torch.as_tensor(np.ascontiguousarray(np.repeat(_fixture_noise(g, K)[:, :, None], T, axis=2)), device='cuda')
    out = uvs.engine.analytical_closed_loop(fp, uvs.SyntheticPlant.ur10().to_struct(), q0, noise, want=('j', 'err', 'q', 'f', 'dq'))
    torch.cuda.synchronize()
    k = int(g['k_done'])
    assert out['status'].cpu().tolist() == [int(g['status'])] * T and out['k_done'].cpu().tolist() == [k] * T
    o = {key: out[key].cpu().numpy()[:k, :, 0] for key in ('j', 'err', 'q', 'f', 'dq')}
    gate = GATE.get(name, 1e-8)
    for key, ref in (('err', g['err']), ('q', g['q']), ('f', g['f'])):
        assert rel_err(o[key], ref) <= gate, (key, rel_err(o[key], ref))
    assert rel_err(o['j'], g['J']) <= GATE.get(name, 1e-10), rel_err(o['j'], g['J'])
    import analytical_ref
    ref = analytical_ref.run(g['q_start'][None], _fixture_noise(g, K)[None], g['desired'], meta['dt'], meta['t_max'], meta['gain'])
    assert rel_err(o['dq'], ref['dq'][0, :k]) <= gate, rel_err(o['dq'], ref['dq'][0, :k])
    if k:
        t = uvs.engine.loop_clock(meta['dt'], meta['t_max'])[:k]
        e = g['err']
        per_row = np.stack([(e * e).sum(0), np.abs(e).sum(0), (t[:, None] * np.abs(e)).sum(0)])
        assert rel_err(out['stats'][0].cpu().numpy(), np.sqrt((per_row ** 2).sum(1))) <= gate


def test_full_size_batch_against_restatement(uvs):
    """BASELINE config 2 (65 536 trials x 299 steps, alpha-stable 1.5 noise from the device generator) through batch.run_batch with ANALYTICAL:
    status, k_done and the three norms of EVERY trial against the numpy restatement on the same noise (16 threads; no trial exempt)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import analytical_ref
    cfg = _cfg()
    res = uvs.batch.run_batch(cfg, cells=[1.5], epoch=65536, want=('err',))
    T = res.hi - res.lo
    assert T == 65536
    noise = res.noise.cpu().numpy()                                          # [step][feature][trial] (an overlapping view, copied here)
    desired = cfg['experiments']['desired_f']

    def chunk(a):                                                            # numpy's linalg and array kernels release the GIL
        r = analytical_ref.run(res.plan.q_start[a:a + 4096], np.ascontiguousarray(noise[:, :, a:a + 4096].transpose(2, 0, 1)), desired,
                               0.05, 15, 0.2, logs=())
        return r['status'], r['k_done'], r['stats']
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        parts = list(pool.map(chunk, range(0, T, 4096)))
    seconds = time.perf_counter() - t0
    ref_status, ref_k, ref_stats = (np.concatenate([p[i] for p in parts]) for i in range(3))
    status, k_done, stats = res.status.cpu().numpy(), res.k_done.cpu().numpy(), res.stats.cpu().numpy()
    ok = status == 0
    worst = float(np.abs(stats[ok] / ref_stats[ok] - 1).max()) if ok.any() else 0.0
    print(f'\nfull-size census: {T} trials compared (all), SUCCESS {int(ok.sum())}, FAIL {int((status == 1).sum())}, status mismatches '
          f'{int((status != ref_status).sum())}, k_done mismatches {int((k_done != ref_k).sum())}, worst norm rel {worst:.3g}; '
          f'restatement {seconds:.1f} s on 16 threads, GPU launch {res.seconds * 1e3:.2f} ms')
    assert np.array_equal(status, ref_status) and np.array_equal(k_done, ref_k)
    assert np.all(np.abs(stats - ref_stats) <= 1e-8 * np.abs(ref_stats)), worst


def _coincident(uvs):
    """UR10 plant whose four discs coincide: J_feature has two distinct rows, repeated four times -- rank 2 of 6 on every step."""
    plant = uvs.SyntheticPlant.ur10()
    plant.points[:] = plant.points[0]
    return plant


def _coincident_run(uvs, strict, T=100):
    import torch
    rng = np.random.default_rng(3)
    q0 = np.tile([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0], (T, 1))  # config.json's q_start, jittered as main.py:132-134 does
    q0[1:, :2] += rng.uniform(-0.2, 0.0, (T - 1, 2))
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', desired=np.array([149.0, 145.0, 125.0, 121.0, 101.0, 145.0, 125.0, 169.0]))
    fp.reserved = 1 if strict else 0
    noise = np.zeros((fp.steps, 8, T))
    noise[40, 3, 7] = np.inf                                                 # trial 7: pinv raises at step 40 -- the careful pass's FAIL probe
    out = uvs.engine.analytical_closed_loop(fp, _coincident(uvs).to_struct(), torch.as_tensor(q0, device='cuda'),
                                            torch.as_tensor(noise, device='cuda'), want=('j', 'err', 'q', 'f', 'dq'))
    torch.cuda.synchronize()
    return q0, noise, fp, {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in out.items() if k != 'events' and v is not None}


def test_rank_deficient_jacobian_takes_numpy_pinv(uvs):
    """Coincident discs: rank(J_feature) = 2 on all 299 steps.  The first pass must mark every trial (its QR's |R_cc| spread is beyond the
    2^34 watch from step 0, checked below on the same J), and the careful pass -- LDS plant and statistics, entry-by-entry FAIL probe,
    QR finished by the SVD with numpy's cutoff -- must return numpy's truncated minimum-norm command: the GPU against the restatement's
    np.linalg.pinv over the whole trajectory, with one trial FAILed by an inf at step 40."""
    import analytical_ref
    q0, noise, fp, out = _coincident_run(uvs, strict=False)
    T = q0.shape[0]
    ref = analytical_ref.run(q0, noise.transpose(2, 0, 1), fp.desired[:8], points=_coincident(uvs).points)
    J0 = ref['j'][:, 0].reshape(T, 8, 6)
    assert np.all(np.linalg.matrix_rank(J0) == 2)
    rdiag = np.abs(np.diagonal(np.linalg.qr(J0)[1], axis1=1, axis2=2))
    assert np.all(rdiag.max(axis=1) / rdiag.min(axis=1) >= 2.0 ** 34)      # what the first pass's spread watch marks
    expect_status = np.zeros(T, np.int32)
    expect_status[7] = 1
    assert np.array_equal(ref['status'], expect_status) and ref['k_done'][7] == 40
    assert np.array_equal(out['status'], ref['status']) and np.array_equal(out['k_done'], ref['k_done'])
    for t in range(T):
        k = int(ref['k_done'][t])
        for key in ('err', 'q', 'f', 'dq'):
            got = out[key].transpose(2, 0, 1)[t, :k]
            assert rel_err(got, ref[key][t, :k]) <= 1e-8, (t, key, rel_err(got, ref[key][t, :k]))
        assert rel_err(out['j'].transpose(2, 0, 1)[t, :k], ref['j'][t, :k]) <= 1e-10
    assert np.all(np.abs(ref['dq']) < 10)                                   # (a plain solve divides by pivots of 1e-30: nothing like this)
    assert np.all(np.abs(out['stats'] - ref['stats']) <= 1e-8 * np.abs(ref['stats']))


def test_rank_deficient_strict_equals_default(uvs):
    a = _coincident_run(uvs, strict=False)[3]
    b = _coincident_run(uvs, strict=True)[3]
    for key in ('status', 'k_done', 'stats'):
        assert np.array_equal(a[key], b[key]), key
    for t in range(len(a['status'])):                                        # streams: the logged rows (later ones are unspecified)
        k = int(a['k_done'][t])
        for key in ('err', 'q', 'f', 'dq', 'j'):
            assert np.array_equal(a[key][:k, :, t], b[key][:k, :, t]), (t, key)


def test_strict_pinv_is_bit_identical_at_full_size(uvs):
    cfg = _cfg()
    a = uvs.batch.run_batch(cfg, cells=[1.5], epoch=65536, want=('err',))
    b = uvs.batch.run_batch(cfg, cells=[1.5], epoch=65536, want=('err',), strict_pinv=True)
    assert np.array_equal(a.status.cpu().numpy(), b.status.cpu().numpy())
    assert np.array_equal(a.stats.cpu().numpy(), b.stats.cpu().numpy())
    assert np.array_equal(a.streams['err'].cpu().numpy(), b.streams['err'].cpu().numpy())


def test_pairing_with_an_estimator(uvs):
    """The same config as GMCKF and as ANALYTICAL reads an identical noise tensor and starts from an identical q."""
    a = uvs.batch.run_batch(_cfg('GMCKF'), cells=[1.0], epoch=512, want=('q',))
    b = uvs.batch.run_batch(_cfg('ANALYTICAL'), cells=[1.0], epoch=512, want=('q',))
    assert np.array_equal(a.noise.cpu().numpy(), b.noise.cpu().numpy())
    assert np.array_equal(a.streams['q'][0].cpu().numpy(), b.streams['q'][0].cpu().numpy())


def test_sharded_sweep_is_bit_identical(uvs):
    cfg = _cfg(epoch=64)
    whole = uvs.batch.run_sweep(cfg)
    parts = [uvs.batch.run_sweep(cfg, rank=r, world=2) for r in (0, 1)]
    assert np.array_equal(whole.rows(), np.concatenate([p.rows() for p in parts]))
    assert (whole.status == 0).sum() > 0


def test_results_csv(uvs, tmp_path):
    import pandas as pd
    cfg = _cfg(epoch=2)
    plant = uvs.SyntheticPlant.ur10(cfg['experiments']['desired_f'])
    res = uvs.batch.run_batch(cfg, epoch=2, want=('q', 'f'))
    assert res.hi - res.lo == 24
    path = tmp_path / 'results.csv'
    uvs.batch.write_results_csv(res, cfg, plant, str(path))
    df = pd.read_csv(path)
    k_done = res.k_done.cpu().numpy()
    assert len(df) == int(k_done.sum())
    assert (df['kernel_bw'] == -1).all()
    assert set(df['status']) <= {'ExperimentStatus.SUCCESS', 'ExperimentStatus.FAIL'}


# ---------------------------------------------------------------------------------------------- off the fixture path
# tests/analytical_common.py: T = 70 (a full wavefront and a ragged one of six lanes) x K = 40 on a general DH / pinhole plant ('tilted',
# 'tilted_placed') and on the UR10 with outliers that take single trials of a wavefront out of the first pass ('mixed'); their
# preconditions are held on the CPU by tests/test_analytical_host.py.  Every launch goes through the C ABI into buffers of its own that are
# filled with NaN (-7 for the integers) beforehand.  Gates, per trial: err, q, f, dq and the statistics of SUCCESS trials 1e-8, J 1e-10,
# status and k_done exact; rows at and after k_done are unspecified and never compared.
J_STREAMS = ('j', 'err', 'q', 'f', 'dq')                                     # the header's order
COMPS = {'j': 48, 'err': 8, 'q': 6, 'f': 8, 'dq': 6}
PER_TRIAL = ('stats', 'status', 'k_done')
_RUNS = {}


def _noise_of(case):
    return ac.mixed_noise() if case == 'mixed' else ac.base_inputs()['noise']


def _device_stream(uvs, a, layout, pitched):
    """(T, K, comp) numpy -> device tensor in `layout`; pitched: rows of engine.alloc_stream under UVS_ROW_PAD (the caller set it)."""
    if not pitched:
        return gh.cuda(a.transpose({'kct': (1, 2, 0), 'ktc': (1, 0, 2), 'tkc': (0, 1, 2)}[layout]))
    dev = uvs.engine.alloc_stream(a.shape[0], a.shape[1], a.shape[2], layout)
    assert not dev.is_contiguous()
    uvs.engine.as_tkc(dev, layout).copy_(gh.cuda(a))
    return dev


def _launch(uvs, case, strict=False, layout='kct', pitched=False, trials=slice(None), steps=ac.K, noise='case', omit=(), rows=None):
    """uvs_analytical_closed_loop_f64 on the trials `trials` of a case of analytical_common, `steps` steps, into poisoned buffers of `rows`
    rows (default: steps).  noise: 'case', None (a NULL view) or a (T, K, 8) array; omit: outputs handed over as NULL.  Returns numpy
    arrays, the streams as [trial][step][component] whatever the layout (None where omitted)."""
    import torch
    inp = ac.base_inputs()
    q0 = inp['q0'][trials]
    T = len(q0)
    rows = steps if rows is None else rows
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', t_s=ac.DT, gain=ac.GAIN, desired=inp['desired'], steps=steps)
    assert fp.steps == steps
    fp.reserved = STRICT if strict else 0
    ps = ac.device_plant(uvs, ac.plant_of(case) or ac.ur10_values()).to_struct()
    noise = _noise_of(case) if isinstance(noise, str) else noise
    noise_dev = None if noise is None else _device_stream(uvs, noise[trials][:, :steps], layout, pitched)
    dev = {}
    for k in J_STREAMS:
        if k in omit:
            dev[k] = None
        elif pitched:
            dev[k] = uvs.engine.alloc_stream(T, rows, COMPS[k], layout).fill_(float('nan'))
        else:
            dev[k] = gh.poisoned(T, rows, COMPS[k], layout)
    dev.update(gh.poisoned_trials(T))
    q0_dev = gh.cuda(q0)
    ptr = lambda k: None if k in omit else dev[k].data_ptr()                 # noqa: E731
    rc = uvs.lib().uvs_analytical_closed_loop_f64(
        C.byref(fp), C.byref(ps), T, uvs._lib.View(q0_dev.data_ptr(), q0_dev.stride(0), 0, q0_dev.stride(1)), uvs.engine.stream_view(noise_dev, layout),
        *(uvs.engine.stream_view(dev[k], layout) for k in J_STREAMS), ptr('stats'), ptr('status'), ptr('k_done'),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    out = {k: None if dev[k] is None else np.ascontiguousarray(uvs.engine.as_tkc(dev[k], layout).cpu().numpy()) for k in J_STREAMS}
    out.update({k: None if k in omit else dev[k].cpu().numpy() for k in PER_TRIAL})
    return out


def _run(uvs, case, strict=False):
    """The dense 'kct' launch of all 70 trials of a case with every output: shared by the tests that compare with it."""
    if (case, strict) not in _RUNS:
        _RUNS[case, strict] = _launch(uvs, case, strict)
    return _RUNS[case, strict]


def _live(out, key, k_done=None):
    return gh.live(dict(out, k_done=out['k_done'] if k_done is None else k_done), key)


def _assert_stored(out, tag):
    """No poison in a status, a k_done, the statistics or a live row of any stream the launch wrote."""
    assert set(out['status'].tolist()) <= {0, 1} and out['k_done'].min() >= 0, tag
    if out['stats'] is not None:
        assert not np.isnan(out['stats']).any(), tag
    for key in J_STREAMS:
        if out[key] is not None:
            assert not np.isnan(_live(out, key)).any(), (key, tag)


def _assert_matches(out, ref, route, tag, trials=slice(None)):
    """A launch of the trials `trials` of a case against the restatement `ref` of the whole case at the gates above."""
    status, k_done = ref['status'][trials], ref['k_done'][trials]
    assert np.array_equal(out['status'], status) and np.array_equal(out['k_done'], k_done), (tag, out['status'].tolist(), out['k_done'].tolist())
    _assert_stored(out, tag)
    for key in J_STREAMS:                                                    # (the restatement's rows at and after k_done are zero)
        d = gh.per_trial_rel(_live(out, key), ref[key][trials][:, :out[key].shape[1]])
        WORST.note(route, key, d.max())
        print(f'{route} {tag} {key}: worst per-trial deviation {d.max():.2e} (trial {int(d.argmax())})')
        assert d.max() <= (TOL_J if key == 'j' else TOL), (key, float(d.max()), int(d.argmax()), tag)
    ok = status == 0
    d = gh.per_trial_rel(out['stats'][ok], ref['stats'][trials][ok])
    WORST.note(route, 'stats', d.max())
    print(f'{route} {tag} stats: worst per-trial deviation {d.max():.2e}')
    assert d.max() <= TOL, ('stats', float(d.max()), tag)


def _assert_same_bits(a, b, tag, trials_a=slice(None), trials_b=slice(None), keys=J_STREAMS + PER_TRIAL):
    """Two launches wrote the same bits: every logged row (by the first one's k_done, which is compared too) and every per-trial output."""
    for key in keys:
        if a.get(key) is None or b.get(key) is None:
            continue
        if key in J_STREAMS:
            x, y = _live(a, key)[trials_a], _live(b, key, None if b['k_done'] is not None else a['k_done'][trials_a])[trials_b]
        else:
            x, y = a[key][trials_a], b[key][trials_b]
        assert gh.same_bits(x, y), (key, tag)


# a. a general plant
@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('case', ['tilted', 'tilted_placed'])
def test_general_plant_against_restatement(uvs, case, strict):
    """Every DH and camera parameter off its UR10 value, in the kernel whose control law IS camera_jacobian and feature_jacobian_row on every
    step: all five streams and the statistics of all 70 trials against the restatement on the same plant."""
    _assert_matches(_run(uvs, case, strict), ac.reference(case), f'general plant{", strict" if strict else ""}', case)


@pytest.mark.parametrize('case', ['tilted', 'tilted_placed'])
def test_general_plant_strict_gives_the_default_bits(uvs, case):
    a, b = _run(uvs, case, False), _run(uvs, case, True)
    assert not a['status'].any()
    _assert_same_bits(a, b, case)


# b. layouts and optional outputs (the tilted plant)
@pytest.mark.parametrize('layout', ['ktc', 'tkc'])
def test_other_layouts_give_the_dense_bits(uvs, layout):
    out = _launch(uvs, 'tilted', layout=layout)
    _assert_stored(out, layout)
    _assert_same_bits(_run(uvs, 'tilted'), out, layout)


def test_pitched_rows_give_the_dense_bits(uvs, monkeypatch):
    """Noise and outputs in rows pitched at T + 37 (UVS_ROW_PAD, engine.alloc_stream): nothing is 16-byte aligned any more."""
    monkeypatch.setenv('UVS_ROW_PAD', '37')
    out = _launch(uvs, 'tilted', pitched=True)
    _assert_stored(out, 'pitched')
    _assert_same_bits(_run(uvs, 'tilted'), out, 'pitched')


@pytest.mark.parametrize('gone', ['j', 'err', 'q', 'f', 'dq', 'stats', 'k_done'])
def test_an_output_left_out_changes_no_other(uvs, gone):
    dense = _run(uvs, 'tilted')
    out = _launch(uvs, 'tilted', omit=(gone,))
    assert out[gone] is None
    if gone != 'k_done':
        _assert_stored(out, gone)
    else:
        assert set(out['status'].tolist()) == {0} and not np.isnan(out['stats']).any()
    _assert_same_bits(dense, out, ('without', gone))
    if gone == 'k_done':                                                     # every trial ran all K steps: every row is logged
        for key in J_STREAMS:
            assert gh.same_bits(dense[key], out[key]), key


def test_no_noise_is_zero_noise(uvs):
    zero = _launch(uvs, 'tilted', noise=np.zeros((ac.T, ac.K, 8)))
    none = _launch(uvs, 'tilted', noise=None)
    _assert_stored(none, 'no noise')
    _assert_same_bits(zero, none, 'no noise')
    assert not gh.same_bits(zero['err'], _run(uvs, 'tilted')['err'])         # (and the noise of the other launches is read)


def test_reuse_writes_the_first_trials_only(uvs):
    """engine.analytical_closed_loop(reuse=), what run_sweep sends cell after cell through: a T = 33 launch into the buffers of a T = 70
    launch equals a fresh T = 33 launch, and trials 33 - 69 of every buffer keep the first launch's bits."""
    import torch
    inp = ac.base_inputs()
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', t_s=ac.DT, gain=ac.GAIN, desired=inp['desired'], steps=ac.K)
    ps = ac.device_plant(uvs, ac.tilted_values()).to_struct()
    q0, noise = gh.cuda(inp['q0']), gh.cuda(inp['noise'].transpose(1, 2, 0))
    shifted = gh.cuda(inp['noise'][::-1][:33].transpose(1, 2, 0))           # other noise for the second launch: its results differ
    first = uvs.engine.analytical_closed_loop(fp, ps, q0, noise, want=J_STREAMS)
    torch.cuda.synchronize()
    keys = J_STREAMS + PER_TRIAL
    before = {k: first[k].cpu().numpy().copy() for k in keys}
    second = uvs.engine.analytical_closed_loop(fp, ps, q0[:33], shifted, want=J_STREAMS, reuse=first)
    fresh = uvs.engine.analytical_closed_loop(fp, ps, q0[:33], shifted, want=J_STREAMS)
    torch.cuda.synchronize()
    after = {k: first[k].cpu().numpy() for k in keys}
    assert not fresh['status'].cpu().numpy().any() and np.all(fresh['k_done'].cpu().numpy() == ac.K)       # every row is logged: whole buffers compare
    for k in keys:
        head = (Ellipsis, slice(0, 33)) if k in J_STREAMS else slice(0, 33)
        tail = (Ellipsis, slice(33, None)) if k in J_STREAMS else slice(33, None)
        assert second[k].data_ptr() == first[k].data_ptr(), k
        assert gh.same_bits(after[k][head], fresh[k].cpu().numpy()), k
        assert gh.same_bits(after[k][tail], before[k][tail]), k
    assert not gh.same_bits(after['err'][..., :33], before['err'][..., :33])


@pytest.mark.parametrize('trials', [slice(69, 70), slice(0, 65)], ids=['trial_69_alone', 'T_65'])
def test_fewer_trials_give_the_same_bits(uvs, trials):
    """T = 1 and T = 65 (one lane in the second wavefront): a trial's bits do not depend on how many lanes run beside it."""
    out = _launch(uvs, 'tilted', trials=trials)
    _assert_stored(out, trials)
    _assert_same_bits(_run(uvs, 'tilted'), out, trials, trials_a=trials)


# c. a mixed wavefront
@pytest.mark.parametrize('strict', [False, True])
def test_mixed_wavefront_against_restatement(uvs, strict):
    """One wavefront with healthy lanes, four trials that turn suspect in mid-trajectory (step 17: a mid lane, the second half, the last lane,
    and one in the ragged tail), a first-pass FAIL (20, step 9), a careful-pass FAIL (41, step 23) and a truncated solve followed by a FAIL
    (64, steps 5 and 30): status and k_done exact, every trial at the gates over all its steps."""
    out, ref = _run(uvs, 'mixed', strict), ac.reference('mixed')
    route = f'mixed wavefront{", strict" if strict else ""}'
    for t, k in ac.FAIL_AT.items():
        assert out['status'][t] == 1 and out['k_done'][t] == k, (t, out['status'][t], out['k_done'][t])
    assert out['status'].sum() == len(ac.FAIL_AT)
    _assert_matches(out, ref, route, 'mixed')
    # the hit trials once more: the 1e13 of their row 17 is the largest entry of err, f and J, so the per-trial norm above says little about
    # their other rows -- those against the restatement with row 17 left out (the same gates: the restatement moves by 1.8e-14 there under
    # a 1e-14 shift of q0) ...
    hit = list(ac.HIT)
    rest = np.arange(ac.K) != ac.HIT_STEP
    for key in J_STREAMS:
        d = gh.per_trial_rel(_live(out, key)[hit][:, rest], ref[key][hit][:, rest])
        WORST.note(route, key + ' (hit trials, other rows)', d.max())
        print(f'{route} {key}: hit trials without row {ac.HIT_STEP}: {d.max():.2e}')
        assert d.max() <= (TOL_J if key == 'j' else TOL), (key, float(d.max()))
    # ... and the command of row 17 by itself: numpy's truncated one (~1e-12; a plain solve gives ~0.05).  The two singular values numpy
    # keeps are 2.5e-11 apart, so one rounding of J moves that command by eps sigma_1 / sigma_2 = 9e-6 of its size: 1e-4.
    d = gh.per_trial_rel(out['dq'][hit, ac.HIT_STEP], ref['dq'][hit, ac.HIT_STEP])
    WORST.note(route, 'dq (row of the truncated solve)', d.max())
    print(f'{route} dq row {ac.HIT_STEP} of the hit trials against numpy pinv: {d.max():.2e}; size {np.abs(out["dq"][hit, ac.HIT_STEP]).max():.2e}')
    assert np.abs(out['dq'][hit, ac.HIT_STEP]).max() <= 1e-10 and d.max() <= 1e-4, float(d.max())


@pytest.mark.parametrize('strict', [False, True])
def test_mixed_wavefront_leaves_the_healthy_trials_alone(uvs, strict):
    """The 63 trials without an outlier: bit for bit what a launch of the base noise gives them -- the careful pass changes no healthy trial,
    and no row of a flagged neighbour's first pass leaks into theirs."""
    mixed, base = _run(uvs, 'mixed', strict), _run(uvs, 'base', strict)
    assert not base['status'].any() and np.all(base['k_done'] == ac.K)
    untouched = list(ac.UNTOUCHED)
    assert len(untouched) == 63
    _assert_same_bits(base, mixed, ('untouched', strict), trials_a=untouched, trials_b=untouched)
    for t in ac.HIT:                                                         # (while a hit trial's rows do change, from the hit on)
        assert not gh.same_bits(base['q'][t, ac.HIT_STEP + 1:], mixed['q'][t, ac.HIT_STEP + 1:])


def test_mixed_wavefront_statistics_agree_with_the_statistics_kernel(uvs):
    """The norms the two passes accumulate (registers in the first, LDS in the careful one) against engine.stats_reduce on the err stream
    the same launch logged: 1e-12 on every SUCCESS trial."""
    out = _run(uvs, 'mixed')
    t = uvs.engine.loop_clock(ac.DT, 15.0)[:ac.K]
    got = uvs.engine.stats_reduce(gh.cuda(_live(out, 'err').transpose(1, 2, 0)), t, gh.cuda(out['k_done'])).cpu().numpy()
    ok = out['status'] == 0
    d = gh.per_trial_rel(out['stats'][ok], got[ok])
    WORST.note('mixed wavefront', 'stats (against the statistics kernel)', d.max())
    assert ok.sum() == ac.T - len(ac.FAIL_AT) and d.max() <= 1e-12, float(d.max())


# d. horizon edges
@pytest.mark.parametrize('noise', ['none', 'no_rows'])
def test_zero_steps(uvs, noise):
    """K = 0: SUCCESS, k_done 0 and zero statistics on every trial, and no stream is touched -- also with a noise view that is on (a base
    address) while the launch has no rows to read through it."""
    import torch
    T = ac.T
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', t_s=ac.DT, gain=ac.GAIN, desired=ac.base_inputs()['desired'], steps=0)
    assert fp.steps == 0
    ps = ac.device_plant(uvs, ac.tilted_values()).to_struct()
    dev = {k: gh.poisoned(T, 2, COMPS[k]) for k in J_STREAMS}
    dev.update(gh.poisoned_trials(T))
    q0 = gh.cuda(ac.base_inputs()['q0'])
    view = uvs._lib.NULL_VIEW
    if noise == 'no_rows':
        holder = gh.poisoned(T, 1, 8)                                        # (torch hands out no address for a tensor of no rows)
        view = uvs.engine.stream_view(holder, 'kct')
        assert view.base and holder[:0].shape == (0, 8, T)
    rc = uvs.lib().uvs_analytical_closed_loop_f64(
        C.byref(fp), C.byref(ps), T, uvs._lib.View(q0.data_ptr(), 6, 0, 1), view, *(uvs.engine.stream_view(dev[k], 'kct') for k in J_STREAMS),
        dev['stats'].data_ptr(), dev['status'].data_ptr(), dev['k_done'].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    assert dev['status'].cpu().tolist() == [0] * T and dev['k_done'].cpu().tolist() == [0] * T
    assert gh.same_bits(dev['stats'].cpu().numpy(), np.zeros((T, 3)))
    for k in J_STREAMS:
        assert np.isnan(dev[k].cpu().numpy()).all(), k


def test_one_step(uvs):
    out, dense = _launch(uvs, 'tilted', steps=1), _run(uvs, 'tilted')
    assert np.all(out['k_done'] == 1)
    _assert_matches(out, ac.reference('tilted', 1), 'one step', 'tilted')
    for key in J_STREAMS:                                                    # and it is the first of the 40
        assert gh.same_bits(out[key], dense[key][:, :1]), key
