"""GPU tests of the calibrated IBVS baseline (Method.ANALYTICAL, uvs_analytical_closed_loop_f64 / engine.analytical_closed_loop /
batch with "method": "ANALYTICAL") against the reference's own runs and the numpy restatement (tests/analytical_ref.py).  Need an MI355X."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden, rel_err

pytestmark = pytest.mark.gpu
FIXTURES = golden_names('analytical_')
GATE = {'analytical_mix_hold': 1e-3}          # intrinsic sensitivity of that trajectory: tests/test_analytical_host.py


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    return uvs_amd


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
