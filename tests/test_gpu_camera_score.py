"""The X log, the true image Jacobian and the score on the GPU (include/uvs_vision.h, "THE ESTIMATE AS A LOG" and "THE TRUE IMAGE
JACOBIAN"; engine.camera_closed_loop(want=(..., 'x')), engine.camera_jacobian, engine.camera_jacobian_score).

(a) x_log = NULL through the C ABI: every output of logged_frames_kernel has its predicted namesake's bits, in all 22 instantiations,
poison past the last row included.  (b) With the log every other output keeps those bits; rows k < k_done of 'x' are the stepwise loop's
X after its step call k on every route that has a stepwise estimator loop; under trial_params and predict, which are one-launch only,
every trial has the bits of its uniform launch.  (c) 'x' against the CPU restatement (camera_score_common.logged_trial, held to the
oracle's loop by the host file) to 1e-10 relative; measured worst value 3.5e-16.  (d) What is not written: rows k >= k_done of a
trial that FAILs mid-run, of a void trial and of the padding keep their sentinel, and the guard bands behind every output of the three
entry points stay poisoned.  (e) camera_jacobian against plant.projection_jacobian, 1e-10 |J|_F per record, and a record's bits do not
depend on the launch.  (f) camera_jacobian_score against plant.jacobian_score.  (g) The three together: from x0 = dt J(q_start) row 0
scores diff2 == 0.0 exactly, and from the reference's guess row 0's scale lies in the band the test computes on the CPU.
Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, the last workgroup with padding wavefronts); K = 16."""
import ctypes as C

import numpy as np
import pytest

import camera_common as cc
import camera_moving_common as mc
import camera_predicted_common as pc
import camera_scenes_common as sc
import camera_score_common as sco
import pixel_loop_common as pl
from test_gpu_camera_moving import BUILT, POISON, TAIL, assert_same_buffers, buffers, dev, loop_operands, motions, params, scenario_kw, scene_set, stream
from test_gpu_camera_predicted import c_estimator_loop as c_predicted_loop
from test_gpu_camera_predicted import route_kw

pytestmark = pytest.mark.gpu

K = sco.K
bits = cc.bits
SENTINEL = 7.25                                                      # what x is prefilled with: finite, and no estimate's value


@pytest.fixture(scope='module')
def uvs():
    import os
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    uvs_amd.lib()
    uvs_amd._vision.lib()
    return uvs_amd


def c_logged_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, predict, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0, log=True):
    """uvs_camera_closed_loop_logged_f64 into poisoned buffers, x prefilled with SENTINEL (log=False: x_log = NULL); returns them on the host,
    tails included."""
    import torch
    buf = buffers(T, n_points)
    buf['x'] = torch.full((K * T * 2 * n_points * 6 + TAIL,), SENTINEL, dtype=torch.float64, device='cuda')
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    cams, n_cams, index = camera
    rc = uvs._vision.lib().uvs_camera_closed_loop_logged_f64(
        C.byref(fp), cams.data_ptr(), n_cams, ptr(index), ptr(motion), ptr(latency), ptr(assumed), ptr(predict), T, None if tp is None else C.byref(tp),
        ptr(occ), ptr(paint), 0 if occ is None else occ.shape[1], hold, q.data_ptr(), ptr(noise), x0.data_ptr(), f0.data_ptr(),
        *(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa')), buf['x'].data_ptr() if log else None,
        *(buf[key].data_ptr() for key in ('status', 'k_done', 'stats', 'pixels', 'held')), stream())
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def x_rows(buf, T, n_points):
    return buf['x'][:K * T * 2 * n_points * 6].reshape(K, T, 2 * n_points * 6)


def assert_x_written_exactly(buf, T, n_points, where):
    """Rows k < k_done hold an estimate, rows from k_done on and the tail keep the sentinel."""
    x, k_done = x_rows(buf, T, n_points), buf['k_done'][:T]
    due = np.arange(K)[:, None] < k_done[None, :]
    assert np.all(x[~due] == SENTINEL), (where, 'a row from k_done on was written')
    assert np.all(np.isfinite(x[due])) and not np.any(x[due] == SENTINEL), (where, 'a due row was not written')
    assert np.all(buf['x'][K * T * 2 * n_points * 6:] == SENTINEL), (where, 'the guard band')


# ------------------------------------------------------------------------------------------------------------- (a), (b): the C ABI
@pytest.mark.parametrize('T', sco.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_without_the_log_the_loop_is_its_predicted_namesake_and_with_it_too(uvs, method, n_points, T):
    """All 22 instantiations on mixed scenes, motions, latencies, assumed latencies and horizons behind painted rectangles with a hold:
    x_log = NULL is the predicted namesake in every output, poison past the last row included; with the log every other output keeps
    those bits, and x is written exactly where the dq rows are."""
    _, _, cams = scene_set(n_points)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, method, n_points), loop_operands(uvs, T, n_points)
    motion = motions(T, n_points)[2]
    d, a, p = (dev(v, np.int32) for v in pc.mixed(T))
    want = c_predicted_loop(uvs, fp, T, n_points, camera, motion, d, a, p, **op)
    assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
    silent = c_logged_loop(uvs, fp, T, n_points, camera, motion, d, a, p, log=False, **op)
    assert_same_buffers(silent, want, (method, n_points, T, 'x_log = NULL'))
    assert np.all(silent['x'] == SENTINEL)
    logged = c_logged_loop(uvs, fp, T, n_points, camera, motion, d, a, p, **op)
    assert_same_buffers(logged, want, (method, n_points, T, 'with the log'))
    assert_x_written_exactly(logged, T, n_points, (method, n_points, T))
    x = x_rows(logged, T, n_points)
    began = logged['k_done'][:T] > 0
    assert began.any() and np.array_equal(bits(x[0])[began], bits(op['x0'])[began]), 'step 0 has no regressor: X_0 is x0, bit for bit'
    bare = c_logged_loop(uvs, fp, T, n_points, camera, None, None, None, None, **op)   # every optional operand NULL
    assert_same_buffers(bare, c_predicted_loop(uvs, fp, T, n_points, camera, None, None, None, None, **op), (method, n_points, T, 'all NULL'))
    assert_x_written_exactly(bare, T, n_points, (method, n_points, T, 'all NULL'))


# ------------------------------------------------------------------------------------------------------------- (b): the stepwise loop
def assert_same_x(got, want, where, trials=None, want_trials=None):
    """Rows k < k_done of 'x', bit for bit; every other output through camera_common.assert_same_bits."""
    cc.assert_same_bits(got, want, K, where, trials, want_trials)
    a, b, k_done = bits(got['x']), bits(want['x']), got['k_done'].cpu().numpy()
    assert a.shape[0] == K and a.shape[2] == b.shape[2]
    trials = list(range(a.shape[1])) if trials is None else trials
    for t, tw in zip(trials, trials if want_trials is None else want_trials):
        assert np.array_equal(a[:k_done[t], t], b[:k_done[t], tw]), (where, 'x', t)


STEPWISE_ROUTES = ('uniform', 'occluded', 'held', 'painted', 'scenes', 'moving', 'delayed', 'aligned')


@pytest.mark.parametrize('route', STEPWISE_ROUTES)
@pytest.mark.parametrize('T', sco.SIZES)
def test_the_log_is_the_stepwise_loops_x_on_every_route(uvs, T, route):
    """engine.camera_closed_loop(want=ESTIMATOR_CAMERA_LOGS), one launch against stepwise, on each flavour's route as the call always was;
    and without 'x' the one launch returns the same bits through the entry point it always took."""
    plants = scene_set(4)[0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    kw = dict(route_kw(route, T, 4), guess='device')
    fp = params(uvs, 'GMCKF', 4)
    logs = uvs.engine.ESTIMATOR_CAMERA_LOGS
    fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, want=logs, **kw)
    stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, want=logs, **kw)
    assert tuple(fused['x'].shape) == (K, T, 48) == tuple(stepwise['x'].shape)
    assert_same_x(fused, stepwise, (route, T))
    plain = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
    assert 'x' not in plain
    cc.assert_same_bits(fused, plain, K, (route, T, "without 'x'"))
    assert ('held' in fused) == ('held' in plain) == ('held' in stepwise)


@pytest.mark.parametrize('T', sco.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_every_instantiation_logs_the_stepwise_x(uvs, method, n_points, T):
    """All 22 instantiations on mixed scenes, motions, latencies and assumed latencies behind the wide bar with a hold."""
    plants, _, cams = scene_set(n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    d, a, _ = pc.mixed(T)
    kw = dict(scenario_kw('held', T, n_points), cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0],
              target_motion=motions(T, n_points)[2], latency=d, assumed_latency=a, want=uvs.engine.ESTIMATOR_CAMERA_LOGS)
    fp = params(uvs, method, n_points)
    fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
    stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, **kw)
    assert_same_x(fused, stepwise, (method, n_points, T))
    assert int(fused['k_done'].max()) == K


@pytest.mark.parametrize('T', sco.SIZES)
def test_under_trial_params_and_predict_every_trial_has_its_uniform_launch(uvs, T):
    """The two one-launch-only operands: per-trial kernel_bw and gain in two cells, and three horizons; trial t of the mixed launch has the
    bits of the launch in which every trial has t's values, 'x' included."""
    import torch
    plants = scene_set(4)[0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    logs = uvs.engine.ESTIMATOR_CAMERA_LOGS
    cells, horizons = [(5.0, 0.1), (20.0, 0.3)], (0, 2, 8)
    cell, horizon = np.arange(T) % 2, np.array([horizons[(t // 2) % 3] for t in range(T)])
    tp = dict(kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    got = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), plants[0], q, noise, fused=True, guess='device', trial_params=tp, latency=2,
                                        predict=horizon, want=logs)
    seen = set()
    for i, (bw, gain) in enumerate(cells):
        for p in horizons:
            mine = [t for t in range(T) if cell[t] == i and horizon[t] == p]
            if not mine:
                continue
            want = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4, kernel_bw=bw, gain=gain), plants[0], q, noise, fused=True, guess='device',
                                                 latency=2, predict=p, want=logs)
            assert_same_x(got, want, (T, i, p), mine)
            seen.add(bits(want['x']).tobytes())
    assert len(seen) == (6 if T > 3 else 3), 'as many different launches as (cell, horizon) pairs'
    with pytest.raises(ValueError, match='predict needs fused=True'):
        uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), plants[0], q, noise, fused=False, predict=2, want=logs)
    assert torch.cuda.is_available()


def test_the_entry_point_is_the_logged_one_only_for_x(uvs, monkeypatch):
    """A spy on the library object: with 'x' in want the one launch is uvs_camera_closed_loop_logged_f64 whatever else is given, and
    without it every call takes the entry point it always took; the stepwise loop launches no loop kernel at all."""
    plants = scene_set(4)[0]
    T = 3
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    real, calls = uvs._vision.lib(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith('uvs_camera_closed_loop'):
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(uvs._vision, '_lib', Spy())
    fp = params(uvs, 'GMCKF', 4)
    always = {'uniform': 'uvs_camera_closed_loop_f64', 'grid': 'uvs_camera_closed_loop_grid_f64', 'occluded': 'uvs_camera_closed_loop_occluded_f64',
              'held': 'uvs_camera_closed_loop_held_f64', 'painted': 'uvs_camera_closed_loop_painted_f64', 'scenes': 'uvs_camera_closed_loop_scenes_f64',
              'moving': 'uvs_camera_closed_loop_moving_f64', 'delayed': 'uvs_camera_closed_loop_delayed_f64',
              'aligned': 'uvs_camera_closed_loop_aligned_f64'}
    for route, entry in always.items():
        kw = dict(route_kw(route, T, 4), guess='device', fused=True)
        for want, expected in ((uvs.engine.CAMERA_LOGS, entry), (('err', 'q'), entry), (uvs.engine.ESTIMATOR_CAMERA_LOGS, 'uvs_camera_closed_loop_logged_f64'),
                               (('x',), 'uvs_camera_closed_loop_logged_f64')):
            del calls[:]
            out = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, want=want, **kw)
            assert calls == [expected], (route, want, calls)
            assert ('x' in out) == ('x' in want) and all((key in out) == (key in want) for key in uvs.engine.CAMERA_LOGS)
    del calls[:]
    uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, guess='device', predict=1)
    assert calls == ['uvs_camera_closed_loop_predicted_f64']
    del calls[:]
    uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, want=uvs.engine.ESTIMATOR_CAMERA_LOGS)
    assert calls == []


# ------------------------------------------------------------------------------------------------------------- (c): the CPU restatement
@pytest.mark.parametrize('d,a,p', [(0, 0, 0), (2, 0, 2), (3, 3, 3)])
@pytest.mark.parametrize('method,n_points', sco.ORACLE)
def test_x_against_the_cpu_restatement(uvs, method, n_points, d, a, p):
    """One trial on the nominal camera from the host's initial guess, as the oracle makes it: every row of 'x' within 1e-10 relative of
    camera_score_common.logged_trial's.  Measured worst value over the twelve cases: 3.5e-16 (KF, (8,6), no latency)."""
    ref, cfg = sco.logged_trial(method, n_points, d, a, p), mc.oracle_settings(n_points)
    fp = params(uvs, method, n_points, kernel_bw=cfg['kernel_bw'], gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=sco.RADIUS, fused=True, latency=d, assumed_latency=a, predict=p, want=uvs.engine.ESTIMATOR_CAMERA_LOGS)
    assert ref['k_done'] == K == int(out['k_done'][0]) and int(out['status'][0]) == 0
    x = out['x'].cpu().numpy()[:, 0]
    worst = float(np.abs(x - ref['x']).max() / np.abs(ref['x']).max())
    print(f'{method} ({2 * n_points},6) d = {d}, a = {a}, p = {p}: x {worst:.2e}')
    assert worst <= sco.X_BOUND, (method, n_points, d, a, p, worst)


# ------------------------------------------------------------------------------------------------------------- (d): what is not written
@pytest.mark.parametrize('T', sco.SIZES)
def test_rows_from_k_done_on_void_trials_and_padding_are_not_written(uvs, T):
    """A wall that covers the whole frame from step 5 on FAILs its trials at k = 5 + their latency (no hold); a source index out of range voids a trial
    (k_done = 0: no row at all); T = 259 ends in a workgroup with padding wavefronts.  Every row of x from k_done on keeps its sentinel,
    every due row is written, and the neighbours keep the bits of the launch without the wall and the void."""
    _, _, cams = scene_set(4)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4, scenario='plain', hold=0)
    assert op['occ'] is None
    walled, void = [0, T - 1] if T > 3 else [0], [1, T // 2] if T > 3 else [1]
    wall = np.zeros((T, 1, 8), np.int32)
    wall[walled, 0] = (0, 0, 256, 256, 0, 0, 5, 2 ** 31 - 1)
    source = np.arange(T, dtype=np.int32)
    source[void] = [-1, T][:len(void)]
    src = dev(source, np.int32)
    tp = uvs._vision.CameraTrialParams(None, None, None, None, None, src.data_ptr(), T)
    d, a, p = (dev(v, np.int32) for v in pc.mixed(T))
    rest = {key: value for key, value in op.items() if key != 'occ'}
    clean = c_logged_loop(uvs, fp, T, 4, camera, None, d, a, p, **op)
    got = c_logged_loop(uvs, fp, T, 4, camera, None, d, a, p, tp=tp, occ=dev(wall, np.int32), **rest)
    k_done = got['k_done'][:T]
    behind = [min(5 + int(pc.mixed(T)[0][t]), K) for t in walled]   # the wall is seen a latency late
    assert k_done[walled].tolist() == behind and k_done[void].tolist() == [0] * len(void) and clean['k_done'][:T].min() == K
    assert got['status'][:T][void].tolist() == [1] * len(void) and got['status'][:T][walled].tolist() == [int(k < K) for k in behind]
    assert_x_written_exactly(got, T, 4, (T, 'walled and void'))
    assert_x_written_exactly(clean, T, 4, (T, 'clean'))
    x, x_clean = x_rows(got, T, 4), x_rows(clean, T, 4)
    others = [t for t in range(T) if t not in walled + void]
    assert np.array_equal(bits(x[:, others]), bits(x_clean[:, others])), 'the neighbours keep their bits'
    for t, rows in zip(walled, behind):
        assert np.array_equal(bits(x[:rows, t]), bits(x_clean[:rows, t])), 'and a walled trial the rows before it FAILs'
    for key in ('q', 'f', 'dq', 'err', 'kappa', 'stats', 'pixels', 'held', 'status', 'k_done'):
        assert np.array_equal(got[key][-TAIL:].view(np.int64 if got[key].dtype == np.float64 else np.int32),
                              clean[key][-TAIL:].view(np.int64 if got[key].dtype == np.float64 else np.int32)), (key, 'the guard band')


# ------------------------------------------------------------------------------------------------------------- (e): the Jacobian
def guarded(shape, fill=float('nan')):
    """A poisoned flat buffer with a guard band, and the view of `shape` at its start."""
    import torch
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), fill, dtype=torch.float64, device='cuda')
    return flat, flat[:n].view(*shape)


def tail_untouched(flat, fill=float('nan')):
    tail = flat[-TAIL:].cpu().numpy()
    return bool(np.all(np.isnan(tail)) if np.isnan(fill) else np.all(tail == fill))


def scene_batch(uvs, T, n_points):
    """Plants per trial (a scene index with repeats), the mixed motions (still, drift, a window that opens at step 4 and closes at 10, NaN
    velocities that never start) and the packed operands."""
    plants, _, cams = scene_set(n_points)
    index = sc.mixed_index(T, True)
    vel, win, packed = motions(T, n_points)
    return [plants[i] for i in index], cams, index, vel, win, packed


@pytest.mark.parametrize('n_points', [4, 3, 1])
@pytest.mark.parametrize('T', sco.SIZES)
def test_the_jacobian_is_the_rule(uvs, T, n_points):
    """engine.camera_jacobian against plant.projection_jacobian, record by record within 1e-10 |J|_F: the (T, 6) form at k = 0, 5 and 12
    and the (K, T, 6) form from k0 = 0 and k0 = 3 (rows before, inside and after the window of the trials whose target moves), over six
    scenes picked by an index with repeats; the guard band behind the output stays poisoned; without cameras the plant is the one scene."""
    mine, cams, index, vel, win, packed = scene_batch(uvs, T, n_points)
    rng = np.random.default_rng(T + n_points)
    q = cc.Q_GOAL + rng.uniform(-sco.SPREAD, sco.SPREAD, (K, T, 6))
    kw = dict(cameras=cams, camera_index=index, target_motion=packed)
    worst = 0.0
    for k0 in (0, 3):
        flat, out = guarded((K, T, 2 * n_points, 6))
        got = uvs.engine.camera_jacobian(mine[0], dev(q), k=k0, out=out, **kw)
        assert got is out and tail_untouched(flat)
        want = sco.numpy_jacobians(uvs, mine, q, vel, win, k0)
        err = np.linalg.norm((got.cpu().numpy() - want).reshape(K, T, -1), axis=2) / np.linalg.norm(want.reshape(K, T, -1), axis=2)
        worst = max(worst, float(err.max()))
        for k in (0, 5, 12):                                         # the (T, 6) form is row k - k0 of the (K, T, 6) form, bit for bit
            if k >= k0:
                one = uvs.engine.camera_jacobian(mine[0], dev(q[k - k0]), k=k, **kw)
                assert tuple(one.shape) == (T, 2 * n_points, 6) and np.array_equal(bits(one), bits(got[k - k0])), (k0, k)
    still = uvs.engine.camera_jacobian(mine[0], dev(q[12]), cameras=cams, camera_index=index)
    moved = uvs.engine.camera_jacobian(mine[0], dev(q[12]), k=12, **kw)
    differs = [not np.array_equal(bits(still[t]), bits(moved[t])) for t in range(T)]
    assert differs == [t % 4 in (1, 2) for t in range(T)], 'a moved target moves the Jacobian, and nothing else does'
    alone = uvs.engine.camera_jacobian(mine[0], dev(q[0]))          # the plant itself as the one scene
    want = sco.numpy_jacobians(uvs, [mine[0]] * T, q[0])
    worst = max(worst, float((np.linalg.norm((alone.cpu().numpy() - want).reshape(T, -1), axis=1) / np.linalg.norm(want.reshape(T, -1), axis=1)).max()))
    print(f'T = {T}, {n_points} points: the worst record {worst:.2e} of its norm')
    assert worst <= sco.J_BOUND


def test_a_jacobian_record_does_not_depend_on_the_launch(uvs):
    """The last trial of T = 259, alone (T = 1), as the last of T = 3 and as row 7 of a (K, T, 6) launch: the same bits.  A device-side
    index that names no scene gives a record of NaNs and its neighbours keep their bits."""
    mine, cams, index, vel, win, packed = scene_batch(uvs, 259, 4)
    q = cc.Q_GOAL + np.random.default_rng(9).uniform(-sco.SPREAD, sco.SPREAD, (259, 6))
    k = 7
    full = uvs.engine.camera_jacobian(mine[0], dev(q), k=k, cameras=cams, camera_index=index, target_motion=packed)
    assert win[258].tolist() == [4, 10] and np.abs(vel[258]).max() > 0, 'the last trial moves'
    for sel in ([258], [5, 77, 258]):
        part = uvs.engine.camera_jacobian(mine[0], dev(q[sel]), k=k, cameras=cams, camera_index=index[sel], target_motion=vel[sel], motion_window=win[sel])
        assert np.array_equal(bits(part), bits(full[dev(sel, np.int64)])), sel
    stack = np.tile(q, (K, 1, 1))
    rows = uvs.engine.camera_jacobian(mine[0], dev(stack), k=0, cameras=cams, camera_index=index, target_motion=packed)
    assert np.array_equal(bits(rows[k]), bits(full))
    holed = index.copy()
    holed[[3, 258]] = (-1, sc.N_SCENES)
    got = uvs.engine.camera_jacobian(mine[0], dev(q), k=k, cameras=cams, camera_index=dev(holed, np.int32), target_motion=packed).cpu().numpy()
    assert np.isnan(got[[3, 258]]).all()
    keep = [t for t in range(259) if t not in (3, 258)]
    assert np.array_equal(bits(got[keep]), bits(full)[keep])


# ------------------------------------------------------------------------------------------------------------- (f): the score
def score_inputs(uvs, T, n_points, seed=0):
    """q around the goal, X = the scaled rule bent by 5 to 40 % (so that rel_err >= 1e-3 by far: the cancellation case is (g)'s) and a dq."""
    mine, cams, index, vel, win, packed = scene_batch(uvs, T, n_points)
    rng = np.random.default_rng(seed)
    q = cc.Q_GOAL + rng.uniform(-sco.SPREAD, sco.SPREAD, (K, T, 6))
    Js = pl.DT * sco.numpy_jacobians(uvs, mine, q, vel, win)
    X = Js * rng.uniform(0.6, 1.4, Js.shape) + rng.standard_normal(Js.shape) * 0.05 * np.abs(Js).max()
    dq = rng.standard_normal((K, T, 6)) * 0.1
    return dict(mine=mine, kw=dict(cameras=cams, camera_index=index, target_motion=packed), q=q, Js=Js, X=X.reshape(K, T, -1), dq=dq)


def assert_sums_close(got, want, dq, where):
    """nx2, nj2 and xd_xd -- sums of squares, nothing cancels -- within 1e-10 of their own magnitude; dot within 1e-10 sqrt(nx2 nj2);
    diff2 within 1e-10 (nx2 + nj2); xd_jd, which can cancel, within 1e-10 of sqrt(nx2 nj2) |dq|^2, the size of its terms."""
    nx2, nj2 = want[..., 0], want[..., 1]
    cross = np.sqrt(nx2 * nj2)
    scale = (nx2, nj2, cross, nx2 + nj2, want[..., 4], cross * (dq * dq).sum(axis=-1))
    worst = {name: float((np.abs(got[..., i] - want[..., i]) / scale[i]).max()) for i, name in enumerate(('nx2', 'nj2', 'dot', 'diff2', 'xd_xd', 'xd_jd'))}
    print(where, ', '.join(f'{name} {d:.1e}' for name, d in worst.items()))
    assert max(worst.values()) <= sco.SUM_BOUND, (where, worst)


@pytest.mark.parametrize('n_points', [4, 3, 1])
@pytest.mark.parametrize('T', sco.SIZES)
def test_the_score_is_the_rule(uvs, T, n_points):
    """engine.camera_jacobian_score against plant.jacobian_score of the numpy J: nx2, nj2, dot, xd_xd and xd_jd within 1e-10 of
    sqrt(nx2 nj2) or their own magnitude, diff2 within 1e-10 (nx2 + nj2); the ratios follow plant.score_ratios; without dq the last two
    sums are 0.0 and step_ratio is NaN; the inputs have rel_err >= 1e-3."""
    P, s = uvs.plant, score_inputs(uvs, T, n_points, T + n_points)
    want = P.jacobian_score(s['X'], s['Js'], s['dq'])
    assert np.sqrt(want[..., 3] / want[..., 1]).min() >= 1e-3
    out = uvs.engine.camera_jacobian_score(dev(s['X']), dev(s['q']), s['mine'][0], pl.DT, dq=dev(s['dq']), **s['kw'])
    assert set(out) == set(uvs.engine.SCORE_KEYS) | {'sums'} and all(tuple(out[key].shape) == (K, T) for key in uvs.engine.SCORE_KEYS)
    got = out['sums'].cpu().numpy()
    assert_sums_close(got, want, s['dq'], f'T = {T}, {n_points} points:')
    ratios = P.score_ratios(got)
    for key in uvs.engine.SCORE_KEYS:
        assert np.allclose(out[key].cpu().numpy(), ratios[key], rtol=1e-12, atol=0, equal_nan=True), key
    bare = uvs.engine.camera_jacobian_score(dev(s['X']), dev(s['q']), s['mine'][0], pl.DT, **s['kw'])
    sums = bare['sums'].cpu().numpy()
    assert np.array_equal(bits(sums[..., :4]), bits(got[..., :4])) and np.all(bits(sums[..., 4:]) == 0), 'dq_log = NULL: +0.0 in the last two'
    assert bool(bare['step_ratio'].isnan().all())


@pytest.mark.parametrize('T', sco.SIZES)
def test_masked_records_are_nan_and_not_read_and_a_record_does_not_depend_on_the_launch(uvs, T):
    """With k_done, the records k >= k_done[t] are six NaNs whether the rows of x, q and dq there hold NaN or huge finite values, and the
    others keep their bits; a record has the same bits alone (K = T = 1), in a (K, 1) launch of its trial and in the full launch; the
    guard band behind the score is not written (the engine allocates it: checked through the C ABI)."""
    import torch
    s = score_inputs(uvs, T, 4, 3)
    k_done = np.array([(5 * t + 3) % (K + 1) for t in range(T)], np.int32)
    k_done[-1] = 9
    full = uvs.engine.camera_jacobian_score(dev(s['X']), dev(s['q']), s['mine'][0], pl.DT, dq=dev(s['dq']), **s['kw'])['sums'].cpu().numpy()
    masked = np.arange(K)[:, None] >= k_done[None, :]
    for junk in (np.nan, 1e300):
        x, q, dq = (np.where(masked[:, :, None], junk, s[key]) for key in ('X', 'q', 'dq'))
        got = uvs.engine.camera_jacobian_score(dev(x), dev(q), s['mine'][0], pl.DT, dq=dev(dq), k_done=dev(k_done, np.int32), **s['kw'])
        sums = got['sums'].cpu().numpy()
        assert np.isnan(sums[masked]).all() and np.array_equal(bits(sums[~masked]), bits(full[~masked])), junk
        assert bool(got['scale'].isnan()[dev(masked, np.bool_)].all())
    mine, cams, index, vel, win, packed = scene_batch(uvs, T, 4)
    t, k = T - 1, 11
    kw = dict(cameras=cams, camera_index=index[[t]], target_motion=vel[[t]], motion_window=win[[t]])
    column = uvs.engine.camera_jacobian_score(dev(s['X'][:, [t]]), dev(s['q'][:, [t]]), mine[0], pl.DT, dq=dev(s['dq'][:, [t]]), **kw)['sums']
    assert np.array_equal(bits(column[:, 0]), bits(full[:, t]))
    # through the C ABI: a guard band behind the score, and a single record at step k (K = 1 would score step 0: the motion says which step)
    flat, score = guarded((K, T, 6))
    X, Q, DQ = dev(s['X']), dev(s['q']), dev(s['dq'])
    rc = uvs._vision.lib().uvs_camera_jacobian_score_f64(cams.data_ptr(), 6, dev(index, np.int32).data_ptr(), packed.data_ptr(), 4, T, K, pl.DT,
                                                         X.data_ptr(), Q.data_ptr(), DQ.data_ptr(), None, score.data_ptr(), stream())
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    assert np.array_equal(bits(score), bits(full)) and tail_untouched(flat)
    still = [u for u in range(T) if u % 4 == 0][-1]                  # a trial whose target stands still: its record at k is its record at step 0
    one = uvs.engine.camera_jacobian_score(dev(s['X'][[k]][:, [still]]), dev(s['q'][[k]][:, [still]]), mine[0], pl.DT, dq=dev(s['dq'][[k]][:, [still]]),
                                           cameras=cams, camera_index=index[[still]])['sums']
    assert np.array_equal(bits(one[0, 0]), bits(full[k, still])), 'alone, K = T = 1'


# ------------------------------------------------------------------------------------------------------------- (g): together
@pytest.mark.parametrize('T', sco.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_the_three_pieces_together(uvs, method, n_points, T):
    """x0 = fp.dt * camera_jacobian(q_start): step 0's regressor is zero, so X_0 = x0 and q_0 = q_start, and the score kernel forms dt J by
    the same single multiply on the same J bits -- row 0 scores diff2 == 0.0 exactly, scale and cosine 1.  From the reference's guess row 0's
    scale lies within the band of the per-trial least-squares scales of plant.analytic_guess against dt * plant.projection_jacobian, which
    this test computes on the CPU for its own starts (about 1 / t_s times 0.68 .. 1.49)."""
    plant = scene_set(n_points)[0][0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    fp = params(uvs, method, n_points)
    logs = uvs.engine.ESTIMATOR_CAMERA_LOGS
    x0 = fp.dt * uvs.engine.camera_jacobian(plant, q)
    out = uvs.engine.camera_closed_loop(fp, plant, q, noise, x0=x0.reshape(T, -1), fused=True, want=logs)
    assert np.array_equal(bits(out['x'][0]), bits(x0.reshape(T, -1))) and np.array_equal(bits(out['q'][0]), bits(q))
    score = uvs.engine.camera_jacobian_score(plant=plant, dt=fp.dt, **{k: out[k] for k in ('x', 'q', 'dq', 'k_done')})
    sums = score['sums'].cpu().numpy()
    assert np.all(sums[0, :, 3] == 0.0) and np.array_equal(bits(sums[0, :, 0]), bits(sums[0, :, 1])) and np.array_equal(bits(sums[0, :, 0]), bits(sums[0, :, 2]))
    assert bool((score['scale'][0] == 1.0).all()) and bool((score['rel_err'][0] == 0.0).all())
    due = (np.arange(K)[:, None] < out['k_done'].cpu().numpy()[None, :])
    assert np.isfinite(sums[due]).all() and np.isnan(sums[~due]).all()
    # from the reference's guess
    guess = uvs.engine.camera_closed_loop(fp, plant, q, noise, guess='device', fused=True, want=logs)
    scored = uvs.engine.camera_jacobian_score(plant=plant, dt=fp.dt, **{k: guess[k] for k in ('x', 'q', 'dq', 'k_done')})
    P, starts = uvs.plant, sc.starts(T)
    band = []
    for t in range(T):
        robot = P.SyntheticRobot(plant, fp.dt)
        robot.start(starts[t])
        G = P.analytic_guess(robot, plant.features(starts[t]), (P.RESOLUTION, P.RESOLUTION), 2 * n_points, 6).reshape(-1, 6)
        Js = fp.dt * P.projection_jacobian(plant, starts[t])
        band.append((G * Js).sum() / (Js * Js).sum())
    band = np.array(band)
    got = scored['scale'][0].cpu().numpy()
    print(f'{method} ({2 * n_points},6) T = {T}: the guess is {band.min():.1f} .. {band.max():.1f} times dt J on the CPU; the device scores '
          f'{got.min():.1f} .. {got.max():.1f}')
    assert 0.5 / fp.dt < band.min() and band.max() < 2.0 / fp.dt, 'about 1 / t_s times 0.68 .. 1.49'
    # the guess on the device is formed from the DETECTED features (pixel quantisation): each trial within 1 % of its own CPU scale
    assert np.all(np.abs(got - band) <= 0.01 * np.abs(band)), float(np.abs(got / band - 1).max())
    assert band.min() * 0.99 <= got.min() and got.max() <= band.max() * 1.01
