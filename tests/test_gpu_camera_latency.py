"""CAMERA LATENCY on the GPU (include/uvs_vision.h, "CAMERA LATENCY"; engine.camera_closed_loop(latency=)): the estimators' one-launch loop
(delayed_frames_kernel, 22 instantiations), the baseline's (delayed_baseline_kernel) and the stepwise companion (delay_line_kernel) over
the latencies of tests/camera_latency_common.py, the motions of tests/camera_moving_common.py and the scene set of
tests/camera_scenes_common.py.

Every comparison but the oracle's is of bits, and none leaves a trial out: (a) without a latency -- None through the entry point the call
always used, NULL and all zeros through the delayed kernels -- a loop is the call without latency on every route, poison past the last row
included; (c) the one launch is the stepwise loop; (b) trial t of a mixed batch is trial t of the launch in which every trial has t's
latency; (d, e) a void trial writes status FAIL and k_done = 0 and nothing else while its delayed neighbours keep their bits, and the
padding wavefront stores nothing.  The oracle (oracle/pixel_loop.py through its sensor= hook, a closure that hands back the detection of
step max(k - d, 0)) is held to pixel_loop_common's gates: 1e-8 for err, q, f and stats, 1e-7 for the command, the integers exact.
Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, the last with a padding wavefront that shadows a trial of
latency 8); K = 16; latencies mixed per trial over {0, 1, 2, 3, 8}; and K = 4 at latency 8, where every reported detection is the step-0
frame's."""
import ctypes as C

import numpy as np
import pytest

import camera_common as cc
import camera_latency_common as lc
import camera_moving_common as mc
import camera_scenes_common as sc
import pixel_loop_common as pl
from test_gpu_camera_moving import (BUILT, INT32_MIN, POISON, against_the_oracle, assert_same_buffers, buffers, dev, loop_operands, motions, params,
                                    raw, scenario_kw, scene_set, stream, trial_view)

pytestmark = pytest.mark.gpu

K = lc.K
bits = cc.bits


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


MOVING_CALL = 'the moving namesake'


def c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0):
    """uvs_camera_closed_loop_delayed_f64 (latency: an int32 device tensor or None = NULL) or, for latency = MOVING_CALL, its moving
    namesake, on the same operands into poisoned buffers; returns them on the host, tails included."""
    import torch
    buf = buffers(T, n_points)
    lib = uvs._vision.lib()
    middle = (T, None if tp is None else C.byref(tp), None if occ is None else occ.data_ptr(), None if paint is None else paint.data_ptr(),
              0 if occ is None else occ.shape[1], hold, q.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr())
    outs = tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels', 'held')) + (stream(),)
    cams, n_cams, index = camera
    front = (C.byref(fp), cams.data_ptr(), n_cams, None if index is None else index.data_ptr(), None if motion is None else motion.data_ptr())
    if isinstance(latency, str):
        rc = lib.uvs_camera_closed_loop_moving_f64(*front, *middle, *outs)
    else:
        rc = lib.uvs_camera_closed_loop_delayed_f64(*front, None if latency is None else latency.data_ptr(), *middle, *outs)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def c_baseline_loop(uvs, fp, T, n_points, camera, motion, latency, believed, q, noise):
    import torch
    buf = buffers(T, n_points, True)
    lib = uvs._vision.lib()
    b_models, b_n, b_index = believed
    rest = (T, b_models.data_ptr(), b_n, None if b_index is None else b_index.data_ptr(), q.data_ptr(), None if noise is None else noise.data_ptr()) + \
        tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')) + (stream(),)
    cams, n_cams, index = camera
    front = (C.byref(fp), cams.data_ptr(), n_cams, None if index is None else index.data_ptr(), None if motion is None else motion.data_ptr())
    if isinstance(latency, str):
        rc = lib.uvs_camera_believed_loop_moving_f64(*front, *rest)
    else:
        rc = lib.uvs_camera_believed_loop_delayed_f64(*front, None if latency is None else latency.data_ptr(), *rest)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


# ------------------------------------------------------------------------------------------------------------- (a): no latency
@pytest.mark.parametrize('T', lc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_without_a_latency_the_loops_are_their_moving_namesakes(uvs, method, n_points, T):
    """latency = NULL and all zeros through the C ABI on the same operands (mixed scenes, mixed motions, rectangles, paints and a hold among
    them): every log row, stats, status, k_done, pixels, held and the poison past the last row; with and without a motion."""
    _, _, cams = scene_set(n_points)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, method, n_points), loop_operands(uvs, T, n_points)
    fa, believed = params(uvs, 'ANALYTICAL', n_points), (cams[:1], 1, None)
    zeros = dev(np.zeros(T), np.int32)
    for motion in (motions(T, n_points)[2], None):
        want = c_estimator_loop(uvs, fp, T, n_points, camera, motion, MOVING_CALL, **op)
        assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
        want_b = c_baseline_loop(uvs, fa, T, n_points, camera, motion, MOVING_CALL, believed, op['q'], op['noise'])
        for latency in (None, zeros):
            where = (method, T, motion is None, latency is None)
            assert_same_buffers(c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, **op), want, where)
            assert_same_buffers(c_baseline_loop(uvs, fa, T, n_points, camera, motion, latency, believed, op['q'], op['noise']), want_b, where)


ROUTES = ('uniform', 'grid', 'occluded', 'held', 'painted', 'scenes', 'moving')


def route_kw(route, T, n_points):
    """The keyword arguments that send camera_closed_loop(fused=True) down each flavour's route, as the call always was."""
    import torch
    kw = {}
    if route == 'grid':
        kw['trial_params'] = dict(kernel_bw=torch.full((T,), 12.0, dtype=torch.float64, device='cuda'))
    if route in ('occluded', 'held', 'painted'):
        kw.update(scenario_kw(route, T, n_points))
    if route == 'scenes':
        kw.update(cameras=scene_set(n_points)[2], camera_index=sc.mixed_index(T, True), believed=scene_set(n_points)[0][0])
    if route == 'moving':
        kw.update(target_motion=motions(T, n_points)[2])
    return kw


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('T', lc.SIZES)
def test_none_and_zeros_are_the_call_without_the_argument_on_every_route(uvs, T, route):
    """engine.camera_closed_loop on each flavour's route: latency=None is that call, and latency 0 -- an int, and T zeros -- gives its bits
    through the delayed kernels, one launch and stepwise; for ANALYTICAL on the routes its one-launch loop has."""
    import torch
    plants = scene_set(4)[0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    kw = dict(route_kw(route, T, 4), guess='device')
    fp = params(uvs, 'GMCKF', 4)
    plain = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
    for latency in (None, 0, np.zeros(T, np.int64)):
        got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, latency=latency, **kw)
        cc.assert_same_bits(got, plain, K, (route, T, 'one launch', latency is None))
        assert ('held' in got) == ('held' in plain) and (route != 'held' or torch.equal(got['held'], plain['held']))
    if route != 'grid':                                              # the stepwise loop has no per-trial flavour
        cc.assert_same_bits(uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, latency=0, **kw), plain, K, (route, T, 'stepwise'))
    if route in ('uniform', 'scenes', 'moving'):
        fa = params(uvs, 'ANALYTICAL', 4)
        kw.pop('guess')
        plain = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=True, **kw)
        for fused, latency in ((True, None), (True, 0), (True, np.zeros(T, np.int64)), (False, 0)):
            got = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=fused, latency=latency, **kw)
            cc.assert_same_bits(got, plain, K, (route, T, 'baseline', fused, latency is None))


# ------------------------------------------------------------------------------------------------------------- (c): one launch, stepwise
@pytest.mark.parametrize('T', lc.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_the_one_launch_is_the_stepwise_loop(uvs, method, n_points, T):
    """The mixed latencies on the mixed motions and a mixed camera_index, under the four rectangle scenarios (occluders, paints, the wide
    bar with a hold): every log, status, k_done, stats, pixels and held.  The delayed trials differ from the launch without latency, and
    the trials of latency 0 do not."""
    import torch
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    vel, win, packed = motions(T, n_points)
    latency = lc.mixed(T)
    plain = None
    for scenario in sc.SCENARIOS:
        kw = dict(scenario_kw(scenario, T, n_points), cameras=cams, camera_index=index, guess='device', believed=plants[0], target_motion=packed)
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, latency=latency, **kw)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, latency=torch.from_numpy(latency), **kw)
        cc.assert_same_bits(fused, stepwise, K, (method, n_points, T, scenario))
        assert ('held' in fused) == (scenario == 'held') == ('held' in stepwise)
        if scenario == 'held':
            assert torch.equal(fused['held'], stepwise['held'])
        if scenario == 'plain':
            plain = fused
            prompt = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            rows = np.minimum(fused['k_done'].cpu().numpy() + 1, K)  # the rows of f that are specified
            same = [np.array_equal(bits(fused['f'])[:rows[t], t], bits(prompt['f'])[:rows[t], t]) for t in range(T)]
            assert same == [d == 0 for d in latency], 'the delayed trials differ from the launch without latency and the others do not'
    assert int(plain['k_done'].max()) == K


@pytest.mark.parametrize('method,n_points', BUILT)
def test_source_next_to_a_latency_is_gathered_by_output_trial(uvs, method, n_points):
    """trial_params with a 'source' permutation and per-trial kernel_bw and gain: two cells x the mixed latencies over three input trials,
    one launch, against the stepwise loop of each cell on the gathered inputs with the latencies, motions, rectangles and paints of its
    OUTPUT trials."""
    import torch
    plants = scene_set(n_points)[0]
    T = 12
    cells = [(5.0, 0.1), (20.0, 0.3)]
    cell, source = np.arange(T) % 2, np.random.default_rng(4).permutation(np.arange(T) % 3).astype(np.int32)
    vel, win, _ = motions(T, n_points)
    latency = lc.mixed(T)
    q, noise = dev(sc.starts(3)), dev(sc.noise(3, n_points))
    tp = dict(source=source, kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    for scenario in ('plain', 'held'):
        kw = scenario_kw(scenario, T, n_points)
        got = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device', trial_params=tp,
                                            target_motion=vel, motion_window=win, latency=latency, **kw)
        for i, (bw, gain) in enumerate(cells):
            sel = np.flatnonzero(cell == i)
            src = dev(source[sel], np.int64)
            mine = {key: (value[sel] if key in ('occluders', 'occluder_colours') else value) for key, value in kw.items()}
            want = uvs.engine.camera_closed_loop(params(uvs, method, n_points, kernel_bw=bw, gain=gain), plants[0], q[src].contiguous(),
                                                 noise[:, src].contiguous(), fused=False, guess='device', target_motion=vel[sel],
                                                 motion_window=win[sel], latency=latency[sel], **mine)
            cc.assert_same_bits(got, want, K, (method, n_points, scenario, i), sel.tolist(), list(range(len(sel))))
            if scenario == 'held':
                assert torch.equal(got['held'][dev(sel, np.int64)], want['held'])


@pytest.mark.parametrize('T', lc.SIZES)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_baseline_one_launch_is_its_stepwise_loop(uvs, n_points, T):
    """ANALYTICAL on the mixed latencies: the law on the nominal model and on the trials' own scenes, with and without a motion; the trials
    of latency 0 keep the bits of the launch without latency, and the others do not."""
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    packed = motions(T, n_points)[2]
    latency = lc.mixed(T)
    for believed in (dict(believed=plants[0]), dict()):
        for motion in (dict(target_motion=packed), dict()):
            kw = dict(cameras=cams, camera_index=index, **believed, **motion)
            fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, latency=latency, **kw)
            stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, latency=latency, **kw)
            cc.assert_same_bits(fused, stepwise, K, (n_points, T, tuple(believed), tuple(motion)))
            prompt = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            cc.assert_same_bits(fused, prompt, K, (n_points, T, 'the trials of latency 0'), [t for t in range(T) if latency[t] == 0])
            assert not np.array_equal(bits(fused['dq'])[:, 0], bits(prompt['dq'])[:, 0]), 'the latency shows in the command'
    alone = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, latency=latency)   # the nominal camera as the one scene
    step = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, latency=latency)
    cc.assert_same_bits(alone, step, K, (n_points, T, 'nominal'))


@pytest.mark.parametrize('fused', [True, False])
def test_behind_the_wide_bar_the_loss_and_the_hold_arrive_late(uvs, fused):
    """An occlusion wider than a disc with a hold, one start, the latencies 0, 1, 2, 3, 8 as five trials: the masks empty d steps later, so
    the first row in which a pair is held -- equal to the row before it -- comes d steps later too, and `held` is equal on both routes."""
    import torch
    plant = pl.plant_of(4)
    rows = np.array(pl.wide_rows(4), np.int64)
    hold = pl.HOLDS[4]['longer']
    T = len(lc.MIX)
    q = dev(np.tile(mc.oracle_start(), (T, 1)))
    latency = np.array(lc.MIX)
    kw = dict(radius=lc.RADIUS, occluders=rows, hold=hold, latency=latency, guess='device', want=('f', 'q', 'dq', 'err', 'kappa'))
    out = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), plant, q, None, fused=fused, **kw)
    other = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), plant, q, None, fused=not fused, **kw)
    cc.assert_same_bits(out, other, K, ('wide bar', fused))
    assert torch.equal(out['held'], other['held']) and int(out['held'].sum()) > 0
    f = bits(out['f'])
    for t in range(T):                                               # without noise the first d + 1 rows are the step-0 detection, bit for bit
        d = int(latency[t])
        assert np.array_equal(f[:d + 1, t], np.tile(f[0, t], (d + 1, 1))), (t, 'the delay line is primed with the step-0 frame')
        assert not np.array_equal(f[d + 1, t], f[d, t]), (t, 'and then moves on')
    assert np.array_equal(f[0], np.tile(f[0, 0], (T, 1))), 'one start, one step-0 frame'


# ------------------------------------------------------------------------------------------------------------- (b): mixed against uniform
@pytest.mark.parametrize('T', lc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_a_mixed_batch_is_every_trial_at_its_own_latency(uvs, method, n_points, T):
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    kw = dict(cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0], fused=True,
              target_motion=motions(T, n_points)[2], **scenario_kw('occluded', T, n_points))
    latency = lc.mixed(T)
    got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=latency, **kw)
    first = {}
    for d in lc.MIX:
        uniform = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=d, **kw)
        cc.assert_same_bits(got, uniform, K, (method, n_points, T, d), [t for t in range(T) if latency[t] == d])
        first[d] = bits(uniform['f'])
    assert len({a.tobytes() for a in first.values()}) == len(lc.MIX), 'five latencies, five different launches'
    fa = params(uvs, 'ANALYTICAL', n_points)
    kw = dict(cameras=cams, camera_index=sc.mixed_index(T, True), fused=True, target_motion=motions(T, n_points)[2])
    got = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, latency=latency, **kw)
    for d in lc.MIX:
        cc.assert_same_bits(got, uniform_baseline(uvs, fa, plants[0], q, noise, d, kw), K, (n_points, T, d, 'baseline'),
                            [t for t in range(T) if latency[t] == d])


def uniform_baseline(uvs, fa, plant, q, noise, d, kw):
    return uvs.engine.camera_closed_loop(fa, plant, q, noise, latency=d, **kw)


# ------------------------------------------------------------------------------------------------------------- K = 4 at latency 8
@pytest.mark.parametrize('T', lc.SIZES)
def test_four_steps_at_latency_eight_report_the_step_0_frame(uvs, T):
    """K = 4 with d = 8: the delay line never gets past its priming, so every reported row is the step-0 detection plus that step's noise,
    one rounded add, and `pixels` the step-0 masks; both routes, estimator and baseline."""
    import torch
    plants, _, cams = scene_set(4)
    index = sc.mixed_index(T, True)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, 4, steps=4))
    pix0 = torch.full((T, 4), POISON, dtype=torch.int32, device='cuda')
    f0 = uvs.engine.camera_features(plants[0], q, pixels=pix0, cameras=cams, camera_index=index)
    want = f0[None] + noise
    for fp, kw in ((params(uvs, 'GMCKF', 4, steps=4), dict(guess='device', believed=plants[0])), (params(uvs, 'ANALYTICAL', 4, steps=4), {})):
        for fused in (True, False):
            out = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=fused, cameras=cams, camera_index=index, latency=8, **kw)
            rows = np.minimum(out['k_done'].cpu().numpy() + 1, 4)     # the rows of f that are specified
            assert int(rows.max()) == 4
            for t in range(T):
                assert np.array_equal(bits(out['f'])[:rows[t], t], bits(want)[:rows[t], t]), (fp.method, fused, t)
            assert torch.equal(out['pixels'], pix0), (fp.method, fused)


# ------------------------------------------------------------------------------------------------------------- (d), (e): void and padding
VOID = (-1, sc.N_SCENES, INT32_MIN)


@pytest.mark.parametrize('T', lc.SIZES)
def test_a_void_trial_fails_alone_next_to_delayed_neighbours(uvs, T):
    """A void scene index (both loops) and a void source (the estimators' loop): status FAIL, k_done = 0, nothing else stored, and the rest
    of the launch keeps the bits of the valid launch.  At T = 259 the last trial has latency 8, and the padding wavefront that shadows it
    stores nothing: the poison past every last row is compared too.  A latency outside 0 .. 8 is clamped on the device."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    motion = motions(T, 4)[2]
    mixed = lc.mixed(T)
    latency = dev(mixed, np.int32)
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2] if T > 3 else [1]
    source = np.arange(T, dtype=np.int32)
    tp_of = lambda s: uvs._vision.CameraTrialParams(None, None, None, None, None, s.data_ptr(), T)          # noqa: E731
    valid = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, **op)
    src = dev(source, np.int32)                                      # kept: the block holds its address alone
    valid_s = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, tp=tp_of(src), **op)
    assert_same_buffers(valid_s, valid, 'the identity as source')
    valid_b = c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, believed, op['q'], op['noise'])
    assert valid['k_done'][:T].max() == K and mixed[T - 1] == (8 if T > 3 else 3), 'the last trial, which the padding wavefront shadows, is delayed'
    wild = np.where(mixed == 0, -5, np.where(mixed == 8, 2 ** 31 - 1, mixed))          # clamped to 0 and to 8 on the device
    assert_same_buffers(c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, dev(wild, np.int32), **op), valid, 'clamped')
    assert_same_buffers(c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, dev(wild, np.int32), believed, op['q'], op['noise']),
                        valid_b, 'clamped, baseline')
    for turn in range(len(VOID)):
        holed, holed_source = index.copy(), source.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
            holed_source[t] = (-1, T, INT32_MIN)[(i + turn) % 3]
        hs = dev(holed_source, np.int32)
        for want, got in ((valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(holed, np.int32)), motion, latency, **op)),
                          (valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, tp=tp_of(hs), **op)),
                          (valid_b, c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(holed, np.int32)), motion, latency, believed, op['q'], op['noise']))):
            want = {key: value.copy() for key, value in want.items()}
            for key in want:
                view = trial_view(want, key, T, 4)
                view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
            assert_same_buffers(got, want, (T, turn))


def test_the_stepwise_companion_gathers_and_adds(uvs):
    """uvs_delay_features_f64 alone, on random logs with NaN pairs among them: row max(k - d_t, 0) per trial plus one add, the counts of that
    row, nothing past the rows; NULL noise adds nothing, NULL latency delays nothing."""
    import torch
    lib = uvs._vision.lib()
    rng = np.random.default_rng(7)
    for T, n_points in ((259, 4), (5, 3), (3, 1)):
        m = 2 * n_points
        sensed, counts, noise = rng.standard_normal((K, T, m)) * 100, rng.integers(0, 500, (K, T, n_points)), rng.standard_normal((K, T, m))
        sensed[counts.repeat(2, axis=2) == 0] = np.nan
        latency = np.array([lc.MIX[t % 5] for t in range(T)])
        latency[0], latency[-1] = -3, 100                            # clamped to 0 and to 8
        d_sensed, d_counts, d_noise, d_latency = dev(sensed), dev(counts, np.int32), dev(noise), dev(latency, np.int32)
        for k in (0, 1, 5, 8, 15):
            kk = np.maximum(k - np.clip(latency, 0, 8), 0)
            for with_noise in (True, False):
                for with_latency in (True, False):
                    f = torch.full((T * m + 8,), 7.0, dtype=torch.float64, device='cuda')
                    pixels = torch.full((T * n_points + 8,), POISON, dtype=torch.int32, device='cuda')
                    uvs._vision.check(lib.uvs_delay_features_f64(T, n_points, k, d_latency.data_ptr() if with_latency else None, d_sensed.data_ptr(),
                                                                 d_counts.data_ptr(), d_noise[k].data_ptr() if with_noise else None, f.data_ptr(),
                                                                 pixels.data_ptr(), stream()))
                    rows = kk if with_latency else np.full(T, k)
                    want = sensed[rows, np.arange(T)]
                    if with_noise:
                        want = want + noise[k]
                    got = f.cpu().numpy()
                    assert np.array_equal(np.isnan(got[:T * m]), np.isnan(want.ravel()))
                    ok = ~np.isnan(want.ravel())
                    assert np.array_equal(raw(got[:T * m][ok]), raw(np.ascontiguousarray(want.ravel()[ok]))), (T, k, with_noise, with_latency)
                    assert np.all(got[T * m:] == 7.0)
                    got_pixels = pixels.cpu().numpy()
                    assert np.array_equal(got_pixels[:T * n_points], counts[rows, np.arange(T)].ravel()) and np.all(got_pixels[T * n_points:] == POISON)


# ------------------------------------------------------------------------------------------------------------- the CPU oracle
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('d', lc.ORACLE_LATENCIES)
@pytest.mark.parametrize('method,n_points', lc.ORACLE)
def test_against_the_oracle(uvs, method, n_points, d, fused):
    """One trial on the nominal camera, the host's initial guess as the oracle makes it, against oracle.pixel_loop.run through its sensor=
    hook on the delayed detections."""
    ref, cfg = lc.oracle_trial(method, n_points, d), mc.oracle_settings(n_points)
    fp = params(uvs, method, n_points, kernel_bw=cfg['kernel_bw'], gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=lc.RADIUS, fused=fused, latency=d)
    assert ref['k_done'] == K
    against_the_oracle(out, ref, f'{method} ({2 * n_points},6) d = {d} {"one launch" if fused else "stepwise"}')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('motion', [None, 'window'])
def test_against_the_oracle_behind_the_wide_bar_with_a_hold(uvs, motion, fused):
    """Latency 2 behind the bar that is wider than a disc, with a hold, still and on the 'window' motion: status, k_done, pixels and held
    exact, the logs within the gates."""
    rows = tuple(tuple(int(v) for v in row) for row in pl.wide_rows(4))
    hold = pl.HOLDS[4]['longer']
    ref = lc.oracle_trial('GMCKF', 4, 2, False, None, rows, hold, motion)
    kw = {}
    if motion is not None:
        vel, window = mc.motion(motion, 4)
        kw = dict(target_motion=vel, motion_window=window)
    out = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), pl.plant_of(4), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(4)[:, None]),
                                        radius=lc.RADIUS, fused=fused, latency=2, occluders=np.array(rows), hold=hold, **kw)
    against_the_oracle(out, ref, f'GMCKF (8,6) d = 2 behind the wide bar, {motion} {"one launch" if fused else "stepwise"}', hold=True)
