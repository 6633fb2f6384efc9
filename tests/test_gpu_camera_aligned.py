"""ASSUMED LATENCY on the GPU (include/uvs_vision.h, "ASSUMED LATENCY"; engine.camera_closed_loop(assumed_latency=)): the estimators'
one-launch loop whose regressor is the command of step k - 1 - a (aligned_frames_kernel, 22 instantiations), the baseline's whose law is
handed the joints of step max(k - a, 0) (aligned_baseline_kernel) and the stepwise loops' per-trial gather, over the (latency, assumed)
pairs of tests/camera_aligned_common.py, the motions of tests/camera_moving_common.py and the scene set of tests/camera_scenes_common.py.

Every comparison but the CPU restatements' is of bits, and none leaves a trial out: (a) without an assumed latency -- None through the entry
point the call always used, NULL and all zeros through the aligned kernels -- a loop is the call without it on every route, poison past
the last row included; (c) the one launch is the stepwise loop; (b) trial t of a mixed batch is trial t of the launch in which every
trial has t's pair; (d, e) a void trial writes status FAIL and k_done = 0 and nothing else while its neighbours keep their bits, and the
padding wavefront and the shadow lanes store nothing; (f) values outside 0 .. 8 are clamped on the device.  The CPU restatements
(camera_aligned_common.estimator_trial, held bit for bit to the untouched oracle at a = 0 and a = 1 by the host file, and law_trial) are
held to pixel_loop_common's gates and to 1e-8.  Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, the last with a
padding wavefront that shadows a trial whose pair no other trial has); K = 16; and K = 4, where an assumed latency of 3 or more never
finds a command and never leaves the step-0 joints."""
import ctypes as C

import numpy as np
import pytest

import camera_aligned_common as ac
import camera_common as cc
import camera_moving_common as mc
import camera_scenes_common as sc
import pixel_loop_common as pl
from test_gpu_camera_moving import (BUILT, INT32_MIN, POISON, against_the_oracle, assert_same_buffers, buffers, dev, loop_operands, motions, params,
                                    scenario_kw, scene_set, stream, trial_view)

pytestmark = pytest.mark.gpu

K = ac.K
bits = cc.bits
DELAYED_CALL = 'the delayed namesake'
MOVING_CALL = 'the moving namesake'


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


def c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0):
    """uvs_camera_closed_loop_aligned_f64 (latency, assumed: int32 device tensors or None = NULL) or, for assumed = DELAYED_CALL, its
    delayed namesake, for MOVING_CALL the moving one (latency is then not passed), on the same operands into poisoned buffers; returns
    them on the host, tails included."""
    import torch
    buf = buffers(T, n_points)
    lib = uvs._vision.lib()
    middle = (T, None if tp is None else C.byref(tp), None if occ is None else occ.data_ptr(), None if paint is None else paint.data_ptr(),
              0 if occ is None else occ.shape[1], hold, q.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr())
    outs = tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels', 'held')) + (stream(),)
    cams, n_cams, index = camera
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    front = (C.byref(fp), cams.data_ptr(), n_cams, ptr(index), ptr(motion))
    if assumed == MOVING_CALL:
        rc = lib.uvs_camera_closed_loop_moving_f64(*front, *middle, *outs)
    elif assumed == DELAYED_CALL:
        rc = lib.uvs_camera_closed_loop_delayed_f64(*front, ptr(latency), *middle, *outs)
    else:
        rc = lib.uvs_camera_closed_loop_aligned_f64(*front, ptr(latency), ptr(assumed), *middle, *outs)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def c_baseline_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, believed, q, noise):
    import torch
    buf = buffers(T, n_points, True)
    lib = uvs._vision.lib()
    b_models, b_n, b_index = believed
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    rest = (T, b_models.data_ptr(), b_n, ptr(b_index), q.data_ptr(), ptr(noise)) + \
        tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')) + (stream(),)
    cams, n_cams, index = camera
    front = (C.byref(fp), cams.data_ptr(), n_cams, ptr(index), ptr(motion))
    if assumed == MOVING_CALL:
        rc = lib.uvs_camera_believed_loop_moving_f64(*front, *rest)
    elif assumed == DELAYED_CALL:
        rc = lib.uvs_camera_believed_loop_delayed_f64(*front, ptr(latency), *rest)
    else:
        rc = lib.uvs_camera_believed_loop_aligned_f64(*front, ptr(latency), ptr(assumed), *rest)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


# ------------------------------------------------------------------------------------------------------------- (a): not told
@pytest.mark.parametrize('T', ac.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1), ('MCKF', 4)])
def test_without_an_assumed_latency_the_loops_are_their_delayed_namesakes(uvs, method, n_points, T):
    """assumed = NULL and all zeros through the C ABI on the same operands (mixed scenes, motions and latencies, rectangles, paints and a
    hold among them): every log row, stats, status, k_done, pixels, held and the poison past the last row.  With latency NULL too, the
    moving namesake's."""
    _, _, cams = scene_set(n_points)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, method, n_points), loop_operands(uvs, T, n_points)
    fa, believed = params(uvs, 'ANALYTICAL', n_points), (cams[:1], 1, None)
    zeros, motion = dev(np.zeros(T), np.int32), motions(T, n_points)[2]
    for latency, namesake in ((dev(ac.mixed(T)[0], np.int32), DELAYED_CALL), (None, MOVING_CALL)):
        want = c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, namesake, **op)
        assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
        want_b = c_baseline_loop(uvs, fa, T, n_points, camera, motion, latency, namesake, believed, op['q'], op['noise'])
        for assumed in (None, zeros):
            where = (method, T, namesake, assumed is None)
            assert_same_buffers(c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, **op), want, where)
            assert_same_buffers(c_baseline_loop(uvs, fa, T, n_points, camera, motion, latency, assumed, believed, op['q'], op['noise']), want_b, where)


ROUTES = ('uniform', 'grid', 'occluded', 'held', 'painted', 'scenes', 'moving', 'delayed')


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
    if route == 'delayed':
        kw.update(latency=ac.mixed(T)[0])
    return kw


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('T', ac.SIZES)
def test_none_and_zeros_are_the_call_without_the_argument_on_every_route(uvs, T, route):
    """engine.camera_closed_loop on each flavour's route: assumed_latency=None is that call, and 0 -- an int, and T zeros -- gives its bits
    through the aligned kernels, one launch and stepwise; for ANALYTICAL on the routes its one-launch loop has."""
    import torch
    plants = scene_set(4)[0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    kw = dict(route_kw(route, T, 4), guess='device')
    fp = params(uvs, 'GMCKF', 4)
    plain = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
    for assumed in (None, 0, np.zeros(T, np.int64)):
        got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, assumed_latency=assumed, **kw)
        cc.assert_same_bits(got, plain, K, (route, T, 'one launch', assumed is None))
        assert ('held' in got) == ('held' in plain) and (route != 'held' or torch.equal(got['held'], plain['held']))
    if route != 'grid':                                              # the stepwise loop has no per-trial flavour
        cc.assert_same_bits(uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, assumed_latency=0, **kw), plain, K,
                            (route, T, 'stepwise'))
    if route in ('uniform', 'scenes', 'moving', 'delayed'):
        fa = params(uvs, 'ANALYTICAL', 4)
        kw.pop('guess')
        plain = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=True, **kw)
        for fused, assumed in ((True, None), (True, 0), (True, np.zeros(T, np.int64)), (False, 0)):
            got = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=fused, assumed_latency=assumed, **kw)
            cc.assert_same_bits(got, plain, K, (route, T, 'baseline', fused, assumed is None))


# ------------------------------------------------------------------------------------------------------------- (c): one launch, stepwise
@pytest.mark.parametrize('T', ac.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_the_one_launch_is_the_stepwise_loop(uvs, method, n_points, T):
    """The mixed (d, a) pairs on the mixed motions and a mixed camera_index, under the four rectangle scenarios (occluders, paints, the wide
    bar with a hold): every log, status, k_done, stats, pixels and held.  The told trials differ from the launch that is not told, and the
    trials of a = 0 do not."""
    import torch
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    packed = motions(T, n_points)[2]
    latency, assumed = ac.mixed(T)
    plain = None
    for scenario in sc.SCENARIOS:
        kw = dict(scenario_kw(scenario, T, n_points), cameras=cams, camera_index=index, guess='device', believed=plants[0], target_motion=packed,
                  latency=latency)
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, assumed_latency=assumed, **kw)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, assumed_latency=torch.from_numpy(assumed), **kw)
        cc.assert_same_bits(fused, stepwise, K, (method, n_points, T, scenario))
        assert ('held' in fused) == (scenario == 'held') == ('held' in stepwise)
        if scenario == 'held':
            assert torch.equal(fused['held'], stepwise['held'])
        if scenario == 'plain':
            plain = fused
            untold = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            rows = fused['k_done'].cpu().numpy()                     # the rows of dq that are specified
            same = [np.array_equal(bits(fused['dq'])[:rows[t], t], bits(untold['dq'])[:rows[t], t]) for t in range(T)]
            assert same == [a == 0 for a in assumed], 'the told trials differ from the launch that is not told and the others do not'
    assert int(plain['k_done'].max()) == K


@pytest.mark.parametrize('method,n_points', BUILT)
def test_source_next_to_an_assumed_latency_is_gathered_by_output_trial(uvs, method, n_points):
    """trial_params with a 'source' permutation and per-trial kernel_bw and gain: two cells x the mixed pairs over three input trials, one
    launch, against the stepwise loop of each cell on the gathered inputs with the pairs, motions, rectangles and paints of its OUTPUT
    trials."""
    import torch
    plants = scene_set(n_points)[0]
    T = 12
    cells = [(5.0, 0.1), (20.0, 0.3)]
    cell, source = np.arange(T) % 2, np.random.default_rng(4).permutation(np.arange(T) % 3).astype(np.int32)
    vel, win, _ = motions(T, n_points)
    latency, assumed = ac.mixed(T)
    q, noise = dev(sc.starts(3)), dev(sc.noise(3, n_points))
    tp = dict(source=source, kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    for scenario in ('plain', 'held'):
        kw = scenario_kw(scenario, T, n_points)
        got = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device', trial_params=tp,
                                            target_motion=vel, motion_window=win, latency=latency, assumed_latency=assumed, **kw)
        for i, (bw, gain) in enumerate(cells):
            sel = np.flatnonzero(cell == i)
            src = dev(source[sel], np.int64)
            mine = {key: (value[sel] if key in ('occluders', 'occluder_colours') else value) for key, value in kw.items()}
            want = uvs.engine.camera_closed_loop(params(uvs, method, n_points, kernel_bw=bw, gain=gain), plants[0], q[src].contiguous(),
                                                 noise[:, src].contiguous(), fused=False, guess='device', target_motion=vel[sel],
                                                 motion_window=win[sel], latency=latency[sel], assumed_latency=assumed[sel], **mine)
            cc.assert_same_bits(got, want, K, (method, n_points, scenario, i), sel.tolist(), list(range(len(sel))))
            if scenario == 'held':
                assert torch.equal(got['held'][dev(sel, np.int64)], want['held'])
    only = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device',
                                         trial_params=dict(source=source), assumed_latency=assumed)   # no latency, no scenes: by output trial too
    want = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q[dev(source, np.int64)].contiguous(),
                                         noise[:, dev(source, np.int64)].contiguous(), fused=False, guess='device', assumed_latency=assumed)
    cc.assert_same_bits(only, want, K, (method, n_points, 'assumed alone'))


@pytest.mark.parametrize('T', ac.SIZES)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_baseline_one_launch_is_its_stepwise_loop(uvs, n_points, T):
    """ANALYTICAL on the mixed pairs: the law on the nominal model and on the trials' own scenes, with and without a motion; the trials of
    a = 0 keep the bits of the launch that is not told, and the others do not."""
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    packed = motions(T, n_points)[2]
    latency, assumed = ac.mixed(T)
    for believed in (dict(believed=plants[0]), dict()):
        for motion in (dict(target_motion=packed), dict()):
            kw = dict(cameras=cams, camera_index=index, latency=latency, **believed, **motion)
            fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, assumed_latency=assumed, **kw)
            stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, assumed_latency=assumed, **kw)
            cc.assert_same_bits(fused, stepwise, K, (n_points, T, tuple(believed), tuple(motion)))
            untold = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            cc.assert_same_bits(fused, untold, K, (n_points, T, 'the trials of a = 0'), [t for t in range(T) if assumed[t] == 0])
            told = [t for t in range(T) if assumed[t] > 0]
            assert all(not np.array_equal(bits(fused['dq'])[:, t], bits(untold['dq'])[:, t]) for t in told), 'telling shows in the command'
    alone = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, assumed_latency=assumed)   # the nominal camera as the one scene
    step = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, assumed_latency=assumed)
    cc.assert_same_bits(alone, step, K, (n_points, T, 'nominal, no latency'))


# ------------------------------------------------------------------------------------------------------------- (b): mixed against uniform
@pytest.mark.parametrize('T', ac.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_a_mixed_batch_is_every_trial_at_its_own_pair(uvs, method, n_points, T):
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    latency, assumed = ac.mixed(T)
    pairs = sorted(set(zip(latency.tolist(), assumed.tolist())))
    assert len(pairs) == (20 if T > 3 else 3)
    kw = dict(cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0], fused=True,
              target_motion=motions(T, n_points)[2], **scenario_kw('occluded', T, n_points))
    got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=latency, assumed_latency=assumed, **kw)
    fa = params(uvs, 'ANALYTICAL', n_points)
    kw_b = dict(cameras=cams, camera_index=sc.mixed_index(T, True), fused=True, target_motion=motions(T, n_points)[2])
    got_b = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, latency=latency, assumed_latency=assumed, **kw_b)
    seen = set()
    for d, a in pairs:
        mine = [t for t in range(T) if (latency[t], assumed[t]) == (d, a)]
        uniform = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=d, assumed_latency=a, **kw)
        cc.assert_same_bits(got, uniform, K, (method, n_points, T, d, a), mine)
        seen.add(bits(uniform['dq']).tobytes())
        uniform = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, latency=d, assumed_latency=a, **kw_b)
        cc.assert_same_bits(got_b, uniform, K, (n_points, T, d, a, 'baseline'), mine)
    assert len(seen) == len(pairs), 'as many different launches as pairs'


# ------------------------------------------------------------------------------------------------------------- K = 4
@pytest.mark.parametrize('T', ac.SIZES)
def test_four_steps_told_three_or_more_never_find_a_command(uvs, T):
    """K = 4: for a >= 3 no step has k - 1 - a >= 0, so every regressor is the zero vector and no ring slot is read after it was written
    (a = 8 reads slot k, which step k writes afterwards); and max(k - a, 0) = 0, so the law never leaves the step-0 joints.  a = 3, 5 and 8
    are therefore one loop, bit for bit, on both routes; a = 2, which finds dq_0 at k = 3, is another."""
    plants, _, cams = scene_set(4)
    index = sc.mixed_index(T, True)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, 4, steps=4))
    latency = ac.mixed(T)[0]
    for fp, kw in ((params(uvs, 'GMCKF', 4, steps=4), dict(guess='device', believed=plants[0])), (params(uvs, 'ANALYTICAL', 4, steps=4), {})):
        run = lambda a, fused: uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=fused, cameras=cams, camera_index=index,   # noqa: E731
                                                             latency=latency, assumed_latency=a, **kw)
        want = run(8, True)
        assert int(want['k_done'].max()) == 4
        for a, fused in ((8, False), (3, True), (5, True), (3, False)):
            cc.assert_same_bits(run(a, fused), want, 4, (fp.method, a, fused))
        two = run(2, True)
        assert np.array_equal(bits(two['dq'])[:3], bits(want['dq'])[:3]), 'the same loop up to k = 2'
        assert not np.array_equal(bits(two['dq'])[3], bits(want['dq'])[3]), 'and at k = 3 a = 2 finds dq_0 (the law: q_1)'


# ------------------------------------------------------------------------------------------------------------- (d), (e), (f)
VOID = (-1, sc.N_SCENES, INT32_MIN)


@pytest.mark.parametrize('T', ac.SIZES)
def test_a_void_trial_fails_alone_next_to_told_neighbours(uvs, T):
    """A void scene index (both loops) and a void source (the estimators' loop): status FAIL, k_done = 0, nothing else stored, and the rest
    of the launch keeps the bits of the valid launch.  At T = 259 the last trial has the pair (3, 8), which no other trial has, and the
    padding wavefront and lanes that shadow it store nothing: the poison past every last row is compared too.  An assumed latency outside
    0 .. 8 is clamped on the device: -3 is 0 and 11 is 8."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    motion = motions(T, 4)[2]
    d_mixed, a_mixed = ac.mixed(T)
    latency, assumed = dev(d_mixed, np.int32), dev(a_mixed, np.int32)
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2] if T > 3 else [1]
    source = np.arange(T, dtype=np.int32)
    tp_of = lambda s: uvs._vision.CameraTrialParams(None, None, None, None, None, s.data_ptr(), T)          # noqa: E731
    valid = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, assumed, **op)
    src = dev(source, np.int32)                                      # kept: the block holds its address alone
    valid_s = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, assumed, tp=tp_of(src), **op)
    assert_same_buffers(valid_s, valid, 'the identity as source')
    valid_b = c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, assumed, believed, op['q'], op['noise'])
    assert valid['k_done'][:T].max() == K
    if T > 3:
        pairs = list(zip(d_mixed.tolist(), a_mixed.tolist()))
        assert pairs[-1] == ac.LAST and pairs.count(ac.LAST) == 1, 'the pair the padding wavefront shadows is absent elsewhere'
    assert (a_mixed == 0).any() and (a_mixed == 8).any()
    wild = np.where(a_mixed == 0, -3, np.where(a_mixed == 8, 11, a_mixed))             # clamped to 0 and to 8 on the device
    assert_same_buffers(c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, dev(wild, np.int32), **op), valid, 'clamped')
    assert_same_buffers(c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, dev(wild, np.int32), believed, op['q'],
                                        op['noise']), valid_b, 'clamped, baseline')
    huge = np.where(a_mixed == 0, INT32_MIN, np.where(a_mixed == 8, 2 ** 31 - 1, a_mixed))
    assert_same_buffers(c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, dev(huge, np.int32), **op), valid, 'clamped')
    for turn in range(len(VOID)):
        holed, holed_source = index.copy(), source.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
            holed_source[t] = (-1, T, INT32_MIN)[(i + turn) % 3]
        hs = dev(holed_source, np.int32)
        for want, got in ((valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(holed, np.int32)), motion, latency, assumed, **op)),
                          (valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, assumed, tp=tp_of(hs), **op)),
                          (valid_b, c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(holed, np.int32)), motion, latency, assumed, believed, op['q'],
                                                    op['noise']))):
            want = {key: value.copy() for key, value in want.items()}
            for key in want:
                view = trial_view(want, key, T, 4)
                view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
            assert_same_buffers(got, want, (T, turn))
    no_model = dev(np.where(np.isin(np.arange(T), where), -1, 0), np.int32)          # (e): no believed model
    got = c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, latency, assumed, (cams[:1], 1, no_model), op['q'], op['noise'])
    want = {key: value.copy() for key, value in valid_b.items()}
    for key in want:
        view = trial_view(want, key, T, 4)
        view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
    assert_same_buffers(got, want, (T, 'no believed model'))


# ------------------------------------------------------------------------------------------------------------- the CPU restatements
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('a', ac.ORACLE_ASSUMED)
@pytest.mark.parametrize('method,n_points', ac.ORACLE)
def test_against_the_cpu_loop(uvs, method, n_points, a, fused):
    """One trial on the nominal camera at d = a, the host's initial guess as the oracle makes it, against camera_aligned_common.estimator_trial
    -- the oracle's loop, which the host file holds bit for bit to oracle.pixel_loop.run at a = 0 and a = 1."""
    ref, cfg = ac.estimator_trial(method, n_points, a, a), mc.oracle_settings(n_points)
    fp = params(uvs, method, n_points, kernel_bw=cfg['kernel_bw'], gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=ac.RADIUS, fused=fused, latency=a, assumed_latency=a)
    assert ref['k_done'] == K
    against_the_oracle(out, ref, f'{method} ({2 * n_points},6) d = a = {a} {"one launch" if fused else "stepwise"}')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('a', ac.LAW_ASSUMED)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_law_against_its_numpy_loop(uvs, n_points, a, fused):
    """ANALYTICAL at d = a against camera_aligned_common.law_trial, at the 1e-8 relative of tests/test_gpu_camera_analytical.py; status, k_done
    and masks exact."""
    ref, cfg = ac.law_trial(n_points, a, a), mc.oracle_settings(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points, gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=ac.RADIUS, fused=fused, latency=a, assumed_latency=a)
    out = {key: value.cpu().numpy() for key, value in out.items()}
    where = f'the law ({2 * n_points},6) d = a = {a} {"one launch" if fused else "stepwise"}'
    assert (out['status'][0], out['k_done'][0]) == (ref['status'], ref['k_done']) == (0, K), where
    assert np.array_equal(out['pixels'][0], ref['pixels']), where
    for key in ('q', 'f', 'dq', 'err'):
        d = float(np.abs(out[key][:len(ref[key]), 0] - ref[key]).max() / np.abs(ref[key]).max())
        print(f'{where} {key}: {d:.2e}')
        assert d <= 1e-8, (where, key, d)
    d = float(np.abs(out['stats'][0] - ref['stats']).max() / np.abs(ref['stats']).max())
    assert d <= 1e-8, (where, 'stats', d)
