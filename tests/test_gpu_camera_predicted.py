"""FEATURE PREDICTION on the GPU (include/uvs_vision.h, "FEATURE PREDICTION"; engine.camera_closed_loop(predict=)): the estimators'
one-launch loop whose law acts on (f + X_k s) - desired (predicted_frames_kernel, 22 instantiations), the baseline's whose law is handed
f + (h(q_k) - h(q_{max(k - p, 0)})) (predicted_baseline_kernel) and the baseline's stepwise loop, over the (latency, assumed, horizon)
triples of tests/camera_predicted_common.py, the motions of tests/camera_moving_common.py and the scene set of tests/camera_scenes_common.py.

Every comparison but the CPU restatements' is of bits, and none leaves a trial out: (a) without a horizon -- None through the entry point
the call always used, NULL and all zeros through the predicted kernels -- a loop is the call without it on every route, poison past the
last row included; (c) the baseline's one launch is its stepwise loop; (b) trial t of a mixed batch is trial t of the launch in which
every trial has t's triple -- for the estimators, which have no stepwise route, that is also how all 22 instantiations are held under
occluders, paints, a hold, scenes, motion and source; (d, e) a void trial writes status FAIL and k_done = 0 and nothing else while its
neighbours keep their bits, and the padding wavefront and the shadow lanes store nothing; (f) values outside 0 .. 8 are clamped on the
device.  The CPU restatements (camera_predicted_common.estimator_trial and law_trial, held bit for bit to camera_aligned_common's at p = 0
by the host file) are held to pixel_loop_common's gates and to 1e-8; the host file shows every one of them within the preconditions, so
none is left out.  Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, the last with a padding wavefront that
shadows a trial whose triple no other trial has); K = 16; and K = 4 and K = 5, where a horizon longer than the run sums what there is."""
import ctypes as C

import numpy as np
import pytest

import camera_common as cc
import camera_moving_common as mc
import camera_predicted_common as pc
import camera_scenes_common as sc
import pixel_loop_common as pl
from test_gpu_camera_moving import (BUILT, INT32_MIN, POISON, against_the_oracle, assert_same_buffers, buffers, dev, loop_operands, motions, params,
                                    scenario_kw, scene_set, stream, trial_view)

pytestmark = pytest.mark.gpu

K = pc.K
bits = cc.bits
ALIGNED_CALL = 'the aligned namesake'


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


def c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, predict, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0):
    """uvs_camera_closed_loop_predicted_f64 (latency, assumed, predict: int32 device tensors or None = NULL) or, for predict = ALIGNED_CALL,
    its aligned namesake, on the same operands into poisoned buffers; returns them on the host, tails included."""
    import torch
    buf = buffers(T, n_points)
    lib = uvs._vision.lib()
    middle = (T, None if tp is None else C.byref(tp), None if occ is None else occ.data_ptr(), None if paint is None else paint.data_ptr(),
              0 if occ is None else occ.shape[1], hold, q.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr())
    outs = tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels', 'held')) + (stream(),)
    cams, n_cams, index = camera
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    front = (C.byref(fp), cams.data_ptr(), n_cams, ptr(index), ptr(motion), ptr(latency), ptr(assumed))
    if predict == ALIGNED_CALL:
        rc = lib.uvs_camera_closed_loop_aligned_f64(*front, *middle, *outs)
    else:
        rc = lib.uvs_camera_closed_loop_predicted_f64(*front, ptr(predict), *middle, *outs)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def c_baseline_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, predict, believed, q, noise):
    import torch
    buf = buffers(T, n_points, True)
    lib = uvs._vision.lib()
    b_models, b_n, b_index = believed
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    rest = (T, b_models.data_ptr(), b_n, ptr(b_index), q.data_ptr(), ptr(noise)) + \
        tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')) + (stream(),)
    cams, n_cams, index = camera
    front = (C.byref(fp), cams.data_ptr(), n_cams, ptr(index), ptr(motion), ptr(latency), ptr(assumed))
    if predict == ALIGNED_CALL:
        rc = lib.uvs_camera_believed_loop_aligned_f64(*front, *rest)
    else:
        rc = lib.uvs_camera_believed_loop_predicted_f64(*front, ptr(predict), *rest)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


# ------------------------------------------------------------------------------------------------------------- (a): no horizon
@pytest.mark.parametrize('T', pc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1), ('MCKF', 4)])
def test_without_a_horizon_the_loops_are_their_aligned_namesakes(uvs, method, n_points, T):
    """predict = NULL and all zeros through the C ABI on the same operands (mixed scenes, motions, latencies and assumed latencies,
    rectangles, paints and a hold among them): every log row, stats, status, k_done, pixels, held and the poison past the last row.  With
    latency and assumed NULL too."""
    _, _, cams = scene_set(n_points)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, method, n_points), loop_operands(uvs, T, n_points)
    fa, believed = params(uvs, 'ANALYTICAL', n_points), (cams[:1], 1, None)
    zeros, motion = dev(np.zeros(T), np.int32), motions(T, n_points)[2]
    d, a, _ = pc.mixed(T)
    for latency, assumed in ((dev(d, np.int32), dev(a, np.int32)), (None, None)):
        want = c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, ALIGNED_CALL, **op)
        assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
        want_b = c_baseline_loop(uvs, fa, T, n_points, camera, motion, latency, assumed, ALIGNED_CALL, believed, op['q'], op['noise'])
        for predict in (None, zeros):
            where = (method, T, latency is None, predict is None)
            assert_same_buffers(c_estimator_loop(uvs, fp, T, n_points, camera, motion, latency, assumed, predict, **op), want, where)
            assert_same_buffers(c_baseline_loop(uvs, fa, T, n_points, camera, motion, latency, assumed, predict, believed, op['q'], op['noise']),
                                want_b, where)


ROUTES = ('uniform', 'grid', 'occluded', 'held', 'painted', 'scenes', 'moving', 'delayed', 'aligned')


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
        kw.update(latency=pc.mixed(T)[0])
    if route == 'aligned':
        kw.update(latency=pc.mixed(T)[0], assumed_latency=pc.mixed(T)[1])
    return kw


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('T', pc.SIZES)
def test_none_and_zeros_are_the_call_without_the_argument_on_every_route(uvs, T, route):
    """engine.camera_closed_loop on each flavour's route: predict=None is that call, and 0 -- an int, and T zeros -- gives its bits through
    the predicted kernels; for ANALYTICAL on the routes its one-launch loop has, one launch and stepwise."""
    import torch
    plants = scene_set(4)[0]
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    kw = dict(route_kw(route, T, 4), guess='device')
    fp = params(uvs, 'GMCKF', 4)
    plain = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
    for predict in (None, 0, np.zeros(T, np.int64)):
        got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, predict=predict, **kw)
        cc.assert_same_bits(got, plain, K, (route, T, 'one launch', predict is None))
        assert ('held' in got) == ('held' in plain) and (route != 'held' or torch.equal(got['held'], plain['held']))
    if route in ('uniform', 'scenes', 'moving', 'delayed', 'aligned'):
        fa = params(uvs, 'ANALYTICAL', 4)
        kw.pop('guess')
        plain = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=True, **kw)
        for fused, predict in ((True, None), (True, 0), (True, np.zeros(T, np.int64)), (False, None), (False, 0)):
            got = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, fused=fused, predict=predict, **kw)
            cc.assert_same_bits(got, plain, K, (route, T, 'baseline', fused, predict is None))


# ------------------------------------------------------------------------------------------------------------- (b): mixed against uniform
def triples_of(d, a, p):
    return list(zip(d.tolist(), a.tolist(), p.tolist()))


@pytest.mark.parametrize('T', pc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_a_mixed_batch_is_every_trial_at_its_own_triple(uvs, method, n_points, T):
    """Every triple of the mix, estimators and baseline: trial t of the mixed launch has the bits of the launch in which every trial has
    t's (d, a, p); and the launches differ from each other."""
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    latency, assumed, predict = pc.mixed(T)
    mine_of = triples_of(latency, assumed, predict)
    triples = sorted(set(mine_of))
    assert len(triples) == (40 if T > 3 else 3)
    kw = dict(cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0], fused=True,
              target_motion=motions(T, n_points)[2], **scenario_kw('occluded', T, n_points))
    got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=latency, assumed_latency=assumed, predict=predict, **kw)
    fa = params(uvs, 'ANALYTICAL', n_points)
    kw_b = dict(cameras=cams, camera_index=sc.mixed_index(T, True), fused=True, target_motion=motions(T, n_points)[2])
    got_b = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, latency=latency, assumed_latency=assumed, predict=predict, **kw_b)
    seen, seen_b = set(), set()
    for d, a, p in triples:
        mine = [t for t in range(T) if mine_of[t] == (d, a, p)]
        uniform = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=d, assumed_latency=a, predict=p, **kw)
        cc.assert_same_bits(got, uniform, K, (method, n_points, T, d, a, p), mine)
        seen.add(bits(uniform['dq']).tobytes())
        uniform = uvs.engine.camera_closed_loop(fa, plants[0], q, noise, latency=d, assumed_latency=a, predict=p, **kw_b)
        cc.assert_same_bits(got_b, uniform, K, (n_points, T, d, a, p, 'baseline'), mine)
        seen_b.add(bits(uniform['dq']).tobytes())
    assert len(seen) == len(triples) == len(seen_b), 'as many different launches as triples'


@pytest.mark.parametrize('T', pc.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_every_instantiation_carries_its_uniform_launch_under_every_scenario(uvs, method, n_points, T):
    """All 22 instantiations (11 estimator-shape pairs, both workgroup forms), mixed scenes, motions and triples under the four rectangle
    scenarios (none, occluders, paints, the wide bar with a hold): every output trial carries the bits of the launch at its own triple,
    for every triple of the batch in every scenario."""
    import torch
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    latency, assumed, predict = pc.mixed(T)
    mine_of = triples_of(latency, assumed, predict)
    triples = sorted(set(mine_of))
    for scenario in sc.SCENARIOS:
        kw = dict(scenario_kw(scenario, T, n_points), cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0],
                  target_motion=motions(T, n_points)[2], fused=True)
        got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=latency, assumed_latency=assumed, predict=predict, **kw)
        assert ('held' in got) == (scenario == 'held')
        if scenario == 'plain':
            assert int(got['k_done'].max()) == K
            unpredicted = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=latency, assumed_latency=assumed, **kw)
            rows = got['k_done'].cpu().numpy()                       # the rows of dq that are specified
            same = [np.array_equal(bits(got['dq'])[:rows[t], t], bits(unpredicted['dq'])[:rows[t], t]) for t in range(T)]
            assert same == [p == 0 for p in predict], 'the predicting trials differ from the launch without a horizon and the others do not'
            assert torch.equal(got['f'][0], unpredicted['f'][0]), 'the f log is the reported row'
        for d, a, p in triples:
            mine = [t for t in range(T) if mine_of[t] == (d, a, p)]
            uniform = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, latency=d, assumed_latency=a, predict=p, **kw)
            cc.assert_same_bits(got, uniform, K, (method, n_points, T, scenario, d, a, p), mine)
            if scenario == 'held':
                sel = dev(mine, np.int64)
                assert torch.equal(got['held'][sel], uniform['held'][sel])


@pytest.mark.parametrize('method,n_points', BUILT)
def test_source_next_to_a_horizon_is_gathered_by_output_trial(uvs, method, n_points):
    """trial_params with a 'source' permutation and per-trial kernel_bw and gain: two cells x the mixed triples over three input trials, one
    launch, against the launch of each cell on the gathered inputs with the triples, motions, rectangles and paints of its OUTPUT trials."""
    import torch
    plants = scene_set(n_points)[0]
    T = 12
    cells = [(5.0, 0.1), (20.0, 0.3)]
    cell, source = np.arange(T) % 2, np.random.default_rng(4).permutation(np.arange(T) % 3).astype(np.int32)
    vel, win, _ = motions(T, n_points)
    latency, assumed, predict = pc.mixed(T)
    q, noise = dev(sc.starts(3)), dev(sc.noise(3, n_points))
    tp = dict(source=source, kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    for scenario in ('plain', 'held'):
        kw = scenario_kw(scenario, T, n_points)
        got = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device', trial_params=tp,
                                            target_motion=vel, motion_window=win, latency=latency, assumed_latency=assumed, predict=predict, **kw)
        for i, (bw, gain) in enumerate(cells):
            sel = np.flatnonzero(cell == i)
            src = dev(source[sel], np.int64)
            mine = {key: (value[sel] if key in ('occluders', 'occluder_colours') else value) for key, value in kw.items()}
            want = uvs.engine.camera_closed_loop(params(uvs, method, n_points, kernel_bw=bw, gain=gain), plants[0], q[src].contiguous(),
                                                 noise[:, src].contiguous(), fused=True, guess='device', target_motion=vel[sel],
                                                 motion_window=win[sel], latency=latency[sel], assumed_latency=assumed[sel], predict=predict[sel],
                                                 **mine)
            cc.assert_same_bits(got, want, K, (method, n_points, scenario, i), sel.tolist(), list(range(len(sel))))
            if scenario == 'held':
                assert torch.equal(got['held'][dev(sel, np.int64)], want['held'])
    only = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device',
                                         trial_params=dict(source=source), predict=predict)   # no latency, no scenes: by output trial too
    want = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q[dev(source, np.int64)].contiguous(),
                                         noise[:, dev(source, np.int64)].contiguous(), fused=True, guess='device', predict=predict)
    cc.assert_same_bits(only, want, K, (method, n_points, 'a horizon alone'))


# ------------------------------------------------------------------------------------------------------------- (c): one launch, stepwise
@pytest.mark.parametrize('T', pc.SIZES)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_baseline_one_launch_is_its_stepwise_loop(uvs, n_points, T):
    """ANALYTICAL on the mixed triples: the law on the nominal model and on the trials' own scenes, with and without a motion; the trials of
    p = 0 keep the bits of the launch without a horizon, and the others do not; the f log is the reported row."""
    import torch
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    packed = motions(T, n_points)[2]
    latency, assumed, predict = pc.mixed(T)
    for believed in (dict(believed=plants[0]), dict()):
        for motion in (dict(target_motion=packed), dict()):
            kw = dict(cameras=cams, camera_index=index, latency=latency, assumed_latency=assumed, **believed, **motion)
            fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, predict=predict, **kw)
            stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, predict=torch.from_numpy(predict), **kw)
            cc.assert_same_bits(fused, stepwise, K, (n_points, T, tuple(believed), tuple(motion)))
            plain = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            cc.assert_same_bits(fused, plain, K, (n_points, T, 'the trials of p = 0'), [t for t in range(T) if predict[t] == 0])
            ahead = [t for t in range(T) if predict[t] > 0]
            assert all(not np.array_equal(bits(fused['dq'])[:, t], bits(plain['dq'])[:, t]) for t in ahead), 'predicting shows in the command'
            assert torch.equal(fused['f'][0], plain['f'][0]), 'the f log is the reported row'
    alone = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, predict=predict)   # the nominal camera as the one scene and model
    step = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, predict=predict)
    cc.assert_same_bits(alone, step, K, (n_points, T, 'nominal, no latency'))


# ------------------------------------------------------------------------------------------------------------- K = 4, K = 5
@pytest.mark.parametrize('T', pc.SIZES)
def test_a_horizon_longer_than_the_run_sums_what_there_is(uvs, T):
    """K = 4: no step has more than three commands behind it, so p = 3, 5 and 8 sum the same terms (the slots further back have not been
    written and read as zeros) and max(k - p, 0) is the same step: one loop, bit for bit, on every route; p = 2, which drops dq_0 at k = 3,
    is another.  K = 5: p = 5 and p = 8 are one loop, and p = 3, which drops dq_0 at k = 4, is another."""
    plants, _, cams = scene_set(4)
    index = sc.mixed_index(T, True)
    q = dev(sc.starts(T))
    latency, assumed, _ = pc.mixed(T)
    for steps, one_loop, other in ((4, (3, 5), 2), (5, (5,), 3)):
        noise = dev(sc.noise(T, 4, steps=steps))
        for fp, kw, routes in ((params(uvs, 'GMCKF', 4, steps=steps), dict(guess='device', believed=plants[0]), (True,)),
                               (params(uvs, 'ANALYTICAL', 4, steps=steps), {}, (True, False))):
            run = lambda p, fused: uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=fused, cameras=cams, camera_index=index,   # noqa: E731
                                                                 latency=latency, assumed_latency=assumed, predict=p, **kw)
            want = run(8, True)
            assert int(want['k_done'].max()) == steps
            for p in one_loop:
                for fused in routes:
                    cc.assert_same_bits(run(p, fused), want, steps, (fp.method, steps, p, fused))
            if False in routes:
                cc.assert_same_bits(run(8, False), want, steps, (fp.method, steps, 8, 'stepwise'))
            less = run(other, True)
            assert np.array_equal(bits(less['dq'])[:steps - 1], bits(want['dq'])[:steps - 1]), 'the same loop up to the last step'
            assert not np.array_equal(bits(less['dq'])[steps - 1], bits(want['dq'])[steps - 1]), 'and at the last step the shorter horizon drops dq_0'


# ------------------------------------------------------------------------------------------------------------- (d), (e), (f)
VOID = (-1, sc.N_SCENES, INT32_MIN)


@pytest.mark.parametrize('T', pc.SIZES)
def test_a_void_trial_fails_alone_next_to_predicting_neighbours(uvs, T):
    """A void scene index (both loops) and a void source (the estimators' loop): status FAIL, k_done = 0, nothing else stored, and the rest
    of the launch keeps the bits of the valid launch.  At T = 259 the last trial has the triple (3, 3, 8), which no other trial has, and
    the padding wavefront and lanes that shadow it store nothing: the poison past every last row is compared too.  A horizon outside
    0 .. 8 is clamped on the device: -3 and the smallest int32 are 0, 11 and the largest int32 are 8.  A trial without a believed model
    starts FAILed."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    motion = motions(T, 4)[2]
    d_mixed, a_mixed, p_mixed = pc.mixed(T)
    if T <= 3:
        p_mixed = np.array([0, 8, 2])                                # both ends of the range are there to be clamped to
    latency, assumed, predict = dev(d_mixed, np.int32), dev(a_mixed, np.int32), dev(p_mixed, np.int32)
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2] if T > 3 else [1]
    source = np.arange(T, dtype=np.int32)
    tp_of = lambda s: uvs._vision.CameraTrialParams(None, None, None, None, None, s.data_ptr(), T)          # noqa: E731
    camera = lambda idx: (cams, 6, dev(idx, np.int32))              # noqa: E731
    valid = c_estimator_loop(uvs, fp, T, 4, camera(index), motion, latency, assumed, predict, **op)
    src = dev(source, np.int32)                                      # kept: the block holds its address alone
    valid_s = c_estimator_loop(uvs, fp, T, 4, camera(index), motion, latency, assumed, predict, tp=tp_of(src), **op)
    assert_same_buffers(valid_s, valid, 'the identity as source')
    valid_b = c_baseline_loop(uvs, fa, T, 4, camera(index), motion, latency, assumed, predict, believed, op['q'], op['noise'])
    assert valid['k_done'][:T].max() == K
    if T > 3:
        triples = triples_of(d_mixed, a_mixed, p_mixed)
        assert triples[-1] == pc.LAST and triples.count(pc.LAST) == 1, 'the triple the padding wavefront shadows is absent elsewhere'
    assert (p_mixed == 0).any() and (p_mixed == 8).any()
    for low, high in ((-3, 11), (INT32_MIN, 2 ** 31 - 1)):           # clamped to 0 and to 8 on the device
        wild = dev(np.where(p_mixed == 0, low, np.where(p_mixed == 8, high, p_mixed)), np.int32)
        assert_same_buffers(c_estimator_loop(uvs, fp, T, 4, camera(index), motion, latency, assumed, wild, **op), valid, ('clamped', low))
        assert_same_buffers(c_baseline_loop(uvs, fa, T, 4, camera(index), motion, latency, assumed, wild, believed, op['q'], op['noise']), valid_b,
                            ('clamped, baseline', low))
    for turn in range(len(VOID)):
        holed, holed_source = index.copy(), source.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
            holed_source[t] = (-1, T, INT32_MIN)[(i + turn) % 3]
        hs = dev(holed_source, np.int32)
        for want, got in ((valid, c_estimator_loop(uvs, fp, T, 4, camera(holed), motion, latency, assumed, predict, **op)),
                          (valid, c_estimator_loop(uvs, fp, T, 4, camera(index), motion, latency, assumed, predict, tp=tp_of(hs), **op)),
                          (valid_b, c_baseline_loop(uvs, fa, T, 4, camera(holed), motion, latency, assumed, predict, believed, op['q'], op['noise']))):
            want = {key: value.copy() for key, value in want.items()}
            for key in want:
                view = trial_view(want, key, T, 4)
                view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
            assert_same_buffers(got, want, (T, turn))
    no_model = dev(np.where(np.isin(np.arange(T), where), -1, 0), np.int32)          # (e): no believed model
    got = c_baseline_loop(uvs, fa, T, 4, camera(index), motion, latency, assumed, predict, (cams[:1], 1, no_model), op['q'], op['noise'])
    want = {key: value.copy() for key, value in valid_b.items()}
    for key in want:
        view = trial_view(want, key, T, 4)
        view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
    assert_same_buffers(got, want, (T, 'no believed model'))


# ------------------------------------------------------------------------------------------------------------- the CPU restatements
@pytest.mark.parametrize('told', ['a = 0', 'a = d'])
@pytest.mark.parametrize('p', pc.ORACLE_HORIZONS)
@pytest.mark.parametrize('method,n_points', pc.ORACLE)
def test_against_the_cpu_loop(uvs, method, n_points, p, told):
    """One trial on the nominal camera at d = p, the host's initial guess as the oracle makes it, against
    camera_predicted_common.estimator_trial, which the host file holds bit for bit to camera_aligned_common's loop at p = 0."""
    a = 0 if told == 'a = 0' else p
    ref, cfg = pc.estimator_trial(method, n_points, p, a, p), mc.oracle_settings(n_points)
    fp = params(uvs, method, n_points, kernel_bw=cfg['kernel_bw'], gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=pc.RADIUS, fused=True, latency=p, assumed_latency=a, predict=p)
    assert ref['k_done'] == K
    against_the_oracle(out, ref, f'{method} ({2 * n_points},6) d = p = {p}, a = {a}')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('p', pc.LAW_HORIZONS)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_law_against_its_numpy_loop(uvs, n_points, p, fused):
    """ANALYTICAL at d = p, a = 0 against camera_predicted_common.law_trial, at the 1e-8 relative of tests/test_gpu_camera_analytical.py;
    status, k_done and masks exact."""
    ref, cfg = pc.law_trial(n_points, p, 0, p), mc.oracle_settings(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points, gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=pc.RADIUS, fused=fused, latency=p, assumed_latency=0, predict=p)
    out = {key: value.cpu().numpy() for key, value in out.items()}
    where = f'the law ({2 * n_points},6) d = p = {p} {"one launch" if fused else "stepwise"}'
    assert (out['status'][0], out['k_done'][0]) == (ref['status'], ref['k_done']) == (0, K), where
    assert np.array_equal(out['pixels'][0], ref['pixels']), where
    for key in ('q', 'f', 'dq', 'err'):
        d = float(np.abs(out[key][:len(ref[key]), 0] - ref[key]).max() / np.abs(ref[key]).max())
        print(f'{where} {key}: {d:.2e}')
        assert d <= 1e-8, (where, key, d)
    d = float(np.abs(out['stats'][0] - ref['stats']).max() / np.abs(ref['stats']).max())
    assert d <= 1e-8, (where, 'stats', d)
