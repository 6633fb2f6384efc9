"""MOVING TARGETS on the GPU (include/uvs_vision.h, "MOVING TARGETS"; engine.*(target_motion=, motion_window=)): the two stand-alone calls,
the estimators' one-launch loop (moving_target_kernel, 22 instantiations) and the baseline's (moving_baseline_kernel) over the motions of
tests/camera_moving_common.py and the scene set of tests/camera_scenes_common.py.

Every comparison but the oracle's is of bits, and none leaves a trial out: at a given k a stand-alone call is the scenes call on cameras
whose points the host moved by plant.target_at; without a motion -- NULL, a batch whose s(k) is 0 at every step, NaN velocities that never
start -- a loop is its *_scenes_* namesake, poison past the last row included; the one launch is the stepwise loop; trial t of a mixed
batch is trial t of the launch in which every trial has t's motion; a void trial writes status FAIL and k_done = 0 and nothing else while
its moving neighbours keep their bits.  The oracle (oracle/pixel_loop.py through its sensor= hook on plant.target_at) is held to
pixel_loop_common's gates: 1e-8 for err, q, f and stats, 1e-7 for the command, the integers exact.
Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, the last with a padding wavefront that shadows a MOVING trial);
K = 16."""
import ctypes as C
import functools

import numpy as np
import pytest

import camera_common as cc
import camera_moving_common as mc
import camera_scenes_common as sc
import pixel_loop_common as pl

pytestmark = pytest.mark.gpu

K = mc.K
BUILT = [(method, n_points) for n_points in (4, 3, 1) for method in pl.METHODS if not (method == 'MCKF' and n_points == 3)]
POISON = -7
TAIL = 16                                                            # poisoned words past the end of every output: nobody writes there
INT32_MIN = -2 ** 31
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


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def scene_set(n_points):
    """Shared and left as it is: the plants, the structs and the packed device array of the six scenes for a camera of n_points discs."""
    import uvs_amd
    plants, structs = sc.plants(uvs_amd, n_points), sc.structs(uvs_amd, n_points)
    return plants, structs, uvs_amd.engine.camera_scenes(plants, sc.RADII)


@functools.lru_cache(maxsize=None)
def motions(T, n_points, kind='mixed'):
    """(velocity, window, the packed device tensor) of a batch: 'mixed', 'still', 'nan', or one of the four kinds 0 .. 3 of the mix for
    every trial.  Shared and left as it is."""
    import uvs_amd
    if kind == 'mixed':
        vel, win = mc.mixed(T, n_points)
    elif kind in ('still', 'nan'):
        vel, win = mc.still(T, n_points, kind == 'nan')
    else:
        v4, w4 = mc.mixed(4, n_points)
        vel, win = np.tile(v4[kind], (T, 1, 1)), np.tile(w4[kind], (T, 1))
    for a in (vel, win):
        a.setflags(write=False)
    return vel, win, uvs_amd.engine.target_motions(vel, win, n_points, T)


def params(uvs, method, n_points, steps=K, kernel_bw=pl.BW, gain=pl.GAIN):
    fp = uvs.engine.make_params(2 * n_points, 6, method, kernel_bw, False, pl.DT, pl.DT * (steps + 0.5), gain, pl.DESIRED[:2 * n_points], True, 0,
                                steps, pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX)
    assert fp.steps == steps
    fp.reg = pl.REG
    return fp


def scenario_kw(scenario, T, n_points):
    rows, paints, hold = sc.rectangles(scenario, n_points)
    kw = dict(hold=hold)
    if rows is not None:
        kw['occluders'] = np.broadcast_to(np.array(rows, np.int64), (T, len(rows), 8)).copy()
        kw['occluders'][1::2, 0, 6] += 2                             # every other trial: the first rectangle comes two steps later
    if paints is not None:
        kw['occluder_colours'] = np.broadcast_to(np.array(paints, np.int64), (T, len(paints))).copy()
    return kw


def raw(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------------------------------------- 1: the stand-alone calls
def host_moved_cameras(uvs, n_points, index, vel, win, k):
    """What contract (b) compares against: one camera per trial whose points the host moved by the numpy rule."""
    plants = scene_set(n_points)[0]
    moved = mc.moved_plants(uvs, [plants[i] for i in index], vel, win, k)
    return uvs.engine.camera_scenes([p.to_camera(sc.RADII[i]) for p, i in zip(moved, index)])


@pytest.mark.parametrize('rects', ['none', 'occluded', 'painted'])
@pytest.mark.parametrize('T', mc.SIZES)
def test_the_stand_alone_calls_are_the_scenes_calls_on_host_moved_cameras(uvs, T, rects):
    """At k = 0, 5, 12, over the six scenes, with the mixed motions: discs, q_out, features and pixels of the moving calls against the
    scenes calls on host-moved cameras; and the features against detect_circles of render_discs of the projected discs."""
    import torch
    plants, _, cams = scene_set(4)
    vel, win, packed = motions(T, 4)
    index = sc.mixed_index(T, True)
    q, dq = dev(sc.starts(T)), dev(np.random.default_rng(3).standard_normal((T, 6)) * 0.01)
    kw = scenario_kw({'none': 'plain'}.get(rects, rects), T, 4)
    kw.pop('hold')
    noise = dev(np.random.default_rng(5).standard_normal((T, 8)))
    at_k0 = None
    for k in (0, 5, 12):
        moved = host_moved_cameras(uvs, 4, index, vel, win, k)
        for motion_kw in (dict(target_motion=vel, motion_window=win), dict(target_motion=packed)):
            q_out = [torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
            got = uvs.engine.camera_project(plants[0], q, dq, 0.05, q_out=q_out[0], cameras=cams, camera_index=index, k=k, **motion_kw)
            want = uvs.engine.camera_project(plants[0], q, dq, 0.05, q_out=q_out[1], cameras=moved)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(q_out[0]), bits(q_out[1])), (k, tuple(motion_kw))
        pix = [torch.full((T, 4), POISON, dtype=torch.int32, device='cuda') for _ in range(3)]
        d_out = [torch.full((T, 4, 3), 7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
        f = uvs.engine.camera_features(plants[0], q, dq, 0.05, noise=noise, pixels=pix[0], discs=d_out[0], k=k, cameras=cams, camera_index=index,
                                       target_motion=packed, **kw)
        f_want = uvs.engine.camera_features(plants[0], q, dq, 0.05, noise=noise, pixels=pix[1], discs=d_out[1], k=k, cameras=moved, **kw)
        assert np.array_equal(bits(f), bits(f_want)) and torch.equal(pix[0], pix[1]) and np.array_equal(bits(d_out[0]), bits(d_out[1])), k
        assert np.array_equal(bits(d_out[0]), bits(got))
        frames = uvs.engine.render_discs(got, 4, k=k, **kw)
        assert np.array_equal(bits(f), bits(uvs.engine.detect_circles(frames, 4, noise=noise, pixels=pix[2]))) and torch.equal(pix[0], pix[2]), k
        if k == 0:
            at_k0 = bits(got)
        else:
            moving = (np.arange(T) % 4 == 1) | (np.arange(T) % 4 == 2)
            changed = (bits(got) != at_k0).reshape(T, -1).any(axis=1)
            assert np.array_equal(changed, moving), (k, 'the moving trials moved and the others did not')
    # without cameras the nominal camera is the one scene
    alone = uvs.engine.camera_project(plants[0], q, dq, 0.05, k=12, target_motion=packed)
    want = uvs.engine.camera_project(plants[0], q, dq, 0.05, cameras=host_moved_cameras(uvs, 4, np.zeros(T, int), vel, win, 12))
    assert np.array_equal(bits(alone), bits(want))


# ------------------------------------------------------------------------------------------------------------- the C ABI, poisoned buffers
def buffers(T, n_points, baseline=False):
    import torch
    m = 2 * n_points
    nan = lambda n: torch.full((n + TAIL,), float('nan'), dtype=torch.float64, device='cuda')               # noqa: E731
    ints = lambda n: torch.full((n + TAIL,), POISON, dtype=torch.int32, device='cuda')                     # noqa: E731
    buf = dict(q=nan(K * T * 6), f=nan(K * T * m), dq=nan(K * T * 6), err=nan(K * T * m), status=ints(T), k_done=ints(T), stats=nan(T * 3),
               pixels=ints(T * n_points))
    if not baseline:
        buf.update(kappa=nan(K * T * m), held=ints(T * n_points))
    return buf


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


SCENES_CALL = 'the scenes namesake'


def c_estimator_loop(uvs, fp, T, n_points, camera, motion, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0):
    """uvs_camera_closed_loop_moving_f64 (motion: a packed tensor or None = NULL) or, for motion = SCENES_CALL, its scenes namesake, on the
    same operands into poisoned buffers; returns them on the host, tails included.  camera = (cams tensor, n_cams, index tensor or None)."""
    import torch
    buf = buffers(T, n_points)
    lib = uvs._vision.lib()
    middle = (T, None if tp is None else C.byref(tp), None if occ is None else occ.data_ptr(), None if paint is None else paint.data_ptr(),
              0 if occ is None else occ.shape[1], hold, q.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr())
    outs = tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels', 'held')) + (stream(),)
    cams, n_cams, index = camera
    triple = (cams.data_ptr(), n_cams, None if index is None else index.data_ptr())
    if isinstance(motion, str):
        rc = lib.uvs_camera_closed_loop_scenes_f64(C.byref(fp), *triple, *middle, *outs)
    else:
        rc = lib.uvs_camera_closed_loop_moving_f64(C.byref(fp), *triple, None if motion is None else motion.data_ptr(), *middle, *outs)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def c_baseline_loop(uvs, fp, T, n_points, camera, motion, believed, q, noise):
    import torch
    buf = buffers(T, n_points, True)
    lib = uvs._vision.lib()
    b_models, b_n, b_index = believed
    rest = (T, b_models.data_ptr(), b_n, None if b_index is None else b_index.data_ptr(), q.data_ptr(), None if noise is None else noise.data_ptr()) + \
        tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')) + (stream(),)
    cams, n_cams, index = camera
    triple = (cams.data_ptr(), n_cams, None if index is None else index.data_ptr())
    if isinstance(motion, str):
        rc = lib.uvs_camera_believed_loop_scenes_f64(C.byref(fp), *triple, *rest)
    else:
        rc = lib.uvs_camera_believed_loop_moving_f64(C.byref(fp), *triple, None if motion is None else motion.data_ptr(), *rest)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def assert_same_buffers(got, want, where):
    for key in want:
        assert np.array_equal(raw(got[key]), raw(want[key])), (where, key)


def trial_view(buf, key, T, n_points):
    """[..., T, comp] view of the live part of a flat buffer, so that a trial's entries can be picked."""
    comp = dict(q=6, dq=6, f=2 * n_points, err=2 * n_points, kappa=2 * n_points, stats=3, pixels=n_points, held=n_points, status=1, k_done=1)[key]
    rows = K if key in ('q', 'dq', 'f', 'err', 'kappa') else 1
    return buf[key][:rows * T * comp].reshape(rows, T, comp)


def loop_operands(uvs, T, n_points, scenario='painted', hold=2, seed=1):
    """Device operands of a C-ABI estimator launch: starts, noise, the nominal guess and the nominal detection as f0 (both sides of every
    comparison get the same), rectangles and paints per trial."""
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points, seed))
    nominal = scene_set(n_points)[0][0]
    f0 = uvs.engine.camera_features(nominal, q)
    x0 = uvs.engine.camera_guess(nominal, q, f0)
    kw = scenario_kw(scenario, T, n_points)
    occ = dev(kw['occluders'], np.int32) if 'occluders' in kw else None
    paint = dev(kw['occluder_colours'], np.int32) if 'occluder_colours' in kw else None
    return dict(q=q, noise=noise, x0=x0, f0=f0, occ=occ, paint=paint, hold=hold)


# ------------------------------------------------------------------------------------------------------------- 2: motion absent
@pytest.mark.parametrize('T', mc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_without_a_motion_the_loops_are_their_scenes_namesakes(uvs, method, n_points, T):
    """motion = NULL, a batch whose s(k) == 0 at every step, and NaN velocities whose k_on = K, through the C ABI on the same operands
    (rectangles, paints and a hold among them): every log row, stats, status, k_done, pixels, held and the poison past the last row."""
    _, _, cams = scene_set(n_points)
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    fp, op = params(uvs, method, n_points), loop_operands(uvs, T, n_points)
    want = c_estimator_loop(uvs, fp, T, n_points, camera, SCENES_CALL, **op)
    assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
    fa, believed = params(uvs, 'ANALYTICAL', n_points), (cams[:1], 1, None)
    want_b = c_baseline_loop(uvs, fa, T, n_points, camera, SCENES_CALL, believed, op['q'], op['noise'])
    for kind in (None, 'still', 'nan'):
        motion = None if kind is None else motions(T, n_points, kind)[2]
        assert_same_buffers(c_estimator_loop(uvs, fp, T, n_points, camera, motion, **op), want, (method, T, kind))
        assert_same_buffers(c_baseline_loop(uvs, fa, T, n_points, camera, motion, believed, op['q'], op['noise']), want_b, (T, kind, 'baseline'))


def test_none_is_the_call_without_the_arguments(uvs):
    plants = scene_set(4)[0]
    T = 5
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    none = dict(target_motion=None, motion_window=None)
    assert np.array_equal(bits(uvs.engine.camera_project(plants[1], q, **none)), bits(uvs.engine.camera_project(plants[1], q)))
    assert np.array_equal(bits(uvs.engine.camera_features(plants[1], q, **none)), bits(uvs.engine.camera_features(plants[1], q)))
    for method, fused in (('GMCKF', True), ('GMCKF', False), ('ANALYTICAL', True), ('ANALYTICAL', False)):
        fp = params(uvs, method, 4)
        kw = {} if method == 'ANALYTICAL' else dict(guess='device')
        plain = uvs.engine.camera_closed_loop(fp, plants[1], q, noise, fused=fused, **kw)
        cc.assert_same_bits(uvs.engine.camera_closed_loop(fp, plants[1], q, noise, fused=fused, **kw, **none), plain, K, (method, fused))
        vel, win, packed = motions(T, 4, 'nan')                      # and a motion that never starts, on the nominal camera as the one scene
        cc.assert_same_bits(uvs.engine.camera_closed_loop(fp, plants[1], q, noise, fused=fused, target_motion=packed, **kw), plain, K,
                            (method, fused, 'never starts'))


# ------------------------------------------------------------------------------------------------------------- 3: one launch, stepwise
@pytest.mark.parametrize('T', mc.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_the_one_launch_is_the_stepwise_loop(uvs, method, n_points, T):
    """The mixed motions on a mixed camera_index, under the four rectangle scenarios: every log, status, k_done, stats, pixels and held."""
    import torch
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    vel, win, packed = motions(T, n_points)
    plain = None
    for scenario in sc.SCENARIOS:
        kw = dict(scenario_kw(scenario, T, n_points), cameras=cams, camera_index=index, guess='device', believed=plants[0])
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, target_motion=packed, **kw)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, target_motion=vel, motion_window=win, **kw)
        cc.assert_same_bits(fused, stepwise, K, (method, n_points, T, scenario))
        assert ('held' in fused) == (scenario == 'held') == ('held' in stepwise)
        if scenario == 'held':
            assert torch.equal(fused['held'], stepwise['held'])
        if scenario == 'plain':
            plain = fused
            static = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
            rows = np.minimum(fused['k_done'].cpu().numpy() + 1, K)   # the rows of f that are specified
            same = [np.array_equal(bits(fused['f'])[:rows[t], t], bits(static['f'])[:rows[t], t]) for t in range(T)]
            assert same == [t % 4 in (0, 3) for t in range(T)], 'the moving trials differ from the static launch and the others do not'
    assert int(plain['k_done'].max()) == K


@pytest.mark.parametrize('method,n_points', BUILT)
def test_source_next_to_a_motion_is_gathered_by_output_trial(uvs, method, n_points):
    """trial_params with a 'source' permutation and per-trial kernel_bw and gain: two cells x the mixed motions over three input trials, one
    launch, against the stepwise loop of each cell on the gathered inputs with the motions -- and, under the four scenarios, the rectangles
    and paints -- of its OUTPUT trials."""
    import torch
    plants = scene_set(n_points)[0]
    T = 12
    cells = [(5.0, 0.1), (20.0, 0.3)]
    cell, source = np.arange(T) % 2, np.random.default_rng(4).permutation(np.arange(T) % 3).astype(np.int32)
    vel, win, _ = motions(T, n_points)
    q, noise = dev(sc.starts(3)), dev(sc.noise(3, n_points))
    tp = dict(source=source, kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    for scenario in sc.SCENARIOS:
        kw = scenario_kw(scenario, T, n_points)
        got = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, guess='device', trial_params=tp,
                                            target_motion=vel, motion_window=win, **kw)
        for i, (bw, gain) in enumerate(cells):
            sel = np.flatnonzero(cell == i)
            src = dev(source[sel], np.int64)
            mine = {key: (value[sel] if key in ('occluders', 'occluder_colours') else value) for key, value in kw.items()}
            want = uvs.engine.camera_closed_loop(params(uvs, method, n_points, kernel_bw=bw, gain=gain), plants[0], q[src].contiguous(),
                                                 noise[:, src].contiguous(), fused=False, guess='device', target_motion=vel[sel],
                                                 motion_window=win[sel], **mine)
            cc.assert_same_bits(got, want, K, (method, n_points, scenario, i), sel.tolist(), list(range(len(sel))))
            if scenario == 'held':
                assert torch.equal(got['held'][dev(sel, np.int64)], want['held'])


@pytest.mark.parametrize('T', mc.SIZES)
def test_the_motion_is_by_output_trial_next_to_source(uvs, T):
    """Through the C ABI, where `source` reaches the kernel: q_start, noise, x0 and f0 by source (two input trials), the motion -- like the
    rectangles and the scene -- by OUTPUT trial.  Trial t equals trial t of the launch with the same block in which every trial has t's motion."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    source, bw = dev((np.arange(T) // 3) % 2, np.int32), dev(np.where(np.arange(T) % 2, 5.0, 20.0))
    tp = uvs._vision.CameraTrialParams(bw.data_ptr(), None, None, None, None, source.data_ptr(), 2)
    op.update(q=op['q'][:2].contiguous(), noise=op['noise'][:, :2].contiguous(), x0=op['x0'][:2].contiguous(), f0=op['f0'][:2].contiguous())
    camera = (cams, 6, dev(sc.mixed_index(T, True), np.int32))
    got = c_estimator_loop(uvs, fp, T, 4, camera, motions(T, 4)[2], tp=tp, **op)
    for kind in range(4):
        want = c_estimator_loop(uvs, fp, T, 4, camera, motions(T, 4, kind)[2], tp=tp, **op)
        sel = np.arange(T) % 4 == kind
        for key in want:
            a, b = trial_view(got, key, T, 4), trial_view(want, key, T, 4)
            assert np.array_equal(raw(a)[:, sel], raw(b)[:, sel]), (T, kind, key)
        assert np.array_equal(raw(got['q'][K * T * 6:]), raw(want['q'][K * T * 6:]))


# ------------------------------------------------------------------------------------------------------------- 4: mixed against uniform
@pytest.mark.parametrize('T', mc.SIZES)
@pytest.mark.parametrize('method,n_points', [('GMCKF', 4), ('KF', 4), ('IMCCKF', 3), ('MCKF', 1)])
def test_a_mixed_batch_is_every_trial_on_its_own_motion(uvs, method, n_points, T):
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    kw = dict(cameras=cams, camera_index=sc.mixed_index(T, True), guess='device', believed=plants[0], fused=True)
    got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, target_motion=motions(T, n_points)[2], **kw)
    first = {}
    for kind in range(4):
        uniform = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, target_motion=motions(T, n_points, kind)[2], **kw)
        cc.assert_same_bits(got, uniform, K, (method, n_points, T, kind), [t for t in range(T) if t % 4 == kind])
        first[kind] = bits(uniform['f'])
    assert np.array_equal(first[0], first[3]) and not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])


# ------------------------------------------------------------------------------------------------------------- 5: the baseline
@pytest.mark.parametrize('T', mc.SIZES)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_baseline_one_launch_is_its_stepwise_loop(uvs, n_points, T):
    """ANALYTICAL on the mixed motions: the law on the nominal model and on the trials' own scenes, neither of which moves; the trials that
    never move keep the bits of the static launch, and the others do not."""
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    vel, win, packed = motions(T, n_points)
    for believed in (dict(believed=plants[0]), dict()):
        kw = dict(cameras=cams, camera_index=index, **believed)
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, target_motion=packed, **kw)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, target_motion=vel, motion_window=win, **kw)
        cc.assert_same_bits(fused, stepwise, K, (n_points, T, tuple(believed)))
        static = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
        quiet = [t for t in range(T) if t % 4 in (0, 3)]
        cc.assert_same_bits(fused, static, K, (n_points, T, 'the trials that never move'), quiet)
        assert not np.array_equal(bits(fused['dq'])[:, 1], bits(static['dq'])[:, 1]), 'the moving target shows in the command'
    alone = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, target_motion=packed)   # the nominal camera as the one scene
    step = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, target_motion=packed)
    cc.assert_same_bits(alone, step, K, (n_points, T, 'nominal'))


# ------------------------------------------------------------------------------------------------------------- 6: void and padding
VOID = (-1, sc.N_SCENES, INT32_MIN)


@pytest.mark.parametrize('T', mc.SIZES)
def test_a_void_trial_fails_alone_next_to_moving_neighbours(uvs, T):
    """A void scene index (both loops) and a void source (the estimators' loop): status FAIL, k_done = 0, nothing else stored, and the rest
    of the launch -- its moving workgroup neighbours among it -- keeps the bits of the valid launch.  At T = 259 the last trial moves, and
    the padding wavefront that shadows it stores nothing: the poison past every last row is compared too."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    motion = motions(T, 4)[2]
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2] if T > 3 else [1]                     # the trials next to a moving one (t % 4 in (1, 2)) among them
    source = np.arange(T, dtype=np.int32)
    tp_of = lambda s: uvs._vision.CameraTrialParams(None, None, None, None, None, s.data_ptr(), T)          # noqa: E731
    src = dev(source, np.int32)
    valid = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, **op)
    valid_s = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, tp=tp_of(src), **op)
    assert_same_buffers(valid_s, valid, 'the identity as source')
    valid_b = c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), motion, believed, op['q'], op['noise'])
    assert valid['k_done'][:T].max() == K and (T - 1) % 4 == 2, 'the last trial, which the padding wavefront shadows, moves'
    for turn in range(len(VOID)):
        holed, holed_source = index.copy(), source.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
            holed_source[t] = (-1, T, INT32_MIN)[(i + turn) % 3]
        hs = dev(holed_source, np.int32)
        for want, got in ((valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(holed, np.int32)), motion, **op)),
                          (valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), motion, tp=tp_of(hs), **op)),
                          (valid_b, c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(holed, np.int32)), motion, believed, op['q'], op['noise']))):
            want = {key: value.copy() for key, value in want.items()}
            for key in want:
                view = trial_view(want, key, T, 4)
                view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
            assert_same_buffers(got, want, (T, turn))


def test_a_void_trial_of_the_stand_alone_calls_is_left_unwritten(uvs):
    import torch
    plants, _, cams = scene_set(4)
    T = 259
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2]
    q = dev(sc.starts(T))
    packed = motions(T, 4)[2]
    outs = {}
    holed = index.copy()
    holed[where] = VOID
    for name, idx in (('valid', index), ('holed', holed)):
        d, f, d2 = (torch.full(shape, 7.0, dtype=torch.float64, device='cuda') for shape in ((T, 4, 3), (T, 8), (T, 4, 3)))
        pix, q_out = torch.full((T, 4), POISON, dtype=torch.int32, device='cuda'), torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda')
        uvs.engine.camera_project(plants[0], q, out=d, cameras=cams, camera_index=dev(idx, np.int32), target_motion=packed, k=7)
        uvs.engine.camera_features(plants[0], q, out=f, pixels=pix, discs=d2, q_out=q_out, cameras=cams, camera_index=dev(idx, np.int32),
                                   target_motion=packed, k=7)
        outs[name] = [t.cpu().numpy() for t in (d, f, d2, pix, q_out)]
    for a, b in zip(outs['valid'], outs['holed']):
        a = a.copy()
        a[where] = POISON if a.dtype == np.int32 else 7.0
        assert np.array_equal(raw(a), raw(b))


# ------------------------------------------------------------------------------------------------------------- 7: the CPU oracle
def against_the_oracle(out, ref, where, hold=False):
    out = {key: value.cpu().numpy() for key, value in out.items()}
    assert (out['status'][0], out['k_done'][0]) == (ref['status'], ref['k_done']), where
    assert np.array_equal(out['pixels'][0], ref['pixels']), (where, out['pixels'][0], ref['pixels'])
    if hold:
        assert out['held'][0].tolist() == [len(steps) for steps in ref['held']], (where, 'held')
    gates = {'err': pl.GATE, 'q': pl.GATE, 'f': pl.GATE, 'dq': pl.GATE_DQ, 'kappa': pl.GATE_KAPPA}
    for key, gate in gates.items():
        rows = len(ref[key])
        if rows == 0:
            continue
        d = float(np.abs(out[key][:rows, 0] - ref[key]).max() / np.abs(ref[key]).max())
        print(f'{where} {key}: {d:.2e}')
        assert d <= gate, (where, key, d)
    if ref['k_done']:
        d = float(np.abs(out['stats'][0] - ref['stats']).max() / np.abs(ref['stats']).max())
        assert d <= pl.GATE, (where, 'stats', d)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', sorted(mc.MOTIONS))
@pytest.mark.parametrize('method,n_points', mc.ORACLE)
def test_against_the_oracle(uvs, method, n_points, name, fused):
    """One trial on the nominal camera, the host's initial guess as the oracle makes it, against oracle.pixel_loop.run through its sensor=
    hook on plant.target_at."""
    ref, cfg = mc.oracle_trial(method, n_points, name), mc.oracle_settings(n_points)
    vel, window = mc.motion(name, n_points)
    fp = params(uvs, method, n_points, kernel_bw=cfg['kernel_bw'], gain=cfg['gain'])
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(n_points), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(n_points)[:, None]),
                                        radius=mc.RADIUS, fused=fused, target_motion=vel, motion_window=window)
    assert ref['k_done'] == K
    against_the_oracle(out, ref, f'{method} ({2 * n_points},6) {name} {"one launch" if fused else "stepwise"}')


@pytest.mark.parametrize('fused', [True, False])
def test_against_the_oracle_behind_the_bar_with_a_hold(uvs, fused):
    rows = tuple(tuple(int(v) for v in row) for row in pl.bar_rows(4))
    ref = mc.oracle_trial('GMCKF', 4, 'window', False, rows, 2)
    vel, window = mc.motion('window', 4)
    out = uvs.engine.camera_closed_loop(params(uvs, 'GMCKF', 4), pl.plant_of(4), dev(mc.oracle_start()[None]), dev(mc.oracle_noise(4)[:, None]),
                                        radius=mc.RADIUS, fused=fused, target_motion=vel, motion_window=window, occluders=np.array(rows), hold=2)
    against_the_oracle(out, ref, f'GMCKF (8,6) window behind the bar {"one launch" if fused else "stepwise"}', hold=True)
