"""A SCENE PER TRIAL on the GPU (include/uvs_vision.h, "A SCENE PER TRIAL"; engine.*(cameras=, camera_index=)): the two stand-alone calls,
the estimators' one-launch loop (camera_scene_kernel, 22 instantiations) and the baseline's (scene_baseline_loop_kernel) over the scene set
of tests/camera_scenes_common.py -- six cameras that differ in every field the sensor side reads.  (tests/test_gpu_camera_scenes.py is an
older file about something else: edge scenes through one designed camera.)

Every comparison but the oracle's is of bits, and none leaves a trial out: trial t of a scene batch is trial t of the call that always was
(one host struct `cam`, the parent's kernels) on t's own camera; the one launch is the stepwise loop; a trial whose index names no scene
writes status FAIL and k_done = 0 and nothing else while its neighbours keep their bits.  The oracle (oracle/pixel_loop.py on the trial's
own plant and radius) is held to pixel_loop_common's gates: 1e-8 for err, q, f and stats, 1e-7 for the command, the integers exact.
Shapes: T = 3 (one trial per workgroup) and T = 259 (four per workgroup, two and more scenes in each, the last with a padding wavefront
next to a scene other than cams[0]); K = 16."""
import ctypes as C
import functools

import numpy as np
import pytest

import camera_common as cc
import camera_scenes_common as sc
import pixel_loop_common as pl

pytestmark = pytest.mark.gpu

K = sc.K
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


def params(uvs, method, n_points, steps=K, kernel_bw=pl.BW, gain=pl.GAIN):
    fp = uvs.engine.make_params(2 * n_points, 6, method, kernel_bw, False, pl.DT, pl.DT * (steps + 0.5), gain, pl.DESIRED[:2 * n_points], True, 0,
                                steps, pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX)
    assert fp.steps == steps
    fp.reg = pl.REG
    return fp


def nominal_guess(uvs, n_points, q):
    """The estimators' start in the bit-for-bit tests: the nominal model's analytic guess at the nominal camera's detection, for every trial."""
    nominal = scene_set(n_points)[0][0]
    return uvs.engine.camera_guess(nominal, q, uvs.engine.camera_features(nominal, q))


def scenario_kw(scenario, T, n_points):
    rows, paints, hold = sc.rectangles(scenario, n_points)
    kw = dict(hold=hold)
    if rows is not None:
        kw['occluders'] = np.broadcast_to(np.array(rows, np.int64), (T, len(rows), 8)).copy()
        kw['occluders'][1::2, 0, 6] += 2                             # every other trial: the first rectangle comes two steps later
    if paints is not None:
        kw['occluder_colours'] = np.broadcast_to(np.array(paints, np.int64), (T, len(paints))).copy()
    return kw


def per_trial(kw, sel):
    """The per-trial operands of kw for the trials sel."""
    return {key: (value[sel] if key in ('occluders', 'occluder_colours') else value) for key, value in kw.items()}


# ------------------------------------------------------------------------------------------------------------- 1: the stand-alone kernels
def index_forms(T, cams):
    """(name, cameras, camera_index, scene of every trial): NULL with n_cams = T, an explicit shuffled index, and a device index."""
    import torch
    mod, shuffled = sc.mixed_index(T), sc.mixed_index(T, True)
    return (('per trial', cams[torch.from_numpy(mod.astype(np.int64)).cuda()].contiguous(), None, mod), ('shuffled', cams, shuffled, shuffled),
            ('device index', cams, dev(mod, np.int32), mod))


@pytest.mark.parametrize('T', sc.SIZES)
def test_project_per_scene_is_the_call_per_camera(uvs, T):
    import torch
    plants, structs, cams = scene_set(4)
    q, dq = dev(sc.starts(T)), dev(np.random.default_rng(3).standard_normal((T, 6)) * 0.01)
    want = [uvs.engine.camera_project(s, q, dq, 0.05) for s in structs]
    for name, cameras, index, scene in index_forms(T, cams):
        q_out = torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda')
        got = uvs.engine.camera_project(plants[0], q, dq, 0.05, q_out=q_out, cameras=cameras, camera_index=index)
        for c in range(sc.N_SCENES):
            assert np.array_equal(bits(got)[scene == c], bits(want[c])[scene == c]), (name, c)
        assert np.array_equal(bits(q_out), bits(q + dq * 0.05))
    for c in range(sc.N_SCENES):                                     # NULL with n_cams = 1
        assert np.array_equal(bits(uvs.engine.camera_project(plants[0], q, dq, 0.05, cameras=cams[c:c + 1])), bits(want[c])), c


@pytest.mark.parametrize('rects', ['none', 'occluded', 'painted'])
@pytest.mark.parametrize('T', sc.SIZES)
def test_features_per_scene_are_the_frame_detectors(uvs, T, rects):
    """camera_features(cameras=), `pixels` included, against detect_circles of render_discs of the discs camera_project(cameras=) gives
    (held to the per-camera calls above), at steps 0, 1 and 11, without rectangles, with the sweeping bar and with the still distractor."""
    import torch
    plants, structs, cams = scene_set(4)
    q = dev(sc.starts(T))
    kw = per_trial(scenario_kw({'none': 'plain'}.get(rects, rects), T, 4), slice(None))
    kw.pop('hold')
    noise = dev(np.random.default_rng(5).standard_normal((T, 8)))
    for name, cameras, index, scene in index_forms(T, cams) + (('one', cams[4:5], None, np.full(T, 4)),):
        discs = uvs.engine.camera_project(plants[0], q, cameras=cameras, camera_index=index)
        for k in (0, 1, 11):
            frames = uvs.engine.render_discs(discs, 4, k=k, **kw)
            pix = [torch.full((T, 4), POISON, dtype=torch.int32, device='cuda') for _ in range(2)]
            want = uvs.engine.detect_circles(frames, 4, noise=noise, pixels=pix[0])
            d_out = torch.full((T, 4, 3), 7.0, dtype=torch.float64, device='cuda')
            got = uvs.engine.camera_features(plants[0], q, noise=noise, pixels=pix[1], discs=d_out, k=k, cameras=cameras, camera_index=index, **kw)
            assert np.array_equal(bits(got), bits(want)), (name, k)
            assert torch.equal(pix[0], pix[1]) and np.array_equal(bits(d_out), bits(discs)), (name, k)
            if name == 'shuffled' and k == 0 and rects == 'none':    # and the call per camera itself
                for c in range(sc.N_SCENES):
                    alone = uvs.engine.camera_features(structs[c], q, noise=noise)
                    assert np.array_equal(bits(got)[scene == c], bits(alone)[scene == c]), c


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


def c_estimator_loop(uvs, fp, T, n_points, camera, q, noise, x0, f0, tp=None, occ=None, paint=None, hold=0):
    """uvs_camera_closed_loop_scenes_f64 (camera = (cams tensor, n_cams, index tensor or None)) or uvs_camera_closed_loop_painted_f64
    (camera = a struct) on the same operands, into poisoned buffers; returns them on the host, tails included."""
    import torch
    buf = buffers(T, n_points)
    lib = uvs._vision.lib()
    middle = (T, None if tp is None else C.byref(tp), None if occ is None else occ.data_ptr(), None if paint is None else paint.data_ptr(),
              0 if occ is None else occ.shape[1], hold, q.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr())
    outs = tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels', 'held')) + (stream(),)
    if isinstance(camera, tuple):
        cams, n_cams, index = camera
        rc = lib.uvs_camera_closed_loop_scenes_f64(C.byref(fp), cams.data_ptr(), n_cams, None if index is None else index.data_ptr(), *middle, *outs)
    else:
        rc = lib.uvs_camera_closed_loop_painted_f64(C.byref(fp), C.byref(camera), *middle, *outs)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def c_baseline_loop(uvs, fp, T, n_points, camera, believed, q, noise):
    import torch
    buf = buffers(T, n_points, True)
    lib = uvs._vision.lib()
    b_models, b_n, b_index = believed
    rest = (b_models.data_ptr(), b_n, None if b_index is None else b_index.data_ptr(), q.data_ptr(), None if noise is None else noise.data_ptr()) + \
        tuple(buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')) + (stream(),)
    if isinstance(camera, tuple):
        cams, n_cams, index = camera
        rc = lib.uvs_camera_believed_loop_scenes_f64(C.byref(fp), cams.data_ptr(), n_cams, None if index is None else index.data_ptr(), T, *rest)
    else:
        rc = lib.uvs_camera_believed_loop_f64(C.byref(fp), C.byref(camera), T, *rest)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    return {key: value.cpu().numpy() for key, value in buf.items()}


def raw(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same_buffers(got, want, where):
    for key in want:
        assert np.array_equal(raw(got[key]), raw(want[key])), (where, key)


def trial_view(buf, key, T, n_points):
    """[..., T, comp] view of the live part of a flat buffer, so that a trial's entries can be picked."""
    comp = dict(q=6, dq=6, f=2 * n_points, err=2 * n_points, kappa=2 * n_points, stats=3, pixels=n_points, held=n_points, status=1, k_done=1)[key]
    rows = K if key in ('q', 'dq', 'f', 'err', 'kappa') else 1
    return buf[key][:rows * T * comp].reshape(rows, T, comp)


def loop_operands(uvs, T, n_points, scenario='painted', hold=2, seed=1):
    """Device operands of a C-ABI estimator launch: starts, noise, the nominal guess, f0 = zeros' stand-in (the nominal detection: both
    sides of every comparison get the same), rectangles and paints per trial."""
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points, seed))
    nominal = scene_set(n_points)[0][0]
    f0 = uvs.engine.camera_features(nominal, q)
    x0 = uvs.engine.camera_guess(nominal, q, f0)
    kw = scenario_kw(scenario, T, n_points)
    occ = dev(kw['occluders'], np.int32) if 'occluders' in kw else None
    paint = dev(kw['occluder_colours'], np.int32) if 'occluder_colours' in kw else None
    return dict(q=q, noise=noise, x0=x0, f0=f0, occ=occ, paint=paint, hold=hold)


# ------------------------------------------------------------------------------------------------------------- 2: uniform identity
@pytest.mark.parametrize('T', sc.SIZES)
@pytest.mark.parametrize('c', range(sc.N_SCENES))
def test_a_uniform_scene_batch_is_the_painted_launch(uvs, c, T):
    """Every trial on camera c, through the C ABI on the same operands (rectangles, paints and a hold among them): every log row, stats,
    status, k_done, pixels, held and the poison past the last row, bit for bit.  The same for the baseline's launch."""
    _, structs, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    want = c_estimator_loop(uvs, fp, T, 4, structs[c], **op)
    for camera in ((cams[c:c + 1], 1, None), (cams, 6, dev(np.full(T, c), np.int32))):
        assert_same_buffers(c_estimator_loop(uvs, fp, T, 4, camera, **op), want, (c, T, camera[1]))
    assert not (want['status'][:T] == POISON).any() and want['k_done'][:T].max() == K
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    want = c_baseline_loop(uvs, fa, T, 4, structs[c], believed, op['q'], op['noise'])
    for camera in ((cams[c:c + 1], 1, None), (cams, 6, dev(np.full(T, c), np.int32))):
        assert_same_buffers(c_baseline_loop(uvs, fa, T, 4, camera, believed, op['q'], op['noise']), want, (c, T, 'baseline'))


@pytest.mark.parametrize('T', sc.SIZES)
def test_the_scene_index_is_by_output_trial_next_to_source(uvs, T):
    """Through the C ABI, where `source` reaches the kernel: q_start, noise, x0 and f0 by source (two input trials), the scene -- like the
    rectangles -- by OUTPUT trial.  Trial t equals trial t of the painted launch with the same block on t's camera."""
    _, structs, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    source, bw = dev((np.arange(T) // 3) % 2, np.int32), dev(np.where(np.arange(T) % 2, 5.0, 20.0))
    tp = uvs._vision.CameraTrialParams(bw.data_ptr(), None, None, None, None, source.data_ptr(), 2)
    op.update(q=op['q'][:2].contiguous(), noise=op['noise'][:, :2].contiguous(), x0=op['x0'][:2].contiguous(), f0=op['f0'][:2].contiguous())
    index = sc.mixed_index(T, True)
    got = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), tp=tp, **op)
    for c in range(sc.N_SCENES):
        want = c_estimator_loop(uvs, fp, T, 4, structs[c], tp=tp, **op)
        for key in want:
            a, b = trial_view(got, key, T, 4), trial_view(want, key, T, 4)
            assert np.array_equal(raw(a)[:, index == c], raw(b)[:, index == c]), (T, c, key)


# ------------------------------------------------------------------------------------------------------------- 3: the mixed batch
@pytest.mark.parametrize('T', sc.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_a_mixed_batch_is_every_trial_on_its_own_camera(uvs, method, n_points, T):
    """camera_index = t % 6 and a shuffle of it: trial t of the one launch equals trial t of the launch that always was (one `cam`, the
    parent's kernel) on its camera, bit for bit, for every built estimator and shape."""
    plants, structs, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    x0 = nominal_guess(uvs, n_points, q)
    uniform = [uvs.engine.camera_closed_loop(fp, s, q, noise, x0=x0, fused=True) for s in structs]
    for shuffled in (False, True):
        index = sc.mixed_index(T, shuffled)
        assert shuffled is False or T < 6 or index[-1] != 0, 'the padding wavefront stands next to a scene other than cams[0]'
        got = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, x0=x0, fused=True, cameras=cams, camera_index=index)
        for c in range(sc.N_SCENES):
            sel = np.flatnonzero(index == c).tolist()
            if sel:
                cc.assert_same_bits(got, uniform[c], K, (method, n_points, T, shuffled, c), sel)
    if T > 6:
        done = np.stack([u['k_done'].cpu().numpy() for u in uniform])
        differ = sum(not np.array_equal(bits(uniform[0]['f'][0]), bits(u['f'][0])) for u in uniform[1:])
        assert differ == 5 and done.max() == K, 'the comparison would be vacuous'


# ------------------------------------------------------------------------------------------------------------- 4: one launch, stepwise
@pytest.mark.parametrize('T', sc.SIZES)
@pytest.mark.parametrize('method,n_points', BUILT)
def test_the_one_launch_is_the_stepwise_loop(uvs, method, n_points, T):
    plants, _, cams = scene_set(n_points)
    fp = params(uvs, method, n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    for scenario in sc.SCENARIOS:
        kw = dict(scenario_kw(scenario, T, n_points), cameras=cams, camera_index=index, guess='device', believed=plants[0])
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, **kw)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, **kw)
        cc.assert_same_bits(fused, stepwise, K, (method, n_points, T, scenario))
        assert ('held' in fused) == (scenario == 'held') == ('held' in stepwise)
        if scenario == 'held':
            import torch
            assert torch.equal(fused['held'], stepwise['held'])
            assert n_points == 1 or int(fused['held'].sum()) > 0, 'nothing was held'


@pytest.mark.parametrize('method,n_points', BUILT)
def test_source_next_to_scenes_is_gathered_by_output_trial(uvs, method, n_points):
    """trial_params with 'source': two cells (bandwidth, gain) x the six scenes over two input trials, one launch, against the stepwise loop
    of each cell on the gathered inputs."""
    plants, _, cams = scene_set(n_points)
    T = 12
    cells = [(5.0, 0.1), (20.0, 0.3)]
    cell, index, source = np.arange(T) % 2, (np.arange(T) // 2).astype(np.int32), ((np.arange(T) // 2) % 2).astype(np.int32)
    q, noise = dev(sc.starts(2)), dev(sc.noise(2, n_points))
    tp = dict(source=source, kernel_bw=dev([cells[i][0] for i in cell]), gain=dev([cells[i][1] for i in cell]))
    kw = dict(cameras=cams, guess='device')
    got = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=True, trial_params=tp, camera_index=index, **kw)
    for i, (bw, gain) in enumerate(cells):
        sel = np.flatnonzero(cell == i)
        src = dev(source[sel], np.int64)
        want = uvs.engine.camera_closed_loop(params(uvs, method, n_points, kernel_bw=bw, gain=gain), plants[0], q[src].contiguous(),
                                             noise[:, src].contiguous(), fused=False, camera_index=index[sel], **kw)
        cc.assert_same_bits(got, want, K, (method, n_points, i), sel.tolist(), list(range(len(sel))))


@pytest.mark.parametrize('T', sc.SIZES)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_baseline_one_launch_is_its_stepwise_loop(uvs, n_points, T):
    """ANALYTICAL, plain: the law on the nominal model and on the truth (every trial's own scene); and on the truth a uniform batch is the
    calibrated loop that always was."""
    plants, structs, cams = scene_set(n_points)
    fp = params(uvs, 'ANALYTICAL', n_points)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T, n_points))
    index = sc.mixed_index(T, True)
    for believed in (dict(believed=plants[0]), dict()):
        fused = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=True, cameras=cams, camera_index=index, **believed)
        stepwise = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, fused=False, cameras=cams, camera_index=index, **believed)
        cc.assert_same_bits(fused, stepwise, K, (n_points, T, tuple(believed)))
        for c in (1, 3):
            sel = np.flatnonzero(index == c).tolist()
            kw = dict(believed=plants[0]) if believed else {}
            alone = uvs.engine.camera_closed_loop(fp, structs[c], q, noise, fused=True, **kw)
            cc.assert_same_bits(fused, alone, K, (n_points, T, c, 'the call per camera'), sel)


# ------------------------------------------------------------------------------------------------------------- 5: the CPU oracle
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('method,n_points', sc.ORACLE)
def test_against_the_oracle_on_every_scene(uvs, method, n_points, fused):
    """T = 6, one trial per scene, each against oracle.pixel_loop.run on that scene's plant and radius."""
    plants, _, cams = scene_set(n_points)
    refs = [sc.oracle_trial(method, n_points, s) for s in range(sc.N_SCENES)]
    q = dev(np.stack([sc.oracle_start(s) for s in range(sc.N_SCENES)]))
    noise = dev(np.stack([sc.oracle_noise(s, n_points) for s in range(sc.N_SCENES)], axis=1))
    out = uvs.engine.camera_closed_loop(params(uvs, method, n_points), plants[0], q, noise, fused=fused, guess='device', cameras=cams)
    out = {key: value.cpu().numpy() for key, value in out.items()}
    gates = {'err': pl.GATE, 'q': pl.GATE, 'f': pl.GATE, 'dq': pl.GATE_DQ, 'kappa': pl.GATE_KAPPA}
    for s, ref in enumerate(refs):
        assert (out['status'][s], out['k_done'][s]) == (ref['status'], ref['k_done']) == (0, K), s
        assert np.array_equal(out['pixels'][s], ref['pixels']), (s, out['pixels'][s], ref['pixels'])
        for key, gate in gates.items():
            d = float(np.abs(out[key][:, s] - ref[key]).max() / np.abs(ref[key]).max())
            print(f'{method} ({2 * n_points},6) {"one launch" if fused else "stepwise"} scene {s} {key}: {d:.2e}')
            assert d <= gate, (s, key, d)
        d = float(np.abs(out['stats'][s] - ref['stats']).max() / np.abs(ref['stats']).max())
        assert d <= pl.GATE, (s, 'stats', d)


# ------------------------------------------------------------------------------------------------------------- 6: void trials
VOID = (-1, sc.N_SCENES, INT32_MIN)


def void_index(T):
    """A valid index, and the same with -1, n_cams and INT32_MIN written over three trials (T = 3: over one each, in turn)."""
    index = sc.mixed_index(T, True)
    where = [1, T // 2, T - 2] if T > 3 else [1]
    return index, where


@pytest.mark.parametrize('T', sc.SIZES)
def test_a_void_trial_fails_alone(uvs, T):
    """The documented total rule, on valid memory: status FAIL, k_done = 0, nothing else stored, and the rest of the launch -- its
    workgroup neighbours among it -- keeps the bits of the launch with a valid index."""
    _, _, cams = scene_set(4)
    fp, op = params(uvs, 'GMCKF', 4), loop_operands(uvs, T, 4)
    fa, believed = params(uvs, 'ANALYTICAL', 4), (cams[:1], 1, None)
    index, where = void_index(T)
    valid = c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(index, np.int32)), **op)
    valid_b = c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(index, np.int32)), believed, op['q'], op['noise'])
    for turn in range(len(VOID)):
        holed = index.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
        for want, got in ((valid, c_estimator_loop(uvs, fp, T, 4, (cams, 6, dev(holed, np.int32)), **op)),
                          (valid_b, c_baseline_loop(uvs, fa, T, 4, (cams, 6, dev(holed, np.int32)), believed, op['q'], op['noise']))):
            want = {key: value.copy() for key, value in want.items()}
            for key in want:
                view = trial_view(want, key, T, 4)
                view[:, where] = {'status': 1, 'k_done': 0}.get(key, POISON if view.dtype == np.int32 else np.nan)
            assert_same_buffers(got, want, (T, turn))


def test_a_void_trial_of_the_stand_alone_calls_is_left_unwritten(uvs):
    import torch
    plants, _, cams = scene_set(4)
    T = 259
    index, where = void_index(T)
    q = dev(sc.starts(T))
    for turn in range(len(VOID)):
        holed = index.copy()
        for i, t in enumerate(where):
            holed[t] = VOID[(i + turn) % len(VOID)]
        outs = {}
        for name, idx in (('valid', index), ('holed', holed)):
            d, f, d2 = (torch.full(shape, 7.0, dtype=torch.float64, device='cuda') for shape in ((T, 4, 3), (T, 8), (T, 4, 3)))
            pix, q_out = torch.full((T, 4), POISON, dtype=torch.int32, device='cuda'), torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda')
            uvs.engine.camera_project(plants[0], q, out=d, cameras=cams, camera_index=dev(idx, np.int32))
            uvs.engine.camera_features(plants[0], q, out=f, pixels=pix, discs=d2, q_out=q_out, cameras=cams, camera_index=dev(idx, np.int32))
            outs[name] = [t.cpu().numpy() for t in (d, f, d2, pix, q_out)]
        for a, b in zip(outs['valid'], outs['holed']):
            a = a.copy()
            a[where] = POISON if a.dtype == np.int32 else 7.0
            assert np.array_equal(raw(a), raw(b)), turn


# ------------------------------------------------------------------------------------------------------------- 7, 8: radii; cameras=None
def test_per_model_radii(uvs):
    """Scenes that differ in their radii alone, against the calls where `radius` is the only difference."""
    plants = scene_set(4)[0]
    radii = (0.02, 0.024, 0.03)
    T = 9
    cams = uvs.engine.camera_scenes([plants[0]] * 3, radii)
    index = (np.arange(T) % 3).astype(np.int32)
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    x0 = nominal_guess(uvs, 4, q)
    fp = params(uvs, 'GMCKF', 4)
    f = uvs.engine.camera_features(plants[0], q, cameras=cams, camera_index=index)
    d = uvs.engine.camera_project(plants[0], q, cameras=cams, camera_index=index)
    loop = uvs.engine.camera_closed_loop(fp, plants[0], q, noise, x0=x0, fused=True, cameras=cams, camera_index=index)
    for c, radius in enumerate(radii):
        sel = np.flatnonzero(index == c)
        assert np.array_equal(bits(f)[sel], bits(uvs.engine.camera_features(plants[0], q, radius=radius))[sel])
        assert np.array_equal(bits(d)[sel], bits(uvs.engine.camera_project(plants[0], q, radius=radius))[sel])
        cc.assert_same_bits(loop, uvs.engine.camera_closed_loop(fp, plants[0], q, noise, radius=radius, x0=x0, fused=True), K, radius, sel.tolist())
    assert len({tuple(row) for row in loop['pixels'][:3].cpu().numpy().tolist()}) == 3, 'the radii show in the masks'


def test_cameras_none_is_the_call_without_the_argument(uvs):
    plants = scene_set(4)[0]
    T = 5
    q, noise = dev(sc.starts(T)), dev(sc.noise(T))
    none = dict(cameras=None, camera_index=None)
    assert np.array_equal(bits(uvs.engine.camera_project(plants[1], q, **none)), bits(uvs.engine.camera_project(plants[1], q)))
    assert np.array_equal(bits(uvs.engine.camera_features(plants[1], q, **none)), bits(uvs.engine.camera_features(plants[1], q)))
    for method, fused in (('GMCKF', True), ('GMCKF', False), ('ANALYTICAL', True), ('ANALYTICAL', False)):
        fp = params(uvs, method, 4)
        kw = {} if method == 'ANALYTICAL' else dict(guess='device')
        cc.assert_same_bits(uvs.engine.camera_closed_loop(fp, plants[1], q, noise, fused=fused, **kw, **none),
                            uvs.engine.camera_closed_loop(fp, plants[1], q, noise, fused=fused, **kw), K, (method, fused))
