"""Occluders in the synthetic camera (include/uvs_vision.h: uvs_occluder): rectangles that slide in front of the discs.

The statement of the rule is plant.render_discs(discs, occluders=..., k=...) on the host.  The rasteriser is held to it byte for byte; the
frame-free detectors to detect_circles of those frames bit for bit; the one-launch loop (uvs_camera_closed_loop_occluded_f64) to the stepwise
loop bit for bit -- every specified log row, stats, status, k_done, pixels (camera_common.assert_same_bits) -- and, independently, its feature
rows to detect-of-render at its own logged joints.  Batch sizes come on both sides of 256 trials, where the loop kernel changes from one trial
per workgroup to four.  Only the host route (test 7) has a tolerance: the 1e-8 gate of tests/test_gpu_camera.py.

What each test catches was tried on the kernels with one-line mutations."""
import ctypes

import numpy as np
import pytest

import camera_common as cc
import camera_occluders_common as oc
import test_gpu_camera_grid as g

pytestmark = pytest.mark.gpu

uvs = g.uvs                                                          # the module fixture of tests/test_gpu_camera_grid.py
K, DT, DESIRED, SMALL = g.K, g.DT, g.DESIRED, g.SMALL
dev, bits, assert_same_bits = g.dev, cc.bits, cc.assert_same_bits
assert K == oc.K


def frames_of(uvs, discs, occ, k):
    """The statement: host frames of (T, n, 3) discs behind (T, n_occ, 8) occluders at step k, on the device for detect_circles."""
    import torch
    discs = discs.cpu().numpy() if hasattr(discs, 'cpu') else discs
    return torch.from_numpy(uvs.plant.render_discs(discs, discs.shape[1], occluders=occ, k=k)).cuda()


def detected(uvs, frames, n_colours=4, noise=None):
    import torch
    pixels = torch.zeros((frames.shape[0], n_colours), dtype=torch.int32, device='cuda')
    return uvs.engine.detect_circles(frames, n_colours, noise=noise, pixels=pixels), pixels


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------- 1: stand-alone kernels
@pytest.mark.parametrize('name', oc.STATIC_SCENES)
def test_stand_alone_kernels_are_detect_of_render(uvs, name):
    import torch
    eng = uvs.engine
    names, discs_h, occ = oc.static_batch(name)
    T, discs = len(names), dev(discs_h)
    noise = dev(np.random.default_rng(3).standard_normal((T, 8)) * 0.5)
    plant, radius = cc.scene_plant(uvs, discs_h[0])
    q = dev(cc.scene_joints(T, name))
    plain_f, plain_pix = detected(uvs, eng.render_discs(discs))
    moved = 0
    for k in oc.STEPS:
        want = frames_of(uvs, discs_h, occ, k)
        got = eng.render_discs(discs, occluders=occ, k=k)
        assert torch.equal(got, want), (name, k, 'frames')
        want_f, want_pix = detected(uvs, want)
        pix = torch.full((T, 4), -1, dtype=torch.int32, device='cuda')
        got_f = eng.disc_features(discs, occluders=occ, k=k, pixels=pix)
        assert same(got_f, want_f) and torch.equal(pix, want_pix), (name, k, 'disc_features')
        assert same(eng.disc_features(discs, noise=noise, occluders=occ, k=k), detected(uvs, want, noise=noise)[0]), (name, k, 'noise')
        moved += int((bits(got_f) != bits(plain_f)).any(axis=1).sum())
        # joints in: the projection's own discs, then the same statement
        seen, pix = torch.empty((T, 4, 3), dtype=torch.float64, device='cuda'), torch.full((T, 4), -1, dtype=torch.int32, device='cuda')
        cam_f = eng.camera_features(plant, q, radius=radius, noise=noise, occluders=occ, k=k, discs=seen, pixels=pix)
        assert same(seen, eng.camera_project(plant, q, radius=radius)), (name, k)
        cam_want, cam_pix = detected(uvs, frames_of(uvs, seen, occ, k), noise=noise)
        assert same(cam_f, cam_want) and torch.equal(pix, cam_pix), (name, k, 'camera_features')
        assert same(eng.camera_features(plant, q, radius=radius, occluders=occ, k=k), detected(uvs, frames_of(uvs, seen, occ, k))[0]), (name, k)
        if k == 0:
            i = names.index('red_entirely')
            assert want_pix[i, 0].item() == 0 and bool(torch.isnan(got_f[i, :2]).all()), 'a full cover is an empty mask and a NaN pair'
            if 'slack_column' in names:                              # meets the box, covers nothing: the bits of the unoccluded call
                i = names.index('slack_column')
                assert same(got_f[i], eng.disc_features(discs)[i]) and torch.equal(want_pix[i], plain_pix[i])
            if name == 'whole_frame':
                x0, x1, y0, y1 = uvs.plant.occluder_rects(occ[names.index('half')], 0)[0]
                assert want_pix[names.index('half'), 0].item() == 65536 - (x1 - x0 + 1) * (y1 - y0 + 1)
    assert moved >= 8, 'the comparison would be vacuous: the occluders move no feature'
    # memory kinds and a padded stride whose sentinel survives (k = 1, where the extremes are in the frame)
    want = frames_of(uvs, discs_h, occ, 1)
    pinned = torch.empty((T, 256, 256, 3), dtype=torch.uint8).pin_memory()
    eng.render_discs(discs, occluders=occ, k=1, out=pinned)
    torch.cuda.synchronize()
    assert torch.equal(pinned, want.cpu()), (name, 'pinned frames')
    wide = torch.full((T, cc.DENSE + 64), 0xAB, dtype=torch.uint8, device='cuda')
    eng.render_discs(discs, occluders=occ, k=1, out=wide[:, :cc.DENSE].view(T, 256, 256, 3))
    assert torch.equal(wide[:, :cc.DENSE].reshape(T, 256, 256, 3), want) and bool((wide[:, cc.DENSE:] == 0xAB).all()), (name, 'padded stride')
    packed = eng.occluders(occ, T)                                   # a packed operand, on the device and pinned
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (T, 4, 8)
    for operand in (packed, packed.cpu().pin_memory()):
        assert same(eng.disc_features(discs, occluders=operand, k=1), detected(uvs, want)[0])
    # n_occ = 1 (each set's first rectangle) and n_occ = 0 (the existing entry points' bits, through each new one)
    one = frames_of(uvs, discs_h, occ[:, :1], 1)
    assert torch.equal(eng.render_discs(discs, occluders=occ[:, :1], k=1), one)
    assert same(eng.disc_features(discs, occluders=occ[:, :1], k=1), detected(uvs, one)[0])
    none = occ[:, :0]
    assert torch.equal(eng.render_discs(discs, occluders=none, k=1, shade=7), eng.render_discs(discs))
    pix0, pix1 = (torch.full((T, 4), -1, dtype=torch.int32, device='cuda') for _ in range(2))
    assert same(eng.disc_features(discs, noise=noise, occluders=none, k=1, pixels=pix0), eng.disc_features(discs, noise=noise, pixels=pix1))
    assert torch.equal(pix0, pix1)
    assert same(eng.camera_features(plant, q, radius=radius, occluders=none, k=3), eng.camera_features(plant, q, radius=radius))
    assert same(eng.disc_features(discs, occluders=[oc.NEVER] * 4, k=1), eng.disc_features(discs))


# ------------------------------------------------------------------------------------------------------------- the loops
def loop(uvs, fp, inp, fused=True, occluders=None, **kw):
    return uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=fused, occluders=occluders, **kw)


def occluders_for(T, rows):
    """(T, n_occ, 8): the same rows for every trial."""
    return np.broadcast_to(oc.padded(rows, len(rows)), (T, len(rows), 8)).copy()


def assert_features_are_detect_of_render(uvs, out, inp, occ, trials=8):
    """Every written feature row of the first trials: detect_circles(render_discs(camera_project(q_log[k]), occluders, k)) + noise[k]."""
    n_points = inp.m // 2
    t = min(trials, out['status'].shape[0])
    k_done = out['k_done'].cpu().numpy()
    smallest = np.full((t, n_points), 2 ** 31 - 1)
    for k in range(K):
        discs = uvs.engine.camera_project(inp.plant, out['q'][k, :t].contiguous())
        want, pix = detected(uvs, frames_of(uvs, discs, occ[:t], k), n_points, None if inp.noise is None else inp.noise[k, :t].contiguous())
        rows = [i for i in range(t) if k <= k_done[i]]
        assert np.array_equal(bits(out['f'][k, :t])[rows], bits(want)[rows]), ('detect of render', k)
        smallest[rows] = np.minimum(smallest[rows], pix.cpu().numpy()[rows])
    assert np.array_equal(out['pixels'][:t].cpu().numpy(), smallest), 'pixels is the smallest covered mask'


SCENARIOS = {'bar': lambda n_points: [oc.sweeping_bar()], 'half': lambda n_points: [oc.half_cover(DESIRED, 0 if n_points == 1 else 1)]}


@pytest.mark.parametrize('scenario', sorted(SCENARIOS))
@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('method,n_points', g.CASES)
def test_one_launch_has_the_bits_of_the_stepwise_loop(uvs, method, n_points, T, scenario):
    import torch
    fp = g.params(uvs, method, 2 * n_points)
    inp = g.Inputs(uvs, n_points, g.jittered(T, 11), seed=200 + n_points)
    occ = occluders_for(T, SCENARIOS[scenario](n_points))
    fused, stepwise = loop(uvs, fp, inp, True, occ), loop(uvs, fp, inp, False, occ)
    torch.cuda.synchronize()
    assert_same_bits(fused, stepwise, K, (method, n_points, T, scenario))
    assert_features_are_detect_of_render(uvs, fused, inp, occ)
    clear = loop(uvs, fp, inp, True)
    assert not same(fused['f'], clear['f']), 'the comparison would be vacuous: the occluders move no feature'
    assert (fused['k_done'] == K).sum().item() >= T // 2, 'the comparison would be vacuous: most trials FAIL'


# ------------------------------------------------------------------------------------------------------------- 3: the time window
@pytest.mark.parametrize('T', [3, SMALL + 3])
def test_an_occluder_acts_inside_its_time_window_only(uvs, T):
    """Per trial, a rectangle over the left half of green where the unoccluded launch sees it at step 4, active at steps 4, 5 and 6."""
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 12), seed=31)
    clear = loop(uvs, fp, inp)
    assert clear['k_done'].tolist() == [K] * T
    green = (clear['f'][4, :, 2:4] - inp.noise[4, :, 2:4]).cpu().numpy()
    occ = np.array([[oc.still(np.floor(u) - 14, np.floor(v) - 14, 15, 29)[:6] + (4, 7)] for u, v in green], np.int64)
    got = loop(uvs, fp, inp, occluders=occ)
    k_done = got['k_done'].cpu().numpy()
    assert (k_done >= 4).all()
    for key in cc.LOGS:
        assert same(got[key][:4], clear[key][:4]), (key, 'rows before the window')
    assert same(got['q'][4], clear['q'][4]), 'the joints of step 4 follow from step 3'
    assert (bits(got['f'][4, :, 2:4]) != bits(clear['f'][4, :, 2:4])).any(axis=1).all(), 'row 4 of f differs in every trial'
    assert_features_are_detect_of_render(uvs, got, inp, occ)
    assert (got['pixels'][:, 1] < clear['pixels'][:, 1]).all(), 'the smallest green mask is a covered one'
    assert_same_bits(got, loop(uvs, fp, inp, False, occ), K, ('window', T))


# ------------------------------------------------------------------------------------------------------------- 4: per trial
def test_occluded_and_unoccluded_trials_share_a_workgroup(uvs):
    T = SMALL + 3
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 13), seed=32)
    occ = occluders_for(T, [oc.sweeping_bar()])
    occ[1::2] = oc.NEVER                                             # odd trials: an occluder that never covers anything
    got, clear = loop(uvs, fp, inp, occluders=occ), loop(uvs, fp, inp)
    odd, even = list(range(1, T, 2)), list(range(0, T, 2))
    assert_same_bits(got, clear, K, 'unoccluded neighbours', trials=odd)
    assert (bits(got['f'])[:, even] != bits(clear['f'])[:, even]).any(axis=(0, 2)).all(), 'every occluded trial sees the bar'
    assert_same_bits(got, loop(uvs, fp, inp, occluders=occluders_for(T, [oc.sweeping_bar()])), K, 'occluded trials', trials=even)
    assert_features_are_detect_of_render(uvs, got, inp, occ)


@pytest.mark.parametrize('T,covered', [(3, 1), (SMALL + 3, SMALL + 1)])
def test_a_full_cover_fails_its_trial_alone(uvs, T, covered):
    """Red is covered completely from step 5 on (a 41 x 41 rectangle around where the unoccluded launch sees it at step 5): an empty mask,
    a NaN pair, FAIL at step 5 with rows 0 .. 5 of q and f written -- the documented meaning of full occlusion."""
    import torch
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 14), seed=33)
    clear = loop(uvs, fp, inp)
    u, v = (clear['f'][5, covered, :2] - inp.noise[5, covered, :2]).tolist()
    occ = occluders_for(T, [oc.NEVER])
    occ[covered, 0] = (int(u) - 20, int(v) - 20, 41, 41, 0, 0, 5, oc.INT32_MAX)
    got = loop(uvs, fp, inp, occluders=occ)
    assert got['status'][covered].item() == 1 and got['k_done'][covered].item() == 5 and got['pixels'][covered, 0].item() == 0
    assert same(got['q'][:6, covered], clear['q'][:6, covered]) and same(got['f'][:5, covered], clear['f'][:5, covered])
    assert bool(torch.isnan(got['f'][5, covered, :2]).all()) and bool(torch.isfinite(got['f'][5, covered, 2:]).all())
    others = [t for t in range(T) if t != covered]
    assert_same_bits(got, clear, K, 'the neighbours of the covered trial', trials=others)
    assert_same_bits(got, loop(uvs, fp, inp, False, occ), K, ('full cover, stepwise', T))


# ------------------------------------------------------------------------------------------------------------- 5: with trial_params
def cell_occluders(cell):
    """Cell c of the grid: the bar, starting 5 c columns further left, and a still cover of green in every other cell."""
    bar = list(oc.sweeping_bar())
    bar[0] -= 5 * cell
    return [tuple(bar), oc.half_cover(DESIRED) if cell % 2 else oc.NEVER]


@pytest.mark.parametrize('E', [1, 22])                               # T = 12: one trial per workgroup; T = 264: four, and 22 % 4 != 0 mixes cells
def test_a_grid_with_per_cell_occluders_has_the_bits_of_its_uniform_launches(uvs, E):
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(E, 7), seed=104)
    host = g.bandwidth_gain_grid(E)
    T = len(host['source'])
    occ = np.stack([oc.padded(cell_occluders(t // E), 2) for t in range(T)])
    tp = {key: dev(np.asarray(value, np.int32 if key == 'source' else np.float64)) for key, value in host.items()}
    got = loop(uvs, fp, inp, occluders=occ, trial_params=tp)
    assert got['status'].shape[0] == T
    seen = set()
    for cell in range(T // E):
        trials = list(range(cell * E, (cell + 1) * E))
        one = type(fp).from_buffer_copy(fp)
        one.kernel_bw, one.gain = host['kernel_bw'][trials[0]], host['gain'][trials[0]]
        want = loop(uvs, one, inp, occluders=occluders_for(E, cell_occluders(cell)))
        assert_same_bits(got, want, K, ('cell', cell), trials=trials, want_trials=list(range(E)))
        seen.add(bits(want['err']).tobytes())
    assert len(seen) == T // E, 'the comparison would be vacuous: two cells have the same errors'
    assert_features_are_detect_of_render(uvs, got, inp.only(host['source'][:8].tolist()), occ)


def test_a_null_block_is_the_empty_dict_and_the_kernel_reads_by_source(uvs):
    """Through the C ABI: tp = NULL against trial_params={}; and a source index next to occluders that start at step 1, so that f0 -- the
    step-0 detection, which the Python layer computes per output trial -- is the same for every copy of an input trial."""
    import torch
    E, T = 3, 7
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(E, 15), seed=34)
    cam = inp.plant.to_camera()
    f0 = uvs.engine.camera_features(inp.plant, inp.q0)

    def call(T, tp, occ):
        f64 = dict(dtype=torch.float64, device='cuda')
        log = {key: torch.zeros((K, T, comp), **f64) for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8), ('kappa', 8))}
        status, k_done = (torch.zeros(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.zeros((T, 3), **f64), torch.zeros((T, 4), dtype=torch.int32, device='cuda')
        packed = uvs.engine.occluders(occ, T)
        uvs._vision.check(uvs._vision.lib().uvs_camera_closed_loop_occluded_f64(
            ctypes.byref(fp), ctypes.byref(cam), T, None if tp is None else ctypes.byref(tp), packed.data_ptr(), packed.shape[1],
            inp.q0.data_ptr(), inp.noise.data_ptr(), inp.x0.data_ptr(), f0.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(),
            log['dq'].data_ptr(), log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), None))
        torch.cuda.synchronize()
        return dict(log, status=status, k_done=k_done, stats=stats, pixels=pixels)

    late = [oc.sweeping_bar(1)]
    occ = occluders_for(E, late)
    assert_same_bits(call(E, None, occ), loop(uvs, fp, inp, occluders=occ, trial_params={}), K, 'tp = NULL')
    source_host = np.arange(T) % E
    source = dev(source_host.astype(np.int32))
    tp = uvs._vision.CameraTrialParams(None, None, None, None, None, source.data_ptr(), E)
    occ = occluders_for(T, late)
    occ[3:] = oc.NEVER
    want = loop(uvs, fp, inp, occluders=occ, trial_params={'source': source_host})
    assert_same_bits(call(T, tp, occ), want, K, 'source in the kernel')
    assert not same(want['f'][:, 0], want['f'][:, 3]), 'trials 0 and 3 share an input trial and differ by the bar'


# ------------------------------------------------------------------------------------------------------------- 6: stepwise baselines
@pytest.mark.parametrize('believed', [False, True])
def test_the_stepwise_baselines_see_the_occluders(uvs, believed):
    T = 5
    fp = g.params(uvs, 'ANALYTICAL')
    inp = g.Inputs(uvs, 4, g.jittered(T, 16), seed=35)
    occ = occluders_for(T, [oc.sweeping_bar()])
    kw = dict(believed=uvs.plant.miscalibrated(inp.plant, focal_scale=1.05)) if believed else {}
    run = lambda **more: uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, **kw, **more)   # noqa: E731
    got, clear = run(occluders=occ), run()
    assert_features_are_detect_of_render(uvs, got, inp, occ)
    assert not same(got['f'], clear['f']) and got['k_done'].tolist() == [K] * T
    assert_same_bits(run(occluders=occ[:, :0]), clear, K, 'no occluder')
    with pytest.raises(ValueError, match='fused=False'):
        run(occluders=occ, fused=True)


# ------------------------------------------------------------------------------------------------------------- 7: the host route
def test_loop_against_the_host_route_behind_the_bar(uvs):
    """Two trials of Experiment(robot=CameraRobot(occluders=bar)) under both perceptions against the one launch: the 1e-8 gate of
    tests/test_gpu_camera.py, exact status and k_done."""
    import test_gpu_camera as tg
    T = 2
    plant = uvs.SyntheticPlant.ur10()
    noise = np.random.default_rng(21).standard_normal((K, T, 8)) * 0.3
    bar = [oc.sweeping_bar()]
    fp = g.params(uvs, 'GMCKF')
    out = uvs.engine.camera_closed_loop(fp, plant, dev(g.Q_HOST_ROUTE), dev(noise), fused=True, occluders=bar)
    clear = uvs.engine.camera_closed_loop(fp, plant, dev(g.Q_HOST_ROUTE), dev(noise), fused=True)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0] and not same(out['f'], clear['f'])
    for t in range(T):
        for perception in ('host', 'device'):
            robot = uvs.CameraRobot(plant, dt=DT, occluders=bar)
            status, t_log, err, q_log, f_log = tg.host_route(uvs, plant, g.Q_HOST_ROUTE[t], noise[:, t], K, perception, robot)[:5]
            assert status == uvs.ExperimentStatus.SUCCESS and len(t_log) == K == out['k_done'][t].item(), (t, perception)
            for name, dev_log, host_log in (('err', out['err'], err), ('q', out['q'], q_log), ('f', out['f'], f_log)):
                rel = tg.rel(dev_log[:, t].cpu().numpy(), host_log)
                print(f'trial {t} {perception} {name}: rel {rel:.3e}')
                assert rel < 1e-8, (t, perception, name)
