"""Painted occluders -- distractors -- in the synthetic camera (include/uvs_vision.h: the paint operand): rectangles in
front of the discs that show a disc's colour and so ADD pixels to its mask.

The statement of the rule is plant.render_discs(discs, occluders=, k=, occluder_colours=) on the host (tests/test_camera_painted_host.py
holds it to a per-pixel restatement).  The rasteriser is held to it byte for byte; the frame-free detectors to detect_circles of those
frames bit for bit, mask sizes included; the one-launch loop (uvs_camera_closed_loop_painted_f64) to the stepwise loop bit for bit -- every
specified log row, stats, status, k_done, pixels (camera_common.assert_same_bits) and held -- and, independently, its feature rows to
detect-of-render at its own logged joints.  Batch sizes come on both sides of 256 trials, where the loop kernel changes from one trial per
workgroup to four.  Only the host route (the last test) has a tolerance: the 1e-8 gate of tests/test_gpu_camera.py.

What each test catches was tried on the kernels with one-line mutations (profiles/camera_painted.txt)."""
import ctypes

import numpy as np
import pytest

import camera_common as cc
import camera_hold_common as hc
import camera_occluders_common as oc
import camera_painted_common as pc
import test_gpu_camera_grid as g
import test_gpu_camera_occluders as go

pytestmark = pytest.mark.gpu

uvs = g.uvs                                                          # the module fixture of tests/test_gpu_camera_grid.py
K, DT, DESIRED, SMALL = g.K, g.DT, g.DESIRED, g.SMALL
dev, bits, assert_same_bits, same, detected = g.dev, cc.bits, cc.assert_same_bits, go.same, go.detected
assert K == pc.K
INT32_MIN = -2 ** 31


def frames_of(uvs, discs, occ, paints, k):
    """The statement: host frames of (T, n, 3) discs behind (T, n_occ, 8) occluders painted (T, n_occ) at step k, on the device."""
    import torch
    discs = discs.cpu().numpy() if hasattr(discs, 'cpu') else discs
    return torch.from_numpy(uvs.plant.render_discs(discs, discs.shape[1], occluders=occ, k=k, occluder_colours=paints)).cuda()


def device_paints(paints):
    """A packed paint operand as the C ABI takes it: int32 (T, n_occ) on the device, values written as they are."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(paints, dtype=np.int64).astype(np.int32)).cuda()


# ------------------------------------------------------------------------------------------------------------- 1, 2: stand-alone kernels
@pytest.mark.parametrize('name', sorted(pc.SCENES))
def test_stand_alone_kernels_are_detect_of_render(uvs, name):
    import torch
    eng = uvs.engine
    names, n, discs_h, occ, paints = pc.static_batch(name)
    T, discs = len(names), dev(discs_h)
    noise = dev(np.random.default_rng(3).standard_normal((T, 2 * n)) * 0.5)
    finite = bool(np.all(np.isfinite(discs_h)))
    if finite:
        plant, radius = cc.scene_plant(uvs, discs_h[0])
        q = dev(cc.scene_joints(T, name))
    opaque = np.full_like(paints, pc.OPAQUE)
    moved = 0
    for k in oc.STEPS:
        want = frames_of(uvs, discs_h, occ, paints, k)
        got = eng.render_discs(discs, n, occluders=occ, k=k, occluder_colours=paints)
        assert torch.equal(got, want), (name, k, 'frames')
        want_f, want_pix = detected(uvs, want, n)
        pix = torch.full((T, n), -1, dtype=torch.int32, device='cuda')
        got_f = eng.disc_features(discs, n, occluders=occ, k=k, pixels=pix, occluder_colours=paints)
        assert same(got_f, want_f) and torch.equal(pix, want_pix), (name, k, 'disc_features')
        assert same(eng.disc_features(discs, n, noise=noise, occluders=occ, k=k, occluder_colours=paints), detected(uvs, want, n, noise=noise)[0])
        moved += int((bits(got_f) != bits(eng.disc_features(discs, n, occluders=occ, k=k))).any(axis=1).sum())
        # all opaque, and no paint operand: the occluded namesakes' bits
        assert torch.equal(eng.render_discs(discs, n, occluders=occ, k=k, occluder_colours=opaque), eng.render_discs(discs, n, occluders=occ, k=k))
        assert same(eng.disc_features(discs, n, noise=noise, occluders=occ, k=k, occluder_colours=opaque),
                    eng.disc_features(discs, n, noise=noise, occluders=occ, k=k))
        if finite:                                                   # joints in: the projection's own discs, then the same statement
            seen, pix = torch.empty((T, n, 3), dtype=torch.float64, device='cuda'), torch.full((T, n), -1, dtype=torch.int32, device='cuda')
            cam_f = eng.camera_features(plant, q, radius=radius, noise=noise, occluders=occ, k=k, discs=seen, pixels=pix, occluder_colours=paints)
            assert same(seen, eng.camera_project(plant, q, radius=radius)), (name, k)
            cam_want, cam_pix = detected(uvs, frames_of(uvs, seen, occ, paints, k), n, noise=noise)
            assert same(cam_f, cam_want) and torch.equal(pix, cam_pix), (name, k, 'camera_features')
            assert same(eng.camera_features(plant, q, radius=radius, noise=noise, occluders=occ, k=k, occluder_colours=opaque),
                        eng.camera_features(plant, q, radius=radius, noise=noise, occluders=occ, k=k))
        if k == 0:
            c, _ = pc.target(discs_h[0])
            at = names.index
            assert want_pix[at('h_whole_frame'), c].item() == 65536 and int(want_pix[at('h_whole_frame')].sum()) == 65536
            lone = oc.still(77, 33, 1, 1)
            base = want_pix[at('all_opaque'), c].item() if name in ('not_drawn', 'outside', 'green_alone_absent') else None
            if base == 0:                                            # (e), (h): the disc draws nothing: the pair is the rectangle's centre
                assert want_pix[at('h_one_pixel'), c].item() == 1
                assert float((got_f[at('h_one_pixel'), 2 * c:2 * c + 2].cpu() - torch.tensor(lone[:2], dtype=torch.float64)).abs().max()) < 1e-11
            every = got_f[at('e_every_colour')]
            if name in ('not_drawn', 'outside', 'green_alone_absent', 'rgb_blue_absent'):
                assert bool(torch.isfinite(every).all()), '(e): a colour whose disc draws nothing has its distractor\'s finite pair'
    assert moved >= 8, 'the comparison would be vacuous: the paints move no feature'
    # (j): a paint of n_colours and of INT32_MIN written straight into device memory is opaque; the packed operand, on the device and pinned
    raw = paints.copy()
    raw[::2] = np.where(raw[::2] == pc.OPAQUE, n, raw[::2])
    raw[1::2] = np.where(raw[1::2] == pc.OPAQUE, INT32_MIN, raw[1::2])
    assert (raw == n).any() and (raw == INT32_MIN).any()
    want = frames_of(uvs, discs_h, occ, paints, 1)
    packed_occ = eng.occluders(occ, T)
    for operand in (device_paints(raw), device_paints(raw).cpu().pin_memory(), device_paints(paints)):
        assert torch.equal(eng.render_discs(discs, n, occluders=packed_occ, k=1, occluder_colours=operand), want), (name, '(j) frames')
        assert same(eng.disc_features(discs, n, occluders=packed_occ, k=1, occluder_colours=operand), detected(uvs, want, n)[0]), (name, '(j)')
    everything = np.full_like(paints, n)                             # and where every rectangle holds such a value: the occluded call
    everything[:, 1::2] = INT32_MIN
    assert same(eng.disc_features(discs, n, occluders=packed_occ, k=1, occluder_colours=device_paints(everything)),
                eng.disc_features(discs, n, occluders=packed_occ, k=1))
    # memory kinds and a padded stride whose sentinel survives (k = 1, where the extremes are in the frame)
    pinned = torch.empty((T, 256, 256, 3), dtype=torch.uint8).pin_memory()
    eng.render_discs(discs, n, occluders=occ, k=1, out=pinned, occluder_colours=paints)
    torch.cuda.synchronize()
    assert torch.equal(pinned, want.cpu()), (name, 'pinned frames')
    wide = torch.full((T, cc.DENSE + 64), 0xAB, dtype=torch.uint8, device='cuda')
    eng.render_discs(discs, n, occluders=occ, k=1, out=wide[:, :cc.DENSE].view(T, 256, 256, 3), occluder_colours=paints)
    assert torch.equal(wide[:, :cc.DENSE].reshape(T, 256, 256, 3), want) and bool((wide[:, cc.DENSE:] == 0xAB).all()), (name, 'padded stride')
    # n_occ = 1 (each set's first rectangle) and n_occ = 0 (the unoccluded entry points' bits, through each new one)
    one = frames_of(uvs, discs_h, occ[:, :1], paints[:, :1], 1)
    assert torch.equal(eng.render_discs(discs, n, occluders=occ[:, :1], k=1, occluder_colours=paints[:, :1]), one)
    assert same(eng.disc_features(discs, n, occluders=occ[:, :1], k=1, occluder_colours=paints[:, :1]), detected(uvs, one, n)[0])
    assert torch.equal(eng.render_discs(discs, n, occluders=occ[:, :0], k=1, occluder_colours=paints[:, :0]), eng.render_discs(discs, n))
    assert same(eng.disc_features(discs, n, noise=noise, occluders=occ[:, :0], k=1, occluder_colours=paints[:, :0]),
                eng.disc_features(discs, n, noise=noise))


# ------------------------------------------------------------------------------------------------------------- 3: the loops
def loop(uvs, fp, inp, fused=True, occluders=None, paints=None, **kw):
    return uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=fused, occluders=occluders, occluder_colours=paints, **kw)


def for_trials(T, rows, paints):
    """((T, n_occ, 8), (T, n_occ)): the same rows and paints for every trial."""
    return go.occluders_for(T, rows), np.broadcast_to(np.asarray(paints, np.int64), (T, len(paints))).copy()


def assert_same_held(got, want, where):
    assert ('held' in got) == ('held' in want), where
    if 'held' in got:
        assert np.array_equal(got['held'].cpu().numpy(), want['held'].cpu().numpy()), (where, 'held')


def assert_features_are_detect_of_render(uvs, out, inp, occ, paints, hold=0, trials=4):
    """Every written feature row of the first trials: detect_circles(render_discs(camera_project(q_log[k]), occluders, k, paints)) +
    noise[k], through plant.hold_features where the loop holds; pixels is the smallest mask of those frames."""
    n_points = inp.m // 2
    t = min(trials, out['status'].shape[0])
    k_done = out['k_done'].cpu().numpy()
    smallest = np.full((t, n_points), 2 ** 31 - 1)
    miss, reported = np.zeros((t, n_points), np.int32), None
    for k in range(K):
        discs = uvs.engine.camera_project(inp.plant, out['q'][k, :t].contiguous())
        want, pix = detected(uvs, frames_of(uvs, discs, occ[:t], paints[:t], k), n_points, None if inp.noise is None else inp.noise[k, :t].contiguous())
        want, pix = want.cpu().numpy(), pix.cpu().numpy()
        if hold:
            want, miss, _ = uvs.plant.hold_features(want, reported, pix, miss, hold)
            reported = want
        rows = [i for i in range(t) if k <= k_done[i]]
        assert np.array_equal(bits(out['f'][k, :t])[rows], bits(want)[rows]), ('detect of render', k)
        smallest[rows] = np.minimum(smallest[rows], pix[rows])
    assert np.array_equal(out['pixels'][:t].cpu().numpy(), smallest), 'pixels is the smallest mask, distractor pixels included'


def target_of(n_points):
    """(the disc the loops' paints aim at -- green --, its desired centre)."""
    j = 0 if n_points == 1 else 1
    return j, DESIRED[2 * j], DESIRED[2 * j + 1]


def scenario(name, n_points, T):
    """(occluders (T, n_occ, 8), paints (T, n_occ), hold) of one loop scenario."""
    j, u, v = target_of(n_points)
    if name == 'crossing_bar':                                       # a 4 x 30 bar of the target's colour that crosses its goal position at 1 px a step
        return for_trials(T, [(int(u) - 6, int(v) - 15, 4, 30, 1, 0) + oc.ALWAYS], [j]) + (0,)
    if name == 'still_distractor':                                   # in a block of columns and of rows that no disc touches
        return for_trials(T, *pc.still_distractor(j)) + (0,)
    if name == 'hold_with_distractor':                               # the wide opaque bar empties every disc in turn; the target's colour stays visible
        return for_trials(T, [hc.wide_bar()] + pc.still_distractor(j)[0], [pc.OPAQUE, j]) + (K,)
    if name == 'leaves':                                             # trial T // 2 leaves the frame (Q_LEAVES); its distractor, one pixel, remains
        return for_trials(T, *pc.still_distractor(j, w=1, h=1)) + (K,)
    if name == 'mixed_workgroup':                                    # consecutive trials: painted, opaque, no rectangle at all
        occ, paints = for_trials(T, [(int(u) - 6, int(v) - 15, 4, 30, 1, 0) + oc.ALWAYS, oc.half_cover(DESIRED, j)], [j, (j + 1) % n_points])
        paints[1::3] = pc.OPAQUE
        occ[2::3] = oc.NEVER
        return occ, paints, 0
    raise KeyError(name)


SCENARIOS = ('crossing_bar', 'still_distractor', 'hold_with_distractor', 'leaves', 'mixed_workgroup')


@pytest.mark.parametrize('name', SCENARIOS)
@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('method,n_points', g.CASES)
def test_one_launch_has_the_bits_of_the_stepwise_loop(uvs, method, n_points, T, name):
    import torch
    fp = g.params(uvs, method, 2 * n_points)
    q_host = g.jittered(T, 11)
    if name == 'leaves':
        q_host[T // 2] = g.Q_LEAVES
    inp = g.Inputs(uvs, n_points, q_host, seed=400 + n_points)
    if name == 'leaves':
        inp.noise[:, T // 2] = 0.0                                   # Q_LEAVES was found without noise
    occ, paints, hold = scenario(name, n_points, T)
    j = target_of(n_points)[0]
    fused, stepwise = loop(uvs, fp, inp, True, occ, paints, hold=hold), loop(uvs, fp, inp, False, occ, paints, hold=hold)
    torch.cuda.synchronize()
    where = (method, n_points, T, name)
    assert_same_bits(fused, stepwise, K, where)
    assert_same_held(fused, stepwise, where)
    assert ('held' in fused) == (hold > 0)
    check = [0, 1, 2, T // 2] if name == 'leaves' else list(range(4))
    check = sorted({t for t in check if t < T})
    assert_features_are_detect_of_render(uvs, {key: (v[:, check] if key in cc.LOGS else v[check]) for key, v in fused.items()},
                                         inp.only(check), occ[check], paints[check], hold)
    opaque = loop(uvs, fp, inp, True, occ, np.full_like(paints, pc.OPAQUE), hold=hold)
    assert not same(fused['f'], opaque['f']), 'the comparison would be vacuous: the paints move no feature'
    assert_same_bits(opaque, loop(uvs, fp, inp, True, occ, hold=hold), K, where + ('all opaque is the call without paints',))
    if name in ('hold_with_distractor', 'leaves'):
        held, rows = fused['held'].cpu().numpy(), fused['k_done'].cpu().numpy()
        assert not held[:, j].any(), 'a disc whose distractor is visible is never lost'
        assert (fused['pixels'][:, j] > 0).all()
        for t in range(T):                                           # and its pair is finite in every row that is due
            assert bool(torch.isfinite(fused['f'][:min(K, rows[t] + 1), t, 2 * j:2 * j + 2]).all()), (where, t)
        if name == 'hold_with_distractor':
            assert int(opaque['held'][:, j].sum()) > 0, 'without the paint the same disc is lost and held'
            short = loop(uvs, fp, inp, True, occ, np.full_like(paints, pc.OPAQUE), hold=1)
            assert (short['k_done'] < opaque['k_done']).any(), 'and with a hold that runs out it FAILs where the rule says'
            assert_same_bits(short, loop(uvs, fp, inp, False, occ, np.full_like(paints, pc.OPAQUE), hold=1), K, where + ('short hold',))
    if name == 'leaves' and (method, n_points) == ('GMCKF', 4):      # the case Q_LEAVES was found for
        gone = loop(uvs, fp, inp, True, hold=0)
        assert gone['k_done'][T // 2].item() < K and gone['pixels'][T // 2].min().item() == 0, 'the trial does leave the frame'
        assert opaque['held'][T // 2, j].item() > 0, 'without the paint green is lost there, and held'
        assert fused['pixels'][T // 2, j].item() == 1, 'with it the smallest green mask of that trial is the distractor alone'
    if name == 'mixed_workgroup':
        assert_same_bits(fused, loop(uvs, fp, inp, True), K, where + ('no rectangle',), trials=list(range(2, T, 3)))
        assert_same_bits(fused, opaque, K, where + ('opaque',), trials=list(range(1, T, 3)))
        differs = (bits(fused['f']) != bits(opaque['f'])).any(axis=(0, 2))
        assert differs[0::3].all() and not differs[1::3].any() and not differs[2::3].any()


@pytest.mark.parametrize('with_hold', [False, True])
def test_two_cells_behind_the_same_painted_bar_and_source_next_to_paints(uvs, with_hold):
    """kernel_bw per cell over the same input trials (source), paints per OUTPUT trial: every second output trial's bar is opaque."""
    E, hold = 3, (K if with_hold else 0)
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(E, 89), seed=90)
    bandwidths = (5.0, 20.0)
    T = E * len(bandwidths)
    source = np.arange(T) % E
    tp = dict(kernel_bw=dev(np.repeat(bandwidths, E)), source=dev(source.astype(np.int32)))
    occ, paints, _ = scenario('crossing_bar', 4, T)
    if with_hold:
        occ, paints, _ = scenario('hold_with_distractor', 4, T)
    paints[1::2] = pc.OPAQUE
    got = loop(uvs, fp, inp, True, occ, paints, trial_params=tp, hold=hold)
    assert got['status'].shape[0] == T and ('held' in got) == with_hold
    seen = set()
    for cell, bw in enumerate(bandwidths):
        one = type(fp).from_buffer_copy(fp)
        one.kernel_bw = bw
        trials = list(range(cell * E, (cell + 1) * E))
        want = loop(uvs, one, inp, True, occ[trials], paints[trials], hold=hold)
        assert_same_bits(got, want, K, ('cell', cell), trials=trials, want_trials=list(range(E)))
        if with_hold:
            assert np.array_equal(got['held'].cpu().numpy()[trials], want['held'].cpu().numpy())
        seen.add(bits(want['err']).tobytes())
    assert len(seen) == 2, 'the comparison would be vacuous: the two cells have the same errors'
    assert not same(got['f'][:, 0], got['f'][:, 3]), 'output trials 0 and 3 share an input trial and differ by their paints'
    assert_features_are_detect_of_render(uvs, got, inp.only(source[:4].tolist()), occ, paints, hold)


# ------------------------------------------------------------------------------------------------------------- 4: the C ABI
def c_abi(uvs, entry, fp, inp, T, occ, paint='absent', hold=0, spare=0):
    """uvs_camera_closed_loop_{held,painted}_f64 on buffers of T + spare trials filled with sentinels."""
    import torch
    cam = inp.plant.to_camera()
    n_points, rows = inp.m // 2, T + spare
    f0 = uvs.engine.camera_features(inp.plant, inp.q0, occluders=occ)
    f64 = dict(dtype=torch.float64, device='cuda')
    log = {key: torch.full((K, T, comp), -7.0, **f64) for key, comp in (('q', 6), ('f', inp.m), ('dq', 6), ('err', inp.m), ('kappa', inp.m))}
    status, k_done = (torch.full((rows,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    stats = torch.full((rows, 3), -7.0, **f64)
    pixels, held = (torch.full((rows, n_points), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    packed = uvs.engine.occluders(occ, T)
    head = (ctypes.byref(fp), ctypes.byref(cam), T, None, packed.data_ptr())
    tail = (inp.q0.data_ptr(), inp.noise.data_ptr(), inp.x0.data_ptr(), f0.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(),
            log['dq'].data_ptr(), log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), held.data_ptr(), None)
    lib = uvs._vision.lib()
    if entry == 'held':
        uvs._vision.check(lib.uvs_camera_closed_loop_held_f64(*head, packed.shape[1], hold, *tail))
    else:
        uvs._vision.check(lib.uvs_camera_closed_loop_painted_f64(*head, None if paint is None else paint.data_ptr(), packed.shape[1], hold, *tail))
    torch.cuda.synchronize()
    return dict(log, status=status[:T], k_done=k_done[:T], stats=stats[:T], pixels=pixels[:T], held=held[:T],
                spare=(status[T:], k_done[T:], stats[T:], pixels[T:], held[T:]))


@pytest.mark.parametrize('hold', [0, K])
@pytest.mark.parametrize('T', [3, SMALL + 3])
def test_a_null_paint_is_the_held_flavour(uvs, T, hold):
    """Through the C ABI, on the same operands, a batch in which masks are emptied: every byte, the sentinels of unwritten rows and of the
    rows past T - 1 included (T = 259: the last workgroup has a padding wavefront, which shadows trial T - 1 and stores nothing)."""
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 83), seed=84)
    occ = go.occluders_for(T, [hc.wide_bar(), oc.half_cover(DESIRED)])
    want = c_abi(uvs, 'held', fp, inp, T, occ, hold=hold)
    opaque = device_paints(np.full((T, 2), pc.OPAQUE))
    for paint in (None, opaque):
        got = c_abi(uvs, 'painted', fp, inp, T, occ, paint, hold=hold, spare=5)
        assert_same_bits(got, want, K, ('C ABI, paint = NULL', T, hold))
        for key in cc.LOGS + ('held',):
            assert np.array_equal(got[key].cpu().numpy().view(np.int64 if key != 'held' else np.int32),
                                  want[key].cpu().numpy().view(np.int64 if key != 'held' else np.int32)), (key, 'every byte')
        assert all(bool((t == -7).all()) for t in got['spare']), 'a padding trial stored something'
    assert (want['k_done'] < K).any() or int(want['held'].sum()) > 0, 'the comparison would be vacuous: no mask is emptied'


def test_the_stand_alone_entry_points_with_a_null_paint_are_their_occluded_namesakes(uvs):
    import torch
    lib = uvs._vision.lib()
    names, n, discs_h, occ_h, _ = pc.static_batch('overlap_four')
    T = len(names)
    discs, occ = dev(discs_h), uvs.engine.occluders(occ_h, T)
    plant, radius = cc.scene_plant(uvs, discs_h[0])
    cam, q = plant.to_camera(radius), dev(cc.scene_joints(T, 'overlap_four'))
    noise = dev(np.random.default_rng(5).standard_normal((T, 8)))
    for paint in (None, device_paints(np.full((T, 4), pc.OPAQUE))):
        p = None if paint is None else paint.data_ptr()
        frames = [torch.full((T + 1, cc.DENSE), 0xAB, dtype=torch.uint8, device='cuda') for _ in range(2)]
        uvs._vision.check(lib.uvs_render_discs_occluded_u8(T, discs.data_ptr(), 4, 96, occ.data_ptr(), 4, 1, 32, frames[0].data_ptr(), cc.DENSE, None))
        uvs._vision.check(lib.uvs_render_discs_painted_u8(T, discs.data_ptr(), 4, 96, occ.data_ptr(), p, 4, 1, 32, frames[1].data_ptr(), cc.DENSE, None))
        assert torch.equal(frames[0], frames[1]) and bool((frames[1][T] == 0xAB).all())
        f = [torch.full((T + 1, 8), -7.0, dtype=torch.float64, device='cuda') for _ in range(4)]
        pix = [torch.full((T + 1, 4), -7, dtype=torch.int32, device='cuda') for _ in range(4)]
        uvs._vision.check(lib.uvs_disc_features_occluded_f64(T, discs.data_ptr(), 4, occ.data_ptr(), 4, 1, noise.data_ptr(), f[0].data_ptr(),
                                                            pix[0].data_ptr(), None))
        uvs._vision.check(lib.uvs_disc_features_painted_f64(T, discs.data_ptr(), 4, occ.data_ptr(), p, 4, 1, noise.data_ptr(), f[1].data_ptr(),
                                                           pix[1].data_ptr(), None))
        uvs._vision.check(lib.uvs_camera_features_occluded_f64(ctypes.byref(cam), T, q.data_ptr(), None, 0.0, None, occ.data_ptr(), 4, 1,
                                                              noise.data_ptr(), f[2].data_ptr(), pix[2].data_ptr(), None, None))
        uvs._vision.check(lib.uvs_camera_features_painted_f64(ctypes.byref(cam), T, q.data_ptr(), None, 0.0, None, occ.data_ptr(), p, 4, 1,
                                                             noise.data_ptr(), f[3].data_ptr(), pix[3].data_ptr(), None, None))
        torch.cuda.synchronize()
        assert same(f[0], f[1]) and same(f[2], f[3]) and torch.equal(pix[0], pix[1]) and torch.equal(pix[2], pix[3])
        assert f[1][T].tolist() == [-7.0] * 8 and pix[3][T].tolist() == [-7] * 4
    assert not same(f[0][:T], uvs.engine.disc_features(discs, noise=noise)), 'the comparison would be vacuous: the occluders move no feature'


# ------------------------------------------------------------------------------------------------------------- 5: stepwise baselines
@pytest.mark.parametrize('believed', [False, True])
def test_the_stepwise_baselines_see_the_distractor(uvs, believed):
    """camera_closed_loop(ANALYTICAL, fused=False, occluder_colours=) against the loop written out: camera_project, plant.render_discs with
    the paints, detect_circles, the law -- every row of q, f, dq and err bit for bit."""
    import torch
    T = 5
    eng = uvs.engine
    fp = g.params(uvs, 'ANALYTICAL')
    inp = g.Inputs(uvs, 4, g.jittered(T, 16), seed=35)
    occ, paints, _ = scenario('still_distractor', 4, T)
    kw = dict(believed=uvs.plant.miscalibrated(inp.plant, focal_scale=1.05)) if believed else {}
    run = lambda **more: eng.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, **kw, **more)   # noqa: E731
    got, opaque = run(occluders=occ, occluder_colours=paints), run(occluders=occ)
    assert got['k_done'].tolist() == [K] * T and not same(got['f'], opaque['f'])
    q, dq = inp.q0, None
    for k in range(K):
        q_new = torch.empty_like(q)
        discs = eng.camera_project(inp.plant, q, dq, DT, q_out=q_new)
        f = eng.detect_circles(frames_of(uvs, discs, occ, paints, k), noise=inp.noise[k].contiguous())
        dq, err, status = eng.camera_analytical_step(inp.plant, q_new, f, fp, **kw)
        assert int(status.sum()) == 0
        for key, value in (('q', q_new), ('f', f), ('dq', dq), ('err', err)):
            assert same(got[key][k], value), (key, k)
        q, dq = q_new, dq.clone()
    assert_same_bits(run(occluders=occ, occluder_colours=np.full_like(paints, pc.OPAQUE)), opaque, K, 'all opaque')
    with pytest.raises(ValueError, match='fused=False'):
        run(occluders=occ, occluder_colours=paints, fused=True)


# ------------------------------------------------------------------------------------------------------------- 6: the host route
def test_loop_against_the_host_route_with_a_distractor(uvs):
    """Two trials of Experiment(robot=CameraRobot(occluder_colours=)) under both perceptions against the one launch: the 1e-8 gate of
    tests/test_gpu_camera.py, exact status and k_done."""
    import test_gpu_camera as tg
    T = 2
    plant = uvs.SyntheticPlant.ur10()
    noise = np.random.default_rng(21).standard_normal((K, T, 8)) * 0.3
    rows, paints = pc.still_distractor(1, w=3, h=3)                  # nine green pixels far from the disc: the pair moves by a pixel or two
    fp = g.params(uvs, 'GMCKF')
    out = uvs.engine.camera_closed_loop(fp, plant, dev(g.Q_HOST_ROUTE), dev(noise), fused=True, occluders=rows, occluder_colours=paints)
    opaque = uvs.engine.camera_closed_loop(fp, plant, dev(g.Q_HOST_ROUTE), dev(noise), fused=True, occluders=rows)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0] and not same(out['f'], opaque['f'])
    for t in range(T):
        for perception in ('host', 'device'):
            robot = uvs.CameraRobot(plant, dt=DT, occluders=rows, occluder_colours=paints)
            status, t_log, err, q_log, f_log = tg.host_route(uvs, plant, g.Q_HOST_ROUTE[t], noise[:, t], K, perception, robot)[:5]
            assert status == uvs.ExperimentStatus.SUCCESS and len(t_log) == K == out['k_done'][t].item(), (t, perception)
            for name, dev_log, host_log in (('err', out['err'], err), ('q', out['q'], q_log), ('f', out['f'], f_log)):
                rel = tg.rel(dev_log[:, t].cpu().numpy(), host_log)
                print(f'trial {t} {perception} {name}: rel {rel:.3e}')
                assert rel < 1e-8, (t, perception, name)
