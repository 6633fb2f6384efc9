"""The synthetic camera on the device (include/uvs_vision.h: uvs_camera_project_f64, uvs_render_discs_u8, uvs_disc_features_f64,
uvs_camera_features_f64; engine.camera_project / render_discs / disc_features / camera_features / camera_closed_loop; plant.CameraRobot)
against its host statements in plant.py (SyntheticPlant.discs, render_discs), against the frame detector, and against the host route of
Experiment.

Gates.  Projection: 1e-10 px absolute -- values of at most about 1e3, some 200 fp64 operations deep, device sincos within a few ulp of
libm: about 1e-11 by rounding analysis.  Rasteriser: every byte.  Frame-free detector and fused kernel: every bit.  The loop against its
parts: every bit.  The loop against the host route: 1e-8 relative, the project's closed-loop gate, with exact status, k_done and masks."""
import os

import numpy as np
import pytest

import camera_common as cc
from conftest import load_golden, rel_err as rel

pytestmark = pytest.mark.gpu

DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
DT = 0.05
# chosen on the CPU with the numpy oracle through pixels (oracle.rmckf_block.run_closed_loop fed utils.detect4Circles of plant.render_discs)
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
Q_LEAVES = np.array([-0.47915568, -0.55367504, 2.20583478, -0.05228325, -1.09351535, 0.40221985])     # all four discs out of view at step 6


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    uvs_amd.lib()
    uvs_amd._vision.lib()
    return uvs_amd


@pytest.fixture(scope='module')
def host_frames(uvs):
    """n_colours -> (names, discs (T, n, 3), plant.render_discs of them): computed once, shared, never changed."""
    out = {}
    for n, (names, discs) in cc.batches().items():
        frames = uvs.plant.render_discs(discs, n)
        frames.setflags(write=False)
        out[n] = (names, discs, frames)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """int64 view of an fp64 tensor / array on the host: equality of bits, NaN payloads included."""
    a = t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64)


def random_discs(rng, T, r_lo=4.0, r_hi=12.0):
    """Discs well inside the frame and apart from each other (the scenes of the detector tests)."""
    out = np.empty((T, 4, 3))
    for t in range(T):
        slots = rng.permutation(9)[:4]
        out[t] = [(64.0 * (s % 3) + 64 + rng.uniform(-12, 12), 64.0 * (s // 3) + 64 + rng.uniform(-12, 12), rng.uniform(r_lo, r_hi)) for s in slots]
    return out


# ------------------------------------------------------------------------------------------------------------- projection
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_projection(uvs, n_points):
    import torch
    rng = np.random.default_rng(40 + n_points)
    plant = uvs.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))
    T = 5
    q = cc.Q_GOAL + rng.uniform(-0.2, 0.2, (T, 6))
    dq = rng.standard_normal((T, 6)) * 0.5
    radius = [0.024, 0.02, 0.03, 0.018][:n_points]
    # without the update: q_out = q_prev
    q_out = torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda')
    discs = uvs.engine.camera_project(plant, dev(q), radius=radius, q_out=q_out).cpu().numpy()
    want = np.stack([plant.discs(x, radius) for x in q])
    print(f'projection, {n_points} points: max |diff| {np.abs(discs - want).max():.3e} px, u/v/r up to {np.abs(want).max():.0f}')
    assert discs.shape == (T, n_points, 3) and np.all(want[:, :, 2] > 0)
    assert np.abs(discs - want).max() < 1e-10
    assert np.array_equal(bits(q_out), bits(q))
    # with it: one rounded multiply, one rounded add
    q_new = q + dq * DT
    discs = uvs.engine.camera_project(plant, dev(q), dev(dq), DT, radius=radius, q_out=q_out).cpu().numpy()
    assert np.array_equal(bits(q_out), bits(q_new))
    assert np.abs(discs - np.stack([plant.discs(x, radius) for x in q_new])).max() < 1e-10
    # q_out is optional, and a pinned destination is written in place
    pinned = torch.zeros((T, n_points, 3), dtype=torch.float64).pin_memory()
    uvs.engine.camera_project(plant, dev(q), dev(dq), DT, radius=radius, out=pinned)
    torch.cuda.synchronize()
    assert np.array_equal(bits(pinned), bits(discs))
    with pytest.raises(uvs.UvsError) as exc:
        uvs.engine.camera_project(plant, q_out, q_out=q_out)
    assert exc.value.code == -1


def test_point_behind_the_camera_is_not_drawn(uvs):
    plant = uvs.SyntheticPlant.ur10()
    plant.points[2] = plant.fkine_all(cc.Q_GOAL)[-1][:3, 3] + np.array([0.01, 0.02, 0.3])      # above a camera that looks straight down
    q = np.stack([cc.Q_GOAL, cc.Q_GOAL + 0.01, np.full(6, np.nan)])
    discs = uvs.engine.camera_project(plant, dev(q)).cpu().numpy()
    assert np.all(discs[:2, 2, 2] == -1.0) and np.all(discs[:2, [0, 1, 3], 2] > 0)
    assert np.all(discs[2, :, 2] == -1.0), 'NaN joints: non-finite depth, nothing to draw'
    assert np.abs(discs[:2] - np.stack([plant.discs(x) for x in q[:2]])).max() < 1e-10
    f = uvs.engine.disc_features(dev(discs)).cpu().numpy()
    assert np.all(np.isnan(f[:2, 4:6])) and np.all(np.isfinite(f[:2, [0, 1, 2, 3, 6, 7]])) and np.all(np.isnan(f[2]))


# ------------------------------------------------------------------------------------------------------------- rasteriser, frame-free detector
@pytest.mark.parametrize('n_colours', [4, 3, 1])
def test_rasteriser_byte_for_byte_and_frame_free_detector_bit_for_bit(uvs, host_frames, n_colours):
    """Every scene of camera_common.edge_scenes in one batch per colour count: the device frames against plant.render_discs (same disc bits
    in, every byte compared), then uvs_disc_features_f64 against uvs_detect_circles_u8 on the device-rendered frames."""
    import torch
    names, discs, want = host_frames[n_colours]
    T = len(names)
    d = dev(discs)
    frames = uvs.engine.render_discs(d, n_colours)
    got = frames.cpu().numpy()
    for t, name in enumerate(names):
        assert np.array_equal(got[t], want[t]), f'{name}: {int(np.sum(got[t] != want[t]))} bytes differ'
    counts = cc.host_counts(want)
    counts = {4: counts, 3: counts[:, :3], 1: counts[:, 1:2]}[n_colours]
    rng = np.random.default_rng(n_colours)
    for noise in (None, dev(rng.standard_normal((T, 2 * n_colours)) * 3.0)):
        pix_frame, pix_free = (torch.full((T, n_colours), -7, dtype=torch.int32, device='cuda') for _ in range(2))
        f_frame = uvs.engine.detect_circles(frames, n_colours, noise=noise, pixels=pix_frame)
        f_free = uvs.engine.disc_features(d, n_colours, noise=noise, pixels=pix_free)
        assert f_free.shape == (T, 2 * n_colours)
        differ = [names[t] for t in range(T) if not np.array_equal(bits(f_free[t]), bits(f_frame[t]))]
        assert not differ, f'frame-free features differ from the frame detector in {differ}'
        assert np.array_equal(pix_free.cpu().numpy(), pix_frame.cpu().numpy()) and np.array_equal(pix_free.cpu().numpy(), counts)
    f = uvs.engine.disc_features(d, n_colours).cpu().numpy()
    empty = np.repeat(counts == 0, 2, axis=1)
    assert np.array_equal(np.isnan(f), empty) and empty.any(), 'an empty mask gives a NaN pair, nothing else does'
    print(f'n_colours={n_colours}: {T} scenes, {int(empty.sum()) // 2} empty masks, frames and features identical')
    if n_colours == 4:
        at = {name: t for t, name in enumerate(names)}
        assert counts[at['whole_frame']].tolist() == [65536, 0, 0, 0]
        assert counts[at['point_on_lattice']].tolist() == [1, 1, 1, 1] and counts[at['point_off_lattice']].tolist()[:2] == [0, 0]
        assert counts[at['r5_integer_centre']].tolist() == [81, 81, 0, 0] and counts[at['not_drawn']].tolist() == [0, 0, 0, 0]
        assert counts[at['covered']][0] == 0 and counts[at['outside']].tolist() == [0, 0, 0, 149]


def test_detection_is_within_half_a_pixel_of_the_centre(uvs):
    """Sanity bound (confirmed on the host mirror in tests/test_camera_host.py): unclipped, unoccluded discs with r >= 4."""
    discs = random_discs(np.random.default_rng(77), 5)
    f = uvs.engine.disc_features(dev(discs)).cpu().numpy().reshape(5, 4, 2)
    print(f'worst |detection - centre|: {np.abs(f - discs[:, :, :2]).max():.3f} px')
    assert np.abs(f - discs[:, :, :2]).max() < 0.5


@pytest.mark.parametrize('T', [1, 3, 5])
def test_batch_shapes_memory_kinds_and_padded_stride(uvs, T):
    import torch
    rng = np.random.default_rng(T)
    discs = random_discs(rng, T)
    discs[0, 0] = (253.0, 3.5, 9.0)                                                       # one clipped disc in every batch
    want = uvs.plant.render_discs(discs)
    d = dev(discs)
    hbm = uvs.engine.render_discs(d)
    assert hbm.shape == (T, 256, 256, 3) and hbm.dtype == torch.uint8 and np.array_equal(hbm.cpu().numpy(), want)
    pinned = torch.zeros((T, 256, 256, 3), dtype=torch.uint8).pin_memory()
    assert uvs.engine.render_discs(d, out=pinned) is pinned
    torch.cuda.synchronize()
    assert np.array_equal(pinned.numpy(), want)
    # discs read from pinned memory in place
    d_pinned = torch.from_numpy(discs).pin_memory()
    assert np.array_equal(uvs.engine.render_discs(d_pinned).cpu().numpy(), want)
    assert np.array_equal(bits(uvs.engine.disc_features(d_pinned)), bits(uvs.engine.disc_features(d)))
    # a padded batch: frame stride 196 608 + 64 B, the padding preset to a sentinel that must survive
    for make in (lambda n: torch.empty(n, dtype=torch.uint8, device='cuda'), lambda n: torch.empty(n, dtype=torch.uint8).pin_memory()):
        buf = make(T * (cc.DENSE + 64)).view(T, cc.DENSE + 64)
        buf[:] = 0xA5
        view = buf[:, :cc.DENSE].view(T, 256, 256, 3)
        assert T == 1 or view.stride(0) == cc.DENSE + 64
        uvs.engine.render_discs(d, out=view)
        torch.cuda.synchronize()
        assert np.array_equal(view.cpu().numpy(), want)
        assert bool((buf[:, cc.DENSE:] == 0xA5).all()), 'padding bytes were written'
        assert np.array_equal(bits(uvs.engine.detect_circles(view)), bits(uvs.engine.disc_features(d)))
    # another background; refusals reach Python as errors
    assert np.array_equal(uvs.engine.render_discs(d, background=0).cpu().numpy(), uvs.plant.render_discs(discs, background=0))
    with pytest.raises(uvs.UvsError) as exc:
        uvs.engine.render_discs(d, background=250)
    assert exc.value.code == -1
    with pytest.raises(ValueError):
        uvs.engine.render_discs(torch.from_numpy(discs))                                  # pageable host memory: no hidden copy
    with pytest.raises(ValueError):
        uvs.engine.disc_features(d, n_colours=3)                                          # four discs handed over as three


def test_frames_past_two_gib(uvs):
    """Frame offsets are 64-bit: a batch that spans 2^31 bytes; the first and the last frame are compared (the rest would take minutes
    on the host), and the frame-free detector against the frame detector over the whole batch."""
    import torch
    T = 10924
    assert (T - 2) * cc.DENSE < 1 << 31 < (T - 1) * cc.DENSE                              # the last frame starts past 2^31 bytes
    rng = np.random.default_rng(31)
    discs = np.tile(random_discs(rng, 4), (T // 4, 1, 1))
    discs[0], discs[-1] = random_discs(rng, 2)
    d = dev(discs)
    frames = torch.empty((T, 256, 256, 3), dtype=torch.uint8, device='cuda')
    frames[-1] = 0
    uvs.engine.render_discs(d, out=frames)
    assert np.array_equal(frames[0].cpu().numpy(), uvs.plant.render_discs(discs[0]))
    assert np.array_equal(frames[-1].cpu().numpy(), uvs.plant.render_discs(discs[-1]))
    pix_frame, pix_free = (torch.zeros((T, 4), dtype=torch.int32, device='cuda') for _ in range(2))
    f_frame = uvs.engine.detect_circles(frames, pixels=pix_frame)
    f_free = uvs.engine.disc_features(d, pixels=pix_free)
    assert bool(torch.isfinite(f_free).all()) and torch.equal(f_free.view(torch.int64), f_frame.view(torch.int64)) and torch.equal(pix_free, pix_frame)


# ------------------------------------------------------------------------------------------------------------- fused kernel
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_fused_kernel_is_projection_then_frame_free_detection(uvs, n_points):
    import torch
    rng = np.random.default_rng(60 + n_points)
    plant = uvs.SyntheticPlant.ur10(desired_f=tuple(DESIRED[:2 * n_points]))
    T, m = 5, 2 * n_points
    q = cc.Q_GOAL + rng.uniform(-0.05, 0.05, (T, 6))
    q[4] = cc.Q_GOAL + np.array([0.0, 0.0, 0.6, 0.0, 0.0, 0.0])                           # one trial looks away: NaN features
    dq, noise = dev(rng.standard_normal((T, 6)) * 0.5), dev(rng.standard_normal((T, m)))
    for with_dq in (False, True):
        for with_noise in (False, True):
            args = (dev(q), dq if with_dq else None, DT)
            q_a, q_b = (torch.full((T, 6), 7.0, dtype=torch.float64, device='cuda') for _ in range(2))
            pix_a, pix_b = (torch.full((T, n_points), -7, dtype=torch.int32, device='cuda') for _ in range(2))
            discs_a = uvs.engine.camera_project(plant, *args, q_out=q_a)
            f_a = uvs.engine.disc_features(discs_a, n_points, noise=noise if with_noise else None, pixels=pix_a)
            discs_b = torch.full((T, n_points, 3), 7.0, dtype=torch.float64, device='cuda')
            f_b = uvs.engine.camera_features(plant, *args, noise=noise if with_noise else None, q_out=q_b, pixels=pix_b, discs=discs_b)
            for name, a, b in (('q', q_a, q_b), ('discs', discs_a, discs_b), ('f', f_a, f_b)):
                assert np.array_equal(bits(a), bits(b)), (name, with_dq, with_noise)
            assert torch.equal(pix_a, pix_b)
            assert np.array_equal(bits(uvs.engine.camera_features(plant, *args, noise=noise if with_noise else None)), bits(f_a))   # outputs optional
    f = f_a.cpu().numpy()
    assert np.all(np.isfinite(f[:4])) and np.all(np.isnan(f[4])), 'the comparison would be vacuous'


# ------------------------------------------------------------------------------------------------------------- the loop
def params(uvs, method, K, initial_guess=True):
    return uvs.engine.make_params(8, 6, method, 10.0, False, DT, DT * (K + 0.5), 0.2, DESIRED, initial_guess)


def guesses(uvs, plant, q0, f0):
    x0 = np.empty((len(q0), 48))
    robot = uvs.SyntheticRobot(plant, DT)
    for t in range(len(q0)):
        robot.start(q0[t])
        x0[t] = uvs.plant.analytic_guess(robot, f0[t], (256, 256), 8, 6)
    return x0


@pytest.mark.parametrize('method', ['GMCKF', 'KF'])
def test_loop_is_its_parts(uvs, method):
    """camera_closed_loop against the same loop written out with the public pieces -- camera_project, render_discs, detect_circles,
    FilterBank.step -- through real frames: every log row bit for bit."""
    import torch
    T, K = 3, 12
    rng = np.random.default_rng(12)
    plant = uvs.SyntheticPlant.ur10()
    fp = params(uvs, method, K)
    assert fp.steps == K
    q0 = np.concatenate([Q_HOST_ROUTE, Q_HOST_ROUTE[:1] + rng.uniform(-0.05, 0.05, (1, 6))])
    noise = rng.standard_normal((K, T, 8)) * 0.5
    out = uvs.engine.camera_closed_loop(fp, plant, dev(q0), dev(noise))
    torch.cuda.synchronize()

    f0 = uvs.engine.detect_circles(uvs.engine.render_discs(uvs.engine.camera_project(plant, dev(q0))))
    x0 = guesses(uvs, plant, q0, f0.cpu().numpy())
    bank = uvs.engine.FilterBank(fp, T, x0)
    want = {key: [] for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'pixels')}
    q, f, dq, noise_d = dev(q0), f0, torch.zeros((T, 6), dtype=torch.float64, device='cuda'), dev(noise)
    for k in range(K):
        q_new = torch.empty_like(q)
        discs = uvs.engine.camera_project(plant, q, dq if k else None, DT, q_out=q_new)
        pixels = torch.zeros((T, 4), dtype=torch.int32, device='cuda')
        f_new = uvs.engine.detect_circles(uvs.engine.render_discs(discs), noise=noise_d[k], pixels=pixels)
        step = bank.step(f_new, f, dq, k)
        q, f, dq = q_new, f_new, step[0].clone()
        for key, value in zip(('q', 'f', 'dq', 'err', 'kappa', 'status', 'pixels'), (q, f, dq, step[1], step[2], step[3], pixels)):
            want[key].append(value.clone())
    want = {key: torch.stack(rows) for key, rows in want.items()}
    assert int(want['status'].sum()) == 0 and bool(torch.isfinite(want['err']).all())
    for key in ('q', 'f', 'dq', 'err', 'kappa'):
        assert tuple(out[key].shape) == (K, T, want[key].shape[2]) and out[key].is_contiguous()
        assert np.array_equal(bits(out[key]), bits(want[key])), key
    assert out['k_done'].tolist() == [K] * T and out['status'].tolist() == [0] * T
    assert torch.equal(out['pixels'], want['pixels'].amin(0)) and int(out['pixels'].min()) > 50
    t = uvs.engine.loop_clock(DT, DT * (K + 0.5))
    assert len(t) == K
    stats = uvs.engine.stats_reduce(want['err'].permute(1, 0, 2).contiguous(), t, out['k_done'], layout='tkc')
    assert np.array_equal(bits(out['stats']), bits(stats)) and bool((out['stats'] > 0).all())
    # an explicit x0 (and initial_guess off: f_old of the first step is zeros) goes the same way as FilterBank with set_features' default
    fp_off = params(uvs, method, 2, initial_guess=False)
    off = uvs.engine.camera_closed_loop(fp_off, plant, dev(q0), x0=x0)
    bank = uvs.engine.FilterBank(fp_off, T, x0)
    f_first = uvs.engine.camera_features(plant, dev(q0))
    step = bank.step(f_first, torch.zeros_like(f_first), torch.zeros((T, 6), dtype=torch.float64, device='cuda'), 0)
    assert np.array_equal(bits(off['f'][0]), bits(f_first)) and np.array_equal(bits(off['dq'][0]), bits(step[0]))
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp_off, plant, dev(q0))


class Replay:
    """A noise profile that hands out the rows of a recorded sequence (the duck-type of NoiseProfiler.getNoise)."""

    def __init__(self, rows):
        self.rows, self.i = rows, 0

    def getNoise(self):
        self.i += 1
        return self.rows[self.i - 1].copy()


def host_route(uvs, plant, q_start, noise, steps, perception='host', robot=None):
    g = load_golden('closed_gmckf_a1p5')
    ex = uvs.Experiment(q_start, DESIRED, None if noise is None else Replay(noise), DT, DT * (steps + 0.5), 0.2,
                        robot or uvs.CameraRobot(plant, dt=DT), uvs.Method.GMCKF, **g['meta']['params'], perception=perception)
    return ex.run()


def test_loop_against_the_host_route(uvs):
    """Each trial of one camera_closed_loop launch against Experiment(robot=CameraRobot, perception='host').run(): numpy rasteriser, numpy
    detector, the Python loop of the external-robot route."""
    T, K = 2, 20
    rng = np.random.default_rng(20)
    plant = uvs.SyntheticPlant.ur10()
    noise = rng.standard_normal((K, T, 8)) * 0.3
    fp = params(uvs, 'GMCKF', K)
    assert fp.steps == K and load_golden('closed_gmckf_a1p5')['meta']['params']['kernel_bw'] == 10
    out = uvs.engine.camera_closed_loop(fp, plant, dev(Q_HOST_ROUTE), dev(noise))
    # masks of every step, from the device's own joint log
    import torch
    pix_d = torch.zeros((K * T, 4), dtype=torch.int32, device='cuda')
    uvs.engine.camera_features(plant, out['q'].reshape(K * T, 6), pixels=pix_d)
    pixels = pix_d.cpu().numpy().reshape(K, T, 4)
    assert out['k_done'].tolist() == [K, K] and out['status'].tolist() == [0, 0]
    for t in range(T):
        status, t_log, err, q_log, f_log = host_route(uvs, plant, Q_HOST_ROUTE[t], noise[:, t], K)[:5]
        assert status == uvs.ExperimentStatus.SUCCESS and len(t_log) == K
        # the preconditions under which a 1e-10 px projection difference cannot flip a pixel, on the host trajectory
        discs = np.stack([plant.discs(q) for q in q_log])
        lo, hi = discs[:, :, :2] - discs[:, :, 2:], discs[:, :, :2] + discs[:, :, 2:]
        assert lo.min() > 0.0 and hi.max() < 255.0, 'a disc touches the edge of the frame'
        masks = np.stack([cc.host_counts(uvs.plant.render_discs(d)) for d in discs])
        assert masks.min() >= 50
        assert cc.closest_to_rim(discs) > 1e-6, "a pixel's d^2 comes within 1e-6 of r^2"
        for name, dev_log, host_log in (('err', out['err'], err), ('q', out['q'], q_log), ('f', out['f'], f_log)):
            got = dev_log[:, t].cpu().numpy()
            print(f'trial {t} {name}: rel {rel(got, host_log):.3e}')
            assert rel(got, host_log) < 1e-8, (t, name)
        assert np.array_equal(pixels[:, t], masks), 'mask sizes differ at some step'
        assert np.array_equal(out['pixels'][t].cpu().numpy(), masks.min(axis=0))


def test_leaving_the_frame_fails_that_trial_alone(uvs):
    """From Q_LEAVES the loop swings the camera away and all discs leave the view at step 6 (found on the CPU): NaN features, non-finite X,
    FAIL with k_done = that step -- where the reference's loop ends on the NaN detection.  The other trial of the launch runs as it runs alone."""
    import torch
    K = 12
    plant = uvs.SyntheticPlant.ur10()
    fp = params(uvs, 'GMCKF', K)
    q0 = np.stack([Q_HOST_ROUTE[0], Q_LEAVES])
    out = uvs.engine.camera_closed_loop(fp, plant, dev(q0))
    alone = uvs.engine.camera_closed_loop(fp, plant, dev(q0[:1]))
    assert out['status'].tolist() == [0, 1]
    k_fail = int(out['k_done'][1])
    assert out['k_done'].tolist() == [K, k_fail] and 0 < k_fail < K
    pix = torch.zeros((k_fail + 1, 4), dtype=torch.int32, device='cuda')
    f = uvs.engine.camera_features(plant, out['q'][:k_fail + 1, 1].contiguous(), pixels=pix).cpu().numpy()
    pix = pix.cpu().numpy()
    print(f'k_done {k_fail}; masks per step {pix.tolist()}')
    assert pix[:k_fail].min() > 0 and pix[k_fail].min() == 0, 'k_done is not the step at which a mask became empty'
    assert np.all(np.isfinite(f[:k_fail])) and np.any(np.isnan(f[k_fail]))
    assert np.array_equal(bits(out['f'][:k_fail + 1, 1]), bits(f)) and out['pixels'][1].min() == 0
    assert bool(torch.isfinite(out['err'][:k_fail, 1]).all()) and bool(torch.isfinite(out['stats']).all())
    for key in ('err', 'q', 'f', 'dq', 'kappa'):
        assert np.array_equal(bits(out[key][:, 0]), bits(alone[key][:, 0])), key
    assert np.array_equal(bits(out['stats'][0]), bits(alone['stats'][0])) and torch.equal(out['pixels'][0], alone['pixels'][0])
    # the host route ends the same trial at the same step
    with np.errstate(invalid='ignore'):                                                  # the host detector divides 0 by 0 there, like the reference
        status, t_log = host_route(uvs, plant, Q_LEAVES, None, K)[:2]
    assert status == uvs.ExperimentStatus.FAIL and len(t_log) == k_fail


def test_experiment_with_camera_robot_under_both_perceptions(uvs, monkeypatch):
    """The gates of test_experiment_with_device_perception (tests/test_gpu_detect.py), with the product's own camera-carrying robot."""
    calls = []
    step_image = uvs.engine.FilterBank.step_image
    monkeypatch.setattr(uvs.engine.FilterBank, 'step_image', lambda self, *a, **kw: (calls.append(1), step_image(self, *a, **kw))[1])
    plant = uvs.SyntheticPlant.ur10()
    g = load_golden('closed_gmckf_a1p5')

    def run(perception):
        del calls[:]
        return host_route(uvs, plant, g['q_start'], None, 20, perception), len(calls)

    host, n_host = run('host')
    device, n_dev = run('device')
    assert len(host[1]) == 20 and n_host == 0 and n_dev == 20, 'the device route did not go through step_image'
    assert np.all(np.isfinite(host[4])), 'a disc left the frame: the comparison would be vacuous'
    assert device[0] == host[0] == uvs.ExperimentStatus.SUCCESS and len(device[1]) == len(host[1])
    assert np.array_equal(device[1], host[1])
    same = int(np.sum(device[4] == host[4]))
    print(f'f_log: {"all" if same == host[4].size else same} of {host[4].size} values bit-equal between the perceptions')
    for i, name in ((2, 'err'), (3, 'q'), (4, 'f')):
        assert rel(device[i], host[i]) < 1e-8, name
