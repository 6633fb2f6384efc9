"""The edge scenes of camera_common through a DESIGNED CAMERA: a plant whose discs at Q_GOAL are the scene (camera_common.scene_plant), so
that a disc cut by the frame edge, discs that overlap, a disc wholly under a later one, a disc that fills the frame, an r = 0 point, a
point behind the camera and a point that grazes the focal plane ('grazing': r of some 1e7 px) pass through the fused kernel
(uvs_camera_features_f64) and through the detection loops the three one-launch closed loops carry themselves (camera_loop_kernel,
camera_analytical_loop_kernel, camera_believed_loop_kernel), in both of their forms: up to 256 trials four wavefronts split one trial's
colours, beyond that one wavefront takes a whole trial.  Trial 0 of every batch is Q_GOAL exactly, the others Q_GOAL plus the seeded
jitter of camera_common.scene_joints (chosen on the CPU: tests/test_camera_host.py).

Gates.  Every comparison is of bits or bytes: the fused kernel against real frames (device rasteriser, frame detector) and the device
rasteriser against plant.render_discs on the same disc bits; the one-launch loops against the stepwise loop, and every logged feature
row against the frame detector on the frames of the logged joints.  The one tolerance is the suite's 1e-10 px projection gate of
tests/test_gpu_camera.py, which is stated for values of about 1e3 px at the goal's depth of 0.73 m: it allows the camera-frame depth an
error of 1e-10 / 1e3 * 0.73 = 7e-14 m, and that same allowance at the grazing point's depth of 1e-6 m is 7e-8 of its u, v and r."""
import os

import numpy as np
import pytest

import camera_common as cc

pytestmark = pytest.mark.gpu

DT, K = 0.05, 3
SMALL = 256                                                         # up to SMALL trials: the four wavefronts of a workgroup share one trial
SIZES = (3, SMALL + 3)
FRAMED = 8                                                          # trials per batch that are held to real frames
SCENES = cc.camera_scene_names()
LOOPS = ('GMCKF', 'ANALYTICAL', 'BELIEVED')
bits = cc.bits


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SETUPS = {}


def setup(uvs, name):
    """Everything of one scene that its tests share, computed once and left as it is: the plant, the SIZES[-1] start poses, and what the
    fused kernel returns for them without noise."""
    import torch
    if name not in _SETUPS:
        n, plant, radius = cc.camera_scene(uvs, name)
        T = SIZES[-1]
        q = dev(cc.scene_joints(T, name))
        discs = torch.full((T, n, 3), 7.0, dtype=torch.float64, device='cuda')
        pixels = torch.full((T, n), -7, dtype=torch.int32, device='cuda')
        f = uvs.engine.camera_features(plant, q, radius=radius, discs=discs, pixels=pixels)
        f0 = f[0].cpu().numpy()
        desired = np.where(np.isnan(f0), 128.0, f0)                 # the goal: what the scene shows (the frame's centre for an empty mask)
        _SETUPS[name] = dict(n=n, plant=plant, radius=radius, q=q, discs=discs, pixels=pixels, f=f, desired=desired,
                             believed=uvs.engine.believed_models(uvs.plant.miscalibrated(plant, focal_scale=1.05, joint_offset=0.01), radius))
    return _SETUPS[name]


def own_colours(counts, n):
    """Columns of camera_common.host_counts (red, green, blue, pink) that n_colours = n shows."""
    return {4: counts, 3: counts[..., :3], 1: counts[..., 1:2]}[n]


def solo_count(uvs, disc):
    """Mask size of one disc alone in the frame."""
    return int(cc.host_counts(uvs.plant.render_discs(cc.pad([disc])))[0])


# ------------------------------------------------------------------------------------------------------------- 1, 4: the anchor
@pytest.mark.parametrize('name', SCENES)
def test_fused_kernel_against_real_frames(uvs, name):
    """uvs_camera_features_f64 on the scene's camera: its features and mask sizes are those of the frame detector on the device
    rasteriser's frames of its own discs, and of the frame-free detector, for all 259 trials, with and without noise; for the first
    FRAMED trials the frames are plant.render_discs' byte for byte and the mask sizes those of the host frames.  Then the conditions under
    which the scene is the hard case its name says (from the host frames of trial 0's discs), and the variety of the batch."""
    import torch
    s = setup(uvs, name)
    n, plant, radius, q, D = s['n'], s['plant'], s['radius'], s['q'], s['discs']
    T = q.shape[0]
    frames = uvs.engine.render_discs(D, n)
    host = uvs.plant.render_discs(D[:FRAMED].cpu().numpy(), n)
    got = frames[:FRAMED].cpu().numpy()
    for t in range(FRAMED):
        assert np.array_equal(got[t], host[t]), f'trial {t}: {int(np.sum(got[t] != host[t]))} bytes differ from plant.render_discs'
    counts = own_colours(cc.host_counts(host), n)
    rng = np.random.default_rng(len(name))
    for noise in (None, dev(rng.standard_normal((T, 2 * n)) * 3.0)):
        pix = [torch.full((T, n), -7, dtype=torch.int32, device='cuda') for _ in range(3)]
        D_again = torch.full_like(D, 7.0)
        f = uvs.engine.camera_features(plant, q, radius=radius, noise=noise, discs=D_again, pixels=pix[0])
        f_frame = uvs.engine.detect_circles(frames, n, noise=noise, pixels=pix[1])
        f_free = uvs.engine.disc_features(D, n, noise=noise, pixels=pix[2])
        assert np.array_equal(bits(D_again), bits(D))
        assert np.array_equal(bits(f), bits(f_frame)), 'fused kernel against the frame detector'
        assert np.array_equal(bits(f), bits(f_free)), 'fused kernel against the frame-free detector'
        assert torch.equal(pix[0], pix[1]) and torch.equal(pix[0], pix[2])
        assert np.array_equal(pix[0][:FRAMED].cpu().numpy(), counts)
    assert torch.equal(s['pixels'], pix[0])
    # the projection gate
    q_host, D_host = q.cpu().numpy(), D.cpu().numpy()
    want = np.stack([plant.discs(x, radius) for x in q_host[:FRAMED]])
    gate = np.full(want.shape, 1e-10)
    if name == 'grazing':
        depth = plant.fkine_all(cc.Q_GOAL)[-1][2, 3]
        gate[:, 0] = np.maximum(1e-10, 1e-10 / 1e3 * depth / cc.GRAZING_PC[2] * np.abs(want[:, 0]))     # see the module's docstring
        gate[want[:, 0, 2] < 0, 0] = np.inf                         # a pose at which the point is behind the camera within that allowance
        assert np.isfinite(gate[0]).all() and 1e6 < D_host[0, 0, 2] < 1e8
    assert np.array_equal(D_host[:FRAMED][:, :, 2] < 0, want[:, :, 2] < 0) or name == 'grazing'
    assert np.all(np.abs(D_host[:FRAMED] - want) <= gate), np.abs(D_host[:FRAMED] - want).max()

    # ---- non-vacuity, from the host frames of trial 0's discs
    d0, c0 = D_host[0], counts[0]
    if name.startswith('clip_') or name == 'green_alone_clipped':
        cut = [j for j in range(n) if d0[j, 2] > 0 and (min(d0[j, 0], d0[j, 1]) - d0[j, 2] < 0 or max(d0[j, 0], d0[j, 1]) + d0[j, 2] > 255)]
        assert cut and 0 in cut
        for j in cut:
            assert 0 < c0[j] < solo_count(uvs, (128.0, 128.0, d0[j, 2])), (name, j)
    if name == 'covered':
        assert c0[0] == 0 and d0[0, 2] >= 0 and 0 <= d0[0, 0] <= 255 and 0 <= d0[0, 1] <= 255 and np.all(c0[1:] > 0)
    if 'overlap' in name:
        assert c0.sum() < sum(solo_count(uvs, d0[j]) for j in range(n) if d0[j, 2] >= 0)
    if name == 'whole_frame':
        assert c0.tolist() == [65536, 0, 0, 0]
    if name == 'whole_frame_under':
        assert c0.sum() == 65536 and np.all(c0 > 0)
    if name == 'outside':
        assert c0[:3].tolist() == [0, 0, 0] and c0[3] > 0
    if name == 'grazing':
        assert 0 < c0[0] < 65536 - c0[1:].sum() and np.all(c0[1:] > 0), 'the huge rim does not cross the frame'
    if name in cc.EMPTY_MASK:
        assert (c0 == 0).any()
    rows = {tuple(row) for row in s['pixels'].cpu().numpy().tolist()}
    print(f'{name}: trial 0 masks {c0.tolist()}, {len(rows)} distinct rows of mask sizes in {T} trials')
    if name not in cc.CONSTANT_COUNTS and name != 'point_on_lattice':
        assert len(rows) >= 3


# ------------------------------------------------------------------------------------------------------------- 2: the loops
def run_loop(uvs, s, loop, T, fused, noise):
    n = s['n']
    q0 = s['q'][:T].contiguous()
    method = loop if loop in ('GMCKF', 'KF') else 'ANALYTICAL'
    fp = uvs.engine.make_params(2 * n, 6, method, 10.0, False, DT, DT * (K + 0.5), 0.2, s['desired'], True)
    assert fp.steps == K
    if method == 'ANALYTICAL':
        kw = dict(believed=s['believed']) if loop == 'BELIEVED' else {}
        return uvs.engine.camera_closed_loop(fp, s['plant'], q0, noise, radius=s['radius'], fused=fused, **kw)
    x0 = uvs.engine.camera_guess(s['plant'], q0, s['f'][:T].contiguous(), radius=s['radius'])
    return uvs.engine.camera_closed_loop(fp, s['plant'], q0, noise, radius=s['radius'], x0=x0, fused=fused)


def assert_rows_are_the_frame_detectors(uvs, s, out, noise, where):
    """Every written feature row of the first FRAMED trials is what the frame detector returns for the device rasteriser's frame of the
    logged joints, plus the step's noise; and `pixels` is the smallest of those frames' masks."""
    import torch
    n = s['n']
    F = min(FRAMED, out['status'].shape[0])
    k_done = out['k_done'].cpu().numpy()[:F]
    smallest = np.full((F, n), np.iinfo(np.int32).max)
    for k in range(K):
        q_k = out['q'][k, :F].contiguous()
        pix = torch.full((F, n), -7, dtype=torch.int32, device='cuda')
        frames = uvs.engine.render_discs(uvs.engine.camera_project(s['plant'], q_k, radius=s['radius']), n)
        want = (uvs.engine.detect_circles(frames, n, pixels=pix) + noise[k, :F]).cpu().numpy()
        got, pix = out['f'][k, :F].cpu().numpy(), pix.cpu().numpy()
        for t in np.flatnonzero(k_done >= k):
            assert np.array_equal(np.isnan(got[t]), np.isnan(want[t])), (where, k, t, 'NaN pairs')
            finite = ~np.isnan(want[t])
            assert np.array_equal(bits(got[t][finite]), bits(want[t][finite])), (where, k, t)
            smallest[t] = np.minimum(smallest[t], pix[t])
    assert np.array_equal(out['pixels'][:F].cpu().numpy(), smallest), (where, 'pixels')


@pytest.mark.parametrize('T', SIZES)
@pytest.mark.parametrize('loop', LOOPS)
@pytest.mark.parametrize('name', SCENES)
def test_one_launch_loops_on_edge_scenes(uvs, name, loop, T):
    """The one launch has the bits of the stepwise loop, and -- independently of both -- its feature log and mask sizes are the frame
    detector's on real frames of its joint log."""
    import torch
    s = setup(uvs, name)
    noise = dev(np.random.default_rng(T + len(name)).standard_normal((K, T, 2 * s['n'])) * 0.5)
    fused = run_loop(uvs, s, loop, T, True, noise)
    stepwise = run_loop(uvs, s, loop, T, False, noise)
    torch.cuda.synchronize()
    cc.assert_same_bits(fused, stepwise, K, (name, loop, T))
    assert_rows_are_the_frame_detectors(uvs, s, fused, noise, (name, loop, T))
    assert np.array_equal(bits(fused['q'][0]), bits(s['q'][:T])), 'row 0 of the joint log is the start pose'


@pytest.mark.parametrize('T', SIZES)
def test_kf_loop_on_overlapping_discs(uvs, T):
    import torch
    s = setup(uvs, 'overlap_four')
    noise = dev(np.random.default_rng(T).standard_normal((K, T, 8)) * 0.5)
    fused, stepwise = (run_loop(uvs, s, 'KF', T, form, noise) for form in (True, False))
    torch.cuda.synchronize()
    assert fused['k_done'].tolist() == [K] * T, 'all four discs are in view: the loop runs'
    cc.assert_same_bits(fused, stepwise, K, ('overlap_four', 'KF', T))
    assert_rows_are_the_frame_detectors(uvs, s, fused, noise, ('overlap_four', 'KF', T))


# ------------------------------------------------------------------------------------------------------------- 3: FAIL at step 0
@pytest.mark.parametrize('T', SIZES)
@pytest.mark.parametrize('name', [name for name in SCENES if name in cc.EMPTY_MASK])
def test_an_empty_mask_fails_every_trial_at_step_0(uvs, name, T):
    """A colour without a pixel at the start pose -- covered, outside the frame, behind the camera -- is a NaN pair in the first feature
    row: every trial FAILs with k_done == 0 in all three loops, rows q_log[0] and f_log[0] are written, the NaN pairs sit exactly on the
    empty colours, and the statistics are the stepwise loop's."""
    import torch
    s = setup(uvs, name)
    n = s['n']
    empty = np.repeat(s['pixels'][:T].cpu().numpy() == 0, 2, axis=1)
    assert empty.any(axis=1).all(), 'the comparison would be vacuous'
    noise = dev(np.random.default_rng(T).standard_normal((K, T, 2 * n)) * 0.5)
    f_first = uvs.engine.camera_features(s['plant'], s['q'][:T].contiguous(), radius=s['radius'], noise=noise[0])
    for loop in LOOPS:
        fused = run_loop(uvs, s, loop, T, True, noise)
        stepwise = run_loop(uvs, s, loop, T, False, noise)
        torch.cuda.synchronize()
        assert fused['status'].tolist() == [1] * T and fused['k_done'].tolist() == [0] * T, loop
        assert np.array_equal(bits(fused['q'][0]), bits(s['q'][:T])), loop
        f_log = fused['f'][0].cpu().numpy()
        assert np.array_equal(np.isnan(f_log), empty), loop
        assert np.array_equal(bits(f_log[~empty]), bits(f_first.cpu().numpy()[~empty])), loop
        assert torch.equal(fused['pixels'], s['pixels'][:T]), loop
        assert np.array_equal(bits(fused['stats']), bits(stepwise['stats'])) and bool(torch.isfinite(fused['stats']).all()), loop
        cc.assert_same_bits(fused, stepwise, K, (name, loop, T))
