"""CPU-only tests of the synthetic camera: the entry points of include/uvs_vision.h refuse bad arguments before any HIP call (the buffers
here are host arrays no kernel could use), the host mirror of the pixel rule (plant.render_discs) against the oracle's rasteriser and,
through the host detectors, against the reference's own outputs, and the camera-carrying robot."""
import ctypes

import numpy as np
import pytest

import camera_common as cc
from oracle import plant_ref

ARG = -1
TIED_SCENE = 12                                                     # see test_host_rasteriser_is_the_oracles_on_the_fixture_scenes


@pytest.fixture(scope='module')
def uvs():
    import os
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- refusals
class Buffers:
    """Host arrays with sentinels: a refused (or empty) call must leave every one of them as it is."""

    def __init__(self, uvs, T=2, n_points=4, n_joints=6):
        self.cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
        self.cam.n_points, self.cam.n_joints = n_points, n_joints
        self.q_prev, self.dq, self.q_out = (np.full((T, 8), 7.0) for _ in range(3))
        self.discs, self.f, self.noise = np.full((T, 4, 3), 7.0), np.full((T, 8), 7.0), np.full((T, 8), 7.0)
        self.pixels = np.full((T, 4), 7, np.int32)
        raw = np.full(T * (cc.DENSE + 32) + 32, 7, np.uint8)
        self.raw, self.frames = raw, raw.ctypes.data + (-raw.ctypes.data) % 16
        self.T = T

    def ptr(self, name):
        return getattr(self, name).ctypes.data

    def untouched(self):
        return all(np.all(getattr(self, k) == 7) for k in ('q_prev', 'dq', 'q_out', 'discs', 'f', 'noise', 'pixels', 'raw'))


def test_every_new_symbol_is_bound(uvs):
    for name in ('uvs_camera_project_f64', 'uvs_render_discs_u8', 'uvs_disc_features_f64', 'uvs_camera_features_f64'):
        assert name in uvs._vision.SYMBOLS and getattr(uvs._vision.lib(), name) is not None
    assert ctypes.sizeof(uvs._vision.Camera) == 8 + 5 * 8 * 8 + 12 * 8 + 16 + 4 * 8


def test_camera_project_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)

    def call(cam=b.cam, T=b.T, q_prev=b.ptr('q_prev'), dq=b.ptr('dq'), q_out=b.ptr('q_out'), discs=b.ptr('discs')):
        return lib.uvs_camera_project_f64(None if cam is None else ctypes.byref(cam), T, q_prev, dq, 0.05, q_out, discs, None)

    assert call(cam=None) == ARG and b'NULL' in lib.uvs_vision_last_error()
    assert call(q_prev=None) == ARG and call(discs=None) == ARG
    assert call(T=-1) == ARG
    for n_points in (0, 2, 5, -1):
        assert call(cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    for n_joints in (0, 9, -1):
        assert call(cam=Buffers(uvs, n_joints=n_joints).cam) == ARG, n_joints
    assert call(q_out=b.ptr('q_prev')) == ARG and b'overlap' in lib.uvs_vision_last_error()
    assert call(q_out=b.ptr('q_prev') + 8) == ARG                                          # a partial overlap is one too
    for n_points in (1, 3, 4):
        assert call(cam=Buffers(uvs, n_points=n_points).cam, T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert call(T=0, dq=None, q_out=None) == 0
    assert b.untouched(), 'a refused call wrote'


def test_camera_features_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)

    def call(cam=b.cam, T=b.T, q_prev=b.ptr('q_prev'), q_out=b.ptr('q_out'), f=b.ptr('f')):
        return lib.uvs_camera_features_f64(None if cam is None else ctypes.byref(cam), T, q_prev, b.ptr('dq'), 0.05, q_out, b.ptr('noise'), f,
                                           b.ptr('pixels'), b.ptr('discs'), None)

    assert call(cam=None) == ARG and call(q_prev=None) == ARG and call(f=None) == ARG
    assert call(T=-1) == ARG
    for n_points in (0, 2, 5):
        assert call(cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    for n_joints in (0, 9):
        assert call(cam=Buffers(uvs, n_joints=n_joints).cam) == ARG, n_joints
    assert call(q_out=b.ptr('q_prev')) == ARG
    assert call(T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert b.untouched(), 'a refused call wrote'


def test_render_discs_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)

    def call(T=b.T, discs=b.ptr('discs'), n=4, background=96, frames=b.frames, stride=cc.DENSE):
        return lib.uvs_render_discs_u8(T, discs, n, background, frames, stride, None)

    assert call(discs=None) == ARG and call(frames=None) == ARG
    assert call(T=-1) == ARG
    for n in (0, 2, 5, -1):
        assert call(n=n) == ARG, n
    for background in (250, 251, 255, 256, -1):
        assert call(background=background) == ARG, background
    assert b'250' in lib.uvs_vision_last_error()
    assert call(frames=b.frames + 4) == ARG                                               # 16-byte stores
    assert call(stride=cc.DENSE - 16) == ARG and call(stride=cc.DENSE + 8) == ARG
    for n in (1, 3, 4):
        assert call(T=0, n=n, background=249) == 0 and lib.uvs_vision_last_error() == b''
    assert b.untouched(), 'a refused call wrote'


def test_disc_features_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)

    def call(T=b.T, discs=b.ptr('discs'), n=4, f=b.ptr('f')):
        return lib.uvs_disc_features_f64(T, discs, n, b.ptr('noise'), f, b.ptr('pixels'), None)

    assert call(discs=None) == ARG and call(f=None) == ARG and call(T=-1) == ARG
    for n in (0, 2, 5, -1):
        assert call(n=n) == ARG, n
    for n in (1, 3, 4):
        assert call(T=0, n=n) == 0 and lib.uvs_vision_last_error() == b''
    assert b.untouched(), 'a refused call wrote'


def test_python_wrappers_refuse_what_the_kernels_cannot_read(uvs):
    with pytest.raises(ValueError):
        uvs.plant.render_discs(np.zeros((4, 3)), background=250)
    with pytest.raises(ValueError):
        uvs.plant.render_discs(np.zeros((2, 3)), n_colours=2)
    with pytest.raises(ValueError):
        uvs.plant.render_discs(np.zeros((3, 3)), n_colours=4)


# ------------------------------------------------------------------------------------------------------------- the pixel rule on the host
def oracle_frame(disc):
    centres = {c: (disc[j, 0], disc[j, 1]) for j, c in enumerate(cc.ORDER)}
    return plant_ref.render_discs(centres, {c: disc[j, 2] for j, c in enumerate(cc.ORDER)}, soften=False)


def test_host_rasteriser_is_the_oracles_on_the_fixture_scenes(uvs):
    """The oracle tests hypot(dx, dy) <= r, the contract tests rounded squares: they can part only where a rounded d^2 ties r^2.  Of the
    fixture's unsoftened scenes one has such pixels and is DROPPED here by name: scene 12 (integer centres such as (128, 128) with r = 9, so
    pixels nine columns or rows away sit exactly on the rim, d^2 = 81 = r^2).  Every other scene is checked to have none, and its frames
    must be byte-identical.  (Scene 12 stays in the GPU tests, which hold the kernels to plant.render_discs, ties included.)"""
    discs, idx = cc.fixture_discs(unsoftened_only=True)
    assert 12 in idx and cc.closest_to_rim(discs[idx.index(12)]) == 0.0, 'scene 12 no longer has a tie: take it back in'
    discs, idx = discs[[k for k, i in enumerate(idx) if i != TIED_SCENE]], [i for i in idx if i != TIED_SCENE]
    assert len(idx) >= 7
    for disc, i in zip(discs, idx):
        assert cc.closest_to_rim(disc) > 0.0, f'scene {i} has a pixel exactly on a rim'
        for one in disc:                                                                    # and the two rules agree pixel by pixel
            d2, r2 = cc.squares(one)
            grid = np.arange(cc.SIDE, dtype=float)
            assert np.array_equal(d2 <= r2, np.hypot(grid[None, :] - one[0], grid[:, None] - one[1]) <= one[2]), i
        assert np.array_equal(uvs.plant.render_discs(disc), oracle_frame(disc)), f'scene {i}'
    batch = uvs.plant.render_discs(discs)
    assert batch.shape == (len(idx), 256, 256, 3) and batch.dtype == np.uint8
    assert np.array_equal(batch[3], uvs.plant.render_discs(discs[3]))


def test_host_frames_tie_to_the_reference_detector_outputs(uvs):
    """utils.detect4Circles of the host-rendered frames against the fixture's f4 -- outputs of the reference's own detector on the oracle's
    frames of the same scenes -- within the 1e-11 px gate of the detector tests."""
    discs, idx = cc.fixture_discs(unsoftened_only=True)
    for disc, i in zip(discs, idx):
        f = uvs.utils.detect4Circles(uvs.plant.render_discs(disc))
        assert np.abs(f - cc.G['f4'][i]).max() < 1e-11, i
        assert np.abs(uvs.utils.detectRGBCircles(uvs.plant.render_discs(disc[:3], 3)) - cc.G['f3'][i]).max() < 1e-11, i
        assert np.abs(uvs.utils.detectGreenCircle(uvs.plant.render_discs(disc[1:2], 1)) - cc.G['f1'][i]).max() < 1e-11, i


def test_pixel_rule_edge_cases_on_the_host(uvs):
    scenes = cc.edge_scenes()
    count = lambda name: cc.host_counts(uvs.plant.render_discs(scenes[name][1], scenes[name][0]))         # noqa: E731
    assert count('point_on_lattice').tolist() == [1, 1, 1, 1]                               # r = 0 on a lattice point: that pixel alone
    frame = uvs.plant.render_discs(scenes['point_on_lattice'][1])[::-1]
    assert tuple(frame[33, 17]) == (255, 0, 0) and tuple(frame[255, 255]) == (0, 0, 255) and tuple(frame[0, 0]) == (255, 0, 255)
    assert count('point_off_lattice').tolist()[:2] == [0, 0]                                # r = 0 off the lattice: nothing
    frame = uvs.plant.render_discs(scenes['r5_integer_centre'][1])[::-1]
    for dx, dy in ((3, 4), (4, 3), (-3, 4), (5, 0), (0, -5), (-4, -3)):                     # 9 + 16 = 25 <= 25: boundary pixels are inside
        assert tuple(frame[60 + dy, 50 + dx]) == (255, 0, 0)
    assert tuple(frame[60 + 4, 50 + 4]) == (96, 96, 96) and count('r5_integer_centre').tolist() == [81, 81, 0, 0]
    assert count('not_drawn').tolist() == [0, 0, 0, 0]                                      # r = -1, NaN centre, NaN radius
    assert count('outside').tolist() == [0, 0, 0, 149]                                    # Gauss's circle count for r = 7
    assert count('whole_frame').tolist() == [65536, 0, 0, 0]
    assert count('covered')[0] == 0 and count('covered')[1] > 200                           # the painter's order: green over red
    assert count('green_alone').tolist() == [0, count('green_alone')[1], 0, 0] and count('green_alone')[1] > 200
    # unflipped hand-over: flipped row i is stored at row 255 - i
    one = uvs.plant.render_discs(cc.pad([(10.0, 20.0, 0.0)]))
    assert tuple(one[255 - 20, 10]) == (255, 0, 0) and cc.host_counts(one).tolist() == [1, 0, 0, 0]
    # the background is every other pixel, in all three channels
    assert np.all(uvs.plant.render_discs(cc.pad([]), background=0) == 0) and np.all(uvs.plant.render_discs(cc.pad([]), background=249) == 249)


def test_detection_is_within_half_a_pixel_of_the_centre_on_the_host(uvs):
    """The sanity bound the GPU test relies on, confirmed with the host mirror: for unclipped, unoccluded discs with r >= 4 the centre of mass
    of the rasterised disc is within 0.5 px of (u, v) (the mask is symmetric about the nearest lattice point up to the rim's quantisation)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(40):
        slots = rng.permutation(9)[:4]
        disc = np.array([(64.0 * (s % 3) + 64 + rng.uniform(-12, 12), 64.0 * (s // 3) + 64 + rng.uniform(-12, 12), rng.uniform(4.0, 12.0)) for s in slots])
        f = uvs.utils.detect4Circles(uvs.plant.render_discs(disc)).reshape(4, 2)
        worst = max(worst, float(np.abs(f - disc[:, :2]).max()))
    print(f'worst |detection - centre| over 160 discs: {worst:.3f} px')
    assert worst < 0.5


HUGE_COUNTS = {
    'huge_1e12': [65536, 0, 0, 0], 'huge_off_centre': [65536, 0, 0, 0], 'inf_radius': [65536, 0, 0, 0], 'inf_all': [65536, 0, 0, 0],
    'inf_radius_minus_inf_u': [65536, 0, 0, 0], 'inf_u_small_radius': [0, 0, 0, 0],
    'below_1e9': [39689, 0, 0, 0], 'below_1e9_over_red': [177, 39689, 0, 0],
    'above_1e9': [65325, 0, 0, 0], 'above_1e9_over_red': [0, 65325, 0, 0],
    'above_1e9_rim': [39725, 0, 0, 0], 'above_1e9_rim_over_red': [177, 39725, 0, 0],
    'rim_2_54_right': [14848, 0, 0, 0], 'rim_2_54_right_green_alone': [0, 14848, 0, 0],           # columns 198 .. 255
    'rim_2_54_right_under_green': [14654, 284, 0, 0], 'rim_2_54_right_pink_over_three': [156, 248, 136, 14848],
    'rim_2_54_left': [25856, 0, 0, 0], 'rim_2_54_left_green_alone': [0, 25856, 0, 0],             # columns 0 .. 100
    'rim_2_54_left_under_green': [25856, 284, 0, 0], 'rim_2_54_left_pink_over_three': [0, 248, 136, 25856],
    'rim_2_54_below': [41984, 0, 0, 0], 'rim_2_54_below_green_alone': [0, 41984, 0, 0],           # rows 92 .. 255
    'rim_2_54_below_under_green': [41984, 284, 0, 0], 'rim_2_54_below_pink_over_three': [156, 248, 0, 41984],
}


def test_huge_and_non_finite_discs_on_the_host(uvs):
    """The masks plant.render_discs gives the discs of camera_common.huge_scenes, pinned: what the kernels are held to byte for byte in
    tests/test_gpu_camera.py.  Beyond 2^54 the rule quantises: x - 2^55 is a multiple of 8, so whole columns fall on the rim together."""
    scenes = cc.huge_scenes()
    assert set(scenes) == set(HUGE_COUNTS)
    for name, (n, disc) in scenes.items():
        assert cc.host_counts(uvs.plant.render_discs(disc, n)).tolist() == HUGE_COUNTS[name], name
    flipped = uvs.plant.render_discs(scenes['rim_2_54_right'][1])[::-1]
    assert np.all(flipped[:, 198:, 0] == 255) and np.all(flipped[:, :198, 0] == 96)


def test_box_mirror_keeps_every_pixel_of_the_rule():
    """pixel_range as the kernels have it (camera_common.pixel_range mirrors vision_device.hpp) against the rule, over discs far from the
    frame whose rim crosses it: |centre| = 2^e (1 + rand) along one axis, either sign, e = 20 .. 60.  With the whole-frame rule for
    operands not below 1e9 no disc loses a pixel.  Without it -- the box [centre - r - 1, centre + r + 1] alone -- nothing is lost up to
    2^53 and most discs lose pixels from 2^54 on, where doubles near the centre are 4 apart and the one pixel of slack no longer covers
    the rounding of dx: the reason the rule is there."""
    rng = np.random.default_rng(54)
    lost = {}
    for e in range(20, 61):
        lost[e] = 0
        for _ in range(48):
            far = rng.choice([-1.0, 1.0]) * 2.0 ** e * (1.0 + rng.random())
            near, target = rng.uniform(0, 255), rng.uniform(20, 235, 2)
            u, v = (far, near) if rng.random() < 0.5 else (near, far)
            disc = (u, v, float(np.hypot(u - target[0], v - target[1])))
            assert 0 < cc.rule_mask(disc).sum() < 65536 or e >= 54, disc        # up to 2^53 the rim does cross the frame
            assert cc.pixels_outside_box(disc) == 0, disc
            lost[e] += cc.pixels_outside_box(disc, guarded=False) > 0
    print('discs of 48 that lose pixels to the unguarded box, by exponent:', {e: n for e, n in lost.items() if n})
    assert all(lost[e] == 0 for e in range(20, 54)) and all(lost[e] > 0 for e in (54, 55, 56)), lost
    assert cc.pixel_range(2.0 ** 55, 2.0 ** 55 - 200.0) == (199, 255)                       # the rule gives column 198 as well
    assert cc.pixels_outside_box(cc.RIM_BEYOND_2_54['right'], guarded=False) == 256
    assert cc.disc_box(cc.RIM_BEYOND_2_54['right']) == ((0, 255), (0, 255))
    # an infinite slack is the whole axis whatever the operands are (NaN bounds become frame edges); a slack of one with non-finite operands
    for centre, r in ((np.inf, np.inf), (-np.inf, np.inf), (np.nan, 5.0), (100.0, np.inf), (np.inf, 5.0), (-np.inf, 5.0), (3e300, 1e300)):
        assert cc.pixel_range(centre, r, np.inf) == (0, 255), (centre, r)
    assert cc.pixel_range(np.inf, np.inf) == (0, 255) and cc.pixel_range(np.nan, 5.0) == (0, 255) and cc.pixel_range(np.inf, 5.0) == (256, 255)
    assert cc.disc_box((np.inf, 100.0, 5.0)) == ((0, 255), (0, 255)) and cc.disc_box((np.inf, 100.0, 5.0), guarded=False) == ((256, 255), (94, 106))
    assert cc.disc_box((-2.5, 100.3, 7.0)) == ((0, 5), (93, 108)) and cc.disc_box((254.2, 300.0, 8.0)) == ((246, 255), (256, 255))
    assert cc.disc_box((1e9, 128.0, 5.0)) == ((0, 255), (0, 255)) and cc.disc_box((9.9e8, 128.0, 5.0)) == ((256, 255), (122, 134))


# ------------------------------------------------------------------------------------------------------------- scenes through a camera
@pytest.mark.parametrize('name', cc.camera_scene_names())
def test_jitter_varies_the_masks_and_keeps_the_scenes(uvs, name):
    """camera_common.scene_plant returns the scene at Q_GOAL, and JITTER = 2 mrad is an amplitude at which the 259 start poses of
    tests/test_gpu_camera_scenes.py give at least three different rows of mask sizes (discs move by a pixel or two: clipped and
    overlapping masks change) while a colour that has no pixel in the scene has none in any trial (covered stays covered, outside stays
    outside), so that every trial of such a scene FAILs at step 0."""
    n, plant, radius = cc.camera_scene(uvs, name)
    q = cc.scene_joints(259, name)
    assert np.array_equal(q[0], cc.Q_GOAL) and 0 < np.abs(q[1:] - cc.Q_GOAL).max() <= cc.JITTER
    discs = np.stack([plant.discs(x, radius) for x in q])
    if name == 'grazing':
        assert 1e6 < discs[0, 0, 2] < 1e8 and np.all(discs[0, 1:, 2] < 10.0)
    else:
        want = cc.edge_scenes()[name][1]
        drawn = want[:, 2] >= 0
        assert np.all(discs[0, ~drawn, 2] == -1.0)
        assert not drawn.any() or np.abs(discs[0, drawn] - want[drawn]).max() <= 2e-13
    counts = cc.host_counts(uvs.plant.render_discs(discs, n))
    counts = {4: counts, 3: counts[:, :3], 1: counts[:, 1:2]}[n]
    if name not in cc.CONSTANT_COUNTS and name != 'point_on_lattice':
        assert len({tuple(row) for row in counts.tolist()}) >= 3
    if name in cc.EMPTY_MASK:
        assert np.all((counts == 0).any(axis=1)) and np.array_equal(counts == 0, np.broadcast_to(counts[0] == 0, counts.shape))
    elif name != 'point_on_lattice':
        assert np.all(counts[0] > 0)


# ------------------------------------------------------------------------------------------------------------- projection on the host
def test_discs_of_the_plant(uvs):
    plant = uvs.SyntheticPlant.ur10()
    d = plant.discs(cc.Q_GOAL)
    assert d.shape == (4, 3) and np.array_equal(d[:, :2].ravel(), plant.features(cc.Q_GOAL))
    assert np.all((d[:, 2] >= 6.0) & (d[:, 2] <= 10.0)), d[:, 2]                            # the default radius: 6 to 10 px at the goal pose
    assert np.abs(d[:, 2] - 8.01).max() < 0.01                                              # the figure CameraRobot's docstring gives
    assert np.allclose(plant.discs(cc.Q_GOAL, 0.048)[:, 2], 2 * d[:, 2], rtol=1e-15)
    per_point = plant.discs(cc.Q_GOAL, [0.01, 0.02, 0.03, 0.04])[:, 2]
    assert np.allclose(per_point / per_point[0], [1, 2, 3, 4], rtol=1e-14)
    behind = uvs.SyntheticPlant.ur10()
    behind.points[2] = plant.fkine_all(cc.Q_GOAL)[-1][:3, 3] + np.array([0.0, 0.0, 0.3])    # above a camera that looks straight down
    assert behind.discs(cc.Q_GOAL)[2, 2] == -1.0 and np.all(behind.discs(cc.Q_GOAL)[[0, 1, 3], 2] > 0)
    cam = plant.to_camera(0.03)
    assert (cam.n_joints, cam.n_points) == (6, 4) and cam.radius[3] == 0.03 and cam.focal == plant.focal
    assert [cam.points[1][c] for c in range(3)] == list(plant.points[1])


# ------------------------------------------------------------------------------------------------------------- the robot
def test_camera_robot(uvs):
    robot = uvs.CameraRobot(dt=0.05)
    assert not isinstance(robot, uvs.SyntheticRobot)
    robot.start(cc.Q_GOAL)
    image, resolution = robot.getCameraImage()
    assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (256, 256, 3) and resolution == (256, 256)
    f = uvs.utils.detect4Circles(image)
    assert np.abs(f - robot.features()).max() < 0.5                                         # discs where the plant's features are
    assert cc.host_counts(image).min() > 150                                                # pi * 8.01^2 = 201 pixels each
    # the robot duck-type of the external route, delegated to a SyntheticRobot
    twin = uvs.SyntheticRobot(dt=0.05)
    twin.start(cc.Q_GOAL)
    assert robot.sim.getSimulationTime() == twin.sim.getSimulationTime() == 0.05 and robot.perspective_angle == twin.perspective_angle
    for name in ('getJointsPos', 'computePose', 'jacobian', 'getCameraRotation', 'getCameraPosition', 'fkine'):
        assert np.array_equal(getattr(robot, name)(), getattr(twin, name)()), name
    assert np.array_equal(robot.computeZ(4), twin.computeZ(4))
    q_new = cc.Q_GOAL + 0.01
    robot.setJointsPos(q_new)
    robot.step()
    assert np.array_equal(robot.getJointsPos(), q_new) and robot.sim.getSimulationTime() == 0.05 + 0.05
    assert not np.array_equal(robot.getCameraImage()[0], image)
    robot.stop()


def test_synthetic_robot_is_untouched(uvs):
    robot = uvs.SyntheticRobot()
    robot.start(cc.Q_GOAL)
    image, resolution = robot.getCameraImage()
    assert image is robot and resolution == (256, 256)
    assert np.array_equal(uvs.experiment.detect4Circles(image), robot.plant.features(cc.Q_GOAL))


def test_analytic_guess_is_one_function_for_both_callers(uvs):
    from oracle import rmckf_dense
    assert uvs.Experiment._analytic_guess is uvs.plant.analytic_guess
    robot = plant_ref.PinholeUR10(0.05)
    robot.start(plant_ref.Q_START)
    f = robot.features()
    want = rmckf_dense.analytic_initial_guess(robot, f, 8, 6)
    got = uvs.plant.analytic_guess(robot, f, (256, 256), 8, 6)
    assert got.shape == (48,) and np.abs(got - np.asarray(want).ravel()).max() <= 1e-9 * np.abs(want).max()
