"""CPU-only tests of MOVING TARGETS (include/uvs_vision.h: uvs_target_motion and the four *_moving_* entry points; plant.target_at,
plant.target_motion_array, plant.CameraRobot(target_motion=); engine.*(target_motion=, motion_window=)): the numpy rule is the one the
header states, the packing is the struct's bytes, header and ctypes table agree and each entry point has its *_scenes_* namesake's operands
with `motion` after cam_index (and k for the project call), every refusal comes before any HIP call (host arrays with sentinels no kernel
could use) in the namesake's order, every Python refusal before any device work, a CameraRobot with a motion renders target_at's frame, the
built library holds the 22 + 6 + 2 new kernels without scratch and under no pinned name, and every oracle trial of camera_moving_common.py
meets pixel_loop_common's preconditions with "the motion is ignored" at least TEETH_MIN away."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_moving_common as mc
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED

ARG, SHAPE, METHOD = -1, -2, -4
NAMESAKES = {'uvs_camera_project_moving_f64': 'uvs_camera_project_scenes_f64', 'uvs_camera_features_moving_f64': 'uvs_camera_features_scenes_f64',
             'uvs_camera_closed_loop_moving_f64': 'uvs_camera_closed_loop_scenes_f64',
             'uvs_camera_believed_loop_moving_f64': 'uvs_camera_believed_loop_scenes_f64'}
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


def raw(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------- the numpy rule
def test_the_steps_moved_are_the_clamp_of_the_header(uvs):
    s = uvs.plant.motion_steps
    assert [s(k, (4, 10)) for k in (0, 3, 4, 5, 9, 10, 11, 1000)] == [0, 0, 0, 1, 5, 6, 6, 6]
    assert [s(k) for k in (0, 1, 7)] == [0, 1, 7], 'the default window: from step 0 on'
    assert [s(k, (10, 4)) for k in (0, 4, 9, 10, 11, 99)] == [0] * 6, 'k_off < k_on: nothing ever moves'
    assert [s(k, (5, 5)) for k in (0, 5, 6)] == [0, 0, 0]
    assert s(3, (-2, 10)) == 5 and s(0, (-2, 10)) == 2, 'a window that opened before step 0'
    assert s(INT32_MAX, (INT32_MIN, INT32_MAX)) == INT32_MAX - INT32_MIN == 2 ** 32 - 1, 'formed beyond 32 bits'
    assert s(0, (INT32_MIN, INT32_MAX)) == 2 ** 31 and s(INT32_MAX, (INT32_MAX, INT32_MIN)) == 0
    assert s(5, (INT32_MAX, INT32_MAX)) == 0 and s(INT32_MAX, (0, INT32_MAX)) == INT32_MAX
    with pytest.raises(ValueError):
        s(-1)


def test_no_motion_yet_leaves_the_points_bits_untouched(uvs):
    plant = uvs.SyntheticPlant.ur10()
    plant.points[0, 2], plant.points[1, 0] = -0.0, -0.0
    for vel in (np.full((4, 3), np.nan), np.full((4, 3), np.inf), np.zeros((4, 3)), np.full((4, 3), -0.0)):
        for k, window in ((0, (0, 16)), (3, (4, 10)), (16, (16, INT32_MAX)), (9, (10, 4)), (7, (0, 0))):
            at = uvs.plant.target_at(plant, vel, k, window)
            assert np.array_equal(raw(at.points), raw(plant.points)), (vel[0, 0], k, window)
            assert at.points is not plant.points, 'a copy'
    moved = uvs.plant.target_at(plant, np.zeros((4, 3)), 3, (0, 16))
    assert np.signbit(plant.points[0, 2]) and not np.signbit(moved.points[0, 2]), 'once s != 0 the add is made: -0.0 + 3 * 0.0 = +0.0'
    assert np.isnan(uvs.plant.target_at(plant, np.full((4, 3), np.nan), 1).points).all()
    for name in ('theta_offset', 'd', 'a', 'alpha'):
        assert np.array_equal(getattr(moved, name), getattr(plant, name))
    assert (moved.focal, moved.center, moved.fov_deg) == (plant.focal, plant.center, plant.fov_deg)


def test_a_moved_point_is_one_multiply_then_one_add(uvs):
    rng = np.random.default_rng(0)
    plant = uvs.SyntheticPlant.ur10()
    vel = rng.standard_normal((4, 3)) * 1e-3
    for k, window, s in ((5, (0, 16), 5), (9, (4, 10), 5), (12, (4, 10), 6), (3, (-4, 2), 6)):
        want = np.empty((4, 3))
        for p in range(4):
            for c in range(3):
                step = np.float64(s) * np.float64(vel[p, c])
                want[p, c] = np.float64(plant.points[p, c]) + step
        assert np.array_equal(raw(uvs.plant.target_at(plant, vel, k, window).points), raw(want)), (k, window)
    fused = plant.points + 5 * vel
    assert fused.shape == (4, 3)
    with pytest.raises(ValueError, match='one row per disc'):
        uvs.plant.target_at(plant, vel[:3], 1)


# ------------------------------------------------------------------------------------------------------------- packing
def test_target_motion_array_packs_the_structs_bytes(uvs):
    TM = uvs._vision.TargetMotion
    assert ctypes.sizeof(TM) == 104 == uvs.plant.MOTION_ROW
    assert (TM.v.offset, TM.k_on.offset, TM.k_off.offset) == (0, 96, 100)
    pack = uvs.plant.target_motion_array
    vel, win = mc.mixed(7, 3)
    rows = pack(vel, win, 3)
    assert rows.shape == (7, 104) and rows.dtype == np.uint8
    for t in range(7):
        s = TM.from_buffer_copy(rows[t].tobytes())
        got = np.array([[s.v[p][c] for c in range(3)] for p in range(4)])
        assert np.array_equal(raw(got[:3]), raw(vel[t])) and np.array_equal(raw(got[3]), raw(np.zeros(3))), t
        assert (s.k_on, s.k_off) == tuple(win[t]), t
    one = pack(vel[1], win[1], 3)
    assert one.shape == (1, 104) and np.array_equal(one[0], rows[1])
    assert np.array_equal(pack(vel[1], win[1], 3, 5), np.tile(rows[1], (5, 1))), 'broadcast over the trials'
    assert np.array_equal(pack(vel, win[2], 3)[:, 96:], np.tile(rows[2, 96:], (7, 1)))
    assert np.array_equal(pack(vel[1], win, 3)[:, :96], np.tile(rows[1, :96], (7, 1)))
    default = TM.from_buffer_copy(pack(vel[1], None, 3)[0].tobytes())
    assert (default.k_on, default.k_off) == uvs.plant.MOTION_WINDOW == (0, INT32_MAX)
    extreme = TM.from_buffer_copy(pack(vel[1], (INT32_MIN, INT32_MAX), 3)[0].tobytes())
    assert (extreme.k_on, extreme.k_off) == (INT32_MIN, INT32_MAX)
    assert pack(np.ones((1, 3), np.int64), (0, 1), 1).shape == (1, 104), 'integer velocities are reals'


def test_target_motion_array_refuses(uvs):
    pack = uvs.plant.target_motion_array
    vel, win = mc.mixed(7, 4)
    for bad in (vel[:, :3], vel[0, :3], np.zeros((4,)), np.zeros((4, 2)), np.zeros((2, 7, 4, 3)), vel.astype(str), [[1.0, 2.0], [3.0]], None):
        with pytest.raises(ValueError, match='target_motion'):
            pack(bad, win, 4)
    for bad in (np.zeros((7, 3), np.int64), np.zeros(3, np.int64), np.zeros((2, 7, 2), np.int64), win.astype(float), (0.0, 5.0), 7):
        with pytest.raises(ValueError, match='motion_window'):
            pack(vel, bad, 4)
    for bad in ((0, 2 ** 31), (INT32_MIN - 1, 0), (0, 2 ** 40)):
        with pytest.raises(ValueError, match='int32'):
            pack(vel, bad, 4)
    with pytest.raises(ValueError, match='do not match'):
        pack(vel, win[:5], 4)
    with pytest.raises(ValueError, match='do not match'):
        pack(vel, win, 4, 8)
    with pytest.raises(ValueError, match='do not match'):
        pack(vel[0], win, 4, 8)


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    for new, old in NAMESAKES.items():
        a, b, ta, tb = declared(new), declared(old), types(new), list(types(old))
        at = b.index('const int32_t *cam_index') + 1
        b.insert(at, 'const uvs_target_motion *motion')
        tb.insert(at, VP)
        if 'project' in new:                                         # the call without a k takes one after dt
            b.insert(b.index('double dt') + 1, 'int32_t k')
            tb.insert(b.index('int32_t k'), I32)
        assert a == b, (new, "the namesake's operands with motion after cam_index")
        assert ta == tb, new
        assert getattr(uvs._vision.lib(), new) is not None
    assert re.search(r'typedef struct uvs_target_motion \{\s*/\* 104 bytes \*/\s*double\s+v\[UVS_CAMERA_MAX_POINTS\]\[3\];[^\n]*\n\s*int32_t k_on, k_off;',
                     header)


# ------------------------------------------------------------------------------------------------------------- C refusals
class Moving(Buffers):
    """Buffers with the scene operand, the believed operand, rectangles, paints and motions: host arrays with sentinels."""
    def __init__(self, uvs, **kw):
        Buffers.__init__(self, uvs, **kw)
        self.cams = np.full(self.T * 472 // 8 + 8, 7.0)
        self.index = np.full(self.T, 7, np.int32)
        self.occ = np.full(self.T * 4 * 8, 7, np.int32)
        self.paint = np.full(self.T * 4, 7, np.int32)
        self.held = np.full(self.T * 4, 7, np.int32)
        self.motion = np.full(self.T * 13, 7.0)

    def untouched(self):
        return Buffers.untouched(self) and np.all(self.cams == 7) and np.all(self.motion == 7) and \
            all(np.all(a == 7) for a in (self.index, self.occ, self.paint, self.held))


def loop_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', tp='block', occ='rows', n_occ=1, hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_moving_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.motion.ctypes.data if isinstance(motion, str) else motion, b.T if T is None else T, ref(tp),
        b.occ.ctypes.data if isinstance(occ, str) else occ, b.paint.ctypes.data, n_occ, hold, a['q_start'], a['noise'], a['x0'], a['f0'], a['q'],
        a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'], b.held.ctypes.data, None)


def baseline_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', believed='own', n_believed=1, believed_index=None, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_believed_loop_moving_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.motion.ctypes.data if isinstance(motion, str) else motion, b.T if T is None else T,
        b.cams.ctypes.data if isinstance(believed, str) else believed, n_believed, believed_index, a['q_start'], a['noise'], a['q'], a['f'], a['dq'],
        a['err'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def triple_refusals(call, lib, T):
    """The triple's refusals, which come last: NULL cams, n_cams < 1, n_cams not in {1, T} without an index; each also before T == 0, with
    and without a motion."""
    for motion in ('own', None):
        assert call(cams=None, motion=motion) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
        for n_cams in (0, -1, 2 ** 31):
            assert call(n_cams=n_cams, motion=motion) == ARG and b'n_cams' in lib.uvs_vision_last_error(), n_cams
        for n_cams in (T + 1, 3 * T):
            assert call(n_cams=n_cams, motion=motion) == ARG and b'cam_index' in lib.uvs_vision_last_error(), n_cams
        assert call(cams=None, T=0, motion=motion) == ARG and call(n_cams=0, T=0, motion=motion) == ARG and call(n_cams=5, T=0, motion=motion) == ARG
        assert call(T=0, motion=motion) == 0 and lib.uvs_vision_last_error() == b'' and call(T=0, n_cams=5, index='own', motion=motion) == 0


def test_the_loop_refuses_what_the_scenes_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Moving(uvs)
    call = lambda **kw: loop_call(uvs, b, **kw)                      # noqa: E731
    for name in ('fp', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
        assert call(**{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    assert call(T=-1) == ARG
    bad = Buffers(uvs)
    bad.fp.steps = 0
    assert call(fp=bad.fp) == ARG
    bad = Buffers(uvs)
    bad.fp.lanes_per_filter = 2
    assert call(fp=bad.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    bad = Buffers(uvs)
    bad.fp.m = 4                                                     # two points: no such camera
    assert call(fp=bad.fp) == ARG and b'n_points' in lib.uvs_vision_last_error()
    bad = Buffers(uvs)
    bad.fp.n = 5
    assert call(fp=bad.fp) == SHAPE
    bad = Buffers(uvs)
    bad.fp.method = 1                                                # UVS_METHOD_ANALYTICAL
    assert call(fp=bad.fp) == METHOD
    mckf = Moving(uvs, n_points=3, method='MCKF')
    mckf.fp.m = 6
    assert loop_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
    for n_in in (0, -3):
        assert call(tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    for n_occ in (-1, 5):
        assert call(n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
    assert call(occ=None, n_occ=2) == ARG and b'NULL occ' in lib.uvs_vision_last_error()
    assert call(hold=-1) == ARG and b'hold' in lib.uvs_vision_last_error()
    # the order: the namesake's refusals among themselves, and before the triple's
    assert call(hold=-1, cams=None) == ARG and b'hold' in lib.uvs_vision_last_error()
    assert call(n_occ=9, n_cams=0) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert call(n_occ=9, hold=-1) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert call(fp=bad.fp, cams=None) == METHOD
    triple_refusals(call, lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0, motion=None) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_the_baseline_loop_refuses_what_its_scenes_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Moving(uvs, method='ANALYTICAL')
    call = lambda **kw: baseline_call(uvs, b, **kw)                  # noqa: E731
    for name in ('fp', 'q_start', 'status', 'k_done', 'stats'):
        assert call(**{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    assert call(T=-1) == ARG
    assert call(fp=Buffers(uvs).fp) == METHOD, 'an estimator is not the calibrated law'
    bad = Buffers(uvs, method='ANALYTICAL')
    bad.fp.steps = 0
    assert call(fp=bad.fp) == ARG and b'steps' in lib.uvs_vision_last_error()
    assert call(believed=None) == ARG and b'NULL believed' in lib.uvs_vision_last_error()
    assert call(n_believed=0) == ARG and call(n_believed=b.T + 1) == ARG and b'believed_index' in lib.uvs_vision_last_error()
    assert call(believed=None, cams=None) == ARG and b'NULL believed' in lib.uvs_vision_last_error(), "the believed operand's come first"
    triple_refusals(call, lib, b.T)
    assert b.untouched(), 'a refused call wrote'


def test_the_stand_alone_calls_refuse_before_they_launch(uvs):
    lib = uvs._vision.lib()
    cams, discs, f, q, occ, paint = np.full(64, 7.0), np.full(12, 7.0), np.full(8, 7.0), np.full(6, 7.0), np.full(32, 7, np.int32), np.full(4, 7, np.int32)
    mot = np.full(13, 7.0)
    P = lambda a: None if a is None else a.ctypes.data               # noqa: E731
    project = lambda cams=cams, n_cams=1, index=None, T=1, n=4, out=discs, q_out=None, k=0, motion=mot: lib.uvs_camera_project_moving_f64(   # noqa: E731
        P(cams), n_cams, index, P(motion), n, T, P(q), None, 0.0, k, q_out, P(out), None)
    features = lambda cams=cams, n_cams=1, index=None, T=1, n=4, out=f, n_occ=1, k=0, occ_ptr=occ, motion=mot: lib.uvs_camera_features_moving_f64(   # noqa: E731
        P(cams), n_cams, index, P(motion), n, T, P(q), None, 0.0, None, P(occ_ptr), P(paint), n_occ, k, None, P(out), None, None, None)
    for call in (project, features):
        for motion in (mot, None):
            assert call(out=None, motion=motion) == ARG and b'NULL' in lib.uvs_vision_last_error()
            assert call(T=-1, motion=motion) == ARG and call(n=2, motion=motion) == ARG and b'n_points' in lib.uvs_vision_last_error()
            assert call(out=None, cams=None, motion=motion) == ARG and b'cams' not in lib.uvs_vision_last_error(), "the namesake's refusals come first"
            assert call(cams=None, motion=motion) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
            assert call(n_cams=0, motion=motion) == ARG and call(n_cams=3, motion=motion) == ARG and b'cam_index' in lib.uvs_vision_last_error()
            assert call(n_cams=3, T=0, motion=motion) == ARG, 'refusals come before T == 0'
            assert call(k=-1, motion=motion) == ARG and b'k must be' in lib.uvs_vision_last_error()
            assert call(k=-1, T=0, motion=motion) == ARG
            assert call(T=0, motion=motion) == 0 and lib.uvs_vision_last_error() == b''
    assert project(q_out=q.ctypes.data) == ARG and b'overlaps' in lib.uvs_vision_last_error()
    assert project(k=-1, cams=None) == ARG and b'NULL cams' in lib.uvs_vision_last_error(), "the project call's own k comes after its namesake's refusals"
    assert features(n_occ=5) == ARG and features(occ_ptr=None) == ARG
    assert features(n_occ=5, cams=None) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert features(k=-1, cams=None) == ARG and b'k must be' in lib.uvs_vision_last_error(), 'the features call keeps k where its namesake has it'
    assert features(T=0, occ_ptr=None, n_occ=0) == 0, 'no rectangles stay legal'
    assert all(np.all(a == 7) for a in (cams, discs, f, q, occ, paint, mot)), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python
def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these must be a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    eng = uvs.engine
    plant = uvs.SyntheticPlant.ur10()
    q = torch.zeros((3, 6), dtype=torch.float64)
    fp = eng.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    analytical = eng.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    x0 = np.zeros((3, 48))
    calls = (lambda **kw: eng.camera_project(plant, q, **kw), lambda **kw: eng.camera_features(plant, q, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, guess='device', fused=True, hold=2, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, believed=plant, **kw))
    vel, win = mc.mixed(3, 4)
    for call in calls:
        with pytest.raises(ValueError, match='motion_window without target_motion'):
            call(motion_window=(0, 5))
        for bad in (vel[:, :3], vel[0, 0], np.zeros((3, 4, 2)), vel.astype(str), torch.zeros((3, 4, 3), dtype=torch.float64)[:, :2]):
            with pytest.raises(ValueError, match='target_motion'):
                call(target_motion=bad)
        for bad in (np.zeros((3, 3), np.int64), win.astype(float), (0.5, 2.0), 4):
            with pytest.raises(ValueError, match='motion_window'):
                call(target_motion=vel, motion_window=bad)
        for bad in ((0, 2 ** 31), (INT32_MIN - 1, 3)):
            with pytest.raises(ValueError, match='int32'):
                call(target_motion=vel, motion_window=bad)
        for rows in (2, 4):
            with pytest.raises(ValueError, match='do not match'):
                call(target_motion=mc.mixed(rows, 4)[0])
            with pytest.raises(ValueError, match='do not match'):
                call(target_motion=vel[0], motion_window=mc.mixed(rows, 4)[1])
        with pytest.raises(ValueError, match='what target_motions returns'):
            call(target_motion=torch.zeros((3, 100), dtype=torch.uint8))
        with pytest.raises(ValueError, match='carries its windows'):
            call(target_motion=torch.zeros((3, 104), dtype=torch.uint8), motion_window=(0, 5))
    with pytest.raises(ValueError, match='k is a step count'):
        eng.camera_project(plant, q, target_motion=vel, k=-1)
    with pytest.raises(ValueError, match='4 trials|do not match'):   # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, target_motion=vel)
    bar = [[0, 0, 10, 10, 0, 0, 0, 5]]
    with pytest.raises(ValueError, match='fused=False'):             # the older refusals are still there, and come first
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, target_motion=vel[:, :3])
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=1, motion_window=(0, 3))
    for good in (dict(target_motion=vel, motion_window=win), dict(target_motion=vel[1]), dict(target_motion=vel[2], motion_window=(4, 10))):
        with pytest.raises(ValueError, match='on the device'):       # accepted as far as the host goes
            eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, **good)


# ------------------------------------------------------------------------------------------------------------- CameraRobot
def test_a_camera_robot_with_a_motion_renders_target_at(uvs):
    plant = pl.plant_of(4)
    vel, window = mc.motion('window', 4)
    q = mc.oracle_start()
    rows = [[100, 90, 40, 12, 2, 0, 0, 16]]
    robot = uvs.plant.CameraRobot(plant, mc.RADIUS, occluders=rows, target_motion=vel, motion_window=window)
    still = uvs.plant.CameraRobot(plant, mc.RADIUS, occluders=rows)
    robot.start(q)
    still.start(q)
    seen = []
    for k in range(12):
        at = uvs.plant.target_at(plant, vel, k, window)
        assert np.array_equal(raw(robot.discs()), raw(at.discs(q, mc.RADIUS))), k
        frame, size = robot.getCameraImage()
        assert size == (256, 256)
        assert np.array_equal(frame, uvs.plant.render_discs(at.discs(q, mc.RADIUS), 4, occluders=rows, k=k)), k
        seen.append(np.array_equal(frame, still.getCameraImage()[0]))
        assert np.array_equal(robot.computeZ(4), still.computeZ(4)), "the robot's own kinematics keep the plant's points"
        robot.step()
        still.step()
    assert seen[:5] == [True] * 5 and not any(seen[5:]), 'the same frames until the window opens, others from then on'
    plain = uvs.plant.CameraRobot(plant, mc.RADIUS)
    assert plain.target_motion is None
    with pytest.raises(ValueError, match='motion_window without target_motion'):
        uvs.plant.CameraRobot(plant, motion_window=(0, 3))
    with pytest.raises(ValueError, match='target_motion'):
        uvs.plant.CameraRobot(plant, target_motion=vel[:3])


# ------------------------------------------------------------------------------------------------------------- the built library
PINNED = ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel', 'hold_pairs_kernel', 'camera_loop_kernel', 'camera_grid_kernel',
          'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel', 'camera_scene_kernel', 'scene_baseline_loop_kernel',
          'camera_analytical_', 'camera_believed_')


def test_the_moving_kernels_are_built_without_scratch(uvs):
    """moving_target_kernel: what camera_scene_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1),
    MCKF (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22 -- moving_baseline_kernel at the three shapes in both
    forms, and the two stand-alone kernels; no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    moving = {name: r for name, r in k.items() if 'moving_target_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'moving_target_kernel(<[^>]*>)', name).group(1) for name in moving}
    assert found == expected and len(moving) == 22, (sorted(found ^ expected), len(moving))
    baseline = {name: r for name, r in k.items() if 'moving_baseline_kernel' in name}
    assert {re.search(r'moving_baseline_kernel(<[^>]*>)', name).group(1) for name in baseline} == \
        {f'<{shape}, {g}>' for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1') for g in (1, 4)}
    for name, r in list(moving.items()) + list(baseline.items()):
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
    others = dict(baseline)
    for kernel, wg in (('moving_project_kernel', 64), ('moving_detect_kernel', 1024)):
        (name, r), = [(name, r) for name, r in k.items() if re.search(r'\b' + kernel + r'\b', name)]
        assert r['scratch'] == 0 and r['wg'] == wg and r['vgpr'] <= 512 and r['lds'] <= 40960, (name, r)
        others[name] = r
    assert len(moving) + len(others) == 22 + 6 + 2
    for name in list(moving) + list(others):
        for pinned in PINNED:
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
        assert not re.search(r'\bscene_project_kernel\b|\bscene_camera_detect_kernel\b', name), name
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel',
                   'camera_scene_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
    assert sum('scene_baseline_loop_kernel' in name for name in k) == 6
    assert sum(bool(re.search(r'\bscene_project_kernel\b|\bscene_camera_detect_kernel\b', name)) for name in k) == 2


# ------------------------------------------------------------------------------------------------------------- the oracle's trials
def inside(discs):
    return (discs[:, :, :2] - discs[:, :, 2:]).min() > 0.0 and (discs[:, :, :2] + discs[:, :, 2:]).max() < 255.0 and discs[:, :, 2].min() > 0


@pytest.mark.parametrize('name', sorted(mc.MOTIONS))
@pytest.mark.parametrize('method,n_points', mc.ORACLE)
def test_every_oracle_trial_meets_the_preconditions_and_has_teeth(uvs, method, n_points, name):
    """pixel_loop_common's preconditions on the moving trial -- its 16 steps with status 0, every disc inside the frame with a mask of at
    least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the (1 + 1e-14) nudge -- and the teeth: the still trial, which is
    what "the motion is ignored" computes, sits at least TEETH_MIN away in q or dq."""
    a, b = mc.oracle_trial(method, n_points, name), mc.oracle_trial(method, n_points, name, True)
    assert (a['status'], a['k_done']) == (0, mc.K) == (b['status'], b['k_done'])
    assert np.array_equal(a['counts'], b['counts']) and a['held'] == b['held'] and np.array_equal(a['fpi_iterations'], b['fpi_iterations'])
    drift = max(float(np.abs(a[key] - b[key]).max() / np.abs(a[key]).max()) for key in ('q', 'f', 'dq', 'err', 'kappa'))
    rim, mask = cc.closest_to_rim(a['discs']), int(a['counts'].min())
    still = mc.oracle_trial(method, n_points, None)
    moved_px = float(np.abs(a['f'] - still['f']).max())
    teeth = pl.distance(a, still)
    print(f'{method} ({2 * n_points},6) {name}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, features moved {moved_px:.1f} px, '
          f'motion ignored {teeth:.1e} away')
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(a['discs']) and mask >= pl.MASK_MIN
    assert (still['status'], still['k_done']) == (0, mc.K)
    assert teeth >= pl.TEETH_MIN, 'a loop that ignores the motion would pass the gates'


def test_the_oracle_window_trial_behind_the_bar_is_calm(uvs):
    """The 'window' motion behind pixel_loop_common's sweeping bar with a hold, as the GPU file runs it: the same status, k_done, masks and
    holds under the nudge, logs within CALM_TOL, the discs inside the frame, no pixel within RIM_MIN of a rim."""
    rows = tuple(tuple(int(v) for v in row) for row in pl.bar_rows(4))
    a, b = (mc.oracle_trial('GMCKF', 4, 'window', nudged, rows, 2) for nudged in (False, True))
    assert (a['status'], a['k_done']) == (b['status'], b['k_done']) and a['k_done'] >= 1
    assert np.array_equal(a['counts'], b['counts']) and a['held'] == b['held']
    for key in ('q', 'f', 'dq', 'err', 'kappa'):
        rows_both = min(len(a[key]), len(b[key]))
        with np.errstate(invalid='ignore'):
            d = np.abs(a[key][:rows_both] - b[key][:rows_both]) / np.nanmax(np.abs(a[key]))
        assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])) and (not np.isfinite(d).any() or np.nanmax(d) <= pl.CALM_TOL), key
    assert cc.closest_to_rim(a['discs']) > pl.RIM_MIN and inside(a['discs'])
