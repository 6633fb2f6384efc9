"""CPU-only tests of CAMERA LATENCY (include/uvs_vision.h: UVS_CAMERA_MAX_LATENCY and the three entry points; plant.delayed_step,
plant.CameraRobot(latency=); engine.camera_closed_loop(latency=)): the numpy rule is the one the header states, header and ctypes table
agree and each loop has its *_moving_* namesake's operands with `latency` after `motion`, every refusal comes before any HIP call (host
arrays with sentinels no kernel could use) in the namesake's order, every Python refusal before any device work, a CameraRobot with a
latency shows an undelayed robot's earlier frames, the built library holds the 22 + 6 + 1 new kernels without scratch and under no pinned
name, and every oracle trial of camera_latency_common.py meets pixel_loop_common's preconditions with each misreading of the rule at
least TEETH_MIN away."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_latency_common as lc
import camera_moving_common as mc
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED
from test_camera_moving_host import Moving, inside, triple_refusals

ARG, SHAPE, METHOD = -1, -2, -4
NAMESAKES = {'uvs_camera_closed_loop_delayed_f64': 'uvs_camera_closed_loop_moving_f64',
             'uvs_camera_believed_loop_delayed_f64': 'uvs_camera_believed_loop_moving_f64'}


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the numpy rule
def test_the_delayed_step_is_the_clamp_of_the_header(uvs):
    step = uvs.plant.delayed_step
    assert uvs.plant.MAX_LATENCY == uvs.engine.MAX_LATENCY == lc.MAX_LATENCY == 8
    assert re.search(r'#define UVS_CAMERA_MAX_LATENCY 8\b', open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read())
    assert [step(k, 0) for k in (0, 1, 7, 1000)] == [0, 1, 7, 1000], 'd = 0: the frame of the step itself'
    assert [step(k, 1) for k in (0, 1, 2, 9)] == [0, 0, 1, 8], 'k below, at and above d = 1'
    assert [step(k, 8) for k in (0, 3, 7, 8, 9, 20)] == [0, 0, 0, 0, 1, 12], 'k below, at and above d = 8'
    assert [step(k, -1) for k in (0, 5)] == [0, 5] == [step(k, -2 ** 31) for k in (0, 5)], 'a negative latency is none'
    assert [step(k, 9) for k in (0, 8, 9, 30)] == [0, 0, 1, 22] == [step(k, 2 ** 31 - 1) for k in (0, 8, 9, 30)], 'a huge one is MAX_LATENCY'
    assert step(2 ** 31 - 1, 3) == 2 ** 31 - 4
    with pytest.raises(ValueError):
        step(-1, 0)


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for new, old in NAMESAKES.items():
        a, b, ta, tb = declared(new), declared(old), types(new), list(types(old))
        at = b.index('const uvs_target_motion *motion') + 1
        b.insert(at, 'const int32_t *latency')
        tb.insert(at, VP)
        assert a == b, (new, "the namesake's operands with latency after motion")
        assert ta == tb, new
        assert getattr(uvs._vision.lib(), new) is not None
    assert declared('uvs_delay_features_f64') == ['int64_t T', 'int32_t n_points', 'int32_t k', 'const int32_t *latency', 'const double *sensed_log',
                                                  'const int32_t *count_log', 'const double *noise_row', 'double *f_row', 'int32_t *pixels_row',
                                                  'void *stream']
    assert types('uvs_delay_features_f64') == [I64, I32, I32] + [VP] * 7
    assert uvs._vision.lib().uvs_delay_features_f64 is not None


# ------------------------------------------------------------------------------------------------------------- C refusals
class Delayed(Moving):
    """Moving with a latency per trial: a host array of sentinels."""
    def __init__(self, uvs, **kw):
        Moving.__init__(self, uvs, **kw)
        self.latency = np.full(self.T, 7, np.int32)

    def untouched(self):
        return Moving.untouched(self) and np.all(self.latency == 7)


def loop_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', tp='block', occ='rows', n_occ=1, hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_delayed_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.motion.ctypes.data if isinstance(motion, str) else motion, b.latency.ctypes.data if isinstance(latency, str) else latency,
        b.T if T is None else T, ref(tp), b.occ.ctypes.data if isinstance(occ, str) else occ, b.paint.ctypes.data, n_occ, hold, a['q_start'],
        a['noise'], a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'],
        b.held.ctypes.data, None)


def baseline_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', believed='own', n_believed=1,
                  believed_index=None, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_believed_loop_delayed_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.motion.ctypes.data if isinstance(motion, str) else motion, b.latency.ctypes.data if isinstance(latency, str) else latency,
        b.T if T is None else T, b.cams.ctypes.data if isinstance(believed, str) else believed, n_believed, believed_index, a['q_start'],
        a['noise'], a['q'], a['f'], a['dq'], a['err'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def with_and_without(call):
    """Every refusal with and without a latency and a motion: the two operands are never looked at on the host."""
    def both(**kw):
        codes = {call(latency=latency, motion=motion, **kw) for latency in ('own', None) for motion in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    return both


def test_the_loop_refuses_what_the_moving_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Delayed(uvs)
    call = with_and_without(lambda **kw: loop_call(uvs, b, **kw))
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
    mckf = Delayed(uvs, n_points=3, method='MCKF')
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
    for latency in ('own', None):
        triple_refusals(lambda **kw: loop_call(uvs, b, latency=latency, **kw), lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_the_baseline_loop_refuses_what_its_moving_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Delayed(uvs, method='ANALYTICAL')
    call = with_and_without(lambda **kw: baseline_call(uvs, b, **kw))
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
    for latency in ('own', None):
        triple_refusals(lambda **kw: baseline_call(uvs, b, latency=latency, **kw), lib, b.T)
    assert b.untouched(), 'a refused call wrote'


def test_the_stepwise_companion_refuses_before_it_launches(uvs):
    lib = uvs._vision.lib()
    sensed, counts, noise, f, pixels, latency = (np.full(32, 7.0), np.full(16, 7, np.int32), np.full(8, 7.0), np.full(8, 7.0),
                                                 np.full(4, 7, np.int32), np.full(1, 7, np.int32))
    P = lambda a: None if a is None else a.ctypes.data               # noqa: E731
    call = lambda T=1, n=4, k=2, latency=latency, sensed=sensed, counts=counts, noise=noise, f=f, pixels=pixels: lib.uvs_delay_features_f64(   # noqa: E731
        T, n, k, P(latency), P(sensed), P(counts), P(noise), P(f), P(pixels), None)
    for name in ('sensed', 'counts', 'f', 'pixels'):
        for lat in (latency, None):
            assert call(**{name: None}, latency=lat) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
            assert call(**{name: None}, latency=lat, T=0) == ARG, 'refusals come before T == 0'
    assert call(T=-1) == ARG and call(T=2 ** 31) == ARG and b'T out of range' in lib.uvs_vision_last_error()
    for n in (0, 2, 5):
        assert call(n=n) == ARG and b'n_points' in lib.uvs_vision_last_error(), n
    assert call(k=-1) == ARG and b'k must be' in lib.uvs_vision_last_error()
    assert call(k=-1, T=0) == ARG and call(n=2, T=0) == ARG
    assert call(k=-1, n=2) == ARG and b'n_points' in lib.uvs_vision_last_error(), 'the shape before the step'
    assert call(sensed=None, T=-1) == ARG and b'NULL' in lib.uvs_vision_last_error(), 'NULL before the shape'
    assert call(T=0) == 0 and lib.uvs_vision_last_error() == b'' and call(T=0, latency=None, noise=None) == 0
    assert all(np.all(a == 7) for a in (sensed, counts, noise, f, pixels, latency)), 'a refused call wrote'


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
    calls = (lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, guess='device', fused=True, hold=2, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, believed=plant, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, **kw))
    for call in calls:
        for bad in (-1, 9, 2 ** 31, [0, 1, 9], np.array([0, -1, 2]), torch.tensor([0, 1, 100])):
            with pytest.raises(ValueError, match='latency must lie in 0 .. 8'):
                call(latency=bad)
        for bad in ([0, 1], [0, 1, 2, 3], np.zeros(2, np.int64), torch.zeros(4, dtype=torch.int32)):
            with pytest.raises(ValueError, match='latencies for 3 trials'):
                call(latency=bad)
        for bad in (1.0, 0.5, [0.0, 1.0, 2.0], np.zeros(3), torch.zeros(3), True, [True, False, True], 'two', np.zeros((3, 1), np.int64), [[1, 2, 3]]):
            with pytest.raises(ValueError, match='latency is'):
                call(latency=bad)
        for good in (0, 8, [0, 3, 8], np.array([1, 2, 3], np.int32), torch.tensor([1, 2, 3])):
            with pytest.raises(ValueError, match='on the device'):   # accepted as far as the host goes
                call(latency=good)
    with pytest.raises(ValueError, match='4 trials|latencies for 4'):   # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, latency=[1, 2, 3])
    with pytest.raises(ValueError, match='on the device'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, latency=[1, 2, 3, 0])
    bar = [[0, 0, 10, 10, 0, 0, 0, 5]]
    with pytest.raises(ValueError, match='fused=False'):             # the older refusals are still there, and come first
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, latency=99)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=1, latency=[1.5])
    with pytest.raises(ValueError, match='motion_window without target_motion'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, motion_window=(0, 5), latency=99)
    with pytest.raises(ValueError, match='trial_params needs fused=True'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, trial_params={}, latency=99)
    with pytest.raises(ValueError, match='believed_index without believed'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, believed_index=[0, 0, 0], latency=99)


# ------------------------------------------------------------------------------------------------------------- CameraRobot
@pytest.mark.parametrize('d', [0, 1, 3, 8])
def test_a_camera_robot_with_a_latency_shows_earlier_frames(uvs, d):
    """Behind a sweeping bar and on a moving target, so that joints, occluders and motion must all be those of step max(k - d, 0): the
    delayed robot's frames equal an undelayed robot's earlier frames byte for byte, discs() agrees, and a second look changes nothing."""
    plant = pl.plant_of(4)
    vel, window = mc.motion('window', 4)
    rows = [[100, 90, 40, 12, 2, 0, 0, 16]]
    kw = dict(occluders=rows, target_motion=vel, motion_window=window)
    late, live = uvs.plant.CameraRobot(plant, lc.RADIUS, latency=d, **kw), uvs.plant.CameraRobot(plant, lc.RADIUS, **kw)
    assert late.latency == d and live.latency == 0
    rng = np.random.default_rng(2)
    for start in range(2):                                           # a second start() primes the delay line again
        q0 = mc.oracle_start() + 0.01 * start
        late.start(q0)
        live.start(q0)
        frames, discs = [], []
        for k in range(12):
            frames.append(live.getCameraImage()[0])
            discs.append(live.discs())
            kk = uvs.plant.delayed_step(k, d)
            frame, size = late.getCameraImage()
            assert size == (256, 256) and frame.dtype == np.uint8
            assert np.array_equal(frame, frames[kk]), (d, k)
            assert np.array_equal(late.discs().view(np.int64), discs[kk].view(np.int64)), (d, k)
            assert np.array_equal(late.getCameraImage()[0], frame), 'idempotent within a step'
            assert np.array_equal(late.getJointsPos(), live.getJointsPos()), 'the encoders are not delayed'
            if d and 0 < k:
                assert not np.array_equal(frame, frames[k]), (d, k, 'the bar and the joints have moved on')
            q_next = live.getJointsPos() + rng.standard_normal(6) * 0.01
            for robot in (late, live):
                robot.setJointsPos(q_next)
                robot.step()
    for bad in (-1, 9, 1.0, True, None, [1]):
        with pytest.raises(ValueError, match='latency'):
            uvs.plant.CameraRobot(plant, latency=bad)


# ------------------------------------------------------------------------------------------------------------- the built library
PINNED = ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel', 'hold_pairs_kernel', 'camera_loop_kernel', 'camera_grid_kernel',
          'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel', 'camera_scene_kernel', 'scene_baseline_loop_kernel',
          'moving_target_kernel', 'moving_baseline_kernel', 'camera_analytical_', 'camera_believed_')


def test_the_delayed_kernels_are_built_without_scratch(uvs):
    """delayed_frames_kernel: what moving_target_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1),
    MCKF (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22 -- delayed_baseline_kernel at the three shapes in both
    forms, and delay_line_kernel; no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    loops = {name: r for name, r in k.items() if 'delayed_frames_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'delayed_frames_kernel(<[^>]*>)', name).group(1) for name in loops}
    assert found == expected and len(loops) == 22, (sorted(found ^ expected), len(loops))
    assert all('DelayedLoopArgs' in name for name in loops)
    baseline = {name: r for name, r in k.items() if 'delayed_baseline_kernel' in name}
    assert {re.search(r'delayed_baseline_kernel(<[^>]*>)', name).group(1) for name in baseline} == \
        {f'<{shape}, {g}>' for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1') for g in (1, 4)}
    assert all('DelayedBaselineArgs' in name for name in baseline)
    for name, r in list(loops.items()) + list(baseline.items()):
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 65536 and r['scratch'] == 0, (name, r)
    (name, r), = [(name, r) for name, r in k.items() if re.search(r'\bdelay_line_kernel\b', name)]
    assert r['scratch'] == 0 and r['wg'] == 256 and r['lds'] == 0, (name, r)
    new = list(loops) + list(baseline) + [name]
    assert len(new) == 22 + 6 + 1
    for name in new:
        for pinned in PINNED + ('moving_project_kernel', 'moving_detect_kernel'):
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel',
                   'camera_scene_kernel', 'moving_target_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
    assert sum('scene_baseline_loop_kernel' in name for name in k) == 6 and sum('moving_baseline_kernel' in name for name in k) == 6
    assert sum('hold_pairs_kernel' in name for name in k) == 1


# ------------------------------------------------------------------------------------------------------------- the oracle's trials
@pytest.mark.parametrize('d', lc.ORACLE_LATENCIES)
@pytest.mark.parametrize('method,n_points', lc.ORACLE)
def test_every_oracle_trial_meets_the_preconditions_and_has_teeth(uvs, method, n_points, d):
    """pixel_loop_common's preconditions on the delayed trial -- its 16 steps with status 0, every reported frame's discs inside the frame
    with a mask of at least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the (1 + 1e-14) nudge -- and the teeth: each
    misreading of the rule -- the latency ignored, d - 1, d + 1, the noise of step kk instead of k -- at least TEETH_MIN away in q or dq."""
    a, b = lc.oracle_trial(method, n_points, d), lc.oracle_trial(method, n_points, d, True)
    assert (a['status'], a['k_done']) == (0, lc.K) == (b['status'], b['k_done'])
    assert np.array_equal(a['counts'], b['counts']) and a['held'] == b['held'] and np.array_equal(a['fpi_iterations'], b['fpi_iterations'])
    drift = max(float(np.abs(a[key] - b[key]).max() / np.abs(a[key]).max()) for key in ('q', 'f', 'dq', 'err', 'kappa'))
    rim, mask = cc.closest_to_rim(a['discs']), int(a['counts'].min())
    assert all(np.array_equal(a['counts'][k], a['counts'][0]) for k in range(d + 1)), 'the delay line is primed with the step-0 frame'
    teeth = {name: pl.distance(a, lc.oracle_trial(method, n_points, d, False, name)) for name in lc.MISREADINGS}
    print(f'{method} ({2 * n_points},6) d = {d}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, '
          + ', '.join(f'{name} {t:.1e}' for name, t in teeth.items()))
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(a['discs']) and mask >= pl.MASK_MIN
    for name, t in teeth.items():
        assert t >= pl.TEETH_MIN, (name, 'a loop that misread the rule this way would pass the gates')


def test_the_oracle_trials_behind_the_wide_bar_are_calm(uvs):
    """Latency 2 behind pixel_loop_common's bar that is wider than a disc, with a hold, and on the 'window' motion, as the GPU file runs
    them: the same status, k_done, masks and holds under the nudge, logs within CALM_TOL, no pixel within RIM_MIN of a rim; and the loss
    arrives two steps late: the delayed trial's first held step is the undelayed trial's plus two."""
    rows = tuple(tuple(int(v) for v in row) for row in pl.wide_rows(4))
    hold = pl.HOLDS[4]['longer']
    for motion in (None, 'window'):
        a, b = (lc.oracle_trial('GMCKF', 4, 2, nudged, None, rows, hold, motion) for nudged in (False, True))
        assert (a['status'], a['k_done']) == (b['status'], b['k_done']) and a['k_done'] >= 1
        assert np.array_equal(a['counts'], b['counts']) and a['held'] == b['held']
        for key in ('q', 'f', 'dq', 'err', 'kappa'):
            rows_both = min(len(a[key]), len(b[key]))
            with np.errstate(invalid='ignore'):
                d = np.abs(a[key][:rows_both] - b[key][:rows_both]) / np.nanmax(np.abs(a[key]))
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])) and (not np.isfinite(d).any() or np.nanmax(d) <= pl.CALM_TOL), key
        assert cc.closest_to_rim(a['discs']) > pl.RIM_MIN
        now = lc.oracle_trial('GMCKF', 4, 0, False, None, rows, hold, motion)
        first = lambda out: min(steps[0] for steps in out['held'] if steps)   # noqa: E731
        assert any(a['held']) and any(now['held']), 'the bar empties a mask in both'
        if motion is None:
            assert first(a) == first(now) + 2, (a['held'], now['held'])
