"""CPU-only tests of FEATURE PREDICTION (include/uvs_vision.h: the two *_predicted_* entry points; plant.prediction_steps;
engine.camera_closed_loop(predict=)): the numpy rule is the one the header states, header and ctypes table agree and each loop has its
*_aligned_* namesake's operands with `predict` after `assumed`, every refusal comes before any HIP call (host arrays with sentinels no
kernel could use) in the namesake's order, every Python refusal before any device work, the built library holds the 22 + 6 new kernels
without scratch and under no pinned name, the numpy restatements of camera_predicted_common.py are camera_aligned_common's bit for bit at
p = 0, and every CPU trial the GPU file is held to meets pixel_loop_common's preconditions with each applicable misreading of the rule at
least TEETH_MIN away."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_aligned_common as ac
import camera_common as cc
import camera_predicted_common as pc
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_aligned_host import Aligned
from test_camera_grid_host import Buffers, DESIRED
from test_camera_latency_host import PINNED
from test_camera_moving_host import inside, triple_refusals

ARG, SHAPE, METHOD = -1, -2, -4
NAMESAKES = {'uvs_camera_closed_loop_predicted_f64': 'uvs_camera_closed_loop_aligned_f64',
             'uvs_camera_believed_loop_predicted_f64': 'uvs_camera_believed_loop_aligned_f64'}


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the numpy rule
def test_the_rule_on_a_table(uvs):
    steps = uvs.plant.prediction_steps
    table = {(0, 0): [], (5, 0): [], (0, 3): [], (0, 8): [],                                    # no horizon, or no command yet
             (1, 1): [0], (7, 1): [6], (1, 3): [0], (2, 3): [1, 0], (3, 3): [2, 1, 0], (4, 3): [3, 2, 1], (15, 3): [14, 13, 12],
             (5, 8): [4, 3, 2, 1, 0], (8, 8): [7, 6, 5, 4, 3, 2, 1, 0], (9, 8): [8, 7, 6, 5, 4, 3, 2, 1], (20, 8): list(range(19, 11, -1)),
             (5, -1): [], (5, -2 ** 31): [],                                                      # a negative horizon is none
             (9, 9): [8, 7, 6, 5, 4, 3, 2, 1], (30, 2 ** 31 - 1): list(range(29, 21, -1)), (3, 100): [2, 1, 0]}   # a huge one is MAX_LATENCY
    for (k, p), want in table.items():
        assert steps(k, p) == want, (k, p)
    assert steps(2 ** 31 - 1, 2) == [2 ** 31 - 2, 2 ** 31 - 3]
    for k in range(40):
        for p in range(-2, 12):
            c = min(max(p, 0), 8)
            got = steps(k, p)
            assert got == [k - i for i in range(1, c + 1) if k - i >= 0]
            assert len(got) == min(c, k) and all(k - s <= 8 for s in got), 'the commands are among the last eight'
            assert (got[-1] if got else k) == uvs.plant.delayed_step(k, p), "the law's frame is the last step listed"
    with pytest.raises(ValueError):
        steps(-1, 0)
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert 'FEATURE PREDICTION' in header and 'k - 1, k - 2, ..., max(k - p, 0)' in header and 'fma(X_k[r][j], s[j], acc)' in header


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    for new, old in NAMESAKES.items():
        a, b, ta, tb = declared(new), declared(old), types(new), list(types(old))
        at = b.index('const int32_t *assumed') + 1
        b.insert(at, 'const int32_t *predict')
        tb.insert(at, ctypes.c_void_p)
        assert a == b, (new, "the namesake's operands with predict after assumed")
        assert ta == tb, new
        assert getattr(uvs._vision.lib(), new) is not None


# ------------------------------------------------------------------------------------------------------------- C refusals
class Predicted(Aligned):
    """Aligned with a prediction horizon per trial: a host array of sentinels."""
    def __init__(self, uvs, **kw):
        Aligned.__init__(self, uvs, **kw)
        self.predict = np.full(self.T, 7, np.int32)

    def untouched(self):
        return Aligned.untouched(self) and np.all(self.predict == 7)


def loop_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', assumed='own', predict='own', tp='block', occ='rows',
              n_occ=1, hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    own = lambda given, mine: mine.ctypes.data if isinstance(given, str) else given   # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_predicted_f64(
        ref(a['fp']), own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), own(latency, b.latency), own(assumed, b.assumed),
        own(predict, b.predict), b.T if T is None else T, ref(tp), own(occ, b.occ), b.paint.ctypes.data, n_occ, hold, a['q_start'], a['noise'],
        a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'], b.held.ctypes.data, None)


def baseline_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', assumed='own', predict='own', believed='own',
                  n_believed=1, believed_index=None, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    own = lambda given, mine: mine.ctypes.data if isinstance(given, str) else given   # noqa: E731
    return uvs._vision.lib().uvs_camera_believed_loop_predicted_f64(
        ref(a['fp']), own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), own(latency, b.latency), own(assumed, b.assumed),
        own(predict, b.predict), b.T if T is None else T, own(believed, b.cams), n_believed, believed_index, a['q_start'], a['noise'], a['q'],
        a['f'], a['dq'], a['err'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def with_and_without(call):
    """Every refusal with and without a horizon, an assumed latency, a latency and a motion: the four operands are never looked at on the
    host."""
    def all_sixteen(**kw):
        codes = {call(predict=predict, assumed=assumed, latency=latency, motion=motion, **kw)
                 for predict in ('own', None) for assumed in ('own', None) for latency in ('own', None) for motion in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    return all_sixteen


def test_the_loop_refuses_what_the_aligned_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Predicted(uvs)
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
    mckf = Predicted(uvs, n_points=3, method='MCKF')
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
    for predict in ('own', None):
        for assumed in ('own', None):
            for latency in ('own', None):
                triple_refusals(lambda **kw: loop_call(uvs, b, latency=latency, assumed=assumed, predict=predict, **kw), lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_the_baseline_loop_refuses_what_its_aligned_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Predicted(uvs, method='ANALYTICAL')
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
    for predict in ('own', None):
        for assumed in ('own', None):
            for latency in ('own', None):
                triple_refusals(lambda **kw: baseline_call(uvs, b, latency=latency, assumed=assumed, predict=predict, **kw), lib, b.T)
    assert b.untouched(), 'a refused call wrote'


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
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=[0, 1, 8], assumed_latency=[8, 0, 2], **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, guess='device', fused=True, hold=2, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, believed=plant, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, assumed_latency=3, **kw))
    for call in calls:
        for bad in (-1, 9, 2 ** 31, [0, 1, 9], np.array([0, -1, 2]), torch.tensor([0, 1, 100])):
            with pytest.raises(ValueError, match='predict must lie in 0 .. 8'):
                call(predict=bad)
        for bad in ([0, 1], [0, 1, 2, 3], np.zeros(2, np.int64), torch.zeros(4, dtype=torch.int32)):
            with pytest.raises(ValueError, match='predict values for 3 trials'):
                call(predict=bad)
        for bad in (1.0, 0.5, [0.0, 1.0, 2.0], np.zeros(3), torch.zeros(3), True, [True, False, True], 'two', np.zeros((3, 1), np.int64), [[1, 2, 3]]):
            with pytest.raises(ValueError, match='predict is'):
                call(predict=bad)
        for good in (0, 8, [0, 3, 8], np.array([1, 2, 3], np.int32), torch.tensor([1, 2, 3])):
            with pytest.raises(ValueError, match='on the device'):   # accepted as far as the host goes
                call(predict=good)
        with pytest.raises(ValueError, match='on the device'):       # None reaches the refusals that were there
            call(predict=None)
    with pytest.raises(ValueError, match=r'camera_closed_loop: latency must lie in 0 .. 8'):   # latency's refusals come first, under its own name
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=9, assumed_latency=99, predict=99)
    with pytest.raises(ValueError, match=r'camera_closed_loop: assumed_latency must lie in 0 .. 8'):   # then assumed_latency's
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=8, assumed_latency=99, predict=99)
    with pytest.raises(ValueError, match='predict values for 4 trials'):   # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, predict=[1, 2, 3])
    with pytest.raises(ValueError, match='on the device'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, predict=[1, 2, 3, 0])
    with pytest.raises(ValueError, match='on the device'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, latency=2, assumed_latency=1,
                               predict=[1, 2, 3, 0])
    # the two-launch estimator route forms err inside the estimator library: refused, after predict's own refusals, for a valid horizon alone
    with pytest.raises(ValueError, match='predict needs fused=True'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, predict=2)
    with pytest.raises(ValueError, match='predict needs fused=True'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, predict=[0, 0, 0])
    with pytest.raises(ValueError, match='predict must lie in 0 .. 8'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, predict=9)
    bar = [[0, 0, 10, 10, 0, 0, 0, 5]]
    with pytest.raises(ValueError, match='fused=False'):             # the older refusals are still there, and come first
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, predict=99)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=1, predict=[1.5])
    with pytest.raises(ValueError, match='motion_window without target_motion'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, motion_window=(0, 5), predict=99)
    with pytest.raises(ValueError, match='trial_params needs fused=True'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, trial_params={}, predict=99)
    with pytest.raises(ValueError, match='believed_index without believed'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, believed_index=[0, 0, 0], predict=99)
    with pytest.raises(ValueError, match='latencies for 3 trials'):  # the older messages are what they were
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=[0, 1])
    with pytest.raises(ValueError, match='assumed_latency values for 3 trials'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, assumed_latency=[0, 1])


# ------------------------------------------------------------------------------------------------------------- the built library
def test_the_predicted_kernels_are_built_without_scratch(uvs):
    """predicted_frames_kernel: what aligned_frames_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1),
    MCKF (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22 -- and predicted_baseline_kernel at the three shapes
    in both forms; no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    loops = {name: r for name, r in k.items() if 'predicted_frames_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'predicted_frames_kernel(<[^>]*>)', name).group(1) for name in loops}
    assert found == expected and len(loops) == 22, (sorted(found ^ expected), len(loops))
    assert all('PredictedLoopArgs' in name for name in loops)
    baseline = {name: r for name, r in k.items() if 'predicted_baseline_kernel' in name}
    assert {re.search(r'predicted_baseline_kernel(<[^>]*>)', name).group(1) for name in baseline} == \
        {f'<{shape}, {g}>' for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1') for g in (1, 4)}
    assert all('PredictedBaselineArgs' in name for name in baseline)
    for name, r in list(loops.items()) + list(baseline.items()):
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 65536 and r['scratch'] == 0, (name, r)
    new = list(loops) + list(baseline)
    assert len(new) == 22 + 6
    for name in new:
        for pinned in PINNED + ('moving_project_kernel', 'moving_detect_kernel', 'delayed_frames_kernel', 'delayed_baseline_kernel', 'delay_line_kernel',
                                'aligned_frames_kernel', 'aligned_baseline_kernel'):
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel',
                   'camera_scene_kernel', 'moving_target_kernel', 'delayed_frames_kernel', 'aligned_frames_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
    for six in ('scene_baseline_loop_kernel', 'moving_baseline_kernel', 'delayed_baseline_kernel', 'aligned_baseline_kernel'):
        assert sum(six in name for name in k) == 6, six
    assert sum('hold_pairs_kernel' in name for name in k) == 1 and sum('delay_line_kernel' in name for name in k) == 1


# ------------------------------------------------------------------------------------------------------------- the restatements
def same_bits(a, b, keys, where):
    assert (a['status'], a['k_done']) == (b['status'], b['k_done']), where
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (where, key)


@pytest.mark.parametrize('method,n_points', pc.ORACLE)
def test_the_estimator_restatement_is_the_aligned_one_at_no_horizon(uvs, method, n_points):
    """p = 0, bit for bit, at every (d, a) the trials below use: s = 0, X s = 0 and f + 0 = f."""
    for d in (0,) + pc.ORACLE_HORIZONS:
        for a in {0, d}:
            same_bits(pc.estimator_trial(method, n_points, d, a, 0), ac.estimator_trial(method, n_points, d, a),
                      ('q', 'f', 'dq', 'err', 'kappa', 'stats', 'x0', 'f0', 'counts', 'pixels', 'fpi_iterations', 'discs'), (method, n_points, d, a))


@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_the_law_restatement_is_the_aligned_one_at_no_horizon(uvs, n_points):
    """p = 0, bit for bit: h(q_k) - h(q_k) = 0 and f + 0 = f."""
    for d in (0,) + pc.LAW_HORIZONS:
        for a in {0, min(d, 3)}:
            same_bits(pc.law_trial(n_points, d, a, 0), ac.law_trial(n_points, d, a), ('q', 'f', 'dq', 'err', 'stats', 'counts', 'pixels', 'discs'),
                      (n_points, d, a))


@pytest.mark.parametrize('told', ['a = 0', 'a = d'])
@pytest.mark.parametrize('p', pc.ORACLE_HORIZONS)
@pytest.mark.parametrize('method,n_points', pc.ORACLE)
def test_every_estimator_trial_meets_the_preconditions_and_has_teeth(uvs, method, n_points, p, told):
    """pixel_loop_common's preconditions on the trial at d = p that the GPU file is held to -- its 16 steps with status 0, every reported
    frame's discs inside the frame with a mask of at least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the (1 + 1e-14)
    nudge -- and the teeth: the horizon ignored, p - 1, p + 1, a missing term taken as dq_0 (p >= 2) and X_{k-1} in place of X_k, each at
    least TEETH_MIN away in q or dq (or listed in NO_TEETH with its measured distance)."""
    a = 0 if told == 'a = 0' else p
    t, n = pc.estimator_trial(method, n_points, p, a, p), pc.estimator_trial(method, n_points, p, a, p, True)
    assert (t['status'], t['k_done']) == (0, pc.K) == (n['status'], n['k_done'])
    assert np.array_equal(t['counts'], n['counts']) and np.array_equal(t['fpi_iterations'], n['fpi_iterations'])
    drift = max(float(np.abs(t[key] - n[key]).max() / np.abs(t[key]).max()) for key in ('q', 'f', 'dq', 'err', 'kappa'))
    rim, mask = cc.closest_to_rim(t['discs']), int(t['counts'].min())
    teeth = {name: pl.distance(t, pc.estimator_trial(method, n_points, p, a, p, False, name)) for name in pc.applicable(p)}
    print(f'{method} ({2 * n_points},6) d = p = {p}, a = {a}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, '
          + ', '.join(f'{name} {d:.1e}' for name, d in teeth.items()))
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(t['discs']) and mask >= pl.MASK_MIN
    assert set(teeth) == set(pc.MISREADINGS) - ({'clamped'} if p < 2 else set())
    for name, d in teeth.items():
        if ('estimator', method, n_points, p, a, name) in pc.NO_TEETH:
            assert d < pl.TEETH_MIN and name in ('one less', 'one more'), (name, d, 'listed without need')
        else:
            assert d >= pl.TEETH_MIN, (name, d, 'a loop that misread the rule this way would pass the gates')


@pytest.mark.parametrize('p', pc.LAW_HORIZONS)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_every_law_trial_is_fail_free_and_has_teeth(uvs, n_points, p):
    """The law at d = p, a = 0: FAIL-free over 16 steps, calm under the nudge, masks of at least MASK_MIN pixels away from every rim, and
    "p ignored" and "off by one" at least TEETH_MIN away in q or dq (or listed in NO_TEETH with its measured distance)."""
    t, n = pc.law_trial(n_points, p, 0, p), pc.law_trial(n_points, p, 0, p, True)
    assert (t['status'], t['k_done']) == (0, pc.K) == (n['status'], n['k_done']) and np.array_equal(t['counts'], n['counts'])
    drift = max(float(np.abs(t[key] - n[key]).max() / np.abs(t[key]).max()) for key in ('q', 'f', 'dq', 'err'))
    rim, mask = cc.closest_to_rim(t['discs']), int(t['counts'].min())
    teeth = {name: pl.distance(t, pc.law_trial(n_points, p, 0, p, False, name)) for name in pc.applicable(p, estimator=False)}
    print(f'the law ({2 * n_points},6) d = p = {p}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, '
          + ', '.join(f'{name} {d:.1e}' for name, d in teeth.items()))
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(t['discs']) and mask >= pl.MASK_MIN
    for name, d in teeth.items():
        if ('law', n_points, p, name) in pc.NO_TEETH:
            assert d < pl.TEETH_MIN and name in ('one less', 'one more'), (name, d, 'listed without need')
        else:
            assert d >= pl.TEETH_MIN, (name, d, 'a loop that misread the rule this way would pass the gates')


def test_no_teeth_stays_empty():
    assert pc.NO_TEETH == {}
