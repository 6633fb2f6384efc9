"""CPU-only tests of ASSUMED LATENCY (include/uvs_vision.h: the two *_aligned_* entry points; plant.aligned_regressor_step;
engine.camera_closed_loop(assumed_latency=)): the two numpy rules are the ones the header states, header and ctypes table agree and each
loop has its *_delayed_* namesake's operands with `assumed` after `latency`, every refusal comes before any HIP call (host arrays with
sentinels no kernel could use) in the namesake's order, every Python refusal before any device work, the built library holds the 22 + 6 new
kernels without scratch and under no pinned name, the numpy restatement of camera_aligned_common.py is the untouched oracle bit for bit where
the oracle has the case (a = 0: mutation=None; a = 1: mutation='regressor_stale'), and every CPU trial the GPU file is held to meets
pixel_loop_common's preconditions with each misreading of the rule at least TEETH_MIN away."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_aligned_common as ac
import camera_common as cc
import camera_latency_common as lc
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED
from test_camera_latency_host import PINNED, Delayed
from test_camera_moving_host import inside, triple_refusals

ARG, SHAPE, METHOD = -1, -2, -4
NAMESAKES = {'uvs_camera_closed_loop_aligned_f64': 'uvs_camera_closed_loop_delayed_f64',
             'uvs_camera_believed_loop_aligned_f64': 'uvs_camera_believed_loop_delayed_f64'}


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the numpy rules
def test_the_two_rules_on_a_table(uvs):
    reg, law = uvs.plant.aligned_regressor_step, uvs.plant.delayed_step
    table = {(0, 0): (-1, 0), (1, 0): (0, 1), (7, 0): (6, 7), (1000, 0): (999, 1000),          # a = 0: dq_{k-1}, q_k -- the step as it was
             (0, 1): (-1, 0), (1, 1): (-1, 0), (2, 1): (0, 1), (9, 1): (7, 8),
             (0, 3): (-1, 0), (3, 3): (-1, 0), (4, 3): (0, 1), (15, 3): (11, 12),
             (0, 8): (-1, 0), (8, 8): (-1, 0), (9, 8): (0, 1), (20, 8): (11, 12),
             (5, -1): (4, 5), (5, -2 ** 31): (4, 5),                                             # a negative assumed latency is none
             (9, 9): (0, 1), (30, 2 ** 31 - 1): (21, 22), (8, 100): (-1, 0)}                      # a huge one is MAX_LATENCY
    for (k, a), (kr, kq) in table.items():
        assert (reg(k, a), law(k, a)) == (kr, kq), (k, a)
    assert reg(2 ** 31 - 1, 3) == 2 ** 31 - 5
    for k in range(40):
        for a in range(-2, 12):
            c = min(max(a, 0), 8)
            assert reg(k, a) == (k - 1 - c if k - 1 - c >= 0 else -1) and law(k, a) == max(k - c, 0)
            assert k - reg(k, a) <= 9 or reg(k, a) == -1, 'the command is among the last nine'
    with pytest.raises(ValueError):
        reg(-1, 0)
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert 'ASSUMED LATENCY' in header and 'k - 1 - a' in header


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    for new, old in NAMESAKES.items():
        a, b, ta, tb = declared(new), declared(old), types(new), list(types(old))
        at = b.index('const int32_t *latency') + 1
        b.insert(at, 'const int32_t *assumed')
        tb.insert(at, ctypes.c_void_p)
        assert a == b, (new, "the namesake's operands with assumed after latency")
        assert ta == tb, new
        assert getattr(uvs._vision.lib(), new) is not None


# ------------------------------------------------------------------------------------------------------------- C refusals
class Aligned(Delayed):
    """Delayed with an assumed latency per trial: a host array of sentinels."""
    def __init__(self, uvs, **kw):
        Delayed.__init__(self, uvs, **kw)
        self.assumed = np.full(self.T, 7, np.int32)

    def untouched(self):
        return Delayed.untouched(self) and np.all(self.assumed == 7)


def loop_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', assumed='own', tp='block', occ='rows', n_occ=1,
              hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    own = lambda given, mine: mine.ctypes.data if isinstance(given, str) else given   # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_aligned_f64(
        ref(a['fp']), own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), own(latency, b.latency), own(assumed, b.assumed),
        b.T if T is None else T, ref(tp), own(occ, b.occ), b.paint.ctypes.data, n_occ, hold, a['q_start'], a['noise'], a['x0'], a['f0'], a['q'],
        a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'], b.held.ctypes.data, None)


def baseline_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', assumed='own', believed='own', n_believed=1,
                  believed_index=None, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    own = lambda given, mine: mine.ctypes.data if isinstance(given, str) else given   # noqa: E731
    return uvs._vision.lib().uvs_camera_believed_loop_aligned_f64(
        ref(a['fp']), own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), own(latency, b.latency), own(assumed, b.assumed),
        b.T if T is None else T, own(believed, b.cams), n_believed, believed_index, a['q_start'], a['noise'], a['q'], a['f'], a['dq'], a['err'],
        a['status'], a['k_done'], a['stats'], a['pixels'], None)


def with_and_without(call):
    """Every refusal with and without an assumed latency, a latency and a motion: the three operands are never looked at on the host."""
    def all_eight(**kw):
        codes = {call(assumed=assumed, latency=latency, motion=motion, **kw)
                 for assumed in ('own', None) for latency in ('own', None) for motion in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    return all_eight


def test_the_loop_refuses_what_the_delayed_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Aligned(uvs)
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
    mckf = Aligned(uvs, n_points=3, method='MCKF')
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
    for assumed in ('own', None):
        for latency in ('own', None):
            triple_refusals(lambda **kw: loop_call(uvs, b, latency=latency, assumed=assumed, **kw), lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_the_baseline_loop_refuses_what_its_delayed_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Aligned(uvs, method='ANALYTICAL')
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
    for assumed in ('own', None):
        for latency in ('own', None):
            triple_refusals(lambda **kw: baseline_call(uvs, b, latency=latency, assumed=assumed, **kw), lib, b.T)
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
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=[0, 1, 8], **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, guess='device', fused=True, hold=2, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, believed=plant, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=True, **kw))
    for call in calls:
        for bad in (-1, 9, 2 ** 31, [0, 1, 9], np.array([0, -1, 2]), torch.tensor([0, 1, 100])):
            with pytest.raises(ValueError, match='assumed_latency must lie in 0 .. 8'):
                call(assumed_latency=bad)
        for bad in ([0, 1], [0, 1, 2, 3], np.zeros(2, np.int64), torch.zeros(4, dtype=torch.int32)):
            with pytest.raises(ValueError, match='assumed_latency values for 3 trials'):
                call(assumed_latency=bad)
        for bad in (1.0, 0.5, [0.0, 1.0, 2.0], np.zeros(3), torch.zeros(3), True, [True, False, True], 'two', np.zeros((3, 1), np.int64), [[1, 2, 3]]):
            with pytest.raises(ValueError, match='assumed_latency is'):
                call(assumed_latency=bad)
        for good in (0, 8, [0, 3, 8], np.array([1, 2, 3], np.int32), torch.tensor([1, 2, 3])):
            with pytest.raises(ValueError, match='on the device'):   # accepted as far as the host goes
                call(assumed_latency=good)
        with pytest.raises(ValueError, match='on the device'):       # None reaches the refusals that were there
            call(assumed_latency=None)
    with pytest.raises(ValueError, match=r'camera_closed_loop: latency must lie in 0 .. 8'):   # latency's refusals come first, under its own name
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=9, assumed_latency=99)
    with pytest.raises(ValueError, match='assumed_latency values for 4 trials'):   # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, assumed_latency=[1, 2, 3])
    with pytest.raises(ValueError, match='on the device'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, assumed_latency=[1, 2, 3, 0])
    with pytest.raises(ValueError, match='on the device'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, latency=2, assumed_latency=[1, 2, 3, 0])
    bar = [[0, 0, 10, 10, 0, 0, 0, 5]]
    with pytest.raises(ValueError, match='fused=False'):             # the older refusals are still there, and come first
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, assumed_latency=99)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=1, assumed_latency=[1.5])
    with pytest.raises(ValueError, match='motion_window without target_motion'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, motion_window=(0, 5), assumed_latency=99)
    with pytest.raises(ValueError, match='trial_params needs fused=True'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, trial_params={}, assumed_latency=99)
    with pytest.raises(ValueError, match='believed_index without believed'):
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, believed_index=[0, 0, 0], assumed_latency=99)
    with pytest.raises(ValueError, match='latencies for 3 trials'):  # latency's own messages are what they were
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, latency=[0, 1])


# ------------------------------------------------------------------------------------------------------------- the built library
def test_the_aligned_kernels_are_built_without_scratch(uvs):
    """aligned_frames_kernel: what delayed_frames_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1),
    MCKF (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22 -- and aligned_baseline_kernel at the three shapes in
    both forms; no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    loops = {name: r for name, r in k.items() if 'aligned_frames_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'aligned_frames_kernel(<[^>]*>)', name).group(1) for name in loops}
    assert found == expected and len(loops) == 22, (sorted(found ^ expected), len(loops))
    assert all('AlignedLoopArgs' in name for name in loops)
    baseline = {name: r for name, r in k.items() if 'aligned_baseline_kernel' in name}
    assert {re.search(r'aligned_baseline_kernel(<[^>]*>)', name).group(1) for name in baseline} == \
        {f'<{shape}, {g}>' for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1') for g in (1, 4)}
    assert all('AlignedBaselineArgs' in name for name in baseline)
    for name, r in list(loops.items()) + list(baseline.items()):
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 65536 and r['scratch'] == 0, (name, r)
    new = list(loops) + list(baseline)
    assert len(new) == 22 + 6
    for name in new:
        for pinned in PINNED + ('moving_project_kernel', 'moving_detect_kernel', 'delayed_frames_kernel', 'delayed_baseline_kernel', 'delay_line_kernel'):
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel',
                   'camera_scene_kernel', 'moving_target_kernel', 'delayed_frames_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
    for six in ('scene_baseline_loop_kernel', 'moving_baseline_kernel', 'delayed_baseline_kernel'):
        assert sum(six in name for name in k) == 6, six
    assert sum('hold_pairs_kernel' in name for name in k) == 1 and sum('delay_line_kernel' in name for name in k) == 1


# ------------------------------------------------------------------------------------------------------------- the restatement, the oracle
def same_run(a, b, where):
    assert (a['status'], a['k_done']) == (b['status'], b['k_done']), where
    for key in ('q', 'f', 'dq', 'err', 'kappa', 'stats', 'x0', 'f0', 'counts', 'pixels', 'fpi_iterations', 'discs'):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (where, key)


@pytest.mark.parametrize('d', [0, 1, 2])
@pytest.mark.parametrize('method,n_points', ac.ORACLE)
def test_the_restatement_is_the_untouched_oracle_where_it_has_the_case(uvs, method, n_points, d):
    """Bit for bit: a = 0 against oracle.pixel_loop.run (mutation=None) and a = 1 against its mutation='regressor_stale', both through
    camera_latency_common.delayed_sensor at latency d."""
    from oracle import pixel_loop
    import camera_moving_common as mc
    plant, cfg = pl.plant_of(n_points), mc.oracle_settings(n_points)
    noise = mc.oracle_noise(n_points)[:ac.K]
    for a, mutation in ((0, None), (1, 'regressor_stale')):
        want = pixel_loop.run(plant, mc.oracle_start(), pl.DESIRED[:2 * n_points], noise, pl.DT, ac.K, cfg['gain'], method, cfg['kernel_bw'], False,
                              ac.K, pl.FPI_THRESHOLD, pl.FPI_EPOCH_MAX, pl.REG, pl.ANNEAL_SPAN, initial_guess=True, radius=ac.RADIUS,
                              sensor=lc.delayed_sensor(d), mutation=mutation)
        assert (want['status'], want['k_done']) == (0, ac.K)
        same_run(ac.estimator_trial(method, n_points, d, a), want, (method, n_points, d, a))
    if d:
        same_run(ac.estimator_trial(method, n_points, d, 0), lc.oracle_trial(method, n_points, d), (method, n_points, d, 'the latency file\'s trial'))
    told = pl.distance(ac.estimator_trial(method, n_points, d, 0), ac.estimator_trial(method, n_points, d, 1))
    print(f'{method} ({2 * n_points},6) d = {d}: a = 1 is {told:.1e} from a = 0')
    assert told >= pl.TEETH_MIN


@pytest.mark.parametrize('a', ac.ORACLE_ASSUMED)
@pytest.mark.parametrize('method,n_points', ac.ORACLE)
def test_every_estimator_trial_meets_the_preconditions_and_has_teeth(uvs, method, n_points, a):
    """pixel_loop_common's preconditions on the trial at d = a that the GPU file is held to -- its 16 steps with status 0, every reported
    frame's discs inside the frame with a mask of at least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the (1 + 1e-14)
    nudge -- and the teeth: the assumed latency ignored, a - 1, a + 1, and the regressor clamped to dq_0 instead of zero, each at least
    TEETH_MIN away in q or dq (or listed in NO_TEETH with its measured distance)."""
    t, n = ac.estimator_trial(method, n_points, a, a), ac.estimator_trial(method, n_points, a, a, True)
    assert (t['status'], t['k_done']) == (0, ac.K) == (n['status'], n['k_done'])
    assert np.array_equal(t['counts'], n['counts']) and np.array_equal(t['fpi_iterations'], n['fpi_iterations'])
    drift = max(float(np.abs(t[key] - n[key]).max() / np.abs(t[key]).max()) for key in ('q', 'f', 'dq', 'err', 'kappa'))
    rim, mask = cc.closest_to_rim(t['discs']), int(t['counts'].min())
    teeth = {name: pl.distance(t, ac.estimator_trial(method, n_points, a, a, False, name)) for name in ac.MISREADINGS}
    print(f'{method} ({2 * n_points},6) d = a = {a}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, '
          + ', '.join(f'{name} {d:.1e}' for name, d in teeth.items()))
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(t['discs']) and mask >= pl.MASK_MIN
    for name, d in teeth.items():
        if ('estimator', method, n_points, a, name) in ac.NO_TEETH:
            assert d < pl.TEETH_MIN and name in ('one less', 'one more'), (name, d, 'listed without need')
        else:
            assert d >= pl.TEETH_MIN, (name, d, 'a loop that misread the rule this way would pass the gates')


@pytest.mark.parametrize('a', ac.LAW_ASSUMED)
@pytest.mark.parametrize('n_points', [4, 3, 1])
def test_every_law_trial_is_fail_free_and_has_teeth(uvs, n_points, a):
    """The law at d = a: FAIL-free over 16 steps, calm under the nudge, masks of at least MASK_MIN pixels away from every rim, and "a
    ignored" and "off by one" at least TEETH_MIN away in q or dq (or listed in NO_TEETH with its measured distance)."""
    t, n = ac.law_trial(n_points, a, a), ac.law_trial(n_points, a, a, True)
    assert (t['status'], t['k_done']) == (0, ac.K) == (n['status'], n['k_done']) and np.array_equal(t['counts'], n['counts'])
    drift = max(float(np.abs(t[key] - n[key]).max() / np.abs(t[key]).max()) for key in ('q', 'f', 'dq', 'err'))
    rim, mask = cc.closest_to_rim(t['discs']), int(t['counts'].min())
    teeth = {name: pl.distance(t, ac.law_trial(n_points, a, a, False, name)) for name in ('ignored', 'one less', 'one more')}
    print(f'the law ({2 * n_points},6) d = a = {a}: calm {drift:.1e}, rim {rim:.1e}, smallest mask {mask}, '
          + ', '.join(f'{name} {d:.1e}' for name, d in teeth.items()))
    assert drift <= pl.CALM_TOL and rim > pl.RIM_MIN and inside(t['discs']) and mask >= pl.MASK_MIN
    for name, d in teeth.items():
        if ('law', n_points, a, name) in ac.NO_TEETH:
            assert d < pl.TEETH_MIN and name in ('one less', 'one more'), (name, d, 'listed without need')
        else:
            assert d >= pl.TEETH_MIN, (name, d, 'a loop that misread the rule this way would pass the gates')
