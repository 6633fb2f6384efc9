"""CPU-only tests of holding a lost disc's last detection (include/uvs_vision.h: uvs_camera_closed_loop_held_f64, uvs_hold_features_f64;
plant.hold_features; engine.camera_closed_loop(hold=...), engine.hold_features): the numpy rule agrees with a plain restatement over the
scenes of tests/camera_hold_common.py and over random count patterns, those scenes are the cover schedules their names say (from host
frames), header and ctypes table agree on the two entry points, every refusal comes before any HIP call (host arrays with sentinels no
kernel could use) and every Python refusal before any device work, and the built library holds the 22 instantiations of camera_held_kernel
next to the 22 + 22 + 22 that were there, none with a private segment."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_hold_common as hc
import camera_occluders_common as oc
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED

ARG, SHAPE, METHOD = -1, -2, -4
LOOP, OCCLUDED, STEP = 'uvs_camera_closed_loop_held_f64', 'uvs_camera_closed_loop_occluded_f64', 'uvs_hold_features_f64'


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


@pytest.fixture(scope='module')
def discs(uvs):
    return uvs.SyntheticPlant.ur10().discs(hc.Q_START)


# ------------------------------------------------------------------------------------------------------------- the scenes
def test_the_scenes_are_the_cover_schedules_their_names_say(uvs, discs):
    scenes = hc.scenes(discs)
    clear = cc.host_counts(uvs.plant.render_discs(discs))
    assert np.all(clear > 150), 'four whole discs at the start pose'
    counts = {name: hc.host_schedule(uvs, discs, rows) for name, rows in scenes.items()}
    for name, c in counts.items():
        assert np.array_equal(c[:, 2:], np.broadcast_to(clear[2:], (hc.K, 2))), (name, 'blue and pink are never touched')
    # red_run: one run of n >= 2 empty red masks, not at step 0, with partial covers on both sides of it; green never touched
    (first, n), = hc.runs(counts['red_run'][:, hc.RED])
    assert n >= 2 and first >= 1 and first + n < hc.K, (first, n)
    assert 0 < counts['red_run'][first - 1, hc.RED] < clear[hc.RED] and 0 < counts['red_run'][first + n, hc.RED] < clear[hc.RED]
    assert np.all(counts['red_run'][:, hc.GREEN] == clear[hc.GREEN])
    assert hc.outcome(counts['red_run'], 0) == (first, [0, 0, 0, 0])
    assert hc.outcome(counts['red_run'], n) == (hc.K, [n, 0, 0, 0]) and hc.outcome(counts['red_run'], n + 5) == (hc.K, [n, 0, 0, 0])
    assert hc.outcome(counts['red_run'], n - 1) == (first + n - 1, [n - 1, 0, 0, 0])
    # step0: red is empty from the first frame on
    assert hc.runs(counts['step0'][:, hc.RED]) == [(0, hc.K)] and hc.outcome(counts['step0'], hc.K) == (0, [0, 0, 0, 0])
    # twice: two runs with detections in between, the second the longer; a counter that does not reset would run out in the second
    (a, la), (b, lb) = hc.runs(counts['twice'][:, hc.RED])
    assert (a, la, b, lb) == (2, 2, 6, hc.RESET_HOLD) and a + la < b and la < lb < la + lb and b + lb < hc.K
    assert np.all(counts['twice'][a + la:b, hc.RED] == clear[hc.RED])
    assert hc.outcome(counts['twice'], hc.RESET_HOLD) == (hc.K, [la + lb, 0, 0, 0])
    assert hc.outcome(counts['twice'], hc.RESET_HOLD - 1) == (b + lb - 1, [la + lb - 1, 0, 0, 0])
    # two_discs: red and green over overlapping, different ranges
    assert hc.runs(counts['two_discs'][:, hc.RED]) == [(3, 3)] and hc.runs(counts['two_discs'][:, hc.GREEN]) == [(4, 4)]
    assert hc.outcome(counts['two_discs'], 4) == (hc.K, [3, 4, 0, 0]) and hc.outcome(counts['two_discs'], 3) == (7, [3, 3, 0, 0])
    assert hc.outcome(counts['two_discs'], 2) == (5, [2, 2, 0, 0])


def test_the_bars_of_the_moving_arm_are_wider_than_a_disc(uvs, discs):
    for bar in (hc.wide_bar(), hc.counter_bar()):
        assert bar[2] > 2 * discs[:, 2].max() + 3 and bar[3] == cc.SIDE and bar[4] != 0
    goal = np.stack([DESIRED[0::2], DESIRED[1::2], np.full(4, 8.01)], axis=1)
    counts = hc.host_schedule(uvs, goal, [hc.wide_bar()])
    assert all(len(hc.runs(counts[:, j])) == 1 and hc.runs(counts[:, j])[0][1] >= 2 for j in range(4)), 'every disc at the goal is emptied'
    assert np.all(counts[0] > 0), 'and none at step 0'
    both = hc.host_schedule(uvs, goal, [hc.wide_bar(), hc.counter_bar()])
    assert len({tuple(hc.runs(both[:, j])) for j in range(4)}) >= 3, 'different discs, different ranges'


# ------------------------------------------------------------------------------------------------------------- the rule
def same(a, b):
    return np.array_equal(cc.bits(np.asarray(a, float)), cc.bits(np.asarray(b, float)))


def check_rule(uvs, f, f_prev, pixels, miss, hold):
    before = [None if a is None else np.array(a) for a in (f, f_prev, pixels, miss)]
    got = uvs.plant.hold_features(f, f_prev, pixels, miss, hold)
    want = hc.hold_restated(f, f_prev, pixels, miss, hold)
    assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2].dtype == np.int32 and got[1].dtype == np.asarray(miss).dtype
    for a, b in zip((f, f_prev, pixels, miss), before):
        assert (a is None and b is None) or same(a, b) or np.array_equal(a, b), 'an argument was written'
    return got


def test_hold_features_agrees_with_a_plain_restatement(uvs, discs):
    rng = np.random.default_rng(5)
    seen_held = seen_nan = 0
    for name, rows in hc.scenes(discs).items():
        counts = hc.host_schedule(uvs, discs, rows)
        for hold in (0, 1, 2, 3, hc.K):
            miss, f_prev, total = np.zeros((1, 4), np.int32), None, np.zeros(4, int)
            for k in range(hc.K):
                f = rng.standard_normal((1, 8)) + 100.0
                f[0, np.repeat(counts[k] == 0, 2)] = np.nan          # what the detector reports for an empty mask, noise added or not
                f_new, miss, held = check_rule(uvs, f, f_prev, counts[k][None], miss, hold)
                if f_prev is not None:                               # a held pair is the previous row's, bit for bit; z is +0.0 there
                    pairs = np.repeat(held[0] == 1, 2)
                    assert same(f_new[0, pairs], f_prev[0, pairs]) and not np.signbit(f_new[0, pairs] - f_prev[0, pairs]).any()
                assert same(f_new[0, np.repeat(held[0] == 0, 2)], f[0, np.repeat(held[0] == 0, 2)])
                total += held[0]
                seen_held += int(held.sum())
                if np.isnan(f_new).any():
                    seen_nan += 1
                    assert (k, total.tolist()) == hc.outcome(counts, hold), (name, hold)
                    break
                f_prev = f_new
            else:
                assert (hc.K, total.tolist()) == hc.outcome(counts, hold), (name, hold)
    assert seen_held > 30 and seen_nan > 8
    # random count patterns, counters and holds, several trials at once, the three colour counts; a NaN in f_prev is held like any value
    for n in (1, 3, 4):
        for _ in range(60):
            T = int(rng.integers(1, 6))
            pixels = rng.integers(0, 3, (T, n)) * rng.integers(0, 2, (T, n))
            miss = rng.integers(0, 4, (T, n)).astype(np.int64)
            f, f_prev = rng.standard_normal((T, 2 * n)), rng.standard_normal((T, 2 * n))
            f[np.repeat(pixels == 0, 2, axis=1)] = np.nan
            f_prev[rng.random((T, 2 * n)) < 0.1] = np.nan
            hold = int(rng.integers(0, 5))
            check_rule(uvs, f, f_prev, pixels, miss, hold)
            got = check_rule(uvs, f, None, pixels, miss, hold)
            assert not got[2].any() and np.array_equal(got[1], np.where(pixels == 0, miss, 0)), 'step 0 holds nothing'
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match='hold'):
            uvs.plant.hold_features(np.zeros((1, 8)), None, np.ones((1, 4), int), np.zeros((1, 4), int), bad)
    with pytest.raises(ValueError):
        uvs.plant.hold_features(np.zeros((1, 8)), None, np.ones((1, 3), int), np.zeros((1, 3), int), 1)
    with pytest.raises(ValueError, match='integers'):
        uvs.plant.hold_features(np.zeros((1, 8)), None, np.ones((1, 4)), np.zeros((1, 4), int), 1)


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    held, occluded = declared(LOOP), declared(OCCLUDED)
    assert len(occluded) == 20 == len(types(OCCLUDED)) and len(held) == 22 == len(types(LOOP))
    assert held[:6] == occluded[:6] and held[6] == 'int32_t hold' and held[7:20] == occluded[6:19], 'hold goes after n_occ'
    assert held[20] == 'int32_t *held' and held[21] == occluded[19] == 'void *stream', 'held goes after pixels'
    assert held[19] == 'int32_t *pixels'
    assert types(LOOP)[:6] == types(OCCLUDED)[:6] and types(LOOP)[6] is ctypes.c_int32 and types(LOOP)[7:] == [ctypes.c_void_p] * 15
    step = declared(STEP)
    assert step == ['int64_t T', 'int32_t n_points', 'int32_t hold', 'int32_t k', 'const double *f_prev_row', 'double *f_row',
                    'const int32_t *pixels_row', 'int32_t *miss', 'int32_t *held_row', 'void *stream']
    assert types(STEP) == [ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 6
    for name in (LOOP, STEP):
        assert getattr(uvs._vision.lib(), name) is not None


# ------------------------------------------------------------------------------------------------------------- C refusals
def loop_call(uvs, b, T=None, tp='block', occ='rows', n_occ=1, hold=2, held='rows', **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp, cam=b.cam)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return getattr(uvs._vision.lib(), LOOP)(ref(a['fp']), ref(a['cam']), b.T if T is None else T, ref(tp),
                                            b.occ.ctypes.data if isinstance(occ, str) else occ, n_occ, hold, a['q_start'], a['noise'], a['x0'],
                                            a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'],
                                            a['pixels'], b.held.ctypes.data if isinstance(held, str) else held, None)


def with_hold(b):
    b.occ = np.full(b.T * 4 * 8, 7, np.int32)
    b.held = np.full(b.T * 4, 7, np.int32)
    return b


def test_the_loop_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), with_hold(Buffers(uvs))
    # what the occluded entry point refuses, in its order
    for name in ('fp', 'cam', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
        assert loop_call(uvs, b, **{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    assert loop_call(uvs, b, T=-1) == ARG
    bad = Buffers(uvs)
    bad.fp.steps = 0
    assert loop_call(uvs, b, fp=bad.fp) == ARG
    bad = Buffers(uvs)
    bad.fp.lanes_per_filter = 2
    assert loop_call(uvs, b, fp=bad.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    assert loop_call(uvs, b, cam=Buffers(uvs, n_points=3).cam) == SHAPE and loop_call(uvs, b, cam=Buffers(uvs, n_points=2).cam) == ARG
    bad = Buffers(uvs)
    bad.fp.method = 1                                                # UVS_METHOD_ANALYTICAL
    assert loop_call(uvs, b, fp=bad.fp) == METHOD
    mckf = with_hold(Buffers(uvs, n_points=3, method='MCKF'))
    mckf.fp.m = 6
    assert loop_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
    for n_in in (0, -3):
        assert loop_call(uvs, b, tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    for n_occ in (-1, 5, 2 ** 31 - 1):
        assert loop_call(uvs, b, n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
    for n_occ in (1, 4):
        assert loop_call(uvs, b, occ=None, n_occ=n_occ) == ARG and b'NULL occ' in lib.uvs_vision_last_error(), n_occ
    # its own, after those: a bad n_occ and a bad hold together give n_occ's text
    for hold in (-1, -2 ** 31):
        assert loop_call(uvs, b, hold=hold) == ARG and b'hold' in lib.uvs_vision_last_error(), hold
        assert loop_call(uvs, b, hold=hold, T=0) == ARG, 'refusals come before T == 0'
    assert loop_call(uvs, b, hold=-1, n_occ=9) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert loop_call(uvs, b, hold=-1, fp=bad.fp) == METHOD
    assert b.untouched() and mckf.untouched() and np.all(b.occ == 7) and np.all(b.held == 7), 'a refused call wrote'


def test_nothing_to_do_is_ok(uvs):
    lib, b = uvs._vision.lib(), with_hold(Buffers(uvs))
    assert loop_call(uvs, b, T=0, tp=None) == 0 and lib.uvs_vision_last_error() == b'', 'a NULL tp is allowed: every member NULL'
    assert loop_call(uvs, b, T=0, occ=None, n_occ=0, hold=5) == 0, 'no occluders and hold > 0 is legal: a disc that leaves the frame is held'
    assert loop_call(uvs, b, T=0, hold=0) == 0 and loop_call(uvs, b, T=0, hold=2 ** 31 - 1, held=None) == 0
    assert loop_call(uvs, b, T=0, tp=None, noise=None, q=None, f=None, dq=None, err=None, kappa=None, pixels=None, held=None) == 0
    assert b.untouched() and np.all(b.occ == 7) and np.all(b.held == 7)


def test_the_stepwise_kernel_refuses_before_it_launches(uvs):
    lib = uvs._vision.lib()
    f, f_prev, pixels, miss, held = np.full(8, 7.0), np.full(8, 7.0), np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7, np.int32)
    P = lambda a: None if a is None else a.ctypes.data               # noqa: E731
    call = lambda T=1, n=4, hold=1, k=1, f_prev=f_prev, f=f, pixels=pixels, miss=miss, held=held: lib.uvs_hold_features_f64(   # noqa: E731
        T, n, hold, k, P(f_prev), P(f), P(pixels), P(miss), P(held), None)
    for name in ('f', 'pixels', 'miss'):
        assert call(**{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    assert call(T=-1) == ARG and call(n=2) == ARG and b'n_points' in lib.uvs_vision_last_error()
    assert call(hold=-1) == ARG and b'hold' in lib.uvs_vision_last_error()
    assert call(k=-1) == ARG and b'k must' in lib.uvs_vision_last_error()
    assert call(f_prev=None) == ARG and b'f_prev_row' in lib.uvs_vision_last_error()
    assert call(T=0, hold=-1) == ARG, 'refusals come before T == 0'
    assert call(T=0) == 0 and call(T=0, k=0, f_prev=None, held=None, hold=0) == 0 and lib.uvs_vision_last_error() == b''
    assert all(np.all(a == 7) for a in (f, f_prev, pixels, miss, held)), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python refusals
def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these must be a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    eng, plant = uvs.engine, uvs.SyntheticPlant.ur10()
    q = torch.zeros((2, 6), dtype=torch.float64)
    fp = eng.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    analytical = eng.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    bar = [hc.wide_bar()]
    calls = (lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, occluders=bar, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, believed=plant, occluders=bar, **kw))
    for call in calls:
        for hold in (-1, 1.5, 2.0, True, None, '3', 2 ** 31):
            with pytest.raises(ValueError, match='hold is a number of steps'):
                call(hold=hold)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=2)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=2, believed=plant)
    with pytest.raises(ValueError, match='fused=True'):                                  # the older refusals are still there
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), trial_params={}, hold=2)
    with pytest.raises(ValueError, match='integers'):
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, occluders=[[0.5] * 8], hold=2)
    # hold = 0 and numpy integers are accepted as far as the host goes: the next refusal is the device's
    for hold in (0, np.int32(0), np.int64(4)):
        with pytest.raises(ValueError, match='on the device'):
            eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, hold=hold)
    f = torch.zeros((2, 8), dtype=torch.float64)
    for bad in (dict(hold=-1), dict(hold=1.0), dict(hold=1, k=-1), dict(hold=1, k=0.5)):
        kw = dict(dict(k=0), **bad)
        with pytest.raises(ValueError, match='hold is a number|k is a step count'):
            eng.hold_features(f, None, None, None, **kw)
    with pytest.raises(ValueError, match='f_prev'):
        eng.hold_features(f, None, None, None, 1, 3)


# ------------------------------------------------------------------------------------------------------------- the built library
def test_the_held_instantiations_are_built_without_scratch(uvs):
    """camera_held_kernel: what camera_occluded_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1), MCKF
    (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22, MCKF at (6,6,2) the one documented absence -- and the
    stepwise hold kernel, whose name contains none of the pinned ones."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    held = {name: r for name, r in k.items() if 'camera_held_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'camera_held_kernel(<[^>]*>)', name).group(1) for name in held}
    assert found == expected and len(held) == 22, (sorted(found ^ expected), len(held))
    for name, r in held.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
        for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_analytical_', 'camera_believed_'):
            assert pinned not in name, (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    stepwise = {name: r for name, r in k.items() if 'hold_pairs_kernel' in name}
    assert len(stepwise) == 1 and all(r['scratch'] == 0 and r['lds'] == 0 and r['wg'] == 256 for r in stepwise.values()), stepwise
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2 and not any(kernel in name for name in stepwise), kernel
