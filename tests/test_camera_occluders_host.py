"""CPU-only tests of the occluders (include/uvs_vision.h: uvs_occluder and the four *_occluded_* entry points; plant.occluder_rects,
plant.render_discs(occluders=...), plant.CameraRobot(occluders=...); engine.*(occluders=...)): header and ctypes table agree, every refusal
comes before any HIP call (host arrays with sentinels no kernel could use) and every Python refusal before any device work, the integer rule
agrees with a plain restatement on its extremes, the scenes of tests/camera_occluders_common.py are the cases their names say, and the built
library holds the documented instantiations of camera_occluded_kernel next to the 22 + 22 that were there, none with a private segment."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_occluders_common as oc
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED

ARG, SHAPE, METHOD = -1, -2, -4
LOOP = 'uvs_camera_closed_loop_occluded_f64'


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    count = lambda fn: len(uvs._vision.SYMBOLS[fn][1])              # noqa: E731
    grid, loop = declared('uvs_camera_closed_loop_grid_f64'), declared(LOOP)
    assert len(loop) == 20 == count(LOOP) and getattr(uvs._vision.lib(), LOOP) is not None
    assert loop[:4] == grid[:4] and loop[6:] == grid[4:], 'the fourteen operands of the grid call, in its order'
    assert loop[4] == 'const uvs_occluder *occ' and loop[5] == 'int32_t n_occ'
    for name, base, extra in (('uvs_render_discs_occluded_u8', 'uvs_render_discs_u8', 4), ('uvs_disc_features_occluded_f64', 'uvs_disc_features_f64', 3),
                              ('uvs_camera_features_occluded_f64', 'uvs_camera_features_f64', 3)):
        new, old = declared(name), declared(base)
        assert len(new) == len(old) + extra == count(name) and count(base) == len(old), name
        assert [a for a in new if a not in ('const uvs_occluder *occ', 'int32_t n_occ', 'int32_t k', 'int32_t shade')] == old, name
    body = re.search(r'typedef struct uvs_occluder \{(.*?)\} uvs_occluder;', header, re.S).group(1)
    fields = re.findall(r'(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert fields == [f[0] for f in uvs._vision.Occluder._fields_] == list(uvs.plant.OCCLUDER_FIELDS)
    assert ctypes.sizeof(uvs._vision.Occluder) == 32 and all(f[1] is ctypes.c_int32 for f in uvs._vision.Occluder._fields_)
    assert int(re.search(r'#define UVS_CAMERA_MAX_OCCLUDERS (\d+)', header).group(1)) == uvs._vision.MAX_OCCLUDERS == uvs.plant.MAX_OCCLUDERS == 4


# ------------------------------------------------------------------------------------------------------------- C refusals
def loop_call(uvs, b, T=None, tp='block', occ='rows', n_occ=1, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp, cam=b.cam)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return getattr(uvs._vision.lib(), LOOP)(ref(a['fp']), ref(a['cam']), b.T if T is None else T, ref(tp),
                                            b.occ.ctypes.data if isinstance(occ, str) else occ, n_occ, a['q_start'], a['noise'], a['x0'],
                                            a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'],
                                            a['pixels'], None)


def with_occluders(b):
    b.occ = np.full(b.T * 4 * 8, 7, np.int32)
    return b


def test_the_loop_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), with_occluders(Buffers(uvs))
    # the refusals of the grid entry point, in its order
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
    mckf = with_occluders(Buffers(uvs, n_points=3, method='MCKF'))
    mckf.fp.m = 6
    assert loop_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
    for n_in in (0, -3):
        assert loop_call(uvs, b, tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    # ... which come first: a bad method and a bad n_occ together give the method's code, a bad n_in and a bad n_occ the n_in's text
    assert loop_call(uvs, b, fp=bad.fp, n_occ=9) == METHOD
    assert loop_call(uvs, b, tp=b.trial_params(uvs, n_in=0), n_occ=9) == ARG and b'n_in' in lib.uvs_vision_last_error()
    # its own
    for n_occ in (-1, 5, 2 ** 31 - 1):
        assert loop_call(uvs, b, n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
    for n_occ in (1, 4):
        assert loop_call(uvs, b, occ=None, n_occ=n_occ) == ARG and b'NULL occ' in lib.uvs_vision_last_error(), n_occ
    assert loop_call(uvs, b, T=0, n_occ=5) == ARG and loop_call(uvs, b, T=0, occ=None) == ARG, 'refusals come before T == 0'
    assert b.untouched() and mckf.untouched() and np.all(b.occ == 7), 'a refused call wrote'


def test_a_null_block_and_nothing_to_do_are_ok(uvs):
    lib, b = uvs._vision.lib(), with_occluders(Buffers(uvs))
    assert loop_call(uvs, b, T=0, tp=None) == 0 and lib.uvs_vision_last_error() == b'', 'a NULL tp is allowed: every member NULL'
    assert loop_call(uvs, b, T=0) == 0 and loop_call(uvs, b, T=0, occ=None, n_occ=0) == 0 and loop_call(uvs, b, T=0, tp=None, n_occ=4) == 0
    assert loop_call(uvs, b, T=0, tp=None, noise=None, q=None, f=None, dq=None, err=None, kappa=None, pixels=None) == 0
    assert b.untouched() and np.all(b.occ == 7)


def test_the_stand_alone_kernels_refuse_before_they_launch(uvs):
    lib = uvs._vision.lib()
    cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
    discs, f, q, occ = np.full(12, 7.0), np.full(8, 7.0), np.full(6, 7.0), np.full(32, 7, np.int32)
    frames = np.full(256 * 256 * 3 + 16, 7, np.uint8)
    fr = (frames.ctypes.data + 15) // 16 * 16
    P = lambda a: a.ctypes.data                                      # noqa: E731
    render = lambda n_occ=1, k=0, shade=32, occ_ptr=P(occ), T=1, bg=96: lib.uvs_render_discs_occluded_u8(   # noqa: E731
        T, P(discs), 4, bg, occ_ptr, n_occ, k, shade, fr, 256 * 256 * 3, None)
    features = lambda n_occ=1, k=0, occ_ptr=P(occ), T=1, n=4: lib.uvs_disc_features_occluded_f64(T, P(discs), n, occ_ptr, n_occ, k, None, P(f), None, None)   # noqa: E731
    camera = lambda n_occ=1, k=0, occ_ptr=P(occ), T=1, out=P(f): lib.uvs_camera_features_occluded_f64(   # noqa: E731
        ctypes.byref(cam), T, P(q), None, 0.0, None, occ_ptr, n_occ, k, None, out, None, None, None)
    for call in (render, features, camera):
        for n_occ in (-1, 5):
            assert call(n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error()
        assert call(occ_ptr=None) == ARG and b'NULL occ' in lib.uvs_vision_last_error()
        assert call(k=-1) == ARG and b'k must' in lib.uvs_vision_last_error()
        assert call(T=-1) == ARG
        assert call(T=0) == 0 and call(T=0, occ_ptr=None, n_occ=0) == 0 and lib.uvs_vision_last_error() == b''
        assert call(T=0, n_occ=5) == ARG, 'refusals come before T == 0'
    for shade in (-1, 250, 255):
        assert render(shade=shade) == ARG and b'shade' in lib.uvs_vision_last_error()
    # the namesake's refusals come first
    assert render(bg=250, n_occ=9) == ARG and b'background' in lib.uvs_vision_last_error()
    assert features(n=2, n_occ=9) == ARG and b'n_colours' in lib.uvs_vision_last_error()
    assert camera(out=None, n_occ=9) == ARG and b'f_out' in lib.uvs_vision_last_error()
    assert all(np.all(a == 7) for a in (discs, f, q, occ, frames)), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python refusals
BAD_SPECS = [([[0] * 7], 'integers'), ([[0.5] * 8], 'integers'), ([[[[0] * 8]]], 'integers'), ([[0] * 8] * 5, 'at most 4'),
             ([[2 ** 31] + [0] * 7], 'int32'), ([[[0] * 8]] * 3, '3 trials of occluders for 2'), ('bar', 'integers')]


def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these must be a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    eng, plant = uvs.engine, uvs.SyntheticPlant.ur10()
    discs, q = torch.zeros((2, 4, 3), dtype=torch.float64), torch.zeros((2, 6), dtype=torch.float64)
    fp = eng.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    analytical = eng.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    bar = [oc.sweeping_bar()]
    calls = (lambda **kw: eng.render_discs(discs, **kw), lambda **kw: eng.disc_features(discs, **kw), lambda **kw: eng.camera_features(plant, q, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, **kw), lambda **kw: eng.occluders(kw['occluders'], 2))
    for call in calls:
        for spec, text in BAD_SPECS:
            with pytest.raises(ValueError, match=text):
                call(occluders=spec)
    for call in calls[:3]:
        for k in (-1, 1.5, 2 ** 31):
            with pytest.raises(ValueError, match='k is a step count'):
                call(occluders=bar, k=k)
    for shade in (-1, 250, 31.5):
        with pytest.raises(ValueError, match='shade'):
            eng.render_discs(discs, occluders=bar, shade=shade)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar)
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, believed=plant)
    with pytest.raises(ValueError, match='4 trials of occluders for 3'):                 # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, trial_params={'source': [0, 1, 0]}, occluders=[bar] * 4)
    with pytest.raises(ValueError, match='fused=True'):                                  # the older refusals are still there
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), trial_params={}, occluders=bar)
    # the numpy side
    for spec, text in BAD_SPECS[:5]:
        with pytest.raises(ValueError, match=text):
            uvs.plant.render_discs(np.zeros((2, 4, 3)), occluders=spec)
    for kw in (dict(shade=250), dict(shade=-1), dict(k=-1)):
        with pytest.raises(ValueError):
            uvs.plant.render_discs(np.zeros((4, 3)), occluders=bar, **kw)
    with pytest.raises(ValueError, match='k must'):
        uvs.plant.occluder_rects(bar, -1)
    with pytest.raises(ValueError, match='shade'):
        uvs.plant.CameraRobot(plant, occluders=bar, shade=250)
    with pytest.raises(ValueError, match='at most 4'):
        uvs.plant.CameraRobot(plant, occluders=bar * 5)


# ------------------------------------------------------------------------------------------------------------- the rule
def test_rects_agree_with_a_plain_restatement_on_the_extremes(uvs):
    rows = dict(oc.extremes())
    for name in oc.STATIC_SCENES:
        for key, cover in oc.static_covers(oc.scene(name)).items():
            rows.update({f'{name}_{key}_{i}': row for i, row in enumerate(cover)})
    rows['bar'], rows['bar_window'] = oc.sweeping_bar(), oc.sweeping_bar(4, 7)
    seen_empty = seen_full = 0
    for key, row in rows.items():
        for k in sorted(set(oc.STEPS) | {4, 6, 7}):
            (x0, x1, y0, y1), = uvs.plant.occluder_rects([row], k)
            cols, rws = oc.rects_restated(row, k)
            if not cols:
                assert (x0, x1, y0, y1) == uvs.plant.NO_RECT and x0 > x1, (key, k)
                seen_empty += 1
            else:
                assert (x0, x1, y0, y1) == (cols[0], cols[-1], rws[0], rws[-1]) and len(cols) == x1 - x0 + 1 and len(rws) == y1 - y0 + 1, (key, k)
                seen_full += (x0, x1, y0, y1) == (0, 255, 0, 255)
    assert seen_empty > 20 and seen_full >= 1
    ex = oc.extremes()
    rect = lambda key, k: uvs.plant.occluder_rects([ex[key]], k)[0]  # noqa: E731
    # what the extremes are there for, spelt out
    assert rect('min_x_max_vx', 0) == uvs.plant.NO_RECT and rect('min_x_max_vx', 1) == (0, 255, 10, 49) and rect('min_x_max_vx', oc.K - 1) == uvs.plant.NO_RECT
    assert rect('max_w', 0) == (0, 255, 100, 119) and rect('max_w_max_x', 0) == uvs.plant.NO_RECT
    assert rect('max_h_moving_up', 0) == (120, 149, 250, 255) and rect('max_h_moving_up', oc.K - 1) == (120, 149, 30, 255)
    assert rect('on_equals_off', 1) == rect('off_before_on', 3) == rect('negative_w', 0) == rect('zero_w', 0) == uvs.plant.NO_RECT
    assert rect('one_step_only', 0) == rect('one_step_only', 2) == uvs.plant.NO_RECT and rect('one_step_only', 1) == (100, 149, 100, 149)
    assert all(rect(key, 0) == uvs.plant.NO_RECT for key in ('off_left', 'off_right', 'off_top', 'off_bottom'))
    assert rect('one_column_left', 0) == (0, 0, 0, 255) and rect('corner_pixel', 0) == (255, 255, 255, 255)
    assert rect('whole_frame', 1) == (0, 255, 0, 255) and rect('whole_frame', 0) == rect('whole_frame', 2) == uvs.plant.NO_RECT


def test_render_discs_states_the_rule(uvs):
    render = uvs.plant.render_discs
    discs = oc.scene('overlap_four')
    plain = render(discs)
    assert np.array_equal(render(discs, occluders=None, k=5, shade=7), plain), 'None is the function as it was'
    assert np.array_equal(render(discs, occluders=[]), plain) and np.array_equal(render(discs, occluders=[oc.NEVER] * 4), plain)
    rows = [oc.still(110, 100, 12, 40), oc.still(118, 110, 30, 6)]  # overlapping each other, over the four overlapping discs
    got = render(discs, occluders=rows, shade=40)[::-1]              # flipped: [flipped row, column]
    covered = np.zeros((256, 256), bool)
    covered[100:140, 110:122] = True
    covered[110:116, 118:148] = True
    assert np.all(got[covered] == 40) and np.array_equal(got[~covered], plain[::-1][~covered]), 'the union is shade; nothing else moves'
    assert np.array_equal(render(discs, occluders=rows[::-1], shade=40)[::-1], got), 'no order among occluders'
    batch = render(np.stack([discs, discs]), occluders=[[rows[0]], [rows[1]]], k=3)
    assert np.array_equal(batch[0], render(discs, occluders=[rows[0]])) and np.array_equal(batch[1], render(discs, occluders=[rows[1]]))
    moving = (10, 250, 5, 5, 7, -20, 2, 4)
    for k, rect in ((1, None), (2, (24, 28, 210, 214)), (3, (31, 35, 190, 194)), (4, None)):
        frame = render(discs, occluders=[moving], k=k, shade=0)[::-1]
        want = plain[::-1].copy()
        if rect is not None:
            want[rect[2]:rect[3] + 1, rect[0]:rect[1] + 1] = 0
        assert np.array_equal(frame, want), k


# ------------------------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize('name', oc.STATIC_SCENES)
def test_the_static_scenes_are_what_their_names_say(uvs, name):
    discs = oc.scene(name)
    covers = oc.static_covers(discs)
    first = 1 if discs[1][2] >= 0 else 0
    solo, scene_counts, _ = oc.covered_counts(uvs, discs, [oc.NEVER], 0)
    count = lambda key: oc.covered_counts(uvs, discs, covers[key], 0)[2]   # noqa: E731
    assert 0 < count('half')[first] < scene_counts[first] <= solo[first], 'a partial cover'
    assert count('red_entirely')[0] == 0 < scene_counts[0], 'a full cover of red'
    if name == 'whole_frame':                                        # red is the frame, and the target of the partial covers
        assert scene_counts[0] == 65536 and first == 0
        x0, x1, y0, y1 = uvs.plant.occluder_rects(covers['half'], 0)[0]
        assert count('half')[0] == 65536 - (x1 - x0 + 1) * (y1 - y0 + 1)
    both = count('two_overlapping')[first]
    assert 0 < both < count('half')[first], 'the second rectangle takes more'
    assert 0 < count('four')[first] <= both
    if 'slack_column' in covers:
        assert np.array_equal(count('slack_column'), scene_counts), 'the slack column holds no pixel of any disc'
        (x0, x1), (y0, y1) = cc.disc_box(discs[first])
        rx0, rx1, ry0, ry1 = uvs.plant.occluder_rects(covers['slack_column'], 0)[0]
        assert rx0 <= x1 and rx1 >= x0 and ry0 <= y1 and ry1 >= y0 and (rx0 == x1 or rx1 == x0), 'it meets the box, in one column'
    else:
        assert name in ('whole_frame',), 'only a box clipped on both sides has no slack column'
    if name == 'overlap_four':                                       # red lies under green where the rectangle sits: green loses pixels
        assert count('disc_overlap')[1] < scene_counts[1] and np.all(count('disc_overlap') <= scene_counts)


def test_the_sweeping_bar_and_the_half_cover(uvs):
    discs = np.stack([DESIRED[0::2], DESIRED[1::2], np.full(4, 8.01)], axis=1)      # the discs where the servo wants them
    bar = [oc.sweeping_bar()]
    _, scene_counts, _ = oc.covered_counts(uvs, discs, bar, 0)
    counts = np.stack([oc.covered_counts(uvs, discs, bar, k)[2] for k in range(oc.K)])
    assert np.all(counts.min(axis=0) < scene_counts), 'every disc is partially covered at some step'
    assert np.all(counts > 0), 'and none is ever empty: the bar is narrower than a disc'
    assert len({uvs.plant.occluder_rects(bar, k)[0] for k in range(oc.K)}) == oc.K
    half = oc.covered_counts(uvs, discs, [oc.half_cover(DESIRED)], 0)[2]
    assert 0 < half[1] < scene_counts[1] and np.array_equal(np.delete(half, 1), np.delete(scene_counts, 1)), 'green alone, and partially'
    window = [oc.sweeping_bar(4, 7)]
    active = [uvs.plant.occluder_rects(window, k)[0] != uvs.plant.NO_RECT for k in range(oc.K)]
    assert active == [4 <= k < 7 for k in range(oc.K)]


def test_camera_robot_renders_the_occluders_at_its_step_count(uvs):
    plant = uvs.SyntheticPlant.ur10()
    bar = [oc.sweeping_bar(), oc.still(100, 140, 30, 8)]
    robot = uvs.plant.CameraRobot(plant, occluders=bar, shade=50)
    clean = uvs.plant.CameraRobot(plant)
    q = cc.Q_GOAL + 0.01
    for r in (robot, clean):
        r.start(q)
    differs = 0
    for k in range(4):
        frame, resolution = robot.getCameraImage()
        assert resolution == (256, 256) and robot.k == k
        assert np.array_equal(frame, uvs.plant.render_discs(plant.discs(robot.getJointsPos(), robot.radius), 4, 96, bar, k, 50)), k
        assert np.array_equal(frame, robot.getCameraImage()[0]), 'looking twice is the same instant'
        assert np.array_equal(clean.getCameraImage()[0], uvs.plant.render_discs(plant.discs(clean.getJointsPos(), clean.radius))), k
        differs += not np.array_equal(frame, clean.getCameraImage()[0])
        for r in (robot, clean):
            r.setJointsPos(r.getJointsPos() + 0.002)
            r.step()
    assert differs == 4
    robot.start(q)
    assert robot.k == 0, 'start() is step 0 again'


# ------------------------------------------------------------------------------------------------------------- the built library
def test_the_documented_instantiations_are_built_without_scratch(uvs):
    """camera_occluded_kernel: what camera_grid_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1), MCKF
    (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22, MCKF at (6,6,2) the one documented absence."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    occluded = {name: r for name, r in k.items() if 'camera_occluded_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'camera_occluded_kernel(<[^>]*>)', name).group(1) for name in occluded}
    assert found == expected and len(occluded) == 22, (sorted(found ^ expected), len(occluded))
    for name, r in occluded.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
        for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_analytical_', 'camera_believed_'):
            assert pinned not in name, (pinned, name)
    assert sum('camera_loop_kernel' in name for name in k) == 22 and sum('camera_grid_kernel' in name for name in k) == 22
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        both = {name: r for name, r in k.items() if kernel in name}
        assert len(both) == 2 and all(r['scratch'] == 0 and r['wg'] == 1024 for r in both.values()), (kernel, both)
