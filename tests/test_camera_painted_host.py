"""CPU-only tests of PAINTED occluders -- distractors (include/uvs_vision.h: the paint operand and the four *_painted_* entry points;
plant.render_discs(occluder_colours=), plant.occluder_colour_array, plant.CameraRobot(occluder_colours=); engine.*(occluder_colours=)):
the numpy statement agrees with a per-pixel restatement of the owner rule, None and all-opaque are the function as it was, the order of
two overlapping paints shows, the host detector finds a lone green rectangle's centre, header and ctypes table agree, every refusal comes
before any HIP call (host arrays with sentinels no kernel could use) and every Python refusal before any device work, and the built
library holds the 22 instantiations of camera_painted_kernel and the three stand-alone kernels, none with a private segment and none
under a pinned name."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_occluders_common as oc
import camera_painted_common as pc
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED

ARG, SHAPE, METHOD = -1, -2, -4
LOOP, HELD = 'uvs_camera_closed_loop_painted_f64', 'uvs_camera_closed_loop_held_f64'
STAND_ALONE = (('uvs_render_discs_painted_u8', 'uvs_render_discs_occluded_u8'), ('uvs_disc_features_painted_f64', 'uvs_disc_features_occluded_f64'),
               ('uvs_camera_features_painted_f64', 'uvs_camera_features_occluded_f64'))
PAINT = 'const int32_t *paint'


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the rule
RULE_CASES = [('overlap_four', 'd_two_paints_in_two_orders', 0), ('overlap_four', 'g_four_mixed', 0), ('clip_corner', 'h_clipped_at_every_edge', 0),
              ('not_drawn', 'e_every_colour', 0), ('rgb', 'g_four_of_one_colour', 0), ('green_alone', 'c_over_another_disc', 0),
              ('green_alone_absent', 'b_over_its_own_disc', 0), ('fixture_0', 'extreme_max_h_moving_up', pc.K - 1),
              ('whole_frame', 'extreme_whole_frame', 1)]


@pytest.mark.parametrize('name,key,k', RULE_CASES)
def test_render_discs_agrees_with_the_owner_rule_pixel_by_pixel(uvs, name, key, k):
    n, discs = pc.scene(name)
    rows, paints = pc.paint_sets(discs)[key]
    got = uvs.plant.render_discs(discs, n, 96, rows, k, 32, occluder_colours=paints)
    want = pc.frame_restated(discs, rows, paints, k)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (name, key)
    owners = pc.owners_restated(discs, rows, paints, k)
    mask_sizes = [sum((o == ('disc', c)) or (o is not None and o[0] == 'rect' and paints[o[1]] == c) for line in owners for o in line)
                  for c in range(n)]
    assert np.array_equal(pc.counts(got, n), mask_sizes), 'the mask of a colour is its disc and the rectangles painted it'


def test_none_and_all_opaque_are_the_function_as_it_was(uvs):
    render = uvs.plant.render_discs
    for name in ('overlap_four', 'rgb', 'green_alone'):
        n, discs = pc.scene(name)
        rows, _ = pc.paint_sets(discs)['g_four_mixed']
        for k in (0, 3):
            plain = render(discs, n, 96, rows, k, 40)
            assert np.array_equal(render(discs, n, 96, rows, k, 40, occluder_colours=None), plain)
            assert np.array_equal(render(discs, n, 96, rows, k, 40, occluder_colours=[pc.OPAQUE] * 4), plain)
            assert np.array_equal(render(discs, n, 96, rows[::-1], k, 40, occluder_colours=[pc.OPAQUE] * 4), plain), 'opaque: the union'
        assert np.array_equal(render(discs, n, occluders=[], occluder_colours=[]), render(discs, n))
    batch = render(np.stack([discs, discs]), 1, occluders=[rows[:1], rows[1:2]], occluder_colours=[[0], [pc.OPAQUE]])
    assert np.array_equal(batch[0], render(discs, 1, occluders=rows[:1], occluder_colours=[0]))
    assert np.array_equal(batch[1], render(discs, 1, occluders=rows[1:2]))


def test_two_overlapping_paints_show_their_order(uvs):
    n, discs = pc.scene('overlap_four')
    rows = [oc.still(30, 40, 20, 10), oc.still(40, 44, 20, 10)]     # they share columns 40 .. 49 of rows 44 .. 49
    first = uvs.plant.render_discs(discs, occluders=rows, occluder_colours=[0, 2])[::-1]
    second = uvs.plant.render_discs(discs, occluders=rows[::-1], occluder_colours=[2, 0])[::-1]
    assert not np.array_equal(first, second)
    assert tuple(first[46, 45]) == (0, 0, 255) and tuple(second[46, 45]) == (255, 0, 0), 'the later rectangle is in front'
    differ = (first != second).any(axis=2)
    assert differ.sum() == 60 and differ[44:50, 40:50].all(), 'and nowhere but where they overlap'
    assert np.array_equal(pc.counts(first, 4) - pc.counts(uvs.plant.render_discs(discs), 4), [200 - 60, 0, 200, 0])


@pytest.mark.parametrize('n', [1, 3, 4])
def test_the_host_detector_finds_a_lone_green_rectangle(uvs, n):
    """The disc is absent (r = -1) and one w x h green rectangle lies inside the frame: the pair is the rectangle's centre, the count w h."""
    from uvs_amd import utils
    detect = {1: utils.detectGreenCircle, 3: utils.detectRGBCircles, 4: utils.detect4Circles}[n]
    green = 0 if n == 1 else 1
    discs = cc.pad([], n)
    for x, y, w, h in ((40, 60, 31, 17), (0, 0, 1, 1), (250, 3, 6, 9), (100, 200, 2, 56)):
        frame = uvs.plant.render_discs(discs, n, occluders=[oc.still(x, y, w, h)], occluder_colours=[green])
        assert pc.counts(frame, n)[green] == w * h
        f = np.asarray(detect(frame), float)
        assert np.abs(f[2 * green:2 * green + 2] - [x + (w - 1) / 2, y + (h - 1) / 2]).max() < 1e-11, (n, x, y, w, h, f)
        others = np.delete(f, [2 * green, 2 * green + 1])
        assert np.isnan(others).all(), 'no other colour has a pixel'


def test_camera_robot_renders_the_paints_at_its_step_count(uvs):
    plant = uvs.SyntheticPlant.ur10()
    rows, paints = [oc.sweeping_bar(), oc.still(100, 140, 30, 8)], [pc.OPAQUE, 1]
    robot = uvs.plant.CameraRobot(plant, occluders=rows, shade=50, occluder_colours=paints)
    opaque = uvs.plant.CameraRobot(plant, occluders=rows, shade=50)
    for r in (robot, opaque):
        r.start(cc.Q_GOAL + 0.01)
    for k in range(3):
        frame = robot.getCameraImage()[0]
        assert np.array_equal(frame, uvs.plant.render_discs(plant.discs(robot.getJointsPos(), robot.radius), 4, 96, rows, k, 50, paints)), k
        assert not np.array_equal(frame, opaque.getCameraImage()[0])
        for r in (robot, opaque):
            r.setJointsPos(r.getJointsPos() + 0.002)
            r.step()


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    for new, old in STAND_ALONE + ((LOOP, HELD),):
        a, b = declared(new), declared(old)
        at = b.index('const uvs_occluder *occ')
        assert a == b[:at + 1] + [PAINT] + b[at + 1:], (new, 'the namesake\'s operands with paint directly after occ')
        assert types(new) == types(old)[:at + 1] + [ctypes.c_void_p] + types(old)[at + 1:], new
        assert getattr(uvs._vision.lib(), new) is not None
    assert len(declared(LOOP)) == 23
    body = re.search(r'typedef struct uvs_occluder \{(.*?)\} uvs_occluder;', header, re.S).group(1)
    assert len(re.findall(r'(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', body, flags=re.S))) == 8 and ctypes.sizeof(uvs._vision.Occluder) == 32


# ------------------------------------------------------------------------------------------------------------- C refusals
def loop_call(uvs, b, T=None, tp='block', occ='rows', paint='rows', n_occ=1, hold=2, held='rows', **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp, cam=b.cam)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return getattr(uvs._vision.lib(), LOOP)(ref(a['fp']), ref(a['cam']), b.T if T is None else T, ref(tp),
                                            b.occ.ctypes.data if isinstance(occ, str) else occ, b.paint.ctypes.data if isinstance(paint, str) else paint,
                                            n_occ, hold, a['q_start'], a['noise'], a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'],
                                            a['status'], a['k_done'], a['stats'], a['pixels'], b.held.ctypes.data if isinstance(held, str) else held,
                                            None)


def with_paints(b):
    b.occ = np.full(b.T * 4 * 8, 7, np.int32)
    b.paint = np.full(b.T * 4, 7, np.int32)
    b.held = np.full(b.T * 4, 7, np.int32)
    return b


def test_the_loop_refuses_what_the_held_call_refuses_in_its_order(uvs):
    lib, b = uvs._vision.lib(), with_paints(Buffers(uvs))
    for paint in ('rows', None):                                     # a NULL paint changes no refusal
        for name in ('fp', 'cam', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
            assert loop_call(uvs, b, paint=paint, **{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
        assert loop_call(uvs, b, paint=paint, T=-1) == ARG
        bad = Buffers(uvs)
        bad.fp.steps = 0
        assert loop_call(uvs, b, paint=paint, fp=bad.fp) == ARG
        bad = Buffers(uvs)
        bad.fp.lanes_per_filter = 2
        assert loop_call(uvs, b, paint=paint, fp=bad.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
        assert loop_call(uvs, b, paint=paint, cam=Buffers(uvs, n_points=3).cam) == SHAPE
        assert loop_call(uvs, b, paint=paint, cam=Buffers(uvs, n_points=2).cam) == ARG
        bad = Buffers(uvs)
        bad.fp.method = 1                                            # UVS_METHOD_ANALYTICAL
        assert loop_call(uvs, b, paint=paint, fp=bad.fp) == METHOD
        mckf = with_paints(Buffers(uvs, n_points=3, method='MCKF'))
        mckf.fp.m = 6
        assert loop_call(uvs, mckf, paint=paint) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
        for n_in in (0, -3):
            assert loop_call(uvs, b, paint=paint, tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
        for n_occ in (-1, 5, 2 ** 31 - 1):
            assert loop_call(uvs, b, paint=paint, n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
        for n_occ in (1, 4):
            assert loop_call(uvs, b, paint=paint, occ=None, n_occ=n_occ) == ARG and b'NULL occ' in lib.uvs_vision_last_error(), n_occ
        for hold in (-1, -2 ** 31):
            assert loop_call(uvs, b, paint=paint, hold=hold) == ARG and b'hold' in lib.uvs_vision_last_error(), hold
            assert loop_call(uvs, b, paint=paint, hold=hold, T=0) == ARG, 'refusals come before T == 0'
        assert loop_call(uvs, b, paint=paint, hold=-1, n_occ=9) == ARG and b'n_occ' in lib.uvs_vision_last_error()
        assert loop_call(uvs, b, paint=paint, hold=-1, fp=bad.fp) == METHOD
        assert mckf.untouched()
    assert b.untouched() and all(np.all(a == 7) for a in (b.occ, b.paint, b.held)), 'a refused call wrote'


def test_a_null_paint_and_nothing_to_do_are_ok(uvs):
    lib, b = uvs._vision.lib(), with_paints(Buffers(uvs))
    assert loop_call(uvs, b, T=0, paint=None, n_occ=4) == 0 and lib.uvs_vision_last_error() == b'', 'NULL paint with n_occ > 0: all opaque'
    assert loop_call(uvs, b, T=0, tp=None) == 0 and loop_call(uvs, b, T=0, occ=None, paint=None, n_occ=0, hold=5) == 0
    assert loop_call(uvs, b, T=0, occ=None, n_occ=0) == 0, 'paints without rectangles are never read'
    assert loop_call(uvs, b, T=0, hold=0, held=None) == 0
    assert loop_call(uvs, b, T=0, tp=None, noise=None, q=None, f=None, dq=None, err=None, kappa=None, pixels=None, held=None) == 0
    assert b.untouched() and all(np.all(a == 7) for a in (b.occ, b.paint, b.held))


def test_the_stand_alone_kernels_refuse_before_they_launch(uvs):
    lib = uvs._vision.lib()
    cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
    discs, f, q, occ, paint = np.full(12, 7.0), np.full(8, 7.0), np.full(6, 7.0), np.full(32, 7, np.int32), np.full(4, 7, np.int32)
    frames = np.full(256 * 256 * 3 + 16, 7, np.uint8)
    fr = (frames.ctypes.data + 15) // 16 * 16
    P = lambda a: a.ctypes.data                                      # noqa: E731
    render = lambda n_occ=1, k=0, shade=32, occ_ptr=P(occ), paint_ptr=P(paint), T=1, bg=96: lib.uvs_render_discs_painted_u8(   # noqa: E731
        T, P(discs), 4, bg, occ_ptr, paint_ptr, n_occ, k, shade, fr, 256 * 256 * 3, None)
    features = lambda n_occ=1, k=0, occ_ptr=P(occ), paint_ptr=P(paint), T=1, n=4: lib.uvs_disc_features_painted_f64(   # noqa: E731
        T, P(discs), n, occ_ptr, paint_ptr, n_occ, k, None, P(f), None, None)
    camera = lambda n_occ=1, k=0, occ_ptr=P(occ), paint_ptr=P(paint), T=1, out=P(f): lib.uvs_camera_features_painted_f64(   # noqa: E731
        ctypes.byref(cam), T, P(q), None, 0.0, None, occ_ptr, paint_ptr, n_occ, k, None, out, None, None, None)
    for call in (render, features, camera):
        for paint_ptr in (P(paint), None):
            for n_occ in (-1, 5):
                assert call(n_occ=n_occ, paint_ptr=paint_ptr) == ARG and b'n_occ' in lib.uvs_vision_last_error()
            assert call(occ_ptr=None, paint_ptr=paint_ptr) == ARG and b'NULL occ' in lib.uvs_vision_last_error()
            assert call(k=-1, paint_ptr=paint_ptr) == ARG and b'k must' in lib.uvs_vision_last_error()
            assert call(T=-1, paint_ptr=paint_ptr) == ARG
            assert call(T=0, paint_ptr=paint_ptr) == 0 and call(T=0, occ_ptr=None, n_occ=0, paint_ptr=paint_ptr) == 0
            assert lib.uvs_vision_last_error() == b''
            assert call(T=0, n_occ=5, paint_ptr=paint_ptr) == ARG, 'refusals come before T == 0'
    for shade in (-1, 250, 255):
        assert render(shade=shade) == ARG and b'shade' in lib.uvs_vision_last_error()
    assert render(bg=250, n_occ=9) == ARG and b'background' in lib.uvs_vision_last_error()
    assert features(n=2, n_occ=9) == ARG and b'n_colours' in lib.uvs_vision_last_error()
    assert camera(out=None, n_occ=9) == ARG and b'f_out' in lib.uvs_vision_last_error()
    assert all(np.all(a == 7) for a in (discs, f, q, occ, paint, frames)), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python refusals
BAD_PAINTS = [([0.5], 'integers'), ([[[0]]], 'integers'), ('red', 'integers'), ([0, 1], '2 paints for 1 occluders'), ([], '0 paints for 1'),
              ([4], 'opaque'), ([-2], 'opaque'), ([[0], [0], [0]], '3 trials of paints for 2')]


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
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, hold=2, trial_params={}, **kw),
             lambda **kw: eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, **kw),
             lambda **kw: eng.camera_closed_loop(analytical, plant, q, fused=False, believed=plant, **kw))
    for call in calls:
        for spec, text in BAD_PAINTS:
            with pytest.raises(ValueError, match=text):
                call(occluders=bar, occluder_colours=spec)
        with pytest.raises(ValueError, match='without occluders'):
            call(occluder_colours=[0])
        with pytest.raises(ValueError, match='integers'):             # the occluders' own refusals come first
            call(occluders=[[0.5] * 8], occluder_colours=[9])
    one = eng.make_params(2, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED[:2], steps=3)
    with pytest.raises(ValueError, match='opaque'):                  # a one-disc camera has the paint 0 alone
        eng.camera_closed_loop(one, plant, q, x0=np.zeros((2, 12)), fused=True, occluders=bar, occluder_colours=[1])
    with pytest.raises(ValueError, match='fused=False'):             # as for occluders
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, occluder_colours=[0])
    with pytest.raises(ValueError, match='4 trials of paints for 3'):                    # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, trial_params={'source': [0, 1, 0]}, occluders=bar,
                               occluder_colours=[[0]] * 4)
    with pytest.raises(ValueError, match='fused=True'):              # the older refusals are still there
        eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), trial_params={}, occluders=bar, occluder_colours=[0])
    for good in ([0], [3], [pc.OPAQUE], np.array([[1], [2]]), np.int32([0])):            # accepted as far as the host goes
        with pytest.raises(ValueError, match='on the device'):
            eng.camera_closed_loop(fp, plant, q, x0=np.zeros((2, 48)), fused=True, occluders=bar, occluder_colours=good)
    # the numpy side
    for spec, text in BAD_PAINTS[:7]:
        with pytest.raises(ValueError, match=text):
            uvs.plant.render_discs(np.zeros((2, 4, 3)), occluders=bar, occluder_colours=spec)
    with pytest.raises(ValueError, match='without occluders'):
        uvs.plant.render_discs(np.zeros((4, 3)), occluder_colours=[0])
    with pytest.raises(ValueError, match='opaque'):
        uvs.plant.render_discs(np.zeros((1, 3)), 1, occluders=bar, occluder_colours=[1])
    with pytest.raises(ValueError, match='without occluders'):
        uvs.plant.CameraRobot(plant, occluder_colours=[0])
    with pytest.raises(ValueError, match='opaque'):
        uvs.plant.CameraRobot(plant, occluders=bar, occluder_colours=[4])
    a = uvs.plant.occluder_colour_array([0, pc.OPAQUE], 2, 4, 3)
    assert a.shape == (3, 2) and a.dtype == np.int64 and a.tolist() == [[0, -1]] * 3


# ------------------------------------------------------------------------------------------------------------- the built library
PINNED = ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel', 'hold_pairs_kernel', 'camera_loop_kernel', 'camera_grid_kernel',
          'camera_occluded_kernel', 'camera_held_kernel', 'camera_analytical_', 'camera_believed_')


def test_the_painted_kernels_are_built_without_scratch(uvs):
    """camera_painted_kernel: what camera_held_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1), MCKF
    (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22, MCKF at (6,6,2) the one documented absence -- and the
    three stand-alone kernels with their namesakes' workgroup; no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    painted = {name: r for name, r in k.items() if 'camera_painted_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'camera_painted_kernel(<[^>]*>)', name).group(1) for name in painted}
    assert found == expected and len(painted) == 22, (sorted(found ^ expected), len(painted))
    for name, r in painted.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
    stand_alone = {}
    for kernel in ('paint_frames_kernel', 'paint_detect_kernel', 'paint_camera_detect_kernel'):
        (name, r), = [(name, r) for name, r in k.items() if re.search(r'\b' + kernel + r'\b', name)]
        assert r['scratch'] == 0 and r['wg'] == 1024, (name, r)
        stand_alone[name] = r
    for name in list(painted) + list(stand_alone):
        for pinned in PINNED:
            assert pinned not in name, (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
