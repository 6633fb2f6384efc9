"""CPU-only tests of the SCENE PER TRIAL (include/uvs_vision.h: the scene operand and the four *_scenes_* entry points;
engine.camera_scenes, engine.*(cameras=, camera_index=)): the scene set of camera_scenes_common.py is what it claims to be (six pairwise
different step-0 frames, every disc inside the frame with a mask of at least 50 pixels, every oracle trial calm), header and ctypes table
agree and each entry point has its namesake's operands with the triple in cam's place, every refusal comes before any HIP call (host arrays
with sentinels no kernel could use) in the namesake's order followed by the triple's, every Python refusal before any device work,
camera_scenes packs to_camera's bytes, and the built library holds the 22 instantiations of camera_scene_kernel and the three other new
kernels, none with a private segment and none under a pinned name."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_scenes_common as sc
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED

ARG, SHAPE, METHOD = -1, -2, -4
TRIPLE = ['const uvs_camera *cams', 'int64_t n_cams', 'const int32_t *cam_index']
NAMESAKES = {'uvs_camera_project_scenes_f64': 'uvs_camera_project_f64', 'uvs_camera_features_scenes_f64': 'uvs_camera_features_painted_f64',
             'uvs_camera_closed_loop_scenes_f64': 'uvs_camera_closed_loop_painted_f64',
             'uvs_camera_believed_loop_scenes_f64': 'uvs_camera_believed_loop_f64'}
NO_FP = ('uvs_camera_project_scenes_f64', 'uvs_camera_features_scenes_f64')      # the shape is an n_points argument of their own


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the scene set
def test_the_six_step_0_frames_differ_and_show_every_disc(uvs):
    for n_points in (4, 1):
        plants = sc.plants(uvs, n_points)
        for q in sc.starts(4):
            frames = [uvs.plant.render_discs(plant.discs(q, radius), n_points) for plant, radius in zip(plants, sc.RADII)]
            for a in range(sc.N_SCENES):
                for b in range(a):
                    assert not np.array_equal(frames[a], frames[b]), (n_points, a, b)
            for plant, radius, frame in zip(plants, sc.RADII, frames):
                d = plant.discs(q, radius)
                assert (d[:, :2] - d[:, 2:]).min() > 0.0 and (d[:, :2] + d[:, 2:]).max() < 255.0
                counts = cc.host_counts(frame)
                assert (counts[[1]] if n_points == 1 else counts).min() >= pl.MASK_MIN
    fields = [s for s in sc.structs(uvs)]
    differs = lambda get: len({tuple(np.ravel(get(s))) for s in fields}) > 1          # noqa: E731
    for name in ('theta_offset', 'd', 'a', 'points', 'radius'):
        assert differs(lambda s: [list(np.ravel(getattr(s, name)[i])) for i in range(len(getattr(s, name)))]), name
    assert differs(lambda s: s.focal) and differs(lambda s: s.center)


@pytest.mark.parametrize('method,n_points', sc.ORACLE)
def test_every_oracle_trial_is_calm(uvs, method, n_points):
    """pixel_loop_common's preconditions: from q_start (1 + 1e-14) the same status, k_done and masks and logs within 1e-10; no pixel within
    1e-6 of a rim; the discs inside the frame with masks of at least 50 pixels; and the trial runs its K steps."""
    for scene in range(sc.N_SCENES):
        a, b = sc.oracle_trial(method, n_points, scene), sc.oracle_trial(method, n_points, scene, True)
        assert (a['status'], a['k_done']) == (0, sc.K) == (b['status'], b['k_done'])
        assert np.array_equal(a['counts'], b['counts']) and a['held'] == b['held'] and np.array_equal(a['fpi_iterations'], b['fpi_iterations'])
        for key in ('q', 'f', 'dq', 'err', 'kappa'):
            assert np.abs(a[key] - b[key]).max() / np.abs(a[key]).max() <= pl.CALM_TOL, (scene, key)
        assert cc.closest_to_rim(a['discs']) > pl.RIM_MIN
        d = a['discs']
        assert (d[:, :, :2] - d[:, :, 2:]).min() > 0.0 and (d[:, :, :2] + d[:, :, 2:]).max() < 255.0 and a['counts'].min() >= pl.MASK_MIN


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: uvs._vision.SYMBOLS[fn][1]                    # noqa: E731
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for new, old in NAMESAKES.items():
        a, b = declared(new), declared(old)
        at = b.index('const uvs_camera *cam')
        own = ['int32_t n_points'] if new in NO_FP else []
        assert a == b[:at] + TRIPLE + own + b[at + 1:], (new, "the namesake's operands with the triple in cam's place")
        assert types(new) == types(old)[:at] + [VP, I64, VP] + ([I32] if own else []) + types(old)[at + 1:], new
        assert getattr(uvs._vision.lib(), new) is not None


# ------------------------------------------------------------------------------------------------------------- C refusals
class Scenes(Buffers):
    """Buffers with the scene operand, the believed operand, rectangles and paints: host arrays with sentinels."""
    def __init__(self, uvs, **kw):
        Buffers.__init__(self, uvs, **kw)
        self.cams = np.full(self.T * 472 // 8 + 8, 7.0)
        self.index = np.full(self.T, 7, np.int32)
        self.occ = np.full(self.T * 4 * 8, 7, np.int32)
        self.paint = np.full(self.T * 4, 7, np.int32)
        self.held = np.full(self.T * 4, 7, np.int32)

    def untouched(self):
        return Buffers.untouched(self) and np.all(self.cams == 7) and all(np.all(a == 7) for a in (self.index, self.occ, self.paint, self.held))


def loop_call(uvs, b, T=None, cams='own', n_cams=1, index=None, tp='block', occ='rows', n_occ=1, hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_scenes_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.T if T is None else T, ref(tp), b.occ.ctypes.data if isinstance(occ, str) else occ, b.paint.ctypes.data, n_occ, hold, a['q_start'],
        a['noise'], a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'],
        b.held.ctypes.data, None)


def baseline_call(uvs, b, T=None, cams='own', n_cams=1, index=None, believed='own', n_believed=1, believed_index=None, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_believed_loop_scenes_f64(
        ref(a['fp']), b.cams.ctypes.data if isinstance(cams, str) else cams, n_cams, b.index.ctypes.data if isinstance(index, str) else index,
        b.T if T is None else T, b.cams.ctypes.data if isinstance(believed, str) else believed, n_believed, believed_index, a['q_start'],
        a['noise'], a['q'], a['f'], a['dq'], a['err'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def triple_refusals(call, lib, T):
    """The triple's refusals, which come last: NULL cams, n_cams < 1, n_cams not in {1, T} without an index; each also before T == 0."""
    assert call(cams=None) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
    for n_cams in (0, -1, 2 ** 31):
        assert call(n_cams=n_cams) == ARG and b'n_cams' in lib.uvs_vision_last_error(), n_cams
    for n_cams in (T + 1, 3 * T):
        assert call(n_cams=n_cams) == ARG and b'cam_index' in lib.uvs_vision_last_error(), n_cams
    assert call(cams=None, T=0) == ARG and call(n_cams=0, T=0) == ARG and call(n_cams=5, T=0) == ARG, 'refusals come before T == 0'
    assert call(T=0) == 0 and lib.uvs_vision_last_error() == b'' and call(T=0, n_cams=5, index='own') == 0


def test_the_loop_refuses_what_the_painted_call_refuses_then_the_triple(uvs):
    lib, b = uvs._vision.lib(), Scenes(uvs)
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
    mckf = Scenes(uvs, n_points=3, method='MCKF')
    mckf.fp.m = 6
    assert loop_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
    for n_in in (0, -3):
        assert call(tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    for n_occ in (-1, 5):
        assert call(n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
    assert call(occ=None, n_occ=2) == ARG and b'NULL occ' in lib.uvs_vision_last_error()
    assert call(hold=-1) == ARG and b'hold' in lib.uvs_vision_last_error()
    # the order: the namesake's refusals come before the triple's
    assert call(hold=-1, cams=None) == ARG and b'hold' in lib.uvs_vision_last_error()
    assert call(n_occ=9, n_cams=0) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert call(fp=bad.fp, cams=None) == METHOD
    triple_refusals(call, lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_the_baseline_loop_refuses_what_the_believed_loop_refuses_then_the_triple(uvs):
    lib, b = uvs._vision.lib(), Scenes(uvs, method='ANALYTICAL')
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
    P = lambda a: None if a is None else a.ctypes.data               # noqa: E731
    project = lambda cams=cams, n_cams=1, index=None, T=1, n=4, out=discs, q_out=None: lib.uvs_camera_project_scenes_f64(   # noqa: E731
        P(cams), n_cams, index, n, T, P(q), None, 0.0, q_out, P(out), None)
    features = lambda cams=cams, n_cams=1, index=None, T=1, n=4, out=f, n_occ=1, k=0, occ_ptr=occ: lib.uvs_camera_features_scenes_f64(   # noqa: E731
        P(cams), n_cams, index, n, T, P(q), None, 0.0, None, P(occ_ptr), P(paint), n_occ, k, None, P(out), None, None, None)
    for call in (project, features):
        assert call(out=None) == ARG and b'NULL' in lib.uvs_vision_last_error()
        assert call(T=-1) == ARG and call(n=2) == ARG and b'n_points' in lib.uvs_vision_last_error()
        assert call(out=None, cams=None) == ARG and b'cams' not in lib.uvs_vision_last_error(), "the namesake's refusals come first"
        assert call(cams=None) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
        assert call(n_cams=0) == ARG and call(n_cams=3) == ARG and b'cam_index' in lib.uvs_vision_last_error()
        assert call(n_cams=3, T=0) == ARG, 'refusals come before T == 0'
        assert call(T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert project(q_out=q.ctypes.data) == ARG and b'overlaps' in lib.uvs_vision_last_error()
    assert features(n_occ=5) == ARG and features(occ_ptr=None) == ARG and features(k=-1) == ARG
    assert features(n_occ=5, cams=None) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert features(T=0, occ_ptr=None, n_occ=0) == 0, 'no rectangles stay legal'
    assert all(np.all(a == 7) for a in (cams, discs, f, q, occ, paint)), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python
def test_camera_scenes_packs_the_structs_bytes(uvs, monkeypatch):
    import torch
    monkeypatch.setattr(uvs.engine, '_torch', lambda: torch)         # packing is host work: no device is needed to see the bytes
    monkeypatch.setattr(uvs.engine, 'current_device', lambda device=None: torch.device('cpu'))
    size = ctypes.sizeof(uvs._vision.Camera)
    assert size == 472
    raw = lambda s: np.frombuffer(ctypes.string_at(ctypes.addressof(s), size), np.uint8)          # noqa: E731
    plants = sc.plants(uvs)
    packed = uvs.engine.camera_scenes(plants, sc.RADII).numpy()
    assert packed.shape == (6, size) and packed.dtype == np.uint8
    for i, (plant, radius) in enumerate(zip(plants, sc.RADII)):
        assert np.array_equal(packed[i], raw(plant.to_camera(radius))), i
    assert np.array_equal(uvs.engine.camera_scenes(sc.structs(uvs), 0.5).numpy(), packed), 'a Camera struct keeps its own radius'
    assert np.array_equal(uvs.engine.camera_scenes(plants[2], 0.03).numpy()[0], packed[2])
    rows = np.arange(24).reshape(6, 4) * 1e-3 + 0.01
    per_point = uvs.engine.camera_scenes(plants, rows).numpy()
    assert np.array_equal(per_point[4], raw(plants[4].to_camera(rows[4])))
    assert np.array_equal(uvs.engine.camera_scenes(plants).numpy()[0], raw(plants[0].to_camera()))
    for bad in ([], [1.0], 'x'):
        with pytest.raises((ValueError, TypeError)):
            uvs.engine.camera_scenes(bad)
    with pytest.raises(ValueError, match='per model'):
        uvs.engine.camera_scenes(plants, [0.02, 0.03])


def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these must be a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    eng, plants = uvs.engine, sc.plants(uvs)
    plant = plants[0]
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
    one_disc = uvs.SyntheticPlant.ur10(desired_f=(149.0, 145.0))
    for call in calls:
        with pytest.raises(ValueError, match='camera_index without cameras'):
            call(camera_index=[0, 0, 0])
        for index in ([0, 1, 6], [-1, 0, 0], np.array([0, 0, 2 ** 31])):
            with pytest.raises(ValueError, match=r'must lie in \[0, 6\)'):
                call(cameras=plants, camera_index=index)
        for index in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]], [0.0, 1.0, 2.0]):
            with pytest.raises(ValueError, match='3 integers'):
                call(cameras=plants, camera_index=index)
        with pytest.raises(ValueError, match='6 cameras for 3 trials'):
            call(cameras=plants)
        with pytest.raises(ValueError, match='1 points and 6 joints among'):
            call(cameras=plants[:2] + [one_disc])
        with pytest.raises(ValueError, match='what camera_scenes returns'):
            call(cameras=torch.zeros((3, 100), dtype=torch.uint8))
        with pytest.raises(ValueError, match='a sequence of them'):
            call(cameras=[plant, 'camera', plant])
    with pytest.raises(ValueError, match="pass x0, or guess='device'"):
        eng.camera_closed_loop(fp, plant, q, fused=True, cameras=plants[:3])
    with pytest.raises(ValueError, match="pass x0, or guess='device'"):
        eng.camera_closed_loop(fp, plant, q, fused=False, cameras=plants[:1])
    with pytest.raises(ValueError, match='4 integers'):              # per OUTPUT trial: len(source) of them
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': [0, 1, 2, 0]}, cameras=plants, camera_index=[0, 1, 2])
    bar = [[0, 0, 10, 10, 0, 0, 0, 5]]
    with pytest.raises(ValueError, match='fused=False'):             # the older refusals are still there, and come first
        eng.camera_closed_loop(analytical, plant, q, fused=True, occluders=bar, cameras=plants[:3])
    with pytest.raises(ValueError, match='fused=False'):
        eng.camera_closed_loop(analytical, plant, q, fused=True, hold=1, cameras=plants[:3])
    for good in (dict(cameras=plants[:3]), dict(cameras=plants[1]), dict(cameras=plants, camera_index=[5, 0, 3])):   # accepted as far as the host goes
        with pytest.raises(ValueError, match='on the device'):
            eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, **good)


# ------------------------------------------------------------------------------------------------------------- the built library
PINNED = ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel', 'hold_pairs_kernel', 'camera_loop_kernel', 'camera_grid_kernel',
          'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel', 'camera_analytical_', 'camera_believed_')


def test_the_scene_kernels_are_built_without_scratch(uvs):
    """camera_scene_kernel: what camera_painted_kernel is built for -- GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1),
    MCKF (3) at (8,6,4) and (2,6,1), each in its one-trial and its four-trial form: 22, MCKF at (6,6,2) the one documented absence -- the
    baseline's scene_baseline_loop_kernel at the three shapes in both forms, and the two stand-alone kernels; no name contains a pinned
    one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    scene = {name: r for name, r in k.items() if 'camera_scene_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'camera_scene_kernel(<[^>]*>)', name).group(1) for name in scene}
    assert found == expected and len(scene) == 22, (sorted(found ^ expected), len(scene))
    for name, r in scene.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
    baseline = {name: r for name, r in k.items() if 'scene_baseline_loop_kernel' in name}
    assert {re.search(r'scene_baseline_loop_kernel(<[^>]*>)', name).group(1) for name in baseline} == \
        {f'<{shape}, {g}>' for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1') for g in (1, 4)}
    for name, r in baseline.items():
        assert r['wg'] == 256 and r['scratch'] == 0, (name, r)
    others = dict(baseline)
    for kernel, wg in (('scene_project_kernel', 64), ('scene_camera_detect_kernel', 1024)):
        (name, r), = [(name, r) for name, r in k.items() if re.search(r'\b' + kernel + r'\b', name)]
        assert r['scratch'] == 0 and r['wg'] == wg, (name, r)
        others[name] = r
    for name in list(scene) + list(others):
        for pinned in PINNED:
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):      # each as it was, and with occluders
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
