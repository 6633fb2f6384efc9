"""CPU-only tests of the calibrated baseline on a per-trial believed model (include/uvs_vision.h: uvs_camera_believed_step_f64,
uvs_camera_believed_loop_f64, uvs_camera_believed_guess_f64; plant.miscalibrated; engine.believed_models and the ``believed=`` arguments):
the numpy restatement is the calibrated one when the believed plant is the true one, the wrong plants are what they say, header and ctypes
table agree, the entry points refuse bad arguments before any HIP call (the buffers here are host arrays no kernel could use, filled with
sentinels that must survive), the Python layer refuses what the issue says it refuses without looking at a device, and the built library
holds the new kernels without a private segment."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

ARG, SHAPE, METHOD = -1, -2, -4
STRICT = 1
DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])
JOINT_OFFSETS = (0.03, -0.02, 0.04, -0.03, 0.02, 0.1)


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_with_the_true_plant_is_the_calibrated_one(uvs):
    import camera_analytical_ref
    import camera_believed_ref
    K, dt, gain = 8, 0.05, 0.2
    plant = uvs.SyntheticPlant.ur10()
    noise = np.random.default_rng(5).standard_normal((K, 8)) * 0.3
    noise[6, 3] = np.nan                                             # and a FAIL, so that the tails are compared too
    for q0, nz in ((Q_HOST_ROUTE[0], None), (Q_HOST_ROUTE[1], noise)):
        want = camera_analytical_ref.run(plant, q0, nz, DESIRED, dt, gain, K)
        got = camera_believed_ref.run(plant, plant, q0, nz, DESIRED, dt, gain, K)
        assert set(got) == set(want) and got['k_done'] == want['k_done'] == (K if nz is None else 6) and got['status'] == want['status']
        for key in ('err', 'f', 'q', 'dq', 'j', 'discs', 'masks', 'stats'):
            assert np.array_equal(got[key], want[key], equal_nan=True), key


def test_restatement_on_a_wrong_plant_differs_in_the_law_alone(uvs):
    import camera_believed_ref
    plant = uvs.SyntheticPlant.ur10()
    wrong = uvs.plant.miscalibrated(plant, focal_scale=1.2, point_offset=(0.05, -0.05, -0.2), joint_offset=JOINT_OFFSETS, link_scale=0.97)
    right = camera_believed_ref.run(plant, plant, Q_HOST_ROUTE[0], None, DESIRED, 0.05, 0.2, 3)
    got = camera_believed_ref.run(plant, wrong, Q_HOST_ROUTE[0], None, DESIRED, 0.05, 0.2, 3)
    assert got['k_done'] == 3
    assert np.array_equal(got['f'][0], right['f'][0]) and np.array_equal(got['err'][0], right['err'][0])      # the same frame at the start
    assert not np.allclose(got['j'][0], right['j'][0], rtol=1e-3) and not np.allclose(got['dq'][0], right['dq'][0], rtol=1e-3)
    assert not np.array_equal(got['q'][1], right['q'][1])


# ------------------------------------------------------------------------------------------------------------- miscalibrated
def test_miscalibrated_defaults_give_the_plant_back(uvs):
    plant = uvs.SyntheticPlant.ur10()
    same = uvs.plant.miscalibrated(plant)
    assert same is not plant and isinstance(same, uvs.SyntheticPlant)
    for name in ('theta_offset', 'd', 'a', 'alpha', 'points'):
        assert np.array_equal(getattr(same, name), getattr(plant, name)) and getattr(same, name) is not getattr(plant, name), name
    assert (same.focal, same.center, same.fov_deg) == (plant.focal, plant.center, plant.fov_deg)
    assert bytes(same.to_camera()) == bytes(plant.to_camera())


def test_miscalibrated_moves_what_it_says_and_keeps_fov_consistent(uvs):
    plant = uvs.SyntheticPlant.ur10()
    for scale in (0.8, 1.25, 1.2):
        wrong = uvs.plant.miscalibrated(plant, focal_scale=scale)
        assert wrong.focal == plant.focal * scale
        assert abs(uvs.plant.focal_length(uvs.plant.RESOLUTION, wrong.fov_deg) - wrong.focal) <= 1e-13 * wrong.focal
        assert uvs.SyntheticRobot(wrong).perspective_angle == wrong.fov_deg
        assert np.array_equal(wrong.points, plant.points) and np.array_equal(wrong.d, plant.d)
    wrong = uvs.plant.miscalibrated(plant, point_offset=(0.05, -0.05, -0.2), joint_offset=JOINT_OFFSETS, link_scale=0.97)
    assert np.array_equal(wrong.points, plant.points + np.array([0.05, -0.05, -0.2]))
    assert np.array_equal(wrong.theta_offset, plant.theta_offset + np.array(JOINT_OFFSETS))
    assert np.array_equal(wrong.d, plant.d * 0.97) and np.array_equal(wrong.a, plant.a * 0.97) and np.array_equal(wrong.alpha, plant.alpha)
    assert wrong.focal == plant.focal and wrong.fov_deg == plant.fov_deg
    assert np.array_equal(plant.theta_offset, uvs.SyntheticPlant.ur10().theta_offset), 'the input was modified'
    scalar = uvs.plant.miscalibrated(plant, joint_offset=0.01)
    assert np.array_equal(scalar.theta_offset, plant.theta_offset + 0.01)


# ------------------------------------------------------------------------------------------------------------- ABI
def test_the_three_new_symbols_are_bound_and_the_header_agrees(uvs):
    counts = {'uvs_camera_believed_step_f64': 12, 'uvs_camera_believed_loop_f64': 17, 'uvs_camera_believed_guess_f64': 9}
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    for name, n_args in counts.items():
        assert name in uvs._vision.SYMBOLS and getattr(uvs._vision.lib(), name) is not None
        declaration = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert declaration is not None, name
        assert len(declaration.group(1).split(',')) == n_args == len(uvs._vision.SYMBOLS[name][1]), name
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    assert ctypes.sizeof(uvs._vision.Camera) == 472, 'the LDS figures of DESIGN.md 4.15 are for 472 B'


# ------------------------------------------------------------------------------------------------------------- refusals of the library
class Buffers:
    """Host arrays with sentinels: a refused (or empty) call must leave every one of them as it is."""
    NAMES = ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'j', 'stats', 'f0', 'x0')
    INTS = ('status', 'k_done', 'pixels', 'index')

    def __init__(self, uvs, T=2, K=3, n_points=4, n_joints=6, method='ANALYTICAL'):
        self.cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
        self.cam.n_points, self.cam.n_joints = n_points, n_joints
        self.fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=K)
        for name in self.NAMES:
            setattr(self, name, np.full(K * T * 48, 7.0))
        for name in self.INTS:
            setattr(self, name, np.full(T * 4, 7, np.int32))
        self.models = (uvs._vision.Camera * T)(*[self.cam] * T)      # host memory: no kernel could read it, and none is launched
        self.snapshot = bytes(self.models)
        self.T = T

    def ptr(self, name):
        return getattr(self, name).ctypes.data

    def untouched(self):
        return all(np.all(getattr(self, k) == 7) for k in self.NAMES + self.INTS) and bytes(self.models) == self.snapshot


def _args(b, over):
    a = {name: b.ptr(name) for name in Buffers.NAMES + Buffers.INTS}
    a.update(fp=b.fp, cam=b.cam, T=b.T, believed=ctypes.addressof(b.models), n_believed=b.T, n_points=4)
    a['index'] = None                                                # no index unless asked for
    a.update(over)
    a['fp'], a['cam'] = (None if a[k] is None else ctypes.byref(a[k]) for k in ('fp', 'cam'))
    return a


def loop_call(lib, b, **over):
    a = _args(b, over)
    return lib.uvs_camera_believed_loop_f64(a['fp'], a['cam'], a['T'], a['believed'], a['n_believed'], a['index'], a['q_start'], a['noise'], a['q'],
                                            a['f'], a['dq'], a['err'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def step_call(lib, b, **over):
    a = _args(b, over)
    return lib.uvs_camera_believed_step_f64(a['fp'], a['T'], a['believed'], a['n_believed'], a['index'], a['q'], a['f'], a['dq'], a['err'], a['j'],
                                            a['status'], None)


def guess_call(lib, b, **over):
    a = _args(b, over)
    return lib.uvs_camera_believed_guess_f64(a['T'], a['n_points'], a['believed'], a['n_believed'], a['index'], a['q_start'], a['f0'], a['x0'], None)


def _believed_operand_refusals(lib, b, call):
    assert call(lib, b, believed=None) == ARG and b'NULL' in lib.uvs_vision_last_error()
    for n_believed in (0, -1, b.T + 1, b.T - 1 if b.T > 2 else 3, 5):                     # without an index: 1 or T and nothing else
        assert call(lib, b, n_believed=n_believed) == ARG and b'n_believed' in lib.uvs_vision_last_error(), n_believed
    assert call(lib, b, n_believed=0, index=b.ptr('index')) == ARG                        # with one: at least one model
    assert call(lib, b, T=-1) == ARG


@pytest.mark.parametrize('call,mandatory', [(loop_call, ('fp', 'cam', 'believed', 'q_start', 'status', 'k_done', 'stats')),
                                            (step_call, ('fp', 'believed', 'q', 'f', 'dq', 'err', 'status'))])
def test_refuses_before_it_launches(uvs, call, mandatory):
    """Every refusal of the calibrated entry points (tests/test_camera_analytical_host.py), and those of the believed operand."""
    lib, b = uvs._vision.lib(), Buffers(uvs)
    for name in mandatory:
        assert call(lib, b, **{name: None}) == ARG, name
        assert b'NULL' in lib.uvs_vision_last_error(), name
    _believed_operand_refusals(lib, b, call)
    for method in ('GMCKF', 'KF', 'MCKF', 'IMCCKF'):
        assert call(lib, b, fp=Buffers(uvs, method=method).fp) == METHOD and b'ANALYTICAL' in lib.uvs_vision_last_error(), method
    lanes = Buffers(uvs)
    lanes.fp.lanes_per_filter = 4
    assert call(lib, b, fp=lanes.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    if call is loop_call:                                            # the step has no true camera: its shape is fp's own
        assert call(lib, b, cam=Buffers(uvs, n_points=3).cam) == SHAPE and b'n_points' in lib.uvs_vision_last_error()    # m = 8 of three discs
        assert call(lib, b, cam=Buffers(uvs, n_joints=5).cam) == SHAPE and b'n_joints' in lib.uvs_vision_last_error()
        for n_points in (0, 2, 5):
            assert call(lib, b, cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    for m, n, n_points, n_joints in ((4, 6, 2, 6), (8, 7, 4, 7), (6, 5, 3, 5), (16, 6, 4, 6), (7, 6, 3, 6), (0, 6, 4, 6), (8, 0, 4, 6), (8, 9, 4, 6)):
        other = Buffers(uvs, n_points=n_points, n_joints=n_joints)
        other.fp.m, other.fp.n = m, n
        assert call(lib, other) in (SHAPE, ARG) and other.untouched(), (m, n)
    seven = Buffers(uvs, n_joints=7)                                 # a consistent (8, 7): not an instantiated shape
    seven.fp.n = 7
    assert call(lib, seven) == SHAPE
    for reserved in (2, 3, 4, 256):
        bad = Buffers(uvs)
        bad.fp.reserved = reserved
        assert call(lib, b, fp=bad.fp) == ARG and b'reserved' in lib.uvs_vision_last_error(), reserved
    if call is loop_call:
        for steps in (0, -1):
            bad = Buffers(uvs)
            bad.fp.steps = steps
            assert call(lib, b, fp=bad.fp) == ARG, steps
    # nothing to do: OK and nothing is launched, at every shape, plain and strict, with one model and with an index
    for n_points in (4, 3, 1):
        for reserved in (0, STRICT):
            empty = Buffers(uvs, n_points=n_points)
            empty.fp.m, empty.fp.reserved = 2 * n_points, reserved
            assert call(lib, empty, T=0, n_believed=1) == 0 and lib.uvs_vision_last_error() == b'' and empty.untouched()
            assert call(lib, empty, T=0, index=empty.ptr('index')) == 0 and empty.untouched()
    assert b.untouched(), 'a refused call wrote'


def test_guess_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)
    for name in ('believed', 'q_start', 'f0', 'x0'):
        assert guess_call(lib, b, **{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    _believed_operand_refusals(lib, b, guess_call)
    for n_points in (0, 2, 5, -1):
        assert guess_call(lib, b, n_points=n_points) == ARG and b'n_points' in lib.uvs_vision_last_error(), n_points
    for n_points in (4, 3, 1):
        assert guess_call(lib, b, T=0, n_believed=1, n_points=n_points) == 0 and lib.uvs_vision_last_error() == b''
    assert b.untouched(), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- refusals of the Python layer
def test_python_layer_refuses_on_the_arguments_alone(uvs):
    """None of these reaches a device: the joints are host tensors, the models are never packed."""
    import torch
    plant = uvs.SyntheticPlant.ur10()
    wrong = uvs.plant.miscalibrated(plant, focal_scale=0.8)
    q0 = torch.zeros((2, 6), dtype=torch.float64)
    analytical = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    gmckf = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    for fp in (analytical, gmckf):
        for fused in (False, True):
            with pytest.raises(ValueError, match='believed_index without believed'):
                uvs.engine.camera_closed_loop(fp, plant, q0, fused=fused, believed_index=[0, 0])
    for fused in (False, True):
        with pytest.raises(ValueError, match="guess='device'"):
            uvs.engine.camera_closed_loop(gmckf, plant, q0, fused=fused, believed=wrong)                           # guess='host' is the default
        with pytest.raises(ValueError, match="guess='device'"):
            uvs.engine.camera_closed_loop(gmckf, plant, q0, fused=fused, believed=wrong, guess='host')
        with pytest.raises(ValueError, match='no x0'):
            uvs.engine.camera_closed_loop(gmckf, plant, q0, x0=np.zeros((2, 48)), fused=fused, believed=wrong, guess='device')
        with pytest.raises(ValueError, match='no x0'):                                                             # the baseline's own refusals stay
            uvs.engine.camera_closed_loop(analytical, plant, q0, x0=np.zeros((2, 48)), fused=fused, believed=wrong)
        with pytest.raises(ValueError, match='no x0'):
            uvs.engine.camera_closed_loop(analytical, plant, q0, guess='device', fused=fused, believed=wrong)
    f = torch.zeros((2, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match='believed_index without believed'):
        uvs.engine.camera_analytical_step(plant, q0, f, analytical, believed_index=[0, 0])
    with pytest.raises(ValueError, match='believed_index without believed'):
        uvs.engine.camera_guess(plant, q0, f, believed_index=[0, 0])


def test_a_host_index_is_checked_before_anything_is_uploaded(uvs):
    """Nothing here reaches a device: the joints are host tensors, and the refusal comes before the models are packed."""
    import torch
    plant = uvs.SyntheticPlant.ur10()
    models = [plant, uvs.plant.miscalibrated(plant, focal_scale=0.8), uvs.plant.miscalibrated(plant, link_scale=1.05)]
    packed = torch.zeros((3, ctypes.sizeof(uvs._vision.Camera)), dtype=torch.uint8)          # the shape of believed_models' result, on the host
    q0 = torch.zeros((2, 6), dtype=torch.float64)
    analytical = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    gmckf = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    for believed in (models, packed):
        for fp, guess in ((analytical, 'host'), (gmckf, 'device')):
            for fused in (False, True):
                for index in ([0, 3], [-1, 0], np.array([0, 5]), torch.tensor([2, 3])):
                    with pytest.raises(ValueError, match=r'must lie in \[0, 3\)'):
                        uvs.engine.camera_closed_loop(fp, plant, q0, fused=fused, guess=guess, believed=believed, believed_index=index)
                for index in ([0, 1, 2], [[0, 1]], [0.0, 1.0]):
                    with pytest.raises(ValueError, match='one per trial'):
                        uvs.engine.camera_closed_loop(fp, plant, q0, fused=fused, guess=guess, believed=believed, believed_index=index)
                with pytest.raises(ValueError, match='3 believed models for 2 trials'):
                    uvs.engine.camera_closed_loop(fp, plant, q0, fused=fused, guess=guess, believed=believed)
    check = uvs.engine._check_believed
    assert check(packed, None, 3, 'test') == (3, None) and check(plant, None, 5, 'test') == (1, None)
    n, index = check(models, [2, 0], 2, 'test')
    assert n == 3 and index.dtype == np.int32 and index.tolist() == [2, 0]
    with pytest.raises(ValueError, match='what believed_models returns'):
        check(packed.to(torch.float32), None, 3, 'test')
    with pytest.raises(ValueError, match='what believed_models returns'):
        check(packed[:, :-8], None, 3, 'test')
    with pytest.raises(ValueError, match='at least one'):
        check([], None, 1, 'test')


# ------------------------------------------------------------------------------------------------------------- the built library
def test_new_kernels_are_built_without_scratch(uvs):
    """From the code objects embedded in the built library: the believed step per shape, the believed loop per shape in its one-trial and its
    four-trial form, the believed guess -- no form is refused -- and no private segment anywhere in the library; the calibrated and the
    estimator kernels are counted where they always were (tests/test_camera_analytical_host.py)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    step = {name: r for name, r in k.items() if 'camera_believed_step_kernel' in name}
    loop = {name: r for name, r in k.items() if 'camera_believed_loop_kernel' in name}
    guess = {name: r for name, r in k.items() if 'camera_believed_guess_kernel' in name}
    for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1'):
        assert any(f'<{shape}>' in name for name in step), (shape, sorted(step))
        for per_workgroup in (1, 4):
            assert any(f'<{shape}, {per_workgroup}>' in name for name in loop), (shape, per_workgroup, sorted(loop))
    assert len(step) == 3 and len(loop) == 6 and len(guess) == 1
    assert len([name for name in k if 'camera_believed_' in name]) == 10
    for name in list(step) + list(loop) + list(guess):
        assert not any(old in name for old in ('camera_analytical_step_kernel', 'camera_analytical_loop_kernel', 'camera_loop_kernel')), name
    for name, r in k.items():
        assert r['scratch'] == 0, (name, r)
    for name, r in loop.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960, (name, r)
    for name, r in step.items():                                     # 64 / L models of 472 B
        lanes = int(re.search(r'<\d+, \d+, (\d+)>', name).group(1))
        assert r['wg'] == 64 and r['lds'] == (64 // lanes) * 472, (name, r)
    for r in guess.values():
        assert r['wg'] == 64 and r['lds'] == 0, r
