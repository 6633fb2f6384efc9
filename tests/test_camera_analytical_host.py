"""CPU-only tests of the calibrated baseline's pixel loop (include/uvs_vision.h: uvs_camera_analytical_step_f64,
uvs_camera_analytical_loop_f64): both are bound, the entry points refuse bad arguments before any HIP call (the buffers here are host arrays
no kernel could use, filled with sentinels that must survive), the new kernels are built for every shape without a private segment next to an
unchanged set of estimator loop kernels, and the numpy restatement the GPU tests check against (tests/camera_analytical_ref.py) is, fed ideal
projections, the restatement of the ideal-feature baseline (tests/analytical_ref.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

ARG, SHAPE, METHOD = -1, -2, -4
ANALYTICAL, GMCKF, STRICT = 1, 5, 1
DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
Q_HOST_ROUTE = np.array([[0.00236432, 0.09009274, 1.89232733, 0.08972989, -1.60843004, -0.01533471],
                         [-0.05930895, -0.04753733, 2.01356834, -0.04391825, -1.57375814, 0.09614744]])


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


class Buffers:
    """Host arrays with sentinels: a refused (or empty) call must leave every one of them as it is."""
    NAMES = ('q_start', 'noise', 'q', 'f', 'dq', 'err', 'j', 'stats')
    INTS = ('status', 'k_done', 'pixels')

    def __init__(self, uvs, T=2, K=3, n_points=4, n_joints=6, method='ANALYTICAL'):
        self.cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
        self.cam.n_points, self.cam.n_joints = n_points, n_joints
        self.fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=K)
        for name in self.NAMES:
            setattr(self, name, np.full(K * T * 48, 7.0))
        for name in self.INTS:
            setattr(self, name, np.full(T * 4, 7, np.int32))
        self.T = T

    def ptr(self, name):
        return getattr(self, name).ctypes.data

    def untouched(self):
        return all(np.all(getattr(self, k) == 7) for k in self.NAMES + self.INTS)


def _args(b, over):
    a = {name: b.ptr(name) for name in Buffers.NAMES + Buffers.INTS}
    a.update(fp=b.fp, cam=b.cam, T=b.T)
    a.update(over)
    a['fp'], a['cam'] = (None if a[k] is None else ctypes.byref(a[k]) for k in ('fp', 'cam'))
    return a


def loop_call(lib, b, **over):
    a = _args(b, over)
    return lib.uvs_camera_analytical_loop_f64(a['fp'], a['cam'], a['T'], a['q_start'], a['noise'], a['q'], a['f'], a['dq'], a['err'], a['status'],
                                              a['k_done'], a['stats'], a['pixels'], None)


def step_call(lib, b, **over):
    a = _args(b, over)
    return lib.uvs_camera_analytical_step_f64(a['fp'], a['cam'], a['T'], a['q'], a['f'], a['dq'], a['err'], a['j'], a['status'], None)


def test_both_new_symbols_are_bound_and_the_header_agrees(uvs):
    counts = {'uvs_camera_analytical_step_f64': 10, 'uvs_camera_analytical_loop_f64': 14}
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    for name, n_args in counts.items():
        assert name in uvs._vision.SYMBOLS and getattr(uvs._vision.lib(), name) is not None
        declaration = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert declaration is not None, name
        assert len(declaration.group(1).split(',')) == n_args == len(uvs._vision.SYMBOLS[name][1]), name


@pytest.mark.parametrize('call,mandatory', [(loop_call, ('fp', 'cam', 'q_start', 'status', 'k_done', 'stats')),
                                            (step_call, ('fp', 'cam', 'q', 'f', 'dq', 'err', 'status'))])
def test_refuses_before_it_launches(uvs, call, mandatory):
    lib, b = uvs._vision.lib(), Buffers(uvs)
    for name in mandatory:
        assert call(lib, b, **{name: None}) == ARG, name
        assert b'NULL' in lib.uvs_vision_last_error(), name
    assert call(lib, b, T=-1) == ARG
    for method in ('GMCKF', 'KF', 'MCKF', 'IMCCKF'):
        assert call(lib, b, fp=Buffers(uvs, method=method).fp) == METHOD and b'ANALYTICAL' in lib.uvs_vision_last_error(), method
    lanes = Buffers(uvs)
    lanes.fp.lanes_per_filter = 4
    assert call(lib, b, fp=lanes.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    assert call(lib, b, cam=Buffers(uvs, n_points=3).cam) == SHAPE and b'n_points' in lib.uvs_vision_last_error()        # m = 8 of three discs
    assert call(lib, b, cam=Buffers(uvs, n_joints=5).cam) == SHAPE and b'n_joints' in lib.uvs_vision_last_error()
    for n_points in (0, 2, 5):
        assert call(lib, b, cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    for m, n, n_points, n_joints in ((4, 6, 2, 6), (8, 7, 4, 7), (6, 5, 3, 5), (16, 6, 4, 6)):
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
    # nothing to do: OK and nothing is launched, at every shape, plain and strict, with and without the optional buffers
    for n_points in (4, 3, 1):
        for reserved in (0, STRICT):
            empty = Buffers(uvs, n_points=n_points)
            empty.fp.m, empty.fp.reserved = 2 * n_points, reserved
            assert call(lib, empty, T=0) == 0 and lib.uvs_vision_last_error() == b'' and empty.untouched()
    assert call(lib, b, T=0, noise=None, q=None if call is loop_call else b.ptr('q'), f=None if call is loop_call else b.ptr('f'),
                dq=None if call is loop_call else b.ptr('dq'), err=None if call is loop_call else b.ptr('err'), j=None, pixels=None) == 0
    assert b.untouched(), 'a refused call wrote'


def test_estimator_loop_still_refuses_the_baseline(uvs):
    b = Buffers(uvs)
    x0 = np.full(96, 7.0)
    rc = uvs._vision.lib().uvs_camera_closed_loop_f64(ctypes.byref(b.fp), ctypes.byref(b.cam), b.T, b.ptr('q_start'), b.ptr('noise'), x0.ctypes.data,
                                                      x0.ctypes.data, b.ptr('q'), b.ptr('f'), b.ptr('dq'), b.ptr('err'), b.ptr('j'), b.ptr('status'),
                                                      b.ptr('k_done'), b.ptr('stats'), b.ptr('pixels'), None)
    assert rc == METHOD and b.untouched() and np.all(x0 == 7)


def test_new_kernels_are_built_without_scratch(uvs):
    """From the code objects embedded in the built library: the step kernel per shape, the loop kernel per shape in its one-trial and its
    four-trial form, no private segment anywhere in the library, and the estimator loop's set of 22 as it was."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    step = {name: r for name, r in k.items() if 'camera_analytical_step_kernel' in name}
    loop = {name: r for name, r in k.items() if 'camera_analytical_loop_kernel' in name}
    for shape in ('8, 6, 4', '6, 6, 2', '2, 6, 1'):
        assert any(f'<{shape}>' in name for name in step), (shape, sorted(step))
        for per_workgroup in (1, 4):
            assert any(f'<{shape}, {per_workgroup}>' in name for name in loop), (shape, per_workgroup, sorted(loop))
    assert len(step) == 3 and len(loop) == 6
    for name, r in k.items():
        assert r['scratch'] == 0, (name, r)
    for name, r in loop.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960, (name, r)
    for name, r in step.items():
        assert r['wg'] == 64 and r['lds'] == 0, (name, r)
    assert len([name for name in k if 'camera_loop_kernel' in name]) == 22


def test_restatement_with_ideal_projection_is_the_ideal_feature_checker(uvs):
    """tests/camera_analytical_ref.py with the detection replaced by the ideal projection against tests/analytical_ref.run (the checker of
    uvs_analytical_closed_loop_f64): the same formula from other host pieces (analytic_guess over SyntheticRobot here, stacked matrices
    there), 3 trials x 20 steps, 1e-12 relative."""
    import analytical_ref
    import camera_analytical_ref as ref
    K, dt, gain = 20, 0.05, 0.2
    plant = uvs.SyntheticPlant.ur10()
    q0 = np.concatenate([Q_HOST_ROUTE, Q_HOST_ROUTE[:1] + 0.03])
    noise = np.random.default_rng(5).standard_normal((3, K, 8)) * 0.3
    want = analytical_ref.run(q0, noise, DESIRED, dt, dt * (K + 0.5), gain, steps=K, plant=plant)
    assert want['k_done'].tolist() == [K] * 3
    for t in range(3):
        got = ref.run(plant, q0[t], noise[t], DESIRED, dt, gain, K, ideal=True)
        assert got['status'] == 0 and got['k_done'] == K
        for key in ('err', 'q', 'f', 'dq', 'j'):
            rel = np.abs(got[key] - want[key][t]).max() / np.abs(want[key][t]).max()
            assert rel < 1e-12, (t, key, rel)
        assert np.abs(got['stats'] - want['stats'][t]).max() / np.abs(want['stats'][t]).max() < 1e-12


def test_closed_loop_refuses_estimator_arguments_on_the_baseline(uvs):
    """The refusals come from the arguments alone, before the device is looked at: the joints here are host tensors."""
    import torch
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    plant, q0 = uvs.SyntheticPlant.ur10(), torch.zeros((2, 6), dtype=torch.float64)
    for fused in (False, True):
        with pytest.raises(ValueError, match='no x0'):
            uvs.engine.camera_closed_loop(fp, plant, q0, x0=np.zeros((2, 48)), fused=fused)
        with pytest.raises(ValueError, match='no x0'):
            uvs.engine.camera_closed_loop(fp, plant, q0, guess='device', fused=fused)
        with pytest.raises(ValueError, match='kappa'):
            uvs.engine.camera_closed_loop(fp, plant, q0, want=('err', 'kappa'), fused=fused)
    with pytest.raises(ValueError, match='on the device'):
        uvs.engine.camera_closed_loop(fp, plant, q0, fused=True)
    assert 'kappa' not in uvs.engine.ANALYTICAL_CAMERA_LOGS and set(uvs.engine.ANALYTICAL_CAMERA_LOGS) < set(uvs.engine.CAMERA_LOGS)
