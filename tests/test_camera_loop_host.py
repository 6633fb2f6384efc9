"""CPU-only tests of the one-launch pixel loop and the device guess (include/uvs_vision.h: uvs_camera_closed_loop_f64,
uvs_camera_guess_f64): both are bound, the entry points refuse bad arguments before any HIP call (the buffers here are host arrays no
kernel could use, filled with sentinels that must survive), and no kernel of the new unit carries a private segment."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

ARG, SHAPE, METHOD = -1, -2, -4
DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


class Buffers:
    """Host arrays with sentinels: a refused (or empty) call must leave every one of them as it is."""
    NAMES = ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'stats')

    def __init__(self, uvs, T=2, K=3, n_points=4, n_joints=6, method='GMCKF'):
        self.cam = uvs.SyntheticPlant.ur10().to_camera(0.024)
        self.cam.n_points, self.cam.n_joints = n_points, n_joints
        self.fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=K)
        for name in self.NAMES:
            setattr(self, name, np.full(K * T * 48, 7.0))
        self.status, self.k_done, self.pixels = (np.full(T * 4, 7, np.int32) for _ in range(3))
        self.T = T

    def ptr(self, name):
        return getattr(self, name).ctypes.data

    def untouched(self):
        return all(np.all(getattr(self, k) == 7) for k in self.NAMES + ('status', 'k_done', 'pixels'))


def loop_call(lib, b, T=None, **over):
    a = {name: b.ptr(name) for name in Buffers.NAMES + ('status', 'k_done', 'pixels')}
    a.update(fp=b.fp, cam=b.cam)
    a.update(over)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return lib.uvs_camera_closed_loop_f64(ref(a['fp']), ref(a['cam']), b.T if T is None else T, a['q_start'], a['noise'], a['x0'], a['f0'],
                                          a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'], a['k_done'], a['stats'], a['pixels'], None)


def test_both_new_symbols_are_bound_and_the_header_agrees(uvs):
    for name in ('uvs_camera_closed_loop_f64', 'uvs_camera_guess_f64'):
        assert name in uvs._vision.SYMBOLS and getattr(uvs._vision.lib(), name) is not None
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    assert len(uvs._vision.SYMBOLS['uvs_camera_closed_loop_f64'][1]) == 17 and len(uvs._vision.SYMBOLS['uvs_camera_guess_f64'][1]) == 6


def test_closed_loop_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)
    for name in ('fp', 'cam', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
        assert loop_call(lib, b, **{name: None}) == ARG, name
        assert b'NULL' in lib.uvs_vision_last_error(), name
    assert loop_call(lib, b, T=-1) == ARG
    for steps in (0, -1):
        bad = Buffers(uvs)
        bad.fp.steps = steps
        assert loop_call(lib, b, fp=bad.fp) == ARG, steps
    lanes = Buffers(uvs)
    lanes.fp.lanes_per_filter = 2
    assert loop_call(lib, b, fp=lanes.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    assert loop_call(lib, b, cam=Buffers(uvs, n_points=3).cam) == SHAPE and b'n_points' in lib.uvs_vision_last_error()   # m = 8 of three discs
    assert loop_call(lib, b, cam=Buffers(uvs, n_joints=5).cam) == SHAPE and b'n_joints' in lib.uvs_vision_last_error()
    for n_points in (0, 2, 5):
        assert loop_call(lib, b, cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    analytical = Buffers(uvs)
    analytical.fp.method = 1                                         # UVS_METHOD_ANALYTICAL
    assert loop_call(lib, b, fp=analytical.fp) == METHOD
    # MCKF is built at (8, 6) and (2, 6) and refused at (6, 6), where its instantiation would spill (include/uvs_vision.h says so)
    mckf = Buffers(uvs, n_points=3, method='MCKF')
    mckf.fp.m = 6
    assert loop_call(lib, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error()
    mckf.fp.fpi_epoch_max = 0
    mckf.fp.m, mckf.cam.n_points = 8, 4
    assert loop_call(lib, mckf) == ARG
    # nothing to do: OK, nothing is launched, and that includes a built MCKF shape
    assert loop_call(lib, b, T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert loop_call(lib, Buffers(uvs, method='MCKF'), T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert loop_call(lib, b, T=0, noise=None, q=None, f=None, dq=None, err=None, kappa=None, pixels=None) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_guess_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)

    def call(cam=b.cam, T=b.T, q_start=b.ptr('q_start'), f0=b.ptr('f0'), x0=b.ptr('x0')):
        return lib.uvs_camera_guess_f64(None if cam is None else ctypes.byref(cam), T, q_start, f0, x0, None)

    assert call(cam=None) == ARG and call(q_start=None) == ARG and call(f0=None) == ARG and call(x0=None) == ARG
    assert call(T=-1) == ARG
    assert call(cam=Buffers(uvs, n_points=2).cam) == ARG and call(cam=Buffers(uvs, n_joints=7).cam) == SHAPE
    for n_points in (1, 3, 4):
        assert call(cam=Buffers(uvs, n_points=n_points).cam, T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert b.untouched(), 'a refused call wrote'


def test_new_kernels_have_no_scratch(uvs):
    """Every kernel of libuvs_vision.so, the loop kernel's instantiations first: (8,6,4), (6,6,2), (2,6,1) x GMCKF, KF, IMCC-KF, and MCKF where
    it is built, each in its one-trial and its four-trial form.  Read from the code objects embedded in the built library."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    loop = {name: r for name, r in k.items() if 'camera_loop_kernel' in name}
    for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5))):
        for method in methods:
            for per_workgroup in (1, 4):                             # trials per workgroup: small batches, large batches
                assert any(f'<{shape}, {method}, {per_workgroup}>' in name for name in loop), (shape, method, per_workgroup, sorted(loop))
    assert len(loop) == 22 and not any('<6, 6, 2, 3,' in name for name in loop)
    assert any('camera_guess_kernel' in name for name in k) and any('camera_features_kernel' in name for name in k)
    for name, r in k.items():
        assert r['scratch'] == 0, (name, r)
    for name, r in loop.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960, (name, r)


def test_fused_loop_wants_its_joints_on_the_device(uvs):
    import torch
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp, uvs.SyntheticPlant.ur10(), torch.zeros((2, 6), dtype=torch.float64), fused=True)
    with pytest.raises(ValueError):
        uvs.engine.camera_closed_loop(fp, uvs.SyntheticPlant.ur10(), torch.zeros((2, 6), dtype=torch.float64), fused=True, guess='nowhere')
