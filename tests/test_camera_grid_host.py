"""CPU-only tests of the pixel loop's per-trial entry point (include/uvs_vision.h: uvs_camera_closed_loop_grid_f64) and of its Python route
(engine.camera_closed_loop(trial_params=...)): the symbol is bound and the header agrees with the ctypes table, every refusal comes before
any HIP call (the buffers here are host arrays no kernel could use, filled with sentinels that must survive), the Python layer raises before
any device work, and the built library holds exactly the documented instantiations of camera_grid_kernel, none with a private segment."""
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
    NAMES = ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'stats', 'kernel_bw', 'gain', 'reg', 'fpi_threshold', 'desired')
    INTS = ('status', 'k_done', 'pixels', 'source')

    def __init__(self, uvs, T=2, K=3, n_points=4, n_joints=6, method='GMCKF'):
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

    def trial_params(self, uvs, n_in=2, **over):
        members = {name: self.ptr(name) for name in ('kernel_bw', 'gain', 'reg', 'fpi_threshold', 'desired', 'source')}
        members.update(over)
        return uvs._vision.CameraTrialParams(n_in=n_in, **members)

    def untouched(self):
        return all(np.all(getattr(self, k) == 7) for k in self.NAMES + self.INTS)


TP_DEFAULT = object()


def grid_call(uvs, b, T=None, tp=TP_DEFAULT, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp, cam=b.cam)
    a.update(over)
    if tp is TP_DEFAULT:
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_grid_f64(ref(a['fp']), ref(a['cam']), b.T if T is None else T, ref(tp), a['q_start'], a['noise'],
                                                             a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], a['status'],
                                                             a['k_done'], a['stats'], a['pixels'], None)


def test_the_symbol_is_bound_and_the_header_agrees(uvs):
    name = 'uvs_camera_closed_loop_grid_f64'
    assert name in uvs._vision.SYMBOLS and getattr(uvs._vision.lib(), name) is not None
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: re.search(fn + r'\s*\(([^;]*)\);', header).group(1).split(',')   # noqa: E731
    uniform, grid = declared('int uvs_camera_closed_loop_f64'), declared('int ' + name)
    assert len(uniform) == 17 == len(uvs._vision.SYMBOLS['uvs_camera_closed_loop_f64'][1])
    assert len(grid) == 18 == len(uvs._vision.SYMBOLS[name][1])
    # the uniform call's argument list plus the per-trial block
    strip = lambda args: [' '.join(a.split()) for a in args]        # noqa: E731
    assert strip(grid[:3] + grid[4:]) == strip(uniform) and 'uvs_camera_trial_params *tp' in grid[3]
    # the struct mirror: seven members of pointer size, in the header's order
    body = re.search(r'typedef struct uvs_camera_trial_params \{(.*?)\} uvs_camera_trial_params;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'(\w+)\s*[,;]', body) ==[f[0] for f in uvs._vision.CameraTrialParams._fields_]
    assert ctypes.sizeof(uvs._vision.CameraTrialParams) == 7 * 8
    assert 'uvs_view' not in header and 'uvs_rmckf.h"' not in header, 'the vision header stands alone'


def test_the_grid_refuses_before_it_launches(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)
    # the refusals of uvs_camera_closed_loop_f64
    for name in ('fp', 'cam', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
        assert grid_call(uvs, b, **{name: None}) == ARG, name
        assert b'NULL' in lib.uvs_vision_last_error(), name
    assert grid_call(uvs, b, T=-1) == ARG
    for steps in (0, -1):
        bad = Buffers(uvs)
        bad.fp.steps = steps
        assert grid_call(uvs, b, fp=bad.fp) == ARG, steps
    lanes = Buffers(uvs)
    lanes.fp.lanes_per_filter = 2
    assert grid_call(uvs, b, fp=lanes.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    assert grid_call(uvs, b, cam=Buffers(uvs, n_points=3).cam) == SHAPE and b'n_points' in lib.uvs_vision_last_error()   # m = 8 of three discs
    assert grid_call(uvs, b, cam=Buffers(uvs, n_joints=5).cam) == SHAPE and b'n_joints' in lib.uvs_vision_last_error()
    for n_points in (0, 2, 5):
        assert grid_call(uvs, b, cam=Buffers(uvs, n_points=n_points).cam) == ARG, n_points
    analytical = Buffers(uvs)
    analytical.fp.method = 1                                         # UVS_METHOD_ANALYTICAL
    assert grid_call(uvs, b, fp=analytical.fp) == METHOD
    # MCKF at (6, 6) is the one flavour that is not built (include/uvs_vision.h says so)
    mckf = Buffers(uvs, n_points=3, method='MCKF')
    mckf.fp.m = 6
    assert grid_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error()
    mckf.fp.fpi_epoch_max = 0
    mckf.fp.m, mckf.cam.n_points = 8, 4
    assert grid_call(uvs, mckf) == ARG
    # its own: no block, or a source index with no trials to index
    assert grid_call(uvs, b, tp=None) == ARG and b'tp' in lib.uvs_vision_last_error()
    for n_in in (0, -3):
        assert grid_call(uvs, b, tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    assert grid_call(uvs, b, T=0, tp=None) == ARG and grid_call(uvs, b, T=0, tp=b.trial_params(uvs, n_in=0)) == ARG, 'refusals come before T == 0'
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


def test_nothing_to_do_is_ok(uvs):
    lib, b = uvs._vision.lib(), Buffers(uvs)
    null = uvs._vision.CameraTrialParams()
    assert null.source is None and null.kernel_bw is None and null.n_in == 0
    assert grid_call(uvs, b, T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert grid_call(uvs, b, T=0, tp=null) == 0, 'n_in is read only with source'
    assert grid_call(uvs, b, T=0, tp=b.trial_params(uvs, n_in=0, source=None)) == 0
    assert grid_call(uvs, Buffers(uvs, method='MCKF'), T=0) == 0 and lib.uvs_vision_last_error() == b''
    assert grid_call(uvs, b, T=0, noise=None, q=None, f=None, dq=None, err=None, kappa=None, pixels=None) == 0
    assert b.untouched()


def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these must be a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    loop, plant = uvs.engine.camera_closed_loop, uvs.SyntheticPlant.ur10()
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    q = torch.zeros((2, 6), dtype=torch.float64)
    x0 = np.zeros((2, 48))
    with pytest.raises(ValueError, match='fused=True'):
        loop(fp, plant, q, x0=x0, trial_params={})
    with pytest.raises(ValueError, match='fused=True'):
        loop(fp, plant, q, x0=x0, fused=False, trial_params={'gain': None})
    analytical = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    with pytest.raises(ValueError, match='ANALYTICAL'):
        loop(analytical, plant, q, fused=True, trial_params={})
    with pytest.raises(ValueError, match='believed'):
        loop(fp, plant, q, fused=True, guess='device', believed=plant, trial_params={})
    with pytest.raises(ValueError, match='believed'):
        loop(fp, plant, q, fused=True, believed_index=[0, 0], trial_params={})
    for source in ([0, 2], [-1, 0], np.array([0, 1, 2]), torch.tensor([5], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r'source.*\[0, 2\)'):
            loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': source})
    for source in ([0.0, 1.0], [[0, 1]]):
        with pytest.raises(ValueError, match='source'):
            loop(fp, plant, q, x0=x0, fused=True, trial_params={'source': source})
    with pytest.raises(ValueError, match='unknown keys'):
        loop(fp, plant, q, x0=x0, fused=True, trial_params={'bandwidth': None})
    with pytest.raises(ValueError, match='dict'):
        loop(fp, plant, q, x0=x0, fused=True, trial_params=[1.0, 2.0])
    assert uvs.engine.TRIAL_PARAM_KEYS == tuple(f[0] for f in uvs._vision.CameraTrialParams._fields_[:6])


def test_the_documented_instantiations_are_built_without_scratch(uvs):
    """camera_grid_kernel: GMCKF (5), KF (2) and IMCC-KF (4) at (8,6,4), (6,6,2) and (2,6,1), MCKF (3) at (8,6,4) and (2,6,1), each in its
    one-trial and its four-trial form -- 22 -- and nothing else: MCKF at (6,6,2) is the one documented absence.  Read from the code objects
    embedded in the built library."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    grid = {name: r for name, r in k.items() if 'camera_grid_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'camera_grid_kernel(<[^>]*>)', name).group(1) for name in grid}
    assert found == expected and len(grid) == 22, (sorted(found ^ expected), len(grid))
    assert not any('<6, 6, 2, 3,' in name for name in grid)
    for name, r in grid.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 40960 and r['scratch'] == 0, (name, r)
    # the per-trial unit adds kernels: it renames none of the library's
    for pinned in ('camera_loop_kernel', 'camera_analytical_', 'camera_believed_'):
        assert not any(pinned in name for name in grid), pinned
    assert sum('camera_loop_kernel' in name for name in k) == 22
