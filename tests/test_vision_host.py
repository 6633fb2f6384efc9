"""CPU-only tests of the device circle detector's host side: libuvs_vision.so cross-compiles, loads and exports every symbol of
include/uvs_vision.h, refuses bad arguments before any HIP call (the buffers here are host arrays no kernel could use), and Experiment
validates its ``perception`` option."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


def test_library_exports_every_header_symbol(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    declared = set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header))
    assert declared == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    handle = uvs._vision.lib()
    for name in declared:
        assert getattr(handle, name) is not None
    assert handle.uvs_vision_version().startswith(b'uvs_vision')


def test_return_codes_are_those_of_the_rmckf_header():
    text = {name: open(os.path.join(ROOT, 'include', name)).read() for name in ('uvs_rmckf.h', 'uvs_vision.h')}
    for macro in ('UVS_OK', 'UVS_ERR_ARG', 'UVS_ERR_SHAPE', 'UVS_ERR_HIP'):
        values = {re.search(r'#define\s+' + macro + r'\s+(\S+)', t).group(1) for t in text.values()}
        assert len(values) == 1, (macro, values)


def test_detector_refuses_before_it_launches(uvs):
    lib = uvs._vision.lib()
    S = 256
    dense = S * S * 3
    frames = np.zeros(2 * (dense + 16) + 16, np.uint8)
    base = frames.ctypes.data + (-frames.ctypes.data) % 16                              # 16-byte aligned host address
    f_out = (ctypes.c_double * 16)()
    out = ctypes.cast(f_out, ctypes.c_void_p)
    ARG, SHAPE = -1, -2

    def call(T=2, frames=base, stride=dense, h=S, w=S, n=4, f=out):
        return lib.uvs_detect_circles_u8(T, frames, stride, h, w, n, None, f, None, None)

    assert call(frames=None) == ARG and b'NULL' in lib.uvs_vision_last_error()
    assert call(f=None) == ARG
    assert call(T=-1) == ARG
    for n in (0, 2, 5, -1):
        assert call(n=n) == ARG, n
    assert call(stride=dense - 16) == ARG                                                # frames would overlap
    assert call(stride=dense + 8) == ARG and b'16' in lib.uvs_vision_last_error()         # rows are read with 16-byte loads
    assert call(frames=base + 4) == ARG                                                  # likewise the base address
    for h, w in ((128, 128), (256, 128), (128, 256), (512, 512), (257, 256)):
        assert call(h=h, w=w, stride=-(-h * w * 3 // 16) * 16) == SHAPE, (h, w)
    assert b'256' in lib.uvs_vision_last_error()
    assert call(h=0) == ARG
    for n in (1, 3, 4):                                                                  # nothing to do: OK, and nothing is launched
        assert call(T=0, n=n) == 0 and lib.uvs_vision_last_error() == b''
    assert not np.any(np.frombuffer(f_out)), 'a refused call wrote its output'


def test_missing_library_is_an_error_not_a_fallback(uvs, monkeypatch):
    monkeypatch.setattr(uvs._vision, '_lib', None)
    monkeypatch.setattr(uvs._vision, 'LIB_PATH', os.path.join(ROOT, 'no_such_dir', 'libuvs_vision.so'))
    with pytest.raises(uvs.UvsLibraryError):
        uvs._vision.lib()


def _experiment(uvs, **kw):
    return uvs.Experiment([0.0] * 6, [0.0] * 8, None, 0.05, 15, 0.2, object(), uvs.Method.GMCKF, initial_guess=True, kernel_bw=10,
                          fpi_threshold=0.1, fpi_epoch_max=10, annealing=False, **kw)


def test_experiment_validates_perception(uvs):
    with pytest.raises(ValueError, match='perception'):
        _experiment(uvs, perception='nonsense')
    with pytest.raises(ValueError, match='perception'):
        _experiment(uvs, method_params=dict(initial_guess=True, kernel_bw=10, fpi_threshold=0.1, fpi_epoch_max=10, annealing=False,
                                            perception='GPU'))
    assert _experiment(uvs, perception='device').perception == 'device'
    assert _experiment(uvs, perception='host').perception == 'host'


def test_perception_absent_leaves_the_constructor_as_before(uvs):
    plain, host = _experiment(uvs), _experiment(uvs, perception='host')
    assert plain.perception == 'host'
    for exp in (plain, host):
        assert (exp.initial_guess, exp.kernel_bw, exp.fpi_threshold, exp.fpi_epoch_max, exp.annealing, exp.lanes, exp.x0) == \
            (True, 10, 0.1, 10, False, 0, None)
    assert {k for k in vars(plain)} == {k for k in vars(host)}


def test_device_wrappers_are_public_and_host_detectors_untouched(uvs):
    for name in ('detect4Circles_device', 'detectRGBCircles_device', 'detectGreenCircle_device', 'detect4Circles', 'detectRGBCircles',
                 'detectGreenCircle'):
        assert callable(getattr(uvs.utils, name)), name
    assert callable(uvs.engine.detect_circles) and callable(uvs.engine.FilterBank.step_image) and callable(uvs.engine.FilterBank.set_features)
