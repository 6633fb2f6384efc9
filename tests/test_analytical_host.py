"""CPU tests of the calibrated IBVS baseline (Method.ANALYTICAL): the C-ABI entry point exists and refuses bad arguments before any GPU work,
the numpy restatement (tests/analytical_ref.py) reproduces the reference's own runs, and the new kernels carry no private segment."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden, rel_err

FIXTURES = golden_names('analytical_')
# relative gate against the reference's run.  analytical_mix_hold (mixture outliers of 50 px held for 0.5 s) is intrinsically sensitive:
# moving its start by 1e-14 moves its error log by ~1e-4 relative (test_mix_hold_gate_is_the_trajectory_sensitivity), so no evaluation
# other than the reference's own bits can meet a tight gate there; it is held to 1e-3.  Every other fixture: 1e-12.
GATE = {'analytical_mix_hold': 1e-3}


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    return uvs_amd


def test_entry_point_is_declared_and_bound(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_rmckf.h')).read()
    assert re.search(r'\buvs_analytical_closed_loop_f64\s*\(', header)
    assert 'uvs_analytical_closed_loop_f64' in uvs._lib.SYMBOLS
    assert uvs.lib().uvs_analytical_closed_loop_f64 is not None
    assert uvs.engine.METHOD_CODES['ANALYTICAL'] == 1 == uvs.Method.ANALYTICAL.value


def test_return_codes_without_gpu_work(uvs):
    lib = uvs.lib()
    V = uvs._lib.NULL_VIEW
    fake = ctypes.c_void_p(0x1000)                                           # never dereferenced: every case returns before the launch
    q = uvs._lib.View(0x1000, 6, 0, 1)
    plant = uvs.SyntheticPlant.ur10().to_struct()
    call = lambda fp, pl, status=fake: lib.uvs_analytical_closed_loop_f64(   # noqa: E731
        None if fp is None else ctypes.byref(fp), None if pl is None else ctypes.byref(pl), 4, q, V, V, V, V, V, V, None, status, None, None)
    assert call(None, plant) == -1
    for method in ('GMCKF', 'KF', 'MCKF', 'IMCCKF'):
        assert call(uvs.engine.make_params(8, 6, method, desired=np.zeros(8), steps=3), plant) == -4
    for m, n in ((7, 7), (8, 7)):
        assert call(uvs.engine.make_params(m, n, 'ANALYTICAL', desired=np.zeros(m), steps=3), plant) == -2
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', desired=np.zeros(8), steps=3)
    lin = uvs.SyntheticPlant.ur10().to_struct()
    lin.kind = uvs._lib.PLANT_LINEAR
    assert call(fp, lin) == -1
    assert call(fp, plant, status=None) == -1 and b'status' in lib.uvs_last_error()
    fp.reserved = 2                                                          # UVS_OPT_LATENCY does not apply
    assert call(fp, plant) == -1
    fp.reserved = 4
    assert call(fp, plant) == -1
    # the estimator entry points keep refusing ANALYTICAL
    X = uvs._lib.NULL_VIEW
    fp.reserved = 0
    assert lib.uvs_rmckf_closed_loop_f64(ctypes.byref(fp), ctypes.byref(plant), 4, q, X, X, X, X, X, X, X, None, fake, None, X, X, None) == -4


def test_batch_refuses_lane_options(uvs):
    import json
    cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
    cfg['estimator']['method'] = 'ANALYTICAL'
    with pytest.raises(ValueError):
        uvs.batch.run_batch(cfg, epoch=2, lanes=2)
    with pytest.raises(ValueError):
        uvs.batch.run_sweep(cfg, epoch=2, latency=True)


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_reproduces_reference(name):
    import analytical_ref
    g = load_golden(name)
    meta = g['meta']
    noise = np.zeros((1, 400, 8))
    noise[0, :len(g['noise'])] = g['noise']
    if meta['profile'] == 'InfAt':                                           # the duck-typed profile logs no noise after the FAIL step
        noise[0, 40, 3] = np.inf
    out = analytical_ref.run(g['q_start'][None], noise, g['desired'], meta['dt'], meta['t_max'], meta['gain'])
    k = int(g['k_done'])
    assert int(out['status'][0]) == int(g['status']) and int(out['k_done'][0]) == k
    for key, ref in (('err', g['err']), ('q', g['q']), ('f', g['f']), ('j', g['J'])):
        assert rel_err(out[key][0, :k], ref) <= GATE.get(name, 1e-12), (key, rel_err(out[key][0, :k], ref))
    assert np.allclose(out['t'][:k], g['t'], rtol=0, atol=1e-12)


def test_mix_hold_gate_is_the_trajectory_sensitivity():
    """The loose gate of analytical_mix_hold is the trajectory's own sensitivity, not an error of the restatement: the restatement from
    q_start and from q_start moved by 1e-14 differ by far more than the 1e-12 / 1e-8 gates of the calm fixtures, while a calm fixture
    (analytical_a1p5) stays within them under the same perturbation."""
    import analytical_ref

    def spread(name):
        g = load_golden(name)
        meta = g['meta']
        noise = np.zeros((1, 400, 8))
        noise[0, :len(g['noise'])] = g['noise']
        a, b = (analytical_ref.run(g['q_start'][None] + d, noise, g['desired'], meta['dt'], meta['t_max'], meta['gain'], logs=('err',))
                for d in (0.0, 1e-14))
        return rel_err(b['err'], a['err'])
    s = spread('analytical_mix_hold')
    assert 1e-5 <= s <= 1e-3 / 2, s
    assert spread('analytical_a1p5') <= 1e-11


def test_new_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF):
        pytest.skip('llvm-readelf not available')
    k = kernel_resources.kernels()
    for careful in ('false', 'true'):
        r = k[f'analytical_kernel<8, 6, {careful}>']
        assert r['scratch'] == 0, r
