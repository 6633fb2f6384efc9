"""Per-trial estimator parameters (uvs_rmckf_closed_loop_grid_f64, engine.closed_loop(trial_params=...), batch.run_grid) -- everything that can be
checked without a GPU: the ctypes layout of uvs_trial_params against the compiler's, every refusal of the entry point (each returns before any
device work), the launch plan of run_grid, and the resources of the new kernels read from the built code object."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    return uvs_amd


def test_trial_params_layout_matches_the_header(uvs, tmp_path):
    """sizeof / offsetof of uvs_trial_params as the host compiler lays it out, against the ctypes mirror; the symbol is bound."""
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uvs_rmckf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(uvs_trial_params), offsetof(uvs_trial_params, kernel_bw), '
                   'offsetof(uvs_trial_params, gain), offsetof(uvs_trial_params, reg), offsetof(uvs_trial_params, fpi_threshold), '
                   'offsetof(uvs_trial_params, desired), offsetof(uvs_trial_params, source)); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['cc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    TP = uvs._lib.TrialParams
    assert got == [ctypes.sizeof(TP)] + [getattr(TP, f).offset for f in ('kernel_bw', 'gain', 'reg', 'fpi_threshold', 'desired', 'source')]
    assert 'uvs_rmckf_closed_loop_grid_f64' in uvs._lib.SYMBOLS and hasattr(uvs.lib(), 'uvs_rmckf_closed_loop_grid_f64')
    # ... and the argument list is uvs_rmckf_closed_loop_ws_f64's with the trial parameters after T
    ws, grid = uvs._lib.SYMBOLS['uvs_rmckf_closed_loop_ws_f64'][1], uvs._lib.SYMBOLS['uvs_rmckf_closed_loop_grid_f64'][1]
    assert grid[:3] == ws[:3] and grid[4:] == ws[3:] and grid[3]._type_ is TP


def test_return_codes_without_gpu_work(uvs):
    lib = uvs.lib()
    V = uvs._lib.NULL_VIEW
    fake = ctypes.c_void_p(0x1000)                                           # never dereferenced: every case returns before the launch
    q = uvs._lib.View(0x1000, 6, 0, 1)
    plant = uvs.SyntheticPlant.ur10().to_struct()
    tp = uvs._lib.TrialParams(None, None, None, None, V, None)

    def call(fp, pl=plant, tp=tp):
        return lib.uvs_rmckf_closed_loop_grid_f64(None if fp is None else ctypes.byref(fp), None if pl is None else ctypes.byref(pl), 4,
                                                  None if tp is None else ctypes.byref(tp), q, V, V, V, V, V, V, V, None, fake, None, V, V, None, 0, None)
    mk = lambda m=8, n=6, method='GMCKF', lanes=0: uvs.engine.make_params(m, n, method, desired=np.zeros(m), lanes=lanes, steps=3)   # noqa: E731
    assert call(None) == -1
    assert call(mk(), tp=None) == -1 and b'trial params' in lib.uvs_last_error()
    assert call(mk(method='ANALYTICAL')) == -4 and lib.uvs_last_error()
    for m, n in ((6, 6), (2, 6), (32, 7)):
        assert call(mk(m, n)) == -2, (m, n)
    for lanes in (1, 4, 8, -2):
        assert call(mk(lanes=lanes)) == -2 and b'lanes_per_filter' in lib.uvs_last_error(), lanes
    lin = uvs.SyntheticPlant.ur10().to_struct()
    lin.kind = uvs._lib.PLANT_LINEAR
    assert call(mk(), lin) == -2 and b'plant' in lib.uvs_last_error()
    for bit in (1, 2, 4):                                                    # UVS_OPT_STRICT_PINV, UVS_OPT_LATENCY, UVS_OPT_DIAG_DROP_SEG_FLAG
        for method in ('GMCKF', 'MCKF', 'KF', 'IMCCKF'):
            fp = mk(method=method)
            fp.reserved = bit
            assert call(fp) == -1 and b'UVS_OPT' in lib.uvs_last_error(), (bit, method)
    assert call(mk(), None) == -1                                            # the shared checks behind the refusals: no plant
    for lanes in (0, 2):                                                     # what is in scope passes every refusal and stops at the first shared check
        fp = mk(lanes=lanes)
        assert lib.uvs_rmckf_closed_loop_grid_f64(ctypes.byref(fp), ctypes.byref(plant), 4, ctypes.byref(tp), q, V, V, V, V, V, V, V, None, None, None, V, V,
                                                  None, 0, None) == -1 and b'status' in lib.uvs_last_error()


def test_python_refusals(uvs):
    cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
    cfg['estimator']['method'] = 'ANALYTICAL'
    with pytest.raises(ValueError):
        uvs.batch.run_grid(cfg, {'ibvs_gain': [0.1, 0.2]}, epoch=2)
    cfg['estimator']['method'] = 'GMCKF'
    with pytest.raises(ValueError):
        uvs.batch.run_grid(cfg, {'kernel_bw': [5.0]}, epoch=2, lanes=4)
    with pytest.raises(ValueError):
        uvs.batch.run_grid(cfg, {'t_max': [5.0]}, epoch=2)
    with pytest.raises(TypeError):
        uvs.batch.run_grid(cfg, {'kernel_bw': [5.0]}, epoch=2, strict_pinv=True)
    with pytest.raises(TypeError):
        uvs.batch.run_grid(cfg, {'kernel_bw': [5.0]}, epoch=2, latency=True)
    with pytest.raises(ValueError):
        uvs.batch.plan_grid({}, 10)
    import torch
    with pytest.raises(ValueError):
        uvs.engine.trial_params_struct({'bandwidth': None}, 4, 8, torch.device('cpu'))
    with pytest.raises(ValueError):                                          # fp32 where fp64 is needed
        uvs.engine.trial_params_struct({'gain': torch.zeros(4)}, 4, 8, torch.device('cpu'))
    with pytest.raises(ValueError):                                          # (T,) int32
        uvs.engine.trial_params_struct({'source': torch.zeros(4, dtype=torch.int64)}, 4, 8, torch.device('cpu'))


def test_grid_plan(uvs):
    """Grid-cell order (the product of the axes in the order given, last axis fastest), source = t % epoch, pieces cut at grid-cell boundaries; and the
    trials under every grid cell are plan_trials' own: run_grid draws no seeds or start poses of its own."""
    gp = uvs.batch.plan_grid({'kernel_bw': [2, 5, 10, 20], 'ibvs_gain': [0.1, 0.2, 0.4]}, 100)
    assert len(gp) == 12 and gp.pieces == [(0, 12)]
    assert gp.values.tolist() == [[b, g] for b in (2.0, 5.0, 10.0, 20.0) for g in (0.1, 0.2, 0.4)]
    src = gp.source(0, 12)
    assert src.dtype == np.int32 and np.array_equal(src, np.arange(1200) % 100)
    assert np.array_equal(gp.column('kernel_bw', 0, 12), np.repeat([2.0, 5.0, 10.0, 20.0], 300))
    assert np.array_equal(gp.column('ibvs_gain', 0, 12), np.tile(np.repeat([0.1, 0.2, 0.4], 100), 4))
    # the order of the axes is the caller's
    assert uvs.batch.plan_grid({'ibvs_gain': [0.1, 0.2], 'kernel_bw': [5, 10]}, 3).values.tolist() == [[0.1, 5.0], [0.1, 10.0], [0.2, 5.0], [0.2, 10.0]]
    for cap, want in ((None, [(0, 12)]), (1200, [(0, 12)]), (1199, [(0, 11), (11, 12)]), (500, [(0, 5), (5, 10), (10, 12)]), (250, [(h, min(12, h + 2)) for h in range(0, 12, 2)]),
                      (100, [(h, h + 1) for h in range(12)]), (7, [(h, h + 1) for h in range(12)])):
        pieces = uvs.batch.plan_grid(gp.axes, 100, cap).pieces
        assert pieces == want, cap
        assert [a for a, _ in pieces] == [0] + [b for _, b in pieces[:-1]] and pieces[-1][1] == 12          # a partition, in order
    assert np.array_equal(gp.source(5, 10), np.arange(500) % 100) and np.array_equal(gp.column('ibvs_gain', 5, 7), np.repeat([0.4, 0.1], 100))
    cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
    sub = gp.substituted(cfg, 7)                                             # kernel_bw 10, gain 0.2
    assert sub['estimator']['estimator_params']['kernel_bw'] == 10.0 and sub['experiments']['ibvs_gain'] == 0.2
    assert cfg['experiments']['ibvs_gain'] == 0.2 and cfg['estimator']['estimator_params']['kernel_bw'] == 10                  # (the caller's dict is not touched)
    sub['experiments']['ibvs_gain'] = cfg['experiments']['ibvs_gain']
    sub['estimator']['estimator_params']['kernel_bw'] = cfg['estimator']['estimator_params']['kernel_bw']
    assert sub == uvs.batch.load_config(cfg)                                 # nothing else differs
    # seeds and q_start under a grid cell: those of the substituted config's own sweep
    cells, epoch = [1.2, 1.5], 100
    base = uvs.batch.plan_trials(uvs.batch.load_config(cfg), cells, epoch)
    for h in (0, 7, 11):
        p = uvs.batch.plan_trials(gp.substituted(cfg, h), cells, epoch)
        assert np.array_equal(p.seed, base.seed) and np.array_equal(p.q_start, base.q_start) and np.array_equal(p.cell, base.cell)
    assert np.array_equal(base.seed, cfg['noise']['seed'] + np.arange(200))


def _resources():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    return kernel_resources.kernels()


# closed_loop_tuned_kernel<8, 6, 2, METHOD, PLANT, 2, XOUT, false, SEGMENTED, false, false, false> of the commit before the per-trial kernels: (VGPR + AGPR,
# AGPR, scratch B, LDS B) per (METHOD, XOUT, SEGMENTED), the same for PLANT 0 (DH) and 2 (axis-aligned DH); tools/kernel_resources.py on that commit
PARENT_UNIFORM = {(2, 'false', 'false'): (229, 0, 0, 18784), (2, 'true', 'false'): (231, 0, 0, 18784),
                  (3, 'false', 'true'): (487, 231, 0, 40288), (3, 'true', 'true'): (484, 228, 36, 40288),
                  (4, 'false', 'false'): (256, 0, 0, 18784), (4, 'true', 'false'): (254, 0, 0, 18784),
                  (5, 'false', 'false'): (294, 38, 0, 40288), (5, 'true', 'false'): (294, 38, 0, 40288),
                  (5, 'false', 'true'): (300, 44, 0, 40288), (5, 'true', 'true'): (298, 42, 0, 40288)}


def test_kernel_resources(uvs):
    """Every per-trial instantiation within the 512 registers of a lone wavefront (256 for the two-wavefront KF / IMCC-KF kernels), scratch no greater
    than its uniform counterpart's (0 B for KF, IMCC-KF, RMCKF; MCKF with the X stream carries its 36 B of cold slots), LDS such that as many
    workgroups share a CU as before; and the uniform kernels they were derived from are the parent's, figure for figure."""
    k = _resources()
    grid = {n: r for n, r in k.items() if n.startswith('closed_loop_grid_kernel<')}
    assert len(grid) == 20                                                   # 4 estimators x 2 plants x X stream or not, + RMCKF's segmented flavour
    for (method, xout, seg), parent in PARENT_UNIFORM.items():
        for plant in (0, 2):
            tail = f'8, 6, 2, {method}, {plant}, 2, {xout}, false, {seg}, false, false, false>'
            u, g = k['closed_loop_tuned_kernel<' + tail], grid['closed_loop_grid_kernel<' + tail]
            assert (u['vgpr'], u['agpr'], u['scratch'], u['lds']) == parent, (tail, u)
            assert g['vgpr'] <= (256 if method in (2, 4) else 512), (tail, g)
            assert g['scratch'] <= u['scratch'] and (method == 3 or g['scratch'] == 0), (tail, g)
            per_cu = lambda lds: 163840 // lds                              # noqa: E731
            assert min(per_cu(g['lds']), 8 if method in (2, 4) else 4) == min(per_cu(u['lds']), 8 if method in (2, 4) else 4), (tail, g)
    careful = k['closed_loop_grid_generic_kernel<8, 6, 4, 0, true>']
    assert careful['vgpr'] <= 512 and careful['scratch'] <= k['closed_loop_kernel<8, 6, 4, 0, true>']['scratch']
