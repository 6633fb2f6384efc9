"""Per-trial estimator parameters on the GPU (uvs_rmckf_closed_loop_grid_f64): a hyperparameter grid in ONE launch must be, trial for trial, the
BITS of the uniform launches it replaces -- the kernels form every value with the same operations in the same order, and a trial's results do not
depend on its neighbours in the batch.  Every comparison here is np.array_equal unless it says otherwise; the oracle test is the one that does not
lean on the uniform kernels."""
import ctypes as C
import json

import numpy as np
import pytest

import gpu_harness as gh
from conftest import load_golden, scene_desired, rel_err
from gpu_harness import STREAMS
from sweep_common import STATS_TOL

pytestmark = pytest.mark.gpu
METHODS = ('GMCKF', 'MCKF', 'KF', 'IMCCKF')
BWS, GAINS = (2.0, 5.0, 10.0, 20.0), (0.1, 0.2, 0.4)


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    return uvs_amd


def _grid_vs_uniform(uvs, method, lanes, annealing=False, segments=0, desired_pair=None, E=100, bws=BWS, gains=GAINS, want=STREAMS):
    import torch
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E, annealing)
    cells = [(b, g) for b in bws for g in gains]
    H = len(cells)
    tp = dict(kernel_bw=gh.cuda(np.repeat([c[0] for c in cells], E)), gain=gh.cuda(np.repeat([c[1] for c in cells], E)),
              source=gh.cuda((np.arange(H * E) % E).astype(np.int32)))
    des_of = None
    if desired_pair is not None:                                                    # two targets inside the same scene, alternating from trial to trial
        des_of = np.stack([desired_pair[(t + t // E) % 2] for t in range(H * E)])
        tp['desired'] = gh.cuda(des_of)
    fp_grid = fp(lanes, segments=segments)
    out = uvs.engine.closed_loop(fp_grid, plant, q0, noise, want=want, trial_params=tp)
    torch.cuda.synchronize()
    if segments:
        assert int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(fp_grid), C.byref(plant), H * E)) == segments
        assert uvs.engine.hand_over_fallbacks(fp_grid, plant, H * E) == 0
    got = gh.host(out, want)
    assert got['status'].shape == (H * E,)
    for h, (b, g) in enumerate(cells):
        if des_of is None:
            ref = uvs.engine.closed_loop(fp(lanes, b, g, segments=segments), plant, q0, noise, want=want)
            gh.assert_same_bits(got, h * E, gh.host(ref, want), (method, lanes, b, g))
        else:                                                                       # a uniform launch per target, over the trials that have it
            for which in (0, 1):
                sel = np.nonzero((np.arange(E) + h) % 2 == which)[0]
                ref = gh.host(uvs.engine.closed_loop(fp(lanes, b, g, desired_pair[which], segments=segments), plant, q0[sel], noise[:, :, sel].contiguous(), want=want), want)
                sub = {k: (v[h * E + sel] if k in ('stats', 'status', 'k_done') else v[:, :, h * E + sel]) for k, v in got.items()}
                gh.assert_same_bits(sub, 0, ref, (method, lanes, b, g, which))
    return got


@pytest.mark.parametrize('lanes', (2, 0))
@pytest.mark.parametrize('method', METHODS)
def test_grid_launch_has_the_bits_of_twelve_uniform_launches(uvs, method, lanes):
    """kernel_bw {2, 5, 10, 20} x gain {0.1, 0.2, 0.4}, 100 trials per cell (wavefronts of 32 trials mix cells), alpha = 1.5; chaotic cells included:
    identical arithmetic needs no calm trials.  lanes 0: whatever route the plan picks on each side (the uniform launches of 100 trials: the four-lane
    small-batch kernels, which carry the two-lane bits)."""
    got = _grid_vs_uniform(uvs, method, lanes)
    assert len(got['status']) == 1200


@pytest.mark.parametrize('method', METHODS)
def test_grid_launch_with_annealing(uvs, method):
    _grid_vs_uniform(uvs, method, 2, annealing=True, want=('x', 'err', 'q'))


@pytest.mark.parametrize('method', METHODS)
def test_grid_launch_with_per_trial_targets(uvs, method):
    g = load_golden('closed_gmckf_target_shift')
    cfg = gh.config(method)
    assert np.array_equal(scene_desired(g), cfg['experiments']['desired_f'])       # the fixture's scene is the reference config's
    _grid_vs_uniform(uvs, method, 2, desired_pair=(np.asarray(cfg['experiments']['desired_f'], float), g['desired']), bws=(5.0, 20.0), gains=(0.1, 0.4),
                     want=('x', 'err', 'q'))


@pytest.mark.parametrize('method,segments', [('MCKF', 4), ('MCKF', 8), ('GMCKF', 4)])
def test_grid_launch_in_segments(uvs, method, segments):
    """A forced segment count (bits 8-15): the state crosses through the workspace, the per-trial values are read again by every segment."""
    _grid_vs_uniform(uvs, method, 2, segments=segments, want=('x', 'err', 'q'))


@pytest.mark.parametrize('method', ('GMCKF', 'MCKF'))
def test_grid_launch_at_full_size(uvs, method):
    """65 536 trials -- 512 grid cells x 128 trials -- in one launch (two rounds of wavefronts; MCKF in the plan's segments) against the uniform launch of
    a sample of cells."""
    import torch
    E, H = 128, 512
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    bw = np.linspace(2.0, 33.0, 32)
    gain = np.linspace(0.05, 0.425, 16)
    cells = [(b, g) for b in bw for g in gain]
    tp = dict(kernel_bw=gh.cuda(np.repeat([c[0] for c in cells], E)), gain=gh.cuda(np.repeat([c[1] for c in cells], E)),
              source=gh.cuda((np.arange(H * E) % E).astype(np.int32)))
    want = ('err', 'q')
    got = gh.host(uvs.engine.closed_loop(fp(0), plant, q0, noise, want=want, trial_params=tp), want)
    torch.cuda.synchronize()
    if method == 'MCKF':
        f = fp(0)
        assert int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(f), C.byref(plant), H * E)) > 1 and uvs.engine.hand_over_fallbacks(f, plant, H * E) == 0
    for h in (0, 1, 15, 16, 100, 255, 256, 300, 495, 511):
        ref = gh.host(uvs.engine.closed_loop(fp(2, *cells[h]), plant, q0, noise, want=want), want)
        gh.assert_same_bits(got, h * E, ref, (method, h, cells[h]))


@pytest.mark.parametrize('lanes', (0, 2))
@pytest.mark.parametrize('method', METHODS)
def test_null_trial_params_equal_the_uniform_call(uvs, method, lanes):
    """A uvs_trial_params whose members are all NULL runs, and equals uvs_rmckf_closed_loop_ws_f64 bit for bit."""
    E = 100
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    got = gh.host(uvs.engine.closed_loop(fp(lanes), plant, q0, noise, want=STREAMS, trial_params={}))
    ref = gh.host(uvs.engine.closed_loop(fp(lanes), plant, q0, noise, want=STREAMS))
    gh.assert_same_bits(got, 0, ref, (method, lanes))
    final = uvs.engine.closed_loop(fp(lanes), plant, q0, noise, want=(), final_state=True, trial_params={'gain': None})
    final_ref = uvs.engine.closed_loop(fp(lanes), plant, q0, noise, want=(), final_state=True)
    ok = ref['status'] == 0
    for key in ('x_final', 'p_final'):
        assert np.array_equal(final[key].cpu().numpy()[ok], final_ref[key].cpu().numpy()[ok]), key


def test_careful_pass_reads_the_per_trial_values(uvs):
    """The Kahan fixture's start state (every trial marked at its first solve, so the careful pass computes everything) with three per-trial gains:
    equal to three uniform launches, status included; the fixture's own gain follows the fixture."""
    g = load_golden('rankdef_gmckf_kahan_c1000')
    meta, p = g['meta'], g['meta']['params']
    gains = (0.1, meta['gain'], 0.4)
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    mk = lambda gain: uvs.engine.make_params(8, 6, meta['method'], p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], gain, g['desired'], False)   # noqa: E731
    T = 3
    q0, noise, x0 = gh.cuda(np.tile(g['q_start'], (T, 1))), gh.cuda(np.repeat(g['noise'][:, :, None], T, axis=2)), gh.cuda(np.tile(g['X'][0], (T, 1)))
    want = ('x', 'err', 'q', 'dq')
    got = gh.host(uvs.engine.closed_loop(mk(0.3), plant, q0, noise, x0, want=want, trial_params={'gain': gh.cuda(np.asarray(gains))}), want)
    assert got['status'].tolist() == [0, 0, 0]
    for i, gain in enumerate(gains):
        ref = gh.host(uvs.engine.closed_loop(mk(gain), plant, q0, noise, x0, want=want), want)
        sub = {k: (v[[i] * T] if k in ('stats', 'status', 'k_done') else v[:, :, [i] * T]) for k, v in got.items()}
        gh.assert_same_bits(sub, 0, ref, gain)
    K = len(g['t'])
    assert rel_err(got['err'][:, :, 1], g['err']) <= 1e-7 and rel_err(got['q'][:, :, 1], g['q']) <= 1e-7 and rel_err(got['x'][g['X_steps'], :, 1], g['X']) <= 1e-7
    assert rel_err(got['dq'][:K - 1, :, 1], g['dq_prev'][1:]) <= 1e-6
    # ... and the other gains do not (the test has teeth): the command is proportional to the gain, so half the gain is about half the command
    assert rel_err(got['dq'][:K - 1, :, 0], g['dq_prev'][1:]) > 0.1


def test_careful_pass_in_a_mixed_grid(uvs):
    """Healthy and rank-deficient start states in one grid launch (as test_gpu_rankdef.py::test_second_pass_leaves_healthy_trials_alone), two gains, the
    inputs read through `source`: the sick trials are redone with THEIR gain and inputs -- equal to the uniform launches, bit for bit in the wavefronts
    without a sick trial, to that test's neighbour gate (1e-11: one out-of-range angle of a sick trial's first pass switches its whole wavefront to
    the library sincos) in the others."""
    g, h = load_golden('rankdef_gmckf_rank4_product'), load_golden('closed_gmckf_a1p5')
    K, E = 120, 160
    sick = [3, 40]
    plant = uvs.SyntheticPlant.ur10(scene_desired(g)).to_struct()
    rng = np.random.default_rng(5)
    x0 = np.tile(h['X'][0], (E, 1)) * (1 + 0.02 * rng.standard_normal((E, 1)))
    noise = rng.standard_t(3, size=(K, 8, E))
    for t in sick:
        x0[t] = g['X'][0]
        noise[:, :, t] = g['noise'][:K]
    q0 = np.tile(g['q_start'], (E, 1))
    meta, p = g['meta'], g['meta']['params']
    mk = lambda gain: uvs.engine.make_params(8, 6, meta['method'], p['kernel_bw'], p['annealing'], meta['dt'], meta['t_max'], gain, g['desired'], False, 0, K)   # noqa: E731
    gains = (meta['gain'], 0.35)
    tp = dict(gain=gh.cuda(np.repeat(gains, E)), source=gh.cuda((np.arange(2 * E) % E).astype(np.int32)))
    want = ('x', 'err', 'q')
    got = gh.host(uvs.engine.closed_loop(mk(0.0), plant, gh.cuda(q0), gh.cuda(noise), gh.cuda(x0), want=want, trial_params=tp), want)
    assert not got['status'].any()
    for i, gain in enumerate(gains):
        ref = gh.host(uvs.engine.closed_loop(mk(gain), plant, gh.cuda(q0), gh.cuda(noise), gh.cuda(x0), want=want), want)
        assert not ref['status'].any() and np.array_equal(got['k_done'][i * E:(i + 1) * E], ref['k_done'])
        for key in want:
            assert rel_err(got[key][:, :, i * E:(i + 1) * E], ref[key]) <= 1e-11, (gain, key)
        assert rel_err(got['stats'][i * E:(i + 1) * E], ref['stats']) <= 1e-11
        for t in sick:                                                              # the careful pass itself: bit for bit
            for key in want:
                assert np.array_equal(got[key][:, :, i * E + t], ref[key][:, :, t]), (gain, key, t)
        far = np.arange(64, E)                                                      # wavefronts (32 trials each) without a sick trial, on both sides
        assert np.array_equal(got['err'][:, :, i * E + far], ref['err'][:, :, far])
    for t in sick:                                                                  # the fixture's gain follows the fixture
        assert rel_err(got['err'][:, :, t], g['err'][:K]) <= 1e-7 and rel_err(got['q'][:, :, t], g['q'][:K]) <= 1e-7


@pytest.mark.parametrize('method', METHODS)
def test_grid_against_the_oracle(uvs, method):
    """Independent of the uniform kernels: kernel_bw {5, 10, 20} x gain {0.1, 0.2}, alpha = 1.5, 32 trials per cell, against the plain-C oracle called per
    cell with that cell's parameters.  status and k_done exact and the statistics to STATS_TOL on every trial the oracle reproduces from a 1e-14-moved
    start (sweep_common.calm_mask's rule); at least 95 % of the trials must be such statements (on these inputs the oracle alone finds 192 of 192 calm
    for each estimator)."""
    from oracle import c_oracle
    E, bws, gains = 32, (5.0, 10.0, 20.0), (0.1, 0.2)
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    cells = [(b, g) for b in bws for g in gains]
    H = len(cells)
    tp = dict(kernel_bw=gh.cuda(np.repeat([c[0] for c in cells], E)), gain=gh.cuda(np.repeat([c[1] for c in cells], E)),
              source=gh.cuda((np.arange(H * E) % E).astype(np.int32)))
    got = gh.host(uvs.engine.closed_loop(fp(0), plant, q0, noise, want=(), trial_params=tp), ())
    host_noise = np.ascontiguousarray(noise.cpu().numpy().transpose(2, 0, 1))       # (E, K, m)
    ex, p = cfg['experiments'], cfg['estimator']['estimator_params']
    calm_total = 0
    for h, (b, g) in enumerate(cells):
        kw = dict(method=method, kernel_bw=b, annealing=p['annealing'], dt=ex['dt'], t_max=ex['t_max'], gain=g, fpi_threshold=p['fpi_threshold'],
                  fpi_epoch_max=p['fpi_epoch_max'])
        a = c_oracle.closed_loop_batch(plan.q_start, host_noise, ex['desired_f'], **kw)
        moved = c_oracle.closed_loop_batch(plan.q_start * (1.0 + 1e-14), host_noise, ex['desired_f'], **kw)
        calm = (a['status'] == moved['status']) & (a['k_done'] == moved['k_done']) & \
               (np.abs(a['stats'] - moved['stats']).max(axis=1) / np.abs(a['stats']).max(axis=1) <= 1e-9)
        sl = slice(h * E, (h + 1) * E)
        dev = np.abs(got['stats'][sl] - a['stats']).max(axis=1) / np.abs(a['stats']).max(axis=1)
        print(f'{method} kernel_bw {b} gain {g}: calm {int(calm.sum())}/{E}, max deviation on calm trials {dev[calm].max() if calm.any() else 0.0:.3e}')
        assert np.array_equal(got['status'][sl][calm], a['status'][calm]) and np.array_equal(got['k_done'][sl][calm], a['k_done'][calm]), (b, g)
        ok = calm & (a['status'] == 0)
        assert (dev[ok] <= STATS_TOL).all(), (b, g, dev[ok].max())
        calm_total += int(calm.sum())
    assert calm_total >= 0.95 * H * E, calm_total


@pytest.mark.parametrize('method', METHODS)
def test_source_equals_physical_copies(uvs, method):
    """`source` repeating E trials H times against the launch fed H physical copies of q_start / noise."""
    E, H = 100, 6
    cfg, plan, q0, noise, plant, fp = gh.setup(uvs, method, E)
    cells = [(b, g) for b in (5.0, 20.0) for g in GAINS]
    tp = dict(kernel_bw=gh.cuda(np.repeat([c[0] for c in cells], E)), gain=gh.cuda(np.repeat([c[1] for c in cells], E)))
    want = ('x', 'err', 'q')
    ref = gh.host(uvs.engine.closed_loop(fp(2), plant, q0.repeat(H, 1), noise.repeat(1, 1, H), want=want, trial_params=tp), want)
    got = gh.host(uvs.engine.closed_loop(fp(2), plant, q0, noise, want=want, trial_params=dict(tp, source=gh.cuda((np.arange(H * E) % E).astype(np.int32)))), want)
    gh.assert_same_bits(got, 0, ref, method)
    # ... and a permutation: trial t reads the inputs of trial E - 1 - t, writes at t
    rev = np.arange(E)[::-1].copy()
    flipped = gh.host(uvs.engine.closed_loop(fp(2), plant, q0, noise, want=want, trial_params={'source': gh.cuda(rev.astype(np.int32))}), want)
    plain = gh.host(uvs.engine.closed_loop(fp(2), plant, q0[gh.cuda(rev)], noise[:, :, gh.cuda(rev)].contiguous(), want=want), want)
    gh.assert_same_bits(flipped, 0, plain, (method, 'reversed'))


@pytest.mark.parametrize('method', ('GMCKF', 'MCKF'))
def test_run_grid_equals_run_sweep_per_grid_cell(uvs, method):
    cfg = gh.config(method)
    grid = {'kernel_bw': [5, 20], 'ibvs_gain': [0.1, 0.2, 0.4]}
    cells, E = [1.2, 1.5], 100
    res = uvs.batch.run_grid(cfg, grid, cells=cells, epoch=E)
    assert res.stats.shape == (2, 6, E, 3) and res.rows().shape == (2, 6, E, 5)
    for h in range(6):
        sw = uvs.batch.run_sweep(res.grid.substituted(cfg, h), cells=cells, epoch=E)
        assert np.array_equal(sw.plan.seed, res.plan.seed) and np.array_equal(sw.plan.q_start, res.plan.q_start)
        assert np.array_equal(res.rows()[:, h].reshape(2 * E, 5), sw.rows(), equal_nan=True), h
        summ = sw.cell_summary()
        for c in range(2):
            assert json.dumps(res.cell_summary()[(c, h)], sort_keys=True) == json.dumps(summ[c], sort_keys=True)
    for cap in (250, 100, 599):
        cut = uvs.batch.run_grid(cfg, grid, cells=cells, epoch=E, max_trials=cap)
        assert len(cut.grid.pieces) > 1 and np.array_equal(cut.rows(), res.rows(), equal_nan=True), cap
    third = uvs.batch.run_grid(cfg, {'fpi_threshold': [0.1, 0.01]}, cells=[1.5], epoch=E)
    if method == 'MCKF':
        sw = uvs.batch.run_sweep(third.grid.substituted(cfg, 1), cells=[1.5], epoch=E)
        assert np.array_equal(third.rows()[0, 1], sw.rows(), equal_nan=True)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize('method,segments', [('GMCKF', 0), ('MCKF', 4), ('KF', 0), ('IMCCKF', 0)])
def test_grid_entry_point_is_graph_capturable(uvs, method, segments):
    """The new entry point allocates nothing: captured on a side stream and replayed on fresh inputs (as tests/test_gpu_graph.py does for the others)."""
    import torch
    E, H = 48, 2
    T = E * H
    cfg, plan, q0, noise, plant, fp_of = gh.setup(uvs, method, E)
    K = noise.shape[0]
    fp = fp_of(2, segments=segments)
    tp = dict(kernel_bw=gh.cuda(np.repeat([5.0, 20.0], E)), gain=gh.cuda(np.repeat([0.1, 0.3], E)), source=gh.cuda((np.arange(T) % E).astype(np.int32)))
    eager = uvs.engine.closed_loop(fp, plant, q0, noise, want=('x', 'err', 'q'), trial_params=tp)
    torch.cuda.synchronize()
    q_in, nz_in = torch.empty_like(q0), torch.empty_like(noise)
    x = uvs.engine.alloc_stream(T, K, 48); err = uvs.engine.alloc_stream(T, K, 8); q = uvs.engine.alloc_stream(T, K, 6)
    stats = torch.zeros((T, 3), dtype=torch.float64, device='cuda')
    status = torch.zeros(T, dtype=torch.int32, device='cuda'); k_done = torch.zeros(T, dtype=torch.int32, device='cuda')
    sv, NV, View = uvs.engine.stream_view, uvs.engine.NULL_VIEW, uvs.engine.View
    flat = lambda t: View(t.data_ptr(), t.stride(0), 0, t.stride(1))      # noqa: E731
    tps = uvs.engine.trial_params_struct(tp, T, 8, q0.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ws, ws_bytes = uvs.engine.workspace(fp, plant, T, q0.device)       # the caller's workspace exists before the capture starts
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ws, ws_bytes = uvs.engine.workspace(fp, plant, T, q0.device)
        rc = uvs.lib().uvs_rmckf_closed_loop_grid_f64(C.byref(fp), C.byref(plant), T, C.byref(tps), flat(q_in), sv(nz_in), NV, sv(x), sv(err), sv(q), NV, NV,
                                                      stats.data_ptr(), status.data_ptr(), k_done.data_ptr(), NV, NV, ws, ws_bytes, uvs.engine._stream())
    assert rc == 0, uvs.lib().uvs_last_error()
    assert (ws_bytes > 0) == (segments > 1)
    for rep in range(2):
        q_in.copy_(q0); nz_in.copy_(noise)
        for t in (x, err, q, stats):
            t.fill_(float('nan'))
        status.fill_(7); k_done.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(status, eager['status']) and torch.equal(k_done, eager['k_done']), rep
        ok = status == 0
        assert torch.equal(_bits(stats[ok]), _bits(eager['stats'][ok]))
        for key, t in (('x', x), ('err', err), ('q', q)):
            assert torch.equal(_bits(t[:, :, ok]), _bits(eager[key][:, :, ok])), (rep, key)
