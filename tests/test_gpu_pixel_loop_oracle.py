"""The pixel closed loops -- engine.camera_closed_loop, stepwise (fused=False: uvs_camera_features*_f64, uvs_hold_features_f64 and
uvs_rmckf_step_f64 under the Python glue) and as one launch (fused=True: the five flavours of the loop kernel) -- against
oracle/pixel_loop.py, the loop of include/uvs_vision.h restated on the CPU from parts that are each held to the reference: numpy projection,
numpy rasteriser, the host detector, numpy hold rule, BlockFilter, numpy pinv.  Nothing of the GPU code is on the oracle's side.

The one launch is written to have the bits of the stepwise loop, and the bit-for-bit suites hold it to that; what the glue decides -- the k
of the annealed bandwidth, which row is f_old, which command is the regressor, the noise of a held pair, f0 behind an occluder -- they
reproduce by construction.  Here every estimator, shape and scenario of tests/pixel_loop_common.py runs on both routes and every output
trial is compared with the oracle run on its own inputs; tests/test_pixel_loop_oracle.py (CPU) holds the oracle to
rmckf_block.run_closed_loop, every trial to the preconditions under which a 1e-10 px difference cannot flip a pixel, and every misreading
of the loop's text to at least 100 gates of distance in q or dq.

Batches are tiled from the E <= 8 distinct trials of a case, output trial t taking the inputs of trial t % E: T = E (one trial per
workgroup) and T = 259 (four per workgroup, the last one with a padding wavefront).  Gates: status, k_done, pixels and held exact; err, q, f
and stats 1e-8 relative per trial (gpu_harness.TOL); dq 1e-7 (gpu_harness.STEP_GATES); kappa 1e-8.  camera_closed_loop allocates its own
outputs; test_the_entry_points_into_poisoned_buffers calls the C entry points, where the caller owns them, into NaN and -7.  The worst
deviation per route and quantity is printed when the module finishes (pytest -s; profiles/pixel_loop_oracle.txt)."""
import numpy as np
import pytest

import gpu_harness as gh
import pixel_loop_common as pl

pytestmark = pytest.mark.gpu

WORST = gh.Worst()
BATCHES = ('E', 259)
GATES = {'err': pl.GATE, 'q': pl.GATE, 'f': pl.GATE, 'dq': pl.GATE_DQ, 'kappa': pl.GATE_KAPPA}


@pytest.fixture(scope='module')
def uvs():
    import os
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    uvs_amd.lib()
    uvs_amd._vision.lib()
    yield uvs_amd
    WORST.report('pixel loops against oracle/pixel_loop')


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def routes_of(c):
    if c.grid:
        return (True,)                                               # the two-launch step has no per-trial flavour
    if c.method == 'MCKF' and c.n_points == 3:
        return (False,)                                              # the one launch refuses MCKF at (6,6) (UVS_ERR_METHOD)
    return (False, True)


def launch(uvs, c, T, fused):
    """One camera_closed_loop call of T output trials tiled from the case's trials; numpy arrays, logs as (K, T, comp)."""
    import torch
    E, m = len(c.trials), 2 * c.n_points
    idx = np.arange(T) % E
    first = c.trials[0]
    fp = uvs.engine.make_params(m, 6, c.method, first.kernel_bw, c.annealing, pl.DT, pl.DT * (c.K + 0.5), first.gain, first.desired, c.initial_guess,
                                0, c.K, first.fpi_threshold, pl.FPI_EPOCH_MAX)
    assert fp.steps == c.K == fp.k_max
    fp.reg, fp.anneal_span = first.reg, c.anneal_span
    if c.strict:
        fp.reserved = uvs._lib.UVS_OPT_STRICT_PINV
    q = np.array([tr.q_start for tr in c.trials])
    noise = None if c.noise_px == 0.0 else np.stack([pl.noise_of(c, i) for i in range(E)], axis=1)       # (K, E, m)
    x0 = None if c.initial_guess else np.stack([pl.given_x0(c, i) for i in range(E)])
    kw = dict(fused=fused, guess=c.guess, hold=c.hold)
    if first.occluders is not None:
        assert all(tr.occluders is not None and len(tr.occluders) == len(first.occluders) for tr in c.trials)
        kw['occluders'] = np.array([c.trials[i].occluders for i in idx], np.int64)
        if first.paints is not None:
            kw['occluder_colours'] = np.array([c.trials[i].paints for i in idx], np.int64)
    if c.grid:                                                       # n_in = 2 input trials, read through source; the rest per output trial
        n_in = 2
        for i, tr in enumerate(c.trials):
            assert tr.q_start == c.trials[i % n_in].q_start and tr.seed == c.trials[i % n_in].seed
        tp = {'source': dev(idx % n_in, np.int32)}
        for key in ('kernel_bw', 'gain', 'reg', 'fpi_threshold'):
            if len({getattr(tr, key) for tr in c.trials}) > 1:
                tp[key] = dev([getattr(c.trials[i], key) for i in idx])
        if len({tr.desired for tr in c.trials}) > 1:
            tp['desired'] = dev([c.trials[i].desired for i in idx])
        assert len(tp) > 1
        kw['trial_params'] = tp
        q_in, noise_in, x0_in = q[:n_in], None if noise is None else noise[:, :n_in], None if x0 is None else x0[:n_in]
    else:
        assert len({(tr.kernel_bw, tr.gain, tr.reg, tr.fpi_threshold, tr.desired) for tr in c.trials}) == 1
        q_in, noise_in, x0_in = q[idx], None if noise is None else noise[:, idx], None if x0 is None else x0[idx]
    out = uvs.engine.camera_closed_loop(fp, pl.plant_of(c.n_points), dev(q_in), None if noise_in is None else dev(noise_in), x0=x0_in, **kw)
    torch.cuda.synchronize()
    assert ('held' in out) == (c.hold > 0)
    return {key: value.cpu().numpy() for key, value in out.items()}


def compare(c, out, T, route):
    """Every output trial against the oracle's run of trial t % E."""
    E, K = len(c.trials), c.K
    assert out['status'].shape == (T,) and out['k_done'].shape == (T,) and out['stats'].shape == (T, 3) and out['pixels'].shape == (T, c.n_points)
    for e in range(E):
        ref = pl.oracle_trial(c.name, e)
        sel = np.arange(e, T, E)
        tag = (c.name, route, T, e)
        k = ref['k_done']
        assert out['status'][sel].tolist() == [ref['status']] * len(sel), tag + ('status', out['status'][sel].tolist())
        assert out['k_done'][sel].tolist() == [k] * len(sel), tag + ('k_done', out['k_done'][sel].tolist(), k)
        assert np.array_equal(out['pixels'][sel], np.broadcast_to(ref['pixels'], (len(sel), c.n_points))), tag + ('pixels', out['pixels'][sel[0]], ref['pixels'])
        if c.hold:
            held = np.array([len(h) for h in ref['held']])
            assert np.array_equal(out['held'][sel], np.broadcast_to(held, (len(sel), c.n_points))), tag + ('held', out['held'][sel[0]], held)
        failures = []
        for key, gate in GATES.items():
            rows = min(K, k + 1) if key in ('q', 'f') else k
            if rows == 0:
                continue
            got, want = out[key][:rows, sel], ref[key][:rows, None]  # (rows, trials, comp) against (rows, 1, comp)
            assert got.shape[2] == want.shape[2] and len(ref[key]) == rows, tag + (key, 'rows')
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape)), tag + (key, 'the NaN pairs of empty masks')
            d = float(np.abs(np.where(nan, 0.0, got - want)).max() / np.abs(want[~nan]).max())
            WORST.note(route, key, d)
            if d > gate:
                failures.append((key, d))
        if k:
            d = float((np.abs(out['stats'][sel] - ref['stats']).max(axis=1) / np.abs(ref['stats']).max()).max())
            WORST.note(route, 'stats', d)
            if d > pl.GATE:
                failures.append(('stats', d))
        assert not failures, tag + tuple(failures)


@pytest.mark.parametrize('T', BATCHES)
@pytest.mark.parametrize('name', list(pl.CASES))
def test_against_the_oracle(uvs, name, T):
    c = pl.CASES[name]
    T = len(c.trials) if T == 'E' else T
    for fused in routes_of(c):
        route = f'{"one launch" if fused else "stepwise"}, {c.method}'
        compare(c, launch(uvs, c, T, fused), T, route)


POISONED = ['a_GMCKF_86_anneal', 'a_KF_66_plain', 'a_IMCCKF_26_anneal', 'a_MCKF_86_plain', 'c_GMCKF_86_leaves_hold0', 'c_GMCKF_86_wide_shorter',
            'c_IMCCKF_66_wide_equal']


@pytest.mark.parametrize('T', BATCHES)
@pytest.mark.parametrize('name', POISONED)
def test_the_entry_points_into_poisoned_buffers(uvs, name, T):
    """The C entry points, where the caller owns the outputs: uvs_camera_closed_loop_f64 -- uvs_camera_closed_loop_held_f64 for a case with
    occluders or a hold -- into buffers filled with NaN (-7 for the integers), from the ORACLE's f0 and x0.  Every live row is held to the
    oracle as above; every row the header says is not written -- q, f after k_done, dq, err, kappa from k_done on -- keeps its NaN."""
    import ctypes as C
    import torch
    c = pl.CASES[name]
    E, m, K, npts = len(c.trials), 2 * c.n_points, c.K, c.n_points
    T = E if T == 'E' else T
    idx = np.arange(T) % E
    first = c.trials[0]
    assert first.paints is None and not c.grid
    fp = uvs.engine.make_params(m, 6, c.method, first.kernel_bw, c.annealing, pl.DT, pl.DT * (K + 0.5), first.gain, first.desired, c.initial_guess,
                                0, K, first.fpi_threshold, pl.FPI_EPOCH_MAX)
    fp.reg, fp.anneal_span = first.reg, c.anneal_span
    cam = pl.plant_of(npts).to_camera()
    refs = [pl.oracle_trial(name, e) for e in range(E)]
    q0 = dev(np.array([c.trials[i].q_start for i in idx]))
    noise = None if c.noise_px == 0.0 else dev(np.stack([pl.noise_of(c, i) for i in range(E)], axis=1)[:, idx])
    x0, f0 = dev(np.stack([refs[i]['x0'] for i in idx])), dev(np.stack([refs[i]['f0'] for i in idx]))
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')              # noqa: E731
    ints = lambda *shape: torch.full(shape, gh.POISON_INT, dtype=torch.int32, device='cuda')              # noqa: E731
    buf = dict(q=nan(K, T, 6), f=nan(K, T, m), dq=nan(K, T, 6), err=nan(K, T, m), kappa=nan(K, T, m), status=ints(T), k_done=ints(T),
               stats=nan(T, 3), pixels=ints(T, npts))
    operands = [q0.data_ptr(), None if noise is None else noise.data_ptr(), x0.data_ptr(), f0.data_ptr()] + \
               [buf[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if first.occluders is None and not c.hold:
        rc = uvs._vision.lib().uvs_camera_closed_loop_f64(C.byref(fp), C.byref(cam), T, *operands, stream)
    else:
        occ = None if first.occluders is None else dev(np.array([c.trials[i].occluders for i in idx]), np.int32)
        assert occ is None or tuple(occ.shape) == (T, len(first.occluders), 8)
        buf['held'] = ints(T, npts)
        rc = uvs._vision.lib().uvs_camera_closed_loop_held_f64(C.byref(fp), C.byref(cam), T, None, None if occ is None else occ.data_ptr(),
                                                               0 if occ is None else occ.shape[1], c.hold, *operands, buf['held'].data_ptr(), stream)
    uvs._vision.check(rc)
    torch.cuda.synchronize()
    out = {key: value.cpu().numpy() for key, value in buf.items()}
    if not c.hold:
        out.pop('held', None)
    for key in ('status', 'k_done', 'pixels', 'held'):
        assert key not in out or not (out[key] == gh.POISON_INT).any(), (name, T, key, 'not stored')
    compare(c, out, T, f'entry point, {c.method}')
    for t in range(T):
        k = refs[t % E]['k_done']
        for key in ('q', 'f', 'dq', 'err', 'kappa'):
            rows = min(K, k + 1) if key in ('q', 'f') else k
            assert np.all(np.isnan(out[key][rows:, t])), (name, T, t, key, 'a row past k_done was written')
    assert any(r['k_done'] < K for r in refs) == (name in ('c_GMCKF_86_leaves_hold0', 'c_GMCKF_86_wide_shorter'))


def test_the_one_launch_refuses_mckf_at_66(uvs):
    """Why routes_of leaves that route out: the refusal of include/uvs_vision.h, not a quiet other path."""
    c = pl.CASES['a_MCKF_66_plain']
    with pytest.raises(uvs.UvsError) as refusal:
        launch(uvs, c, len(c.trials), True)
    assert refusal.value.code == -4
