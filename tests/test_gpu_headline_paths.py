"""The rare paths of the headline kernel -- closed_loop_tuned_kernel<8, 6, 2, GMCKF>, whole trials and its SEGMENTED instantiation (same source) --
at the smallest batch that has them all: 33 trials (one full wavefront and one holding a single trial), 19 steps (dt 0.05, t_max 1.0: past the
16-step re-seed of the sine / cosine pairs).  Two lanes per filter are forced (a batch this small would otherwise run on the four-lane kernels)
and uvs_rmckf_closed_loop_segments says which instantiation a launch takes.  Everything is compared bit for bit unless a test says otherwise:
the step loop's control flow may be rearranged, its results may not move."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

T, DT, T_MAX, K = 33, 0.05, 1.0, 19
STREAMS = ('x', 'err', 'q', 'f', 'dq')
PER_TRIAL = ('stats', 'status', 'k_done')
STRICT = 1                                                        # UVS_OPT_STRICT_PINV
FAIL = 1
TOL_FIXTURE = 1e-8                                                # tests/test_gpu_parity.py::test_closed_loop_matches_reference
SEGMENTS = pytest.mark.parametrize('segments', [1, 2], ids=['whole', 'segmented'])
_CLEAN = {}


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    uvs_amd.lib()
    return uvs_amd


@pytest.fixture(scope='module')
def case():
    g = load_golden('closed_gmckf_a1p5')
    rng = np.random.default_rng(33)
    q0 = np.tile(g['q_start'], (T, 1))
    q0[:, :3] += rng.uniform(-0.2, 0.1, (T, 3))
    noise = rng.standard_t(3, size=(K, 8, T))
    noise.setflags(write=False)
    q0.setflags(write=False)
    return dict(desired=g['desired'], q0=q0, noise=noise)


def _cuda(a):
    import torch
    return torch.as_tensor(np.array(a, order='C'), device='cuda')


def run(uvs, case, segments, q0=None, noise=None, want=STREAMS, reserved=0, x0=None, params=None, desired=None, t_max=T_MAX):
    """One launch of K steps of the two-lane RMCKF kernel as `segments` work items per chunk; numpy arrays, streams [step][component][trial]."""
    import torch
    assert len(uvs.engine.loop_clock(DT, T_MAX)) == K
    q0 = case['q0'] if q0 is None else q0
    noise = case['noise'] if noise is None else noise
    bw, anneal, gain = params or (10.0, False, 0.2)
    fp = uvs.engine.make_params(8, 6, 'GMCKF', bw, anneal, DT, t_max, gain, case['desired'] if desired is None else desired, x0 is None, 2, K)
    fp.reserved = reserved | (segments << 8)
    plant = uvs.SyntheticPlant.ur10().to_struct()
    n = len(q0)
    assert int(uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp), C.byref(plant), n)) == 2
    # (a strict launch is never cut: the plan keeps certified trials whole, so its results are held against the default launch's at either cut)
    assert int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(fp), C.byref(plant), n)) == (1 if reserved & STRICT else segments)
    out = uvs.engine.closed_loop(fp, plant, _cuda(q0), _cuda(noise), None if x0 is None else _cuda(x0), want=want)
    torch.cuda.synchronize()
    assert not uvs.engine.hand_over_fallbacks(fp, plant, n)             # (None for an uncut launch)
    return {k: out[k].cpu().numpy() for k in STREAMS + PER_TRIAL if out.get(k) is not None}


def clean(uvs, case, segments):
    if segments not in _CLEAN:
        _CLEAN[segments] = run(uvs, case, segments)
        assert not _CLEAN[segments]['status'].any() and (_CLEAN[segments]['k_done'] == K).all()
    return _CLEAN[segments]


def live(out, key, trials):
    """The stream's columns `trials` with the rows at and after k_done (unspecified) zeroed."""
    a = out[key][:, :, trials]
    return np.where(np.arange(a.shape[0])[:, None, None] < out['k_done'][trials][None, None, :], a, 0.0)


def assert_same_bits(a, ta, b, tb, tag, keys=STREAMS):
    """Trials `ta` of launch `a` carry the bits of trials `tb` of launch `b`: status, k_done, every stream of `keys` up to k_done, statistics of the successes."""
    ta, tb = np.asarray(ta), np.asarray(tb)
    assert np.array_equal(a['status'][ta], b['status'][tb]) and np.array_equal(a['k_done'][ta], b['k_done'][tb]), tag
    for key in keys:
        assert live(a, key, ta).tobytes() == live(b, key, tb).tobytes(), (key,) + tuple(tag)
    ok = b['status'][tb] == 0
    assert a['stats'][ta][ok].tobytes() == b['stats'][tb][ok].tobytes(), ('stats',) + tuple(tag)


@SEGMENTS
def test_partition_invariance(uvs, case, segments):
    """33 trials in one launch against the same trials as launches of 32 and of 1."""
    whole = clean(uvs, case, segments)
    for lo, hi in ((0, 32), (32, 33)):
        part = run(uvs, case, segments, case['q0'][lo:hi], case['noise'][:, :, lo:hi])
        assert_same_bits(whole, np.arange(lo, hi), part, np.arange(hi - lo), ('partition', lo, hi, segments))


@SEGMENTS
@pytest.mark.parametrize('failing', [(7,), tuple(range(32)), (32,)], ids=['one trial', 'all of wavefront 0', 'all of wavefront 1'])
def test_fail_among_live_neighbours(uvs, case, segments, failing):
    """An infinite noise sample at step 5 (as in tests/golden/analytical_inf_at_40.npz): the trial FAILs with k_done 5, every other trial comes out as
    without the injection -- also when a whole wavefront FAILs at once and leaves its step loop while the other one runs on."""
    noise = case['noise'].copy()
    noise[5, 3, list(failing)] = np.inf
    out = run(uvs, case, segments, noise=noise)
    failing = np.asarray(failing)
    assert (out['status'][failing] == FAIL).all() and (out['k_done'][failing] == 5).all()
    others = np.setdiff1d(np.arange(T), failing)
    ref = clean(uvs, case, segments)
    assert_same_bits(out, others, ref, others, ('fail', len(failing), segments))
    assert_same_bits(out, failing, dict(ref, status=out['status'], k_done=out['k_done'], stats=out['stats']), failing, ('before the fail', segments))


@SEGMENTS
def test_per_lane_reseed_after_an_outlier(uvs, case, segments):
    """One trial sees a 50-pixel outlier: its neighbours are unchanged, the trial itself follows oracle/c within the closed-loop fixture gate."""
    from oracle import c_oracle
    t, noise = 9, case['noise'].copy()
    noise[4, 2, t] += 50.0
    out = run(uvs, case, segments, noise=noise)
    others = np.setdiff1d(np.arange(T), [t])
    assert_same_bits(out, others, clean(uvs, case, segments), others, ('outlier', segments))
    ref = c_oracle.closed_loop_batch(case['q0'][t:t + 1], noise.transpose(2, 0, 1)[t:t + 1], case['desired'], dt=DT, t_max=T_MAX, steps=K, want_x=True)
    assert out['status'][t] == ref['status'][0] == 0 and out['k_done'][t] == ref['k_done'][0] == K
    for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
        d = rel_err(out[key][:, :, t], ref[rk][0])
        print(f'outlier trial against oracle/c, {key}: {d:.2e}')
        assert d <= TOL_FIXTURE, (key, d, segments)
    assert rel_err(out['stats'][t], ref['stats'][0]) <= TOL_FIXTURE


@SEGMENTS
@pytest.mark.parametrize('want', [(), ('x',), ('err', 'q'), STREAMS], ids=['none', 'x', 'err+q', 'all'])
def test_stream_subsets(uvs, case, segments, want):
    """Whatever subset of the streams a launch logs, each logged stream -- and every per-trial result -- equals the all-streams launch."""
    out = run(uvs, case, segments, want=want)
    assert set(k for k in STREAMS if k in out) == set(want)
    assert_same_bits(out, np.arange(T), clean(uvs, case, segments), np.arange(T), ('subset', want, segments), keys=want)


@SEGMENTS
def test_strict_pinv_on_healthy_trials(uvs, case, segments):
    """UVS_OPT_STRICT_PINV certifies every solve of a healthy trial: the default launch's bits."""
    out = run(uvs, case, segments, reserved=STRICT)
    assert_same_bits(out, np.arange(T), clean(uvs, case, segments), np.arange(T), ('strict', segments))


@SEGMENTS
@pytest.mark.parametrize('strict', [False, True], ids=['default', 'strict'])
def test_kahan_like_start_is_marked(uvs, case, segments, strict):
    """A Kahan-like X0 (tests/golden/rankdef_gmckf_kahan_c1000.npz): the growth watch (default) resp. the certificate (strict) marks the trial, the careful
    pass returns the reference's truncated command -- the plain least-squares one is hundreds of times larger -- and no internal status leaks out
    (gate: tests/test_gpu_rankdef.py::test_closed_loop_on_the_kahan_fixture)."""
    g = load_golden('rankdef_gmckf_kahan_c1000')
    meta, p = g['meta'], g['meta']['params']
    assert meta['dt'] == DT and len(g['t']) >= K
    out = run(uvs, case, segments, np.tile(g['q_start'], (T, 1)), np.repeat(g['noise'][:K, :, None], T, axis=2), reserved=STRICT if strict else 0,
              x0=np.tile(g['X'][0], (T, 1)), params=(p['kernel_bw'], p['annealing'], meta['gain']), desired=g['desired'], t_max=meta['t_max'])   # its first K steps
    assert not out['status'].any() and (out['k_done'] == K).all()
    steps = [int(k) for k in g['X_steps'] if k < K]
    for t in (0, 31, 32):
        assert rel_err(out['err'][:, :, t], g['err'][:K]) <= 1e-7 and rel_err(out['q'][:, :, t], g['q'][:K]) <= 1e-7
        assert rel_err(out['x'][steps, :, t], g['X'][:len(steps)]) <= 1e-7
        assert rel_err(out['dq'][:K - 1, :, t], g['dq_prev'][1:K]) <= 1e-6
