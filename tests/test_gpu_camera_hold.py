"""Holding a lost disc's last detection through the pixel loops (include/uvs_vision.h: uvs_camera_closed_loop_held_f64,
uvs_hold_features_f64).

The statement of the rule is plant.hold_features on the host.  The stepwise kernel is held to it bit for bit on rows the occluded detector
wrote; the stepwise loop (three launches a step) to the loop written out with the public pieces and the rule on the host; the one launch to
the stepwise loop -- every specified log row, stats, status, k_done, pixels (camera_common.assert_same_bits) and held.  The semantics are
asserted on the gain = 0 scenes of tests/camera_hold_common.py, whose cover schedules tests/test_camera_hold_host.py derives from host frames.
Batch sizes come on both sides of 256 trials, where the loop kernel changes from one trial per workgroup to four.  Nothing has a tolerance.

What each test catches was tried on the kernels with one-line mutations (profiles/camera_hold.txt)."""
import ctypes

import numpy as np
import pytest

import camera_common as cc
import camera_hold_common as hc
import camera_occluders_common as oc
import test_gpu_camera_grid as g
import test_gpu_camera_occluders as go

pytestmark = pytest.mark.gpu

uvs = g.uvs                                                          # the module fixture of tests/test_gpu_camera_grid.py
K, SMALL = g.K, g.SMALL
dev, bits, assert_same_bits, same, occluders_for = g.dev, cc.bits, cc.assert_same_bits, go.same, go.occluders_for
assert K == hc.K


def loop(uvs, fp, inp, fused=True, occluders=None, **kw):
    return uvs.engine.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, x0=inp.x0, fused=fused, occluders=occluders, **kw)


def assert_same_held(got, want, where, trials=None, want_trials=None):
    import torch
    assert got['held'].dtype == torch.int32 and tuple(got['held'].shape) == tuple(got['pixels'].shape), where
    trials = list(range(got['held'].shape[0])) if trials is None else trials
    want_trials = trials if want_trials is None else want_trials
    assert np.array_equal(got['held'].cpu().numpy()[trials], want['held'].cpu().numpy()[want_trials]), (where, 'held')


def still_arm(uvs, T, seed, method='GMCKF', jitter=0.0):
    """(fp with gain = 0, inputs at Q_START, the discs there): the arm never moves, so a scene's cover schedule is the CPU file's."""
    fp = g.params(uvs, method)
    fp.gain = 0.0
    q = np.tile(hc.Q_START, (T, 1))
    if jitter:
        q[1:] += np.random.default_rng(seed).uniform(-jitter, jitter, (T - 1, 6))
    return fp, g.Inputs(uvs, 4, q, seed=seed), uvs.SyntheticPlant.ur10().discs(hc.Q_START)


def cover_schedule(uvs, inp, occ, T):
    """(K, T, n_points) mask counts of the start poses behind ``occ``, step by step (the occluded detector, which the occluder tests hold to
    detect-of-render)."""
    import torch
    pix = torch.zeros((K, T, inp.m // 2), dtype=torch.int32, device='cuda')
    for k in range(K):
        uvs.engine.camera_features(inp.plant, inp.q0, occluders=occ, k=k, pixels=pix[k])
    return pix.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- 1: the stepwise kernel
@pytest.mark.parametrize('T', [3, 70])
def test_the_stepwise_kernel_is_the_rule(uvs, T):
    import torch
    _, inp, discs = still_arm(uvs, T, 41, jitter=cc.JITTER)
    held_steps = nan_rows = 0
    for name, rows in hc.scenes(discs).items():
        occ = occluders_for(T, rows)
        for hold in (0, 1, 2, K):
            miss = torch.zeros((T, 4), dtype=torch.int32, device='cuda')
            miss_h, f_prev, f_prev_h = np.zeros((T, 4), np.int32), None, None
            for k in range(K):
                pix = torch.full((T, 4), -1, dtype=torch.int32, device='cuda')
                f = uvs.engine.camera_features(inp.plant, inp.q0, noise=inp.noise[k].contiguous(), occluders=occ, k=k, pixels=pix)
                want_f, miss_h, want_held = uvs.plant.hold_features(f.cpu().numpy(), f_prev_h, pix.cpu().numpy(), miss_h, hold)
                detected = f.clone()
                held = torch.full((T, 4), -1, dtype=torch.int32, device='cuda')
                out = uvs.engine.hold_features(f, f_prev, pix, miss, hold, k, held=held)
                assert out[0] is f and out[1] is miss and out[2] is held
                assert same(f, want_f), (name, hold, k, 'f')
                assert np.array_equal(miss.cpu().numpy(), miss_h) and np.array_equal(held.cpu().numpy(), want_held), (name, hold, k)
                untouched = np.repeat(want_held == 0, 2, axis=1)
                assert np.array_equal(bits(f)[untouched], bits(detected)[untouched]), 'only held pairs are written'
                held_steps += int(want_held.sum())
                nan_rows += int(np.isnan(want_f).any(axis=1).sum())
                f_prev, f_prev_h = f, want_f
            fresh = uvs.engine.hold_features(detected.clone(), f_prev, pix, torch.zeros_like(miss), hold, K - 1)[2]
            assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (T, 4), 'held=None allocates'
    assert held_steps > 20 * T and nan_rows > 20 * T, 'the comparison would be vacuous'


# ------------------------------------------------------------------------------------------------------------- 2: the loop written out
@pytest.mark.parametrize('method', ['GMCKF', 'KF'])
def test_the_stepwise_loop_is_its_parts_and_the_rule_on_the_host(uvs, method):
    """camera_closed_loop(fused=False, hold=K) on a moving arm behind the wide bar against camera_project, render_discs(occluders=, k=),
    detect_circles, plant.hold_features on the host, FilterBank.step: every log row bit for bit, status, k_done, pixels, held, stats."""
    import torch
    T, hold = 3, K
    eng = uvs.engine
    fp = g.params(uvs, method)
    inp = g.Inputs(uvs, 4, g.jittered(T, 51), seed=52)
    occ = occluders_for(T, [hc.wide_bar()])
    out = loop(uvs, fp, inp, False, occ, hold=hold)
    torch.cuda.synchronize()

    f = eng.detect_circles(eng.render_discs(eng.camera_project(inp.plant, inp.q0), occluders=occ, k=0))
    bank = eng.FilterBank(fp, T, inp.x0.cpu().numpy())
    names = ('q', 'f', 'dq', 'err', 'kappa', 'status', 'pixels', 'held')
    want = {key: [] for key in names}
    q, dq = inp.q0, torch.zeros((T, 6), dtype=torch.float64, device='cuda')
    miss, reported = np.zeros((T, 4), np.int32), None
    for k in range(K):
        q_new = torch.empty_like(q)
        discs = eng.camera_project(inp.plant, q, dq if k else None, g.DT, q_out=q_new)
        pixels = torch.zeros((T, 4), dtype=torch.int32, device='cuda')
        detected = eng.detect_circles(eng.render_discs(discs, occluders=occ, k=k), noise=inp.noise[k].contiguous(), pixels=pixels)
        reported, miss, held = uvs.plant.hold_features(detected.cpu().numpy(), reported, pixels.cpu().numpy(), miss, hold)
        f_new = dev(reported)
        step = bank.step(f_new, f, dq, k)
        q, f, dq = q_new, f_new, step[0].clone()
        for key, value in zip(names, (q, f, dq, step[1], step[2], step[3], pixels, dev(held))):
            want[key].append(value.clone())
    want = {key: torch.stack(rows) for key, rows in want.items()}
    assert int(want['status'].sum()) == 0 and bool(torch.isfinite(want['err']).all()), 'the comparison would be vacuous: a trial FAILs'
    assert int(want['held'].sum()) >= 2 * T and int(want['pixels'].amin(0).min()) == 0, 'the comparison would be vacuous: nothing is held'
    for key in cc.LOGS:
        assert np.array_equal(bits(out[key]), bits(want[key])), key
    assert out['k_done'].tolist() == [K] * T and out['status'].tolist() == [0] * T
    assert torch.equal(out['pixels'], want['pixels'].amin(0)) and torch.equal(out['held'], want['held'].sum(0, dtype=torch.int32))
    stats = eng.stats_reduce(want['err'].permute(1, 0, 2).contiguous(), eng.loop_clock(g.DT, g.DT * (K + 0.5)), out['k_done'], layout='tkc')
    assert np.array_equal(bits(out['stats']), bits(stats))


# ------------------------------------------------------------------------------------------------------------- 3: one launch
def held_runs(out, t, j):
    """The runs of held steps of disc j of trial t, read off the f log: [(first, length)] -- a held pair has the bits of the row before it
    (a detected one never does: its noise is new).  Rows after k_done are not looked at."""
    f = bits(out['f'])[:, t, 2 * j:2 * j + 2]
    last = min(K - 1, int(out['k_done'][t]))
    return hc.runs([1] + [0 if np.array_equal(f[k], f[k - 1]) else 1 for k in range(1, last + 1)])


SCENARIOS = ('long', 'exact', 'short', 'two', 'leaves')


@pytest.mark.parametrize('scenario', SCENARIOS)
@pytest.mark.parametrize('T', [3, SMALL + 3])
@pytest.mark.parametrize('method,n_points', g.CASES)
def test_one_launch_has_the_bits_of_the_stepwise_loop(uvs, method, n_points, T, scenario):
    import torch
    fp = g.params(uvs, method, 2 * n_points)
    q_host = g.jittered(T, 61)
    occ, hold = occluders_for(T, [hc.wide_bar()]), K
    if scenario == 'two':
        occ = occluders_for(T, [hc.wide_bar(), hc.counter_bar()])
    if scenario == 'leaves':
        occ = None
        q_host[T // 2] = g.Q_LEAVES
    inp = g.Inputs(uvs, n_points, q_host, seed=300 + n_points)
    if scenario == 'leaves':
        inp.noise[:, T // 2] = 0.0                                   # Q_LEAVES was found without noise
    if scenario in ('exact', 'short'):                               # the longest cover of the batch, read off the launch that holds them all
        long = loop(uvs, fp, inp, True, occ, hold=K)
        every = [(t, first, n) for t in range(T) for j in range(n_points) for first, n in held_runs(long, t, j)]
        longest = max(n for _, _, n in every)
        assert longest >= 2, 'the comparison would be vacuous: no cover of two steps'
        hold = longest if scenario == 'exact' else longest - 1
    fused, stepwise = loop(uvs, fp, inp, True, occ, hold=hold), loop(uvs, fp, inp, False, occ, hold=hold)
    torch.cuda.synchronize()
    where = (method, n_points, T, scenario)
    assert_same_bits(fused, stepwise, K, where)
    assert_same_held(fused, stepwise, where)
    held, k_done = fused['held'].cpu().numpy(), fused['k_done'].cpu().numpy()
    if scenario == 'exact':                                          # a hold of exactly the longest cover is as good as any longer one
        assert_same_bits(fused, long, K, where + ('hold = K',))
        assert_same_held(fused, long, where)
    if scenario == 'short':                                          # FAIL where the rule says: at the first run's step `hold`, or where hold = K FAILed
        want = long['k_done'].cpu().numpy().copy()
        for t, first, n in every:
            if n > hold:
                want[t] = min(want[t], first + hold)
        assert np.array_equal(k_done, want) and (k_done < long['k_done'].cpu().numpy()).any(), where
    if scenario in ('long', 'two'):
        assert (held.sum(axis=1) > 0).sum() >= T // 2 and ((k_done == K) & (held.sum(axis=1) > 0)).any(), 'the comparison would be vacuous'
        assert not same(fused['f'], loop(uvs, fp, inp, True)['f'])
    if scenario == 'two' and n_points > 1:
        assert any(len(set(held[t][held[t] > 0].tolist())) > 1 for t in range(T)), 'two discs held over different ranges'
    if scenario == 'leaves' and (method, n_points) == ('GMCKF', 4):
        unheld = loop(uvs, fp, inp, True)
        assert unheld['k_done'][T // 2].item() < K and unheld['pixels'][T // 2].min().item() == 0, 'the trial leaves the frame'
        assert held[T // 2].sum() > 0 and k_done[T // 2] > unheld['k_done'][T // 2].item(), 'and is held where it FAILed'


# ------------------------------------------------------------------------------------------------------------- 4: semantics
@pytest.mark.parametrize('fused', [True, False])
def test_the_rule_on_the_scenes_whose_schedule_is_known(uvs, fused):
    import torch
    T = 3
    fp, inp, discs = still_arm(uvs, T, 71)
    scenes = hc.scenes(discs)
    run = lambda name, hold: loop(uvs, fp, inp, fused, occluders_for(T, scenes[name]), hold=hold)   # noqa: E731
    counts = cover_schedule(uvs, inp, occluders_for(T, scenes['red_run']), T)
    assert all(np.array_equal(counts[:, t], counts[:, 0]) for t in range(T))
    (first, n), = hc.runs(counts[:, 0, hc.RED])
    assert n >= 2 and first >= 1
    unheld = loop(uvs, fp, inp, fused, occluders_for(T, scenes['red_run']))
    assert 'held' not in unheld and unheld['k_done'].tolist() == [first] * T and unheld['status'].tolist() == [1] * T
    zero = run('red_run', 0)
    assert_same_bits(zero, unheld, K, 'hold = 0')
    assert 'held' not in zero
    for hold in (n, n + 1, K, 2 ** 31 - 1):
        got = run('red_run', hold)
        assert got['k_done'].tolist() == [K] * T and got['status'].tolist() == [0] * T, hold
        assert got['held'].tolist() == [[n, 0, 0, 0]] * T and got['pixels'][:, hc.RED].tolist() == [0] * T, hold
        f = bits(got['f'])
        for k in range(first, first + n):
            assert np.array_equal(f[k, :, :2], f[first - 1, :, :2]), ('held rows are the row before the cover', k)
            assert not np.array_equal(f[k, :, 2:], f[first - 1, :, 2:]), 'the other discs are detected, noise and all'
        after = uvs.engine.camera_features(inp.plant, inp.q0, noise=inp.noise[first + n].contiguous(), occluders=occluders_for(T, scenes['red_run']),
                                           k=first + n)
        assert np.array_equal(f[first + n], bits(after)), 'the first row after the cover is an unheld detection of that frame'
        assert bool((got['err'][first:first + n, :, :2] == got['err'][first - 1, :, :2]).all()), 'err repeats'
        assert same(got['f'][:first], unheld['f'][:first]) and same(got['err'][:first], unheld['err'][:first]), 'rows before the cover'
    short = run('red_run', n - 1)
    assert short['k_done'].tolist() == [first + n - 1] * T and short['status'].tolist() == [1] * T
    assert short['held'].tolist() == [[n - 1, 0, 0, 0]] * T
    assert bool(torch.isnan(short['f'][first + n - 1, :, :2]).all()) and bool(torch.isfinite(short['f'][first + n - 1, :, 2:]).all())
    # the counter resets on a detection: two covers, held twice with the longer one's length
    twice = run('twice', hc.RESET_HOLD)
    assert twice['k_done'].tolist() == [K] * T and twice['held'].tolist() == [[2 + hc.RESET_HOLD, 0, 0, 0]] * T
    assert run('twice', hc.RESET_HOLD - 1)['k_done'].tolist() == [6 + hc.RESET_HOLD - 1] * T
    # two discs over different ranges
    two = run('two_discs', 4)
    assert two['k_done'].tolist() == [K] * T and two['held'].tolist() == [[3, 4, 0, 0]] * T
    two = run('two_discs', 3)
    assert two['k_done'].tolist() == [7] * T and two['held'].tolist() == [[3, 3, 0, 0]] * T, 'the step that FAILs counts what it held'
    # a cover at step 0 FAILs at 0 whatever hold is
    for hold in (1, K, 2 ** 31 - 1):
        got = run('step0', hold)
        assert got['k_done'].tolist() == [0] * T and got['status'].tolist() == [1] * T and got['held'].tolist() == [[0] * 4] * T


# ------------------------------------------------------------------------------------------------------------- 5: nothing else moved
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('occluded', [True, False])
def test_hold_zero_is_the_call_without_the_argument(uvs, fused, occluded):
    T = 5
    fp = g.params(uvs, 'GMCKF')
    q_host = g.jittered(T, 81)
    q_host[2] = g.Q_LEAVES
    inp = g.Inputs(uvs, 4, q_host, seed=82)
    inp.noise[:, 2] = 0.0                                            # Q_LEAVES was found without noise
    occ = occluders_for(T, [hc.wide_bar()]) if occluded else None
    got, want = loop(uvs, fp, inp, fused, occ, hold=0), loop(uvs, fp, inp, fused, occ)
    assert_same_bits(got, want, K, ('hold = 0', fused, occluded))
    assert 'held' not in got and (want['k_done'] < K).any(), 'a trial FAILs on its empty mask'


def c_abi(uvs, entry, fp, inp, T, occ, hold=None, tp=None, spare=0):
    """uvs_camera_closed_loop_{occluded,held}_f64 on buffers of T + spare trials filled with sentinels."""
    import torch
    cam = inp.plant.to_camera()
    n_points = inp.m // 2
    rows = T + spare
    f0 = uvs.engine.camera_features(inp.plant, inp.q0, occluders=occ)
    f64 = dict(dtype=torch.float64, device='cuda')
    log = {key: torch.full((K, T, comp), -7.0, **f64) for key, comp in (('q', 6), ('f', inp.m), ('dq', 6), ('err', inp.m), ('kappa', inp.m))}
    status, k_done = (torch.full((rows,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    stats = torch.full((rows, 3), -7.0, **f64)
    pixels, held = (torch.full((rows, n_points), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    packed = None if occ is None else uvs.engine.occluders(occ, T)
    head = (ctypes.byref(fp), ctypes.byref(cam), T, None if tp is None else ctypes.byref(tp), None if packed is None else packed.data_ptr(),
            0 if packed is None else packed.shape[1])
    tail = (inp.q0.data_ptr(), inp.noise.data_ptr(), inp.x0.data_ptr(), f0.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(),
            log['dq'].data_ptr(), log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr())
    lib = uvs._vision.lib()
    if entry == 'occluded':
        uvs._vision.check(lib.uvs_camera_closed_loop_occluded_f64(*head, *tail, None))
    else:
        uvs._vision.check(lib.uvs_camera_closed_loop_held_f64(*head, hold, *tail, held.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(log, status=status[:T], k_done=k_done[:T], stats=stats[:T], pixels=pixels[:T], held=held[:T],
                spare=(status[T:], k_done[T:], stats[T:], pixels[T:], held[T:]))


@pytest.mark.parametrize('T', [3, SMALL + 3])
def test_the_held_flavour_with_hold_zero_is_the_occluded_flavour(uvs, T):
    """Through the C ABI, on the same operands, a batch in which masks are emptied and trials FAIL; and what a padding wavefront leaves alone."""
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 83), seed=84)
    occ = occluders_for(T, [hc.wide_bar()])
    want = c_abi(uvs, 'occluded', fp, inp, T, occ)
    got = c_abi(uvs, 'held', fp, inp, T, occ, hold=0, spare=5)
    assert_same_bits(got, want, K, ('C ABI, hold = 0', T))
    for key in cc.LOGS:
        assert same(got[key], want[key]), (key, 'every byte, the sentinels of unwritten rows included')
    assert (want['k_done'] < K).sum().item() >= T // 2 and bool((got['held'] == 0).all())
    held = c_abi(uvs, 'held', fp, inp, T, occ, hold=K, spare=5)
    assert int(held['held'].sum()) > T and (held['k_done'] == K).sum().item() > (want['k_done'] == K).sum().item()
    for out in (got, held):                                          # T = 259: the last workgroup has a padding wavefront, which shadows trial T - 1
        assert all(bool((t == -7).all()) for t in out['spare']), 'a padding trial stored something'
    # no occluder operand at all, and no held output: legal
    bare = c_abi(uvs, 'held', fp, inp, T, None, hold=K)
    assert_same_bits(bare, loop(uvs, fp, inp, True, hold=K), K, 'occ = NULL, n_occ = 0')


def test_held_and_unheld_trials_share_a_workgroup(uvs):
    T = SMALL + 3
    fp = g.params(uvs, 'GMCKF')
    inp = g.Inputs(uvs, 4, g.jittered(T, 85), seed=86)
    occ = occluders_for(T, [hc.wide_bar()])
    occ[1::2] = oc.NEVER                                             # odd trials: nobody is covered
    got, clear = loop(uvs, fp, inp, occluders=occ, hold=K), loop(uvs, fp, inp)
    odd, even = list(range(1, T, 2)), list(range(0, T, 2))
    assert clear['k_done'].tolist() == [K] * T
    assert_same_bits(got, clear, K, 'neighbours of held trials', trials=odd)
    held = got['held'].cpu().numpy()
    assert not held[odd].any() and (held[even].sum(axis=1) > 0).sum() >= len(even) // 2, 'the even trials are held, the odd ones never'
    everyone = loop(uvs, fp, inp, occluders=occluders_for(T, [hc.wide_bar()]), hold=K)
    assert_same_bits(got, everyone, K, 'held trials', trials=even)
    assert_same_held(got, everyone, 'held trials', trials=even)


# ------------------------------------------------------------------------------------------------------------- 6: stepwise baselines
@pytest.mark.parametrize('believed', [False, True])
def test_the_stepwise_baselines_hold_and_survive_the_wide_bar(uvs, believed):
    import torch
    T, hold = 5, K
    eng = uvs.engine
    fp = g.params(uvs, 'ANALYTICAL')
    inp = g.Inputs(uvs, 4, g.jittered(T, 87), seed=88)
    occ = occluders_for(T, [hc.wide_bar()])
    kw = dict(believed=uvs.plant.miscalibrated(inp.plant, focal_scale=1.05)) if believed else {}
    run = lambda **more: eng.camera_closed_loop(fp, inp.plant, inp.q0, inp.noise, occluders=occ, **kw, **more)   # noqa: E731
    got, unheld = run(hold=hold), run()
    assert got['k_done'].tolist() == [K] * T and got['status'].tolist() == [0] * T and (unheld['k_done'] < K).all(), 'held, it survives the bar'
    assert_same_bits(run(hold=0), unheld, K, 'hold = 0')
    miss, reported, total = np.zeros((T, 4), np.int32), None, np.zeros((T, 4), np.int32)
    for k in range(K):                                               # the f rows obey the rule, at the loop's own logged joints
        pix = torch.zeros((T, 4), dtype=torch.int32, device='cuda')
        detected = eng.camera_features(inp.plant, got['q'][k].contiguous(), noise=inp.noise[k].contiguous(), occluders=occ, k=k, pixels=pix)
        reported, miss, held = uvs.plant.hold_features(detected.cpu().numpy(), reported, pix.cpu().numpy(), miss, hold)
        assert np.array_equal(bits(got['f'][k]), bits(reported)), k
        total += held
    assert np.array_equal(got['held'].cpu().numpy(), total) and (total.sum(axis=1) >= 2).all()
    with pytest.raises(ValueError, match='fused=False'):
        run(hold=hold, fused=True)


# ------------------------------------------------------------------------------------------------------------- 7: with trial_params
@pytest.mark.parametrize('occluded', [True, False])
def test_two_cells_behind_the_same_bar_have_the_bits_of_their_uniform_held_launches(uvs, occluded):
    E, hold = 3, K
    fp = g.params(uvs, 'GMCKF')
    q_host = g.jittered(E, 89)
    if not occluded:
        q_host[1] = g.Q_LEAVES
    inp = g.Inputs(uvs, 4, q_host, seed=90)
    if not occluded:
        inp.noise[:, 1] = 0.0                                        # Q_LEAVES was found without noise
    bandwidths = (5.0, 20.0)
    T = E * len(bandwidths)
    source = np.arange(T) % E
    tp = dict(kernel_bw=dev(np.repeat(bandwidths, E)), source=dev(source.astype(np.int32)))
    bar = [hc.wide_bar()]
    got = loop(uvs, fp, inp, occluders=occluders_for(T, bar) if occluded else None, trial_params=tp, hold=hold)
    assert got['status'].shape[0] == T and int(got['held'].sum()) > 0
    seen = set()
    for cell, bw in enumerate(bandwidths):
        one = type(fp).from_buffer_copy(fp)
        one.kernel_bw = bw
        want = loop(uvs, one, inp, occluders=occluders_for(E, bar) if occluded else None, hold=hold)
        trials = list(range(cell * E, (cell + 1) * E))
        assert_same_bits(got, want, K, ('cell', cell), trials=trials, want_trials=list(range(E)))
        assert_same_held(got, want, ('cell', cell), trials=trials, want_trials=list(range(E)))
        seen.add(bits(want['err']).tobytes())
    assert len(seen) == 2, 'the comparison would be vacuous: the two cells have the same errors'
