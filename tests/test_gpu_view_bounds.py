"""The view contract of libuvs_rmckf: every stream of every entry point is a strided view, and whichever store path a launcher picks from the
strides, the launch stores inside the windows of its outputs, reads inside the windows of its inputs, and writes the bits of the same call
into dense buffers.

Every guarded launch (gpu_harness.guarded_closed / guarded_replay) has every input and every requested output in an arena of the cell's view
kind (tests/view_arena_common.py: one allocation, the window, >= 16 KB of NaN on either side, NaN in pitch pads and neighbouring records) and
asserts (1) nothing outside an output window and no input byte changed, (2) every live row, status, k_done, the statistics and the final state
are stored, (3) the bits of the same call through gh.launch / gh.replay into dense exact-size buffers, (4) the CPU references: oracle/c at
gh.TOL for closed loops, rmckf_block.run_replay at gh.REPLAY_GATES for replays.  Which store path a (kind, T) reaches is view_arena_common's
restatement of the launcher predicates; the module prints the number of launches per (entry point, path, raggedness) cell when it finishes."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import closed_shapes_common as cs
import gpu_harness as gh
import view_arena_common as va
from gpu_harness import LATENCY, STREAMS, STRICT, TOL

pytestmark = pytest.mark.gpu
WORST = gh.Worst()
LAUNCHES = collections.Counter()                             # (entry point, path, raggedness) -> guarded launches


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    yield uvs_amd
    WORST.report('view bounds')
    for cell in sorted(LAUNCHES):
        print('view bounds: guarded launches', cell, LAUNCHES[cell])


def _tiled(ref, T):
    """oracle/c's dict on the first T trials of a case (gh.first_trials)."""
    n = len(ref['status'])
    return ref if T <= n else {k: v[np.arange(T) % n] for k, v in ref.items()}


def _closed(uvs, case, method, anneal, lanes, T, kind, family, reserved=0, want=STREAMS, x_kind=None, ref_reserved=None, **kw):
    """One guarded closed-loop launch held to the dense launch of the same call (ref_reserved: of another option word that promises the same
    bits) and to oracle/c."""
    tag = (case, method, anneal, lanes, reserved, T, kind, x_kind)
    out = gh.guarded_launch(uvs, case, method, anneal, lanes, reserved, T=T, want=want, kind=kind, x_kind=x_kind, **kw)
    dense = gh.launch(uvs, case, method, anneal, lanes, reserved if ref_reserved is None else ref_reserved, T=T, want=want, final_state=True)
    assert out['lanes'] == dense['lanes'] or ref_reserved is not None, tag
    gh.assert_same_launch(out, dense, tag)
    key = (case, method, anneal)
    gh.assert_matches_c(out, _tiled(cs.c_reference(*key), len(out['status'])), cs.kept_trials(key) if T <= cs.inputs(case)['T'] else range(T), WORST, family, tag)
    return out


# ---------------------------------------------------------------------------------------------- a. the headline shape
HEADLINE = sorted({(c[3], c[2], c[1]) for _, _, c in va.cells_of('closed')})


@pytest.mark.parametrize('method,lanes,T', HEADLINE)
def test_headline_shape_every_view_kind(uvs, method, lanes, T):
    """'dh86', all five streams and the final state: every stream in the kind, then X alone in the kind while the narrow streams stay dense
    trial-fastest rows.  lanes_per_filter 2 reaches `records` and `pairs` (KF, IMCC-KF); 0 runs the four-lane small-batch kernels."""
    for path, rag, (kind, _, _, _) in [c for c in va.cells_of('closed') if (c[2][3], c[2][2], c[2][1]) == (method, lanes, T)]:
        for own in (False, True):
            if own and kind == 'kct':
                continue
            out = _closed(uvs, 'dh86', method, False, lanes, T, 'kct' if own else kind, f'(8,6) DH L{lanes or 4} {path}', x_kind=kind if own else None)
            assert out['lanes'] == va.lanes_used('closed', lanes)
            LAUNCHES[('closed', path, rag)] += 1


@pytest.mark.parametrize('lanes', [2, 0])
@pytest.mark.parametrize('method', cs.METHODS)
def test_headline_shape_with_one_stream_wanted(uvs, method, lanes):
    """('err',) alone -- the instantiations without the X stream -- and ('x',) alone, at the ragged sizes."""
    for want in (('err',), ('x',)):
        for kind, T in (('ktc_slice', 70), ('kct_pitch_even', 70), ('kct_pitch_odd', 69)):
            _closed(uvs, 'dh86', method, False, lanes, T, kind, f'(8,6) DH L{lanes or 4} one stream', want=want)


# ---------------------------------------------------------------------------------------------- b. every other mapping
OTHER_ROUTES = [('dh66', 2, 0), ('dh66', 1, 0), ('dh66', -2, 0), ('dh66_x0', 2, 0), ('dh66_x0', 1, 0), ('dh26', 1, 0), ('dh26', -1, 0),
                ('lin86', 1, 0), ('lin86', 2, 0), ('lin86', 4, 0), ('lin86', -4, 0), ('lin66', 2, 0), ('lin66', -2, 0),
                ('dh86', 1, 0), ('dh86', 4, 0), ('dh86', 8, 0), ('dh86', -2, 0), ('dh86', 0, LATENCY)]


@pytest.mark.parametrize('method', cs.METHODS)
@pytest.mark.parametrize('case,lanes,reserved', OTHER_ROUTES)
def test_every_other_mapping_stays_inside_its_views(uvs, case, lanes, reserved, method):
    """Each (m, n, L) of the library on its case, the generic templates (lanes < 0) and the plain four-lane kernels of UVS_OPT_LATENCY: a pitched
    odd row, a slice of records, records off by one double, and a slice of per-trial planes; two whole wavefronts and a ragged third."""
    inp = cs.inputs(case)
    for kind in va.WIDE_KINDS:
        for T in (70, 64):
            _closed(uvs, case, method, True, lanes, T, kind, f'({inp["m"]},{inp["n"]}) {inp["kind"]} L{lanes} opt {reserved}', reserved)


@pytest.mark.parametrize('method', va.WIDE_METHODS)
@pytest.mark.parametrize('lanes', [8, 16, 32, -8])
def test_the_wide_shape_stays_inside_its_views(uvs, lanes, method):
    """(32,7): the wide kernel at 8 and 16 lanes (`rec`: whole wavefronts of records, 1 KB stores out of the LDS transposition; the strided
    path otherwise), the generic template at 32 and a forced 8.  T = 4 and 8: the four trials of 'wide', tiled."""
    for kind in va.WIDE_KINDS:
        for T in va.WIDE_T:
            path = va.wide_x_path(lanes, T, va.geometry(T, va.WIDE_K, 224, kind))
            _closed(uvs, 'wide', method, True, lanes, T, kind, f'(32,7) L{lanes} {path}')
            if lanes > 0:
                assert (kind, T, lanes, method) in va.CELLS[('wide', path, va.raggedness(T, 64 // lanes))]
                LAUNCHES[('wide', path, va.raggedness(T, 64 // lanes))] += 1


# ---------------------------------------------------------------------------------------------- c. FAIL placement
@functools.lru_cache(maxsize=None)
def _injected_reference(method):
    from oracle import c_oracle
    inp = cs.inputs('dh86')
    return c_oracle.closed_loop_batch(inp['q0'], va.inject_fails(inp['noise']), inp['desired'], method=method, kernel_bw=inp['bw'], annealing=False, dt=cs.DT,
                                      t_max=inp['t_max'], gain=cs.GAIN, steps=inp['K'], want_x=True, plant=cs.c_plant(inp), fpi_threshold=cs.FPI_THRESHOLD)


@pytest.mark.parametrize('kind', ['ktc_slice', 'kct_pitch_even', 'kct_pitch_odd'])
@pytest.mark.parametrize('method', ['KF', 'GMCKF'])
def test_failing_trials_leave_everything_outside_the_views_alone(uvs, method, kind):
    """NaN noise samples: one trial FAILs mid-wavefront at step 17, one at step 0 (nothing logged), and every trial of the ragged last wavefront
    (64..69) at step 2 -- the wavefront-wide exit, after which the record path still stores the last step's records.  Rows at and after k_done
    inside a window are unspecified; everything outside stays untouched, and the healthy trials keep the bits of the uninjected launch."""
    inp = cs.inputs('dh86')
    tag = ('FAIL placement', method, kind)
    noise = va.inject_fails(inp['noise'])
    out = gh.guarded_launch(uvs, 'dh86', method, False, 2, kind=kind, noise=noise)
    ref = _injected_reference(method)
    assert np.flatnonzero(out['status']).tolist() == sorted(va.FAIL_PLAN) and all(out['k_done'][t] == k for t, k in va.FAIL_PLAN.items()), tag
    gh.assert_matches_c(out, ref, range(inp['T']), WORST, f'(8,6) DH L2 FAIL placement {method}', tag)
    healthy = [t for t in range(inp['T']) if t not in va.FAIL_PLAN]
    gh.assert_same_launch(out, gh.launch(uvs, 'dh86', method, False, 2, want=STREAMS, final_state=True), tag, trials=healthy)
    dense = gh.guarded_launch(uvs, 'dh86', method, False, 2, kind='kct', noise=noise)
    gh.assert_same_launch(out, dense, tag, trials=healthy)
    gh.assert_same_launch(out, dense, tag, keys=STREAMS + ('status', 'k_done'), trials=sorted(va.FAIL_PLAN))
    LAUNCHES[('closed', va.closed_x_path(8, 6, 2, method, 'dh', False, False, 70, va.geometry(70, 60, 48, kind)), 'ragged_even')] += 1


# ---------------------------------------------------------------------------------------------- d. the second pass and strict mode
RANKDEF_K, SICK = 12, 40                                     # test_gpu_closed_shapes.py::test_a_rank_deficient_x0_among_healthy_neighbours


@pytest.mark.parametrize('kind', ['ktc_slice', 'kct_pitch_odd'])
@pytest.mark.parametrize('case,lanes', [('dh66_x0', 0), ('lin86', 0), ('lin86', -2)])
def test_the_careful_pass_rewrites_its_trial_among_the_neighbours_rows(uvs, case, lanes, kind):
    """One trial starts from an X0 with two identical columns: the careful kernel re-runs it from step 0, inside rows and records that belong to
    69 healthy neighbours.  The bits of the dense launch; the sick trial and its neighbours against the numpy oracle at that test's gates."""
    from oracle import rmckf_block
    inp = cs.inputs(case)
    m, n = inp['m'], inp['n']
    x0 = inp['x0'].copy()
    x0[SICK].reshape(m, n)[:, 5] = x0[SICK].reshape(m, n)[:, 4]
    want = ('x', 'err', 'q', 'dq')
    tag = ('rank-deficient x0', case, lanes, kind)
    out = gh.guarded_launch(uvs, case, 'GMCKF', True, lanes, want=want, kind=kind, steps=RANKDEF_K, x0=x0)
    assert not out['status'].any() and np.all(out['k_done'] == RANKDEF_K), tag
    gh.assert_same_launch(out, gh.launch(uvs, case, 'GMCKF', True, lanes, want=want, steps=RANKDEF_K, x0=x0, final_state=True), tag)
    for t in (SICK - 1, SICK, SICK + 1, cs.T - 1):
        ref = rmckf_block.run_closed_loop(inp['features'], inp['q0'][t], inp['desired'], inp['noise'][t, :RANKDEF_K], cs.DT, cs.DT * (RANKDEF_K + 0.5),
                                          cs.GAIN, x0[t], method='GMCKF', kernel_bw=cs.BW, annealing=True, initial_guess=False)
        for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
            d = cs.rel(out[key][t], ref[rk])
            WORST.note('rank-deficient X0', key + (' (sick)' if t == SICK else ' (healthy)'), d)
            assert d <= (1e-6 if t == SICK else TOL), (key, d, t) + tag


@pytest.mark.parametrize('kind', ['ktc_slice', 'kct_pitch_odd'])
@pytest.mark.parametrize('case,lanes,T', [('dh86', 2, 70), ('wide', 8, 8), ('dh86', -2, 70)])
def test_strict_mode_stays_inside_its_views(uvs, case, lanes, T, kind):
    """UVS_OPT_STRICT_PINV on a route whose first pass certifies ((8,6), two lanes: the CERT instantiations, plain stores whatever the view) and
    on two that do not (the wide kernel, the generic template: every trial through the careful pass)."""
    for method in va.WIDE_METHODS if case == 'wide' else cs.METHODS:
        _closed(uvs, case, method, True, lanes, T, kind, f'{case} L{lanes} strict', STRICT)
        if (case, lanes) == ('dh86', 2):
            assert va.closed_x_path(8, 6, 2, method, 'dh', False, True, T, va.geometry(T, 60, 48, kind)) == 'plain'


# ---------------------------------------------------------------------------------------------- e. segments and the workspace
@pytest.mark.parametrize('kind', ['kct_pitch_even', 'ktc_slice', 'kct_pitch_odd'])
@pytest.mark.parametrize('segments', [2, 4])
@pytest.mark.parametrize('method', ['MCKF', 'GMCKF'])
def test_segmented_launches_stay_inside_their_views_and_their_workspace(uvs, method, segments, kind):
    """A forced segment count (bits 8-15 of reserved) and a workspace of exactly uvs_rmckf_closed_loop_workspace_bytes bytes between two guards:
    the state crosses through it from segment to segment.  The guards keep their bytes, no work item fell back, and the outputs have the
    unsegmented launch's bits."""
    for T in (70, 64):
        out = _closed(uvs, 'dh86', method, False, 2, T, kind, f'(8,6) DH L2 {segments} segments', segments << 8, ref_reserved=0, own_workspace=True)
        assert out['segments'] == segments and out['workspace'] > 0 and out['fallbacks'] == 0, (method, segments, kind, T, out['fallbacks'])


# ---------------------------------------------------------------------------------------------- f. the grid entry point
GRID_E = 35
GRID_CELLS = ((cs.BW, cs.GAIN, cs.REG, cs.FPI_THRESHOLD, 0.0), (5.0, 0.3, 4 * cs.REG, 1e-3, 1.5))      # kernel_bw, gain, reg, fpi_threshold, target shift


@pytest.mark.parametrize('kind', ['kct_pitch_even', 'ktc_slice'])
@pytest.mark.parametrize('lanes', [2, 0])
@pytest.mark.parametrize('method', cs.METHODS)
def test_the_grid_entry_point_stays_inside_its_views(uvs, method, lanes, kind):
    """uvs_rmckf_closed_loop_grid_f64: 70 trials in two cells over 35 input trials, read through a permutation; per-trial arrays of exactly T
    doubles, the target view and the permutation in arenas.  Each cell has the bits of its uniform launch and follows oracle/c."""
    from oracle import c_oracle
    inp = cs.inputs('dh86')
    E, K, T = GRID_E, inp['K'], 2 * GRID_E
    perm = (np.arange(E) * 12 + 5) % E
    assert sorted(perm.tolist()) == list(range(E))
    cell = np.arange(T) // E
    col = lambda i: np.array([GRID_CELLS[h][i] for h in cell])                                     # noqa: E731
    trial = dict(kernel_bw=col(0), gain=col(1), reg=col(2), fpi_threshold=col(3), desired=inp['desired'][None, :] + col(4)[:, None],
                 source=np.tile(perm, 2).astype(np.int32))
    fp = gh.params(uvs, 'dh86', method, False, lanes)
    ps = gh.plant(uvs, 'dh86').to_struct()
    tag = ('grid', method, lanes, kind)
    out = gh.guarded_closed(uvs, fp, ps, T, inp['q0'][:E], inp['noise'][:E], None, STREAMS, kind, trial=trial, tag=tag)
    assert not out['status'].any(), tag
    for h, (bw, gain, reg, thr, shift) in enumerate(GRID_CELLS):
        sub = {k: None if v is None or isinstance(v, int) else v[h * E:(h + 1) * E] for k, v in out.items()}
        ufp = uvs.engine.make_params(8, 6, method, bw, False, cs.DT, cs.DT * (K + 0.5), gain, inp['desired'] + shift, True, lanes, K, thr, 1000)
        ufp.reg = reg
        dev = uvs.engine.closed_loop(ufp, ps, gh.cuda(inp['q0'][perm]), gh.cuda(inp['noise'][perm].transpose(1, 2, 0)), want=STREAMS, final_state=True)
        uniform = {k: dev[k].cpu().numpy().transpose(2, 0, 1) for k in STREAMS}
        uniform.update({k: dev[k].cpu().numpy() for k in ('stats', 'status', 'k_done', 'x_final', 'p_final')})
        gh.assert_same_launch(sub, uniform, tag + (h,))
        ref = c_oracle.closed_loop_batch(inp['q0'][perm], inp['noise'][perm], inp['desired'] + shift, method=method, kernel_bw=bw, annealing=False, dt=cs.DT,
                                         t_max=inp['t_max'], gain=gain, steps=K, want_x=True, plant=cs.c_plant(inp), fpi_threshold=thr, reg=reg)
        gh.assert_matches_c(sub, ref, range(E), WORST, '(8,6) DH grid entry point', tag + (h,))


# ---------------------------------------------------------------------------------------------- g. replay, fp64
REPLAY_SEEDS = {(8, 6): 1008, (6, 6): 1006}


@functools.lru_cache(maxsize=None)
def _replay_case(shape):
    return gh.random_replay_case(*shape, va.REPLAY_K, max(va.REPLAY_T), REPLAY_SEEDS[shape])


@functools.lru_cache(maxsize=None)
def _replay_references(shape, method):
    from oracle import rmckf_block
    f, dq, x0, des = _replay_case(shape)
    return [rmckf_block.run_replay(f[t], dq[t], x0[t], des, 0.2, method, 7.5, True, 300, cs.FPI_THRESHOLD) for t in range(len(x0))]


@pytest.mark.parametrize('T', va.REPLAY_T)
@pytest.mark.parametrize('method', cs.METHODS)
@pytest.mark.parametrize('shape,lanes', [((8, 6), 0), ((8, 6), 2), ((8, 6), 4), ((6, 6), 0), ((6, 6), 2)])
def test_replay_stays_inside_its_views(uvs, shape, lanes, method, T):
    """uvs_rmckf_replay_f64 at (8,6) -- the record path (X and err both records, whole wavefronts of 16 trials), the row-group wavefronts, the
    four lane groups, the control wavefronts, the two-lane kernel and the generic template -- and the two-lane kernel at (6,6); f (K + 1 rows),
    dq and x0 are read out of arenas whose padding is NaN."""
    f, dq, x0, des = _replay_case(shape)
    refs = _replay_references(shape, method)[:T]
    fp = uvs.engine.make_params(*shape, method, 7.5, True, 0.05, 15, 0.2, des, False, lanes, va.REPLAY_K, cs.FPI_THRESHOLD, 1000)
    for want in va.REPLAY_WANTS:
        dense = gh.replay(uvs, fp, f[:T], dq[:T], x0[:T], want)
        for kind in va.REPLAY_KINDS:
            path = va.replay_path(method, lanes, want, T, va.geometry(T, va.REPLAY_K, 48, kind), va.geometry(T, va.REPLAY_K, 8, kind), shape)
            tag = ('replay', shape, method, lanes, path)
            out = gh.guarded_replay(uvs, fp, f[:T], dq[:T], x0[:T], want, kind, tag)
            assert not out['status'].any() and np.all(out['k_done'] == va.REPLAY_K), tag
            gh.assert_same_replay(out, dense, tag + (kind, want))
            gh.assert_replay(out, refs, WORST, f'replay {shape} {path}', tag + (kind, want))
            if shape == (8, 6):
                assert (kind, T, lanes, method, want) in va.CELLS[('replay', path, va.raggedness(T, 16))]
                LAUNCHES[('replay', path, va.raggedness(T, 16))] += 1


# ---------------------------------------------------------------------------------------------- h. the small entry points
@pytest.mark.parametrize('method', ['GMCKF', 'MCKF'])
@pytest.mark.parametrize('m,n,lanes', gh.SHAPES)
def test_the_single_step_stays_inside_its_buffers(uvs, m, n, lanes, method):
    """uvs_rmckf_step_f64 on T = 64 / L + 3 filters (two blocks, the second ragged): X and P, inout, the three inputs and the four outputs are
    dense windows between guards; two steps of gh.step_recipe at gh.STEP_GATES."""
    import torch
    rng = np.random.default_rng(100 * m + lanes)
    head, *recipe = gh.step_recipe(rng, m, n, lanes, method, 0, 1.0, 10.0, True, 2)
    T = head['T']
    fp = uvs.engine.make_params(m, n, method, 10.0, True, 0.05, 15.0, head['gain'], head['desired'], False, lanes, 0)
    bank = uvs.engine.FilterBank(fp, T, head['x0'])
    ar = gh.Arenas('tkc')
    for name in ('X', 'P', 'dq', 'err', 'kappa', 'status'):
        buf = getattr(bank, name)
        window = ar.output(name, T, 1, buf[0].numel(), dtype=buf.dtype)
        window.copy_(buf.reshape(T, 1, -1))
        setattr(bank, name, window.view(buf.shape))
    put = lambda a: ar.input(f'input {len(ar.items)}', a).view(a.shape)                            # noqa: E731
    for s, st in enumerate(recipe):
        gh.assert_step(bank, st, head['desired'], WORST, (f'step ({m},{n}) L{lanes}',), (m, n, lanes, method, s), fresh=s == 0, put=put)
        torch.cuda.synchronize()
        ar.check(('step', m, n, lanes, method, s))


@pytest.mark.parametrize('kind', ['kct_pitch_odd', 'ktc_slice', 'tkc_slice'])
def test_the_statistics_kernel_reads_inside_its_view(uvs, kind):
    """uvs_stats_reduce_f64 over two blocks of which the second is one trial long (T = 257), the error stream a window with NaN all around it:
    the longdouble sums of test_stats_kernel_shapes_layouts_and_k_done at its gate."""
    import torch
    rng = np.random.default_rng(257)
    K, T, m = 61, 257, 8
    err = rng.normal(size=(T, K, m)) * 10
    t = uvs.engine.loop_clock(0.05, 15)[:K]
    k_done = rng.integers(0, K + 1, T).astype(np.int32)
    k_done[[0, 255, 256]] = 0, K, K - 1
    e = np.where(np.arange(K)[None, :, None] < k_done[:, None, None], err, 0.0).astype(np.longdouble)
    sums = np.stack([(e * e).sum(axis=1), np.abs(e).sum(axis=1), (t.astype(np.longdouble)[None, :, None] * np.abs(e)).sum(axis=1)], axis=1)
    ref = np.sqrt((sums * sums).sum(axis=2)).astype(np.float64)
    ar = gh.Arenas(kind)
    v_err, v_t, v_k = ar.input('err', err), ar.input('t', t, 'tkc'), ar.input('k_done', k_done, 'tkc', torch.int32)
    stats = ar.output('stats', T, 1, 3, 'tkc')
    uvs._lib.check(uvs.lib().uvs_stats_reduce_f64(T, K, m, gh.stream(uvs, v_err), v_t.data_ptr(), v_k.data_ptr(), stats.data_ptr(), None))
    torch.cuda.synchronize()
    ar.check(('stats', kind))
    got = ar.host('stats').reshape(T, 3)
    assert np.all(np.abs(got - ref) <= 1e-12 * ref), float(np.abs(got / np.where(ref > 0, ref, 1) - 1).max())


def test_device_seeding_stays_inside_its_buffers(uvs):
    """uvs_pcg64_seed_u64, n = 257: numpy's own generator states, and nothing past the 257th."""
    import torch
    seeds = np.random.default_rng(11).integers(0, 2 ** 63, 257, dtype=np.uint64)
    ar = gh.Arenas('tkc')
    v_seeds = ar.input('seeds', seeds.view(np.int64), dtype=torch.int64)
    states = ar.output('states', 257, 1, 4, dtype=torch.int64)
    uvs._lib.check(uvs.lib().uvs_pcg64_seed_u64(257, v_seeds.data_ptr(), states.data_ptr(), None))
    torch.cuda.synchronize()
    ar.check(('pcg64_seed',))
    assert np.array_equal(ar.host('states').reshape(257, 4).view(np.uint64), uvs.pcg.pcg64_states(seeds))


NOISE_T, NOISE_K, NOISE_M, NOISE_SEED0 = 70, 40, 8, 424242
NOISE_PARAMS = dict(alpha=1.5, beta=0, gamma=1, delta=0)


def _noise_operands(uvs, ar, gen_seeds):
    """The generator states of `gen_seeds` and the ziggurat tables as input windows; (states, tables)."""
    import torch
    states = uvs.pcg.pcg64_states(np.asarray(gen_seeds, dtype=np.uint64).ravel()).view(np.int64)
    return ar.input('states', states, 'tkc', torch.int64), ar.input('tables', uvs.noise_device._zig('cuda').cpu().numpy(), 'tkc')


@pytest.mark.parametrize('kind', ['kct_pitch_odd', 'tkc_slice'])
def test_the_noise_generators_stay_inside_their_views(uvs, kind):
    """uvs_noise_generate_f64 (T = 70) and uvs_noise_generate_streams_f64 (S = 70 + 70 shared streams) into a pitched odd row and a slice of
    per-trial planes: the host generator's streams at test_device_batch_matches_host_batch's gate."""
    import torch
    nt = uvs.NoiseType.ALPHA_STABLE
    T, K, m = NOISE_T, NOISE_K, NOISE_M
    seeds = NOISE_SEED0 + np.arange(T)
    host = uvs.noise_batch(nt, NOISE_PARAMS, seeds, m, K, False, 0)
    q = uvs.noise_device.make_noise_params(nt, NOISE_PARAMS, m, K, False, 0)
    ar = gh.Arenas(kind)
    v_states, v_zig = _noise_operands(uvs, ar, uvs.noise_device.generator_seeds(nt, seeds, m))
    out = ar.output('noise', T, K, m)
    uvs._lib.check(uvs.lib().uvs_noise_generate_f64(C.byref(q), T, v_states.data_ptr(), v_zig.data_ptr(), gh.stream(uvs, out), None))
    torch.cuda.synchronize()
    ar.check(('noise_generate', kind))
    got = ar.host('noise')
    assert not np.isnan(got).any() and np.allclose(got, host, rtol=2e-13, atol=1e-12)
    # one stream per distinct generator seed: feature i of trial t is stream t + 10 i
    S = T + uvs.noise_device.SEED_STEP * (m - 1)
    assert S == 70 + 70
    ar = gh.Arenas(kind)
    v_states, v_zig = _noise_operands(uvs, ar, NOISE_SEED0 + np.arange(S))
    out = ar.output('streams', S, K, 1)
    uvs._lib.check(uvs.lib().uvs_noise_generate_streams_f64(C.byref(q), S, v_states.data_ptr(), v_zig.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), None))
    torch.cuda.synchronize()
    ar.check(('noise_generate_streams', kind))
    got = ar.host('streams')[:, :, 0]                                                              # (S, K)
    shared = np.stack([got[uvs.noise_device.SEED_STEP * i:uvs.noise_device.SEED_STEP * i + T] for i in range(m)], axis=2)
    assert not np.isnan(got).any() and np.allclose(shared, host, rtol=2e-13, atol=1e-12)


def test_the_calibrated_baseline_stays_inside_its_views(uvs):
    """uvs_analytical_closed_loop_f64, T = 70 on the tilted plant of analytical_common, every stream -- j_out among them -- a slice of records:
    the bits of engine.analytical_closed_loop's dense launch, and the restatement at test_gpu_analytical.py's gates (J 1e-10, the rest gh.TOL)."""
    import analytical_common as ac
    import torch
    inp = ac.base_inputs()
    T, K = ac.T, ac.K
    fp = uvs.engine.make_params(8, 6, 'ANALYTICAL', t_s=ac.DT, gain=ac.GAIN, desired=inp['desired'], steps=K)
    ps = ac.device_plant(uvs, ac.plant_of('tilted')).to_struct()
    comps = {'j': 48, 'err': 8, 'q': 6, 'f': 8, 'dq': 6}
    ar = gh.Arenas('ktc_slice')
    v_q0, v_noise = ar.input('q0', inp['q0']), ar.input('noise', inp['noise'][:, :K])
    outs = {k: ar.output(k, T, K, c) for k, c in comps.items()}
    stats = ar.output('stats', T, 1, 3, 'tkc')
    status, k_done = (ar.output(k, T, 1, 1, 'tkc', torch.int32) for k in ('status', 'k_done'))
    rc = uvs.lib().uvs_analytical_closed_loop_f64(C.byref(fp), C.byref(ps), T, gh.flat(uvs, v_q0), gh.stream(uvs, v_noise), *(gh.stream(uvs, outs[k]) for k in comps),
                                                  stats.data_ptr(), status.data_ptr(), k_done.data_ptr(), None)
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    ar.check(('analytical',))
    out = {k: ar.host(k) for k in comps}
    out.update(stats=ar.host('stats').reshape(T, 3), status=ar.host('status').reshape(T), k_done=ar.host('k_done').reshape(T))
    ref = ac.reference('tilted')
    assert np.array_equal(out['status'], ref['status']) and np.array_equal(out['k_done'], ref['k_done']) and not np.isnan(out['stats']).any()
    dense = uvs.engine.analytical_closed_loop(fp, ps, gh.cuda(inp['q0']), gh.cuda(inp['noise'][:, :K].transpose(1, 2, 0)), want=tuple(comps))
    for key in comps:
        live = gh.live(out, key)
        assert not np.isnan(live).any(), key
        assert gh.same_bits(live, gh.live(dict(out, **{key: dense[key].cpu().numpy().transpose(2, 0, 1)}), key)), key
        d = gh.per_trial_rel(live, ref[key][:, :K])
        WORST.note('calibrated baseline', key, d.max())
        assert d.max() <= (1e-10 if key == 'j' else TOL), (key, float(d.max()))
    for key in ('stats', 'status', 'k_done'):
        assert gh.same_bits(out[key], dense[key].cpu().numpy()), key
    ok = ref['status'] == 0
    assert gh.per_trial_rel(out['stats'][ok], ref['stats'][ok]).max() <= TOL


# ---------------------------------------------------------------------------------------------- the checker itself, on the device
@pytest.mark.parametrize('kind', ['kct_pitch_even', 'ktc_slice', 'tkc_slice'])
def test_the_checker_sees_a_stray_store_on_the_device(uvs, kind):
    """tests/test_view_arena_host.py's sensitivity cases on device memory: one double in a guard, and a window written for one trial too many."""
    T, K, comp = 70, 9, 8
    whole, window, before = va.arena(T, K, comp, kind, device='cuda')
    window.fill_(3.0)
    va.assert_only_the_window_changed(whole, window, before, (kind,))
    short = va.strays(whole, window[:T - 1], before)
    st, sk, sc = window.stride()
    last = window.storage_offset() + st * (T - 1) + sk * np.arange(K)[:, None] + sc * np.arange(comp)[None, :]
    assert sorted(short.tolist()) == sorted(last.ravel().tolist())
    whole[window.storage_offset() - 1] = 0.0
    assert va.strays(whole, window, before).tolist() == [window.storage_offset() - 1]
    with pytest.raises(AssertionError, match='outside the view'):
        va.assert_only_the_window_changed(whole, window, before, (kind,))
