"""The device side of the suites that hold the kernels to the CPU oracles (test_gpu_closed_shapes.py, test_gpu_estimator_params.py,
test_gpu_step.py, test_gpu_grid.py, test_gpu_view_bounds.py): launches into poisoned buffers -- and, guarded, into windows between guard bands
(view_arena_common.py) --, the comparisons with the references of closed_shapes_common.py, the gates, and the generators of the single-step and
replay inputs.  torch is imported inside the functions: collection on a machine
without a GPU imports every module that imports this one."""
import copy
import ctypes as C
import json
import os

import numpy as np

import closed_shapes_common as cs
from conftest import ROOT
from closed_shapes_common import rel

TOL = 1e-8                                                   # closed loop: err, q, x and stats, relative, per trial (test_gpu_fuzz.py)
TOL_MODES = 1e-9                                             # strict against default mode (test_strict_pinv_agrees_with_the_fast_path_on_healthy_trials)
STRICT, LATENCY = 1, 2                                       # UVS_OPT_STRICT_PINV, UVS_OPT_LATENCY
BLOCK_TRIALS = (0, 14, 28, 42, 56)                           # of cs.sampled(case): compared with the numpy oracle directly as well
STREAMS = ('x', 'err', 'q', 'f', 'dq')                      # the closed loop's per-step outputs, in the header's order
POISON_INT = -7
# single step: X, P, command (tools/fuzz_step.py), kappa (test_replay_other_shapes_match_block_oracle)
TOL_X, TOL_P, TOL_DQ, TOL_KAPPA = 1e-10, 1e-9, 1e-7, 1e-9
STEP_GATES = (('X', TOL_X), ('P', TOL_P), ('dq', TOL_DQ), ('kappa', TOL_KAPPA))
K_MAX = 300                                                  # make_params(t_s = 0.05, t_max = 15)
SHAPES = [(8, 6, 1), (8, 6, 2), (8, 6, 4), (8, 6, 8), (6, 6, 1), (6, 6, 2), (2, 6, 1), (32, 7, 8), (32, 7, 16), (32, 7, 32)]   # UVS_SHAPES
DEFAULT_LANES = {(8, 6): 4, (6, 6): 2, (2, 6): 1, (32, 7): 16}          # what lanes_per_filter = 0 resolves to on the single-step route
# replay, per trial (test_replay_other_shapes_match_block_oracle): output -> (the key of rmckf_block.run_replay's dict, gate)
REPLAY_GATES = {'p_final': ('P_final', 1e-10), 'x_final': ('X', 1e-10), 'x': ('X', 1e-10), 'kappa': ('kappa', 1e-9), 'dqcmd': ('dq_cmd', 1e-8)}
_PLANTS, _LAUNCHES = {}, {}


class Worst(dict):
    """route -> quantity -> worst relative deviation from the references so far; printed when a module finishes (pytest -s)."""

    def note(self, route, key, value):
        worst = self.setdefault(route, {})
        worst[key] = max(worst.get(key, 0.0), float(value))

    def report(self, title):
        for route, worst in self.items():
            print(f'{title}, {route}: worst relative deviations', {k: f'{v:.1e}' for k, v in worst.items()})


def cuda(a):
    import torch
    return torch.as_tensor(np.array(a, order='C'), device='cuda')     # a copy: the shared inputs are read-only arrays


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def poisoned(T, K, comp, layout='kct'):
    """A [trial][step][component] stream in the physical layout `layout`, every double NaN."""
    import torch
    shape = {'kct': (K, comp, T), 'ktc': (K, T, comp), 'tkc': (T, K, comp)}[layout]
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def poisoned_trials(T, stats=True, final=None):
    """The per-trial outputs: status and k_done -7, statistics (T, 3) and -- final = (m, n) -- the final state NaN."""
    import torch
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')      # noqa: E731
    dev = dict(status=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'), k_done=torch.full((T,), POISON_INT, dtype=torch.int32, device='cuda'))
    if stats:
        dev['stats'] = nan(T, 3)
    if final:
        dev.update(x_final=nan(T, final[0] * final[1]), p_final=nan(T, final[0] * final[1] * final[1]))
    return dev


def live(out, key):
    """The stream with the rows at and after k_done (unspecified) zeroed."""
    a = out[key]
    return np.where(np.arange(a.shape[1])[None, :, None] < out['k_done'][:, None, None], a, 0.0)


def per_trial_rel(a, b):
    T = len(a)
    return np.abs(a - b).reshape(T, -1).max(axis=1) / np.maximum(np.abs(b).reshape(T, -1).max(axis=1), 1e-300)


def assert_everything_was_stored(out, tag):
    """No poison is left in a status, a k_done, a live row of a stream, or the statistics and final state of a trial that succeeded."""
    assert set(out['status'].tolist()) <= {0, 1} and out['k_done'].min() >= 0, tag
    ok = out['status'] == 0
    for key in STREAMS:
        if out.get(key) is not None:
            assert not np.isnan(live(out, key)).any(), (key,) + tuple(tag)
    for key in ('stats', 'x_final', 'p_final'):
        if out.get(key) is not None:
            assert not np.isnan(out[key][ok]).any(), (key,) + tuple(tag)


# ---------------------------------------------------------------------------------------------- closed loop
def plant(uvs, case):
    if case not in _PLANTS:
        inp = cs.inputs(case)
        if inp['kind'] == 'dh':
            _PLANTS[case] = uvs.SyntheticPlant.ur10(inp['desired'])
            assert np.allclose(_PLANTS[case].points, inp['discs'], rtol=0, atol=1e-15)
        else:
            _PLANTS[case] = uvs.LinearPlant(*inp['lin'])
    return _PLANTS[case]


def params(uvs, case, method, anneal, lanes=0, reserved=0, steps=None, guess=None, fpi_threshold=cs.FPI_THRESHOLD):
    """The parameter block of a launch of `steps` steps (default: the case's K) with k_max = steps, reg and anneal_span at the defaults."""
    inp = cs.inputs(case)
    steps = inp['K'] if steps is None else steps
    fp = uvs.engine.make_params(inp['m'], inp['n'], method, inp['bw'], anneal, cs.DT, cs.DT * (steps + 0.5), cs.GAIN, inp['desired'],
                                inp['guess'] if guess is None else guess, lanes, steps, fpi_threshold, 1000)
    assert fp.k_max == steps and fp.reg == cs.REG and fp.anneal_span == cs.ANNEAL_SPAN
    fp.reserved = reserved
    return fp


def first_trials(a, T):
    """The first T trials of a per-trial input of a case; beyond the case's own trials they repeat from trial 0 ('wide', T = 4, tiled to 8)."""
    return a[:T] if T <= len(a) else a[np.arange(T) % len(a)]


def launch(uvs, case, method, anneal, lanes=0, reserved=0, T=None, want=('x', 'err', 'q'), layout='kct', x_layout=None, final_state=False,
           steps=None, x0=None, reg=cs.REG, anneal_span=cs.ANNEAL_SPAN):
    """One closed-loop launch (uvs_rmckf_closed_loop_ws_f64) on the first T trials of the case (first_trials), fp.reg and fp.anneal_span set after
    make_params; numpy arrays in [trial][step][component] order whatever the layout, plus what the host-side queries say about the launch.
    Launches are kept: the same one serves several tests (x0: an override, never kept)."""
    import torch
    inp = cs.inputs(case)
    m, n = inp['m'], inp['n']
    T, steps = inp['T'] if T is None else T, inp['K'] if steps is None else steps
    key = (case, method, anneal, lanes, reserved, T, want, layout, x_layout, final_state, steps, reg, anneal_span)
    if x0 is None and key in _LAUNCHES:
        return _LAUNCHES[key]
    fp = params(uvs, case, method, anneal, lanes, reserved, steps)
    fp.reg, fp.anneal_span = reg, anneal_span
    ps = plant(uvs, case).to_struct()
    noise = first_trials(inp['noise'], T)[:, :steps]
    noise = cuda(noise.transpose(1, 2, 0) if layout == 'kct' else noise.transpose(1, 0, 2))
    q0 = cuda(first_trials(inp['q0'], T))
    start = None if inp['guess'] else cuda(first_trials(inp['x0'] if x0 is None else x0, T))
    # Every output is a buffer of this launch's, filled with NaN (-7 for the integers) beforehand: what the kernel does not store shows.
    layouts = {k: (x_layout or layout) if k == 'x' else layout for k in STREAMS}
    comps = {'x': m * n, 'err': m, 'q': n, 'f': m, 'dq': n}
    dev = {k: poisoned(T, steps, comps[k], layouts[k]) if k in want else None for k in STREAMS}
    dev.update(x_final=None, p_final=None)
    dev.update(poisoned_trials(T, final=(m, n) if final_state else None))
    flat = lambda t: uvs._lib.NULL_VIEW if t is None else uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))      # noqa: E731
    rc = uvs.engine.launch_closed_loop(fp, ps, T, flat(q0), uvs.engine.stream_view(noise, layout), flat(start),
                                       *(uvs.engine.stream_view(dev[k], layouts[k]) for k in STREAMS),
                                       dev['stats'].data_ptr(), dev['status'].data_ptr(), dev['k_done'].data_ptr(), flat(dev['x_final']), flat(dev['p_final']))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    assert (fp.reg, fp.anneal_span) == (reg, anneal_span)
    out = {'lanes': int(uvs.lib().uvs_rmckf_closed_loop_lanes(C.byref(fp), C.byref(ps), T)),
           'segments': int(uvs.lib().uvs_rmckf_closed_loop_segments(C.byref(fp), C.byref(ps), T)),
           'workspace': int(uvs.lib().uvs_rmckf_closed_loop_workspace_bytes(C.byref(fp), C.byref(ps), T)),
           'fallbacks': uvs.engine.hand_over_fallbacks(fp, ps, T)}
    for k in STREAMS:
        out[k] = None if dev[k] is None else np.ascontiguousarray(uvs.engine.as_tkc(dev[k], layouts[k]).cpu().numpy())
    for k in ('stats', 'status', 'k_done', 'x_final', 'p_final'):
        out[k] = None if dev[k] is None else dev[k].cpu().numpy()
    assert_everything_was_stored(out, key)
    if x0 is None:
        _LAUNCHES[key] = out
    return out


def assert_matches_c(out, ref, kept, worst, family, tag, tol=TOL, strict=False):
    """status and k_done on every trial, the streams the launch wrote (strict: err, q and x, all three) and the statistics on the trials
    `kept`, against oracle/c (`ref`: cs.c_reference)."""
    T = len(out['status'])
    tag = tuple(tag) + (family, T)
    assert np.array_equal(out['status'], ref['status'][:T]) and np.array_equal(out['k_done'], ref['k_done'][:T]), tag
    kept = [t for t in kept if t < T]
    alive = np.arange(ref['err'].shape[1])[None, :, None] < ref['k_done'][:T, None, None]
    for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X')):
        if out.get(key) is None:
            assert not strict, (key, 'not logged') + tag
            continue
        d = per_trial_rel(live(out, key), np.where(alive, ref[rk][:T], 0.0))[kept]
        worst.note(family, key, d.max())
        assert d.max() <= tol, (key, float(d.max()), kept[int(d.argmax())]) + tag
    ok = [t for t in kept if ref['status'][t] == 0]
    d = per_trial_rel(out['stats'][ok], ref['stats'][ok])
    worst.note(family, 'stats', d.max())
    assert d.max() <= tol, ('stats', float(d.max())) + tag


def assert_matches_block(out, block_of, trials, worst, family, tag, tol=TOL, strict=False):
    """The same against oracle/rmckf_block (numpy pinv; block_of(t): cs.block_reference) on the trials `trials`; f too where the launch
    wrote it.  strict: every one ran at least a step, logged err, q and x, and its statistics are compared whatever its status."""
    for t in trials:
        ref = block_of(t)
        k = ref['k_done']
        assert out['status'][t] == ref['status'] and out['k_done'][t] == k and (k > 0 or not strict), (t,) + tuple(tag)
        for key, rk in (('err', 'err'), ('q', 'q'), ('x', 'X'), ('f', 'f')):
            if out.get(key) is None or k == 0:
                assert not strict or key == 'f', (key, 'not logged', t) + tuple(tag)
                continue
            d = rel(out[key][t, :k], ref[rk])
            worst.note(family, key + ' (numpy)', d)
            assert d <= tol, (key, d, family, t) + tuple(tag)
        if strict or ref['status'] == 0:
            assert rel(out['stats'][t], ref['stats']) <= tol, (family, t) + tuple(tag)


def assert_twins(out, tag, twins=cs.TWINS):
    """One trial in the first, a middle and the last wavefront: identical bits in everything the launch wrote."""
    for t in twins[1:]:
        for key in STREAMS:
            if out.get(key) is not None:
                assert same_bits(live(out, key)[t], live(out, key)[twins[0]]), (key, t) + tuple(tag)
        for key in ('stats', 'status', 'k_done', 'x_final', 'p_final'):
            if out.get(key) is not None:
                assert same_bits(out[key][t], out[key][twins[0]]), (key, t) + tuple(tag)


def assert_same_launch(a, b, tag, keys=STREAMS + ('stats', 'status', 'k_done', 'x_final', 'p_final'), trials=None):
    """Two launches wrote the same bits (of the first len(b) trials, or of `trials`)."""
    sel = slice(0, len(b['status'])) if trials is None else trials
    for key in keys:
        if a.get(key) is None or b.get(key) is None:
            continue
        x, y = (live(o, key) if key in STREAMS else o[key] for o in (a, b))
        assert same_bits(x[sel], y[sel]), (key,) + tuple(tag)


# ---------------------------------------------------------------------------------------------- replay
def random_replay_case(m, n, K, T, seed):
    """Streams of T open-loop trials of K steps: f (T, K + 1, m), dq (T, K, n), x0 (T, m n), desired (m,)."""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(T, m, n)) * 20
    dq = rng.normal(size=(T, K, n)) * 0.3
    f = np.zeros((T, K + 1, m))
    f[:, 0] = rng.uniform(60, 200, (T, m))
    for k in range(K):
        f[:, k + 1] = f[:, k] + np.einsum('tmn,tn->tm', J, dq[:, k]) * 0.05 + rng.standard_t(2, size=(T, m))
    x0 = (J + rng.normal(size=J.shape)).reshape(T, m * n)
    return f, dq, x0, rng.uniform(80, 180, m)


def replay(uvs, fp, f, dq, x0, want, layout='kct'):
    """uvs_rmckf_replay_f64 on the streams f (T, K + 1, m), dq (T, K, n) and x0 (T, m n), into buffers that are filled with NaN (-7 for the
    integers) before the launch: a store the kernel leaves out shows.  numpy arrays in [trial][step][component] order."""
    import torch
    (T, K, n), m = dq.shape, f.shape[2]
    order = (1, 2, 0) if layout == 'kct' else (1, 0, 2)
    f_dev, dq_dev, x0_dev = cuda(f.transpose(order)), cuda(dq.transpose(order)), cuda(x0)
    comps = {'x': m * n, 'err': m, 'kappa': m, 'dqcmd': n}
    dev = {k: poisoned(T, K, comps[k], layout) if k in want else None for k in comps}
    dev.update(poisoned_trials(T, stats=False, final=(m, n)))
    flat = lambda t: uvs._lib.View(t.data_ptr(), t.stride(0), 0, t.stride(1))                # noqa: E731
    view = uvs.engine.stream_view
    rc = uvs.lib().uvs_rmckf_replay_f64(C.byref(fp), T, view(f_dev, layout), view(dq_dev, layout), flat(x0_dev), *(view(dev[k], layout) for k in comps),
                                        dev['status'].data_ptr(), dev['k_done'].data_ptr(), flat(dev['x_final']), flat(dev['p_final']),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    out = {k: None if dev[k] is None else np.ascontiguousarray(uvs.engine.as_tkc(dev[k], layout).cpu().numpy()) for k in comps}
    out.update({k: dev[k].cpu().numpy() for k in ('status', 'k_done', 'x_final', 'p_final')})
    for k, v in out.items():
        if v is not None:
            assert not (np.isnan(v).any() if v.dtype.kind == 'f' else (v == POISON_INT).any()), (k, 'not stored', want, layout, T)
    return out


def assert_replay(out, refs, worst, route, tag, skip=()):
    """Every trial of a replay launch against rmckf_block.run_replay (refs[t]) at REPLAY_GATES: the final state, and the streams it logged."""
    m, n = refs[0]['P_final'].shape[:2]
    for t, ref in enumerate(refs):
        for key, (rk, tol) in REPLAY_GATES.items():
            if out[key] is None or key in skip:
                continue
            a = out[key][t].reshape(m, n, n) if key == 'p_final' else out[key][t]
            d = rel(a, ref[rk][-1] if key == 'x_final' else ref[rk])
            worst.note(route, key, d)
            assert d <= tol, (key, d, t) + tuple(tag)


# ---------------------------------------------------------------------------------------------- the view contract (view_arena_common.py)
class Arenas:
    """The device buffers of one guarded call: every input and every output is a window of view kind `kind` (or the kind given for it) into an
    allocation of its own, guard bands on either side (view_arena_common.arena).  check(): no byte outside an output's window and no byte
    of an input differs from before the call."""

    def __init__(self, kind):
        self.kind, self.items = kind, {}

    def _add(self, name, T, K, comp, kind, dtype, fill, output):
        import view_arena_common as va
        self.items[name] = va.arena(T, K, comp, kind or self.kind, dtype=dtype, device='cuda', fill=fill) + (output,)
        return self.items[name][1]

    def input(self, name, a, kind=None, dtype=None):
        """The window holding `a`: (T, K, comp), (T, comp) -- no step axis -- or (T,); None stays None."""
        if a is None:
            return None
        a = np.asarray(a)
        a = a.reshape(len(a), 1, -1) if a.ndim < 3 else a
        return self._add(name, *a.shape, kind, dtype, a, False)

    def output(self, name, T, K, comp, kind=None, dtype=None):
        return self._add(name, T, K, comp, kind, dtype, None, True)

    def check(self, tag):
        import view_arena_common as va
        for name, (whole, window, before, output) in self.items.items():
            va.assert_only_the_window_changed(whole, window if output else None, before, (name, 'output' if output else 'input') + tuple(tag))

    def host(self, name):
        """An output window as a numpy array: (T, K, comp), or (T, comp) / (T,) for the kinds of input() without a step axis."""
        return None if name not in self.items else np.ascontiguousarray(self.items[name][1].cpu().numpy())


def stream(uvs, window):
    """uvs_view of a [trial][step][comp] window (NULL for None)."""
    return uvs._lib.NULL_VIEW if window is None else uvs._lib.View(window.data_ptr(), *window.stride())


def flat(uvs, window):
    """uvs_view of a per-trial window (T, 1, comp): no step stride."""
    return uvs._lib.NULL_VIEW if window is None else uvs._lib.View(window.data_ptr(), window.stride(0), 0, window.stride(2))


def guarded_closed(uvs, fp, ps, T, q0, noise, x0, want, kind, x_kind=None, final_state=True, trial=None, own_workspace=False, tag=()):
    """uvs_rmckf_closed_loop_ws_f64 -- with `trial` (a dict of numpy arrays: kernel_bw, gain, reg, fpi_threshold (T,), desired (T, m), source
    (T,) int32 over the len(q0) input trials) uvs_rmckf_closed_loop_grid_f64 -- with every input and every output in an arena of view kind
    `kind` (the X stream: x_kind).  The per-trial pointer arguments (stats, status, k_done, the arrays of `trial`) are dense by the header and
    get dense arenas.  own_workspace: the workspace is a byte arena of exactly uvs_rmckf_closed_loop_workspace_bytes.  After the launch: nothing
    outside an output window and no input byte changed (the workspace's guards included), everything was stored.  The dict of launch()."""
    import torch
    import view_arena_common as va
    m, n, K = fp.m, fp.n, fp.steps
    tag = tuple(tag) + (kind, x_kind, T, want)
    ar = Arenas(kind)
    v_q0, v_noise, v_x0 = ar.input('q0', q0), ar.input('noise', noise), ar.input('x0', x0)
    comps = {'x': m * n, 'err': m, 'q': n, 'f': m, 'dq': n}
    outs = {k: ar.output(k, T, K, comps[k], x_kind if k == 'x' else None) if k in want else None for k in STREAMS}
    stats = ar.output('stats', T, 1, 3, 'tkc')
    status, k_done = (ar.output(k, T, 1, 1, 'tkc', torch.int32) for k in ('status', 'k_done'))
    x_final = ar.output('x_final', T, 1, m * n) if final_state else None
    p_final = ar.output('p_final', T, 1, m * n * n) if final_state else None
    lib = uvs.lib()
    need = int(lib.uvs_rmckf_closed_loop_workspace_bytes(C.byref(fp), C.byref(ps), T))
    if own_workspace:
        assert need > 0, ('no workspace wanted',) + tag
        ws_whole, ws, ws_before = va.byte_arena(need, 'cuda')
        ws_ptr = ws.data_ptr()
    else:
        ws_ptr, need = uvs.engine.workspace(fp, ps, T, None)
    args = (flat(uvs, v_q0), stream(uvs, v_noise), flat(uvs, v_x0), *(stream(uvs, outs[k]) for k in STREAMS), stats.data_ptr(), status.data_ptr(),
            k_done.data_ptr(), flat(uvs, x_final), flat(uvs, p_final), ws_ptr, need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if trial is None:
        rc = lib.uvs_rmckf_closed_loop_ws_f64(C.byref(fp), C.byref(ps), T, *args)
    else:
        tp = uvs._lib.TrialParams(None, None, None, None, uvs._lib.NULL_VIEW, None)
        for key, a in trial.items():
            w = ar.input('trial ' + key, a, 'tkc', torch.int32 if key == 'source' else None)
            assert len(a) == T and w.is_contiguous()
            if key == 'desired':
                tp.desired = flat(uvs, w)
            else:
                setattr(tp, key, w.data_ptr())
        rc = lib.uvs_rmckf_closed_loop_grid_f64(C.byref(fp), C.byref(ps), T, C.byref(tp), *args)
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    ar.check(tag)
    out = {'lanes': int(lib.uvs_rmckf_closed_loop_lanes(C.byref(fp), C.byref(ps), T)),
           'segments': int(lib.uvs_rmckf_closed_loop_segments(C.byref(fp), C.byref(ps), T)), 'workspace': need, 'fallbacks': None}
    if own_workspace:
        va.assert_only_the_window_changed(ws_whole, ws, ws_before, ('workspace',) + tag)
        off = int(lib.uvs_rmckf_closed_loop_fallback_offset(C.byref(fp), C.byref(ps), T))
        assert 0 < off <= need - 4, (off, need) + tag
        out['fallbacks'] = int(ws[off:off + 4].view(torch.int32).item())
    for k in STREAMS:
        out[k] = ar.host(k)
    out['stats'] = ar.host('stats').reshape(T, 3)
    out['status'], out['k_done'] = ar.host('status').reshape(T), ar.host('k_done').reshape(T)
    out['x_final'] = ar.host('x_final').reshape(T, -1) if final_state else None
    out['p_final'] = ar.host('p_final').reshape(T, -1) if final_state else None
    assert_everything_was_stored(out, tag)
    return out


def guarded_launch(uvs, case, method, anneal, lanes=0, reserved=0, T=None, want=STREAMS, kind='kct', x_kind=None, final_state=True, steps=None,
                   x0=None, noise=None, own_workspace=False):
    """launch()'s call -- the same parameter block, the same first T trials of the case (noise, x0: overrides) -- through guarded_closed."""
    inp = cs.inputs(case)
    T, steps = inp['T'] if T is None else T, inp['K'] if steps is None else steps
    fp = params(uvs, case, method, anneal, lanes, reserved, steps)
    start = None if inp['guess'] else first_trials(inp['x0'] if x0 is None else x0, T)
    return guarded_closed(uvs, fp, plant(uvs, case).to_struct(), T, first_trials(inp['q0'], T), first_trials(inp['noise'] if noise is None else noise, T)[:, :steps],
                          start, want, kind, x_kind, final_state, own_workspace=own_workspace, tag=(case, method, anneal, lanes, reserved))


def guarded_replay(uvs, fp, f, dq, x0, want, kind, tag=()):
    """replay()'s call with f (K + 1 rows), dq and x0 in input arenas (NaN around them) and every output in an arena of view kind `kind`:
    nothing outside an output window and no input byte changed, everything was stored.  The dict of replay()."""
    import torch
    (T, K, n), m = dq.shape, f.shape[2]
    tag = tuple(tag) + (kind, T, want)
    ar = Arenas(kind)
    v_f, v_dq, v_x0 = ar.input('f', f), ar.input('dq', dq), ar.input('x0', x0)
    comps = {'x': m * n, 'err': m, 'kappa': m, 'dqcmd': n}
    outs = {k: ar.output(k, T, K, comps[k]) if k in want else None for k in comps}
    status, k_done = (ar.output(k, T, 1, 1, 'tkc', torch.int32) for k in ('status', 'k_done'))
    x_final, p_final = ar.output('x_final', T, 1, m * n), ar.output('p_final', T, 1, m * n * n)
    rc = uvs.lib().uvs_rmckf_replay_f64(C.byref(fp), T, stream(uvs, v_f), stream(uvs, v_dq), flat(uvs, v_x0), *(stream(uvs, outs[k]) for k in comps),
                                        status.data_ptr(), k_done.data_ptr(), flat(uvs, x_final), flat(uvs, p_final),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    uvs._lib.check(rc)
    torch.cuda.synchronize()
    ar.check(tag)
    out = {k: ar.host(k) for k in comps}
    out.update(status=ar.host('status').reshape(T), k_done=ar.host('k_done').reshape(T), x_final=ar.host('x_final').reshape(T, -1),
               p_final=ar.host('p_final').reshape(T, -1))
    for k, v in out.items():
        if v is not None:
            assert not (np.isnan(v).any() if v.dtype.kind == 'f' else (v == POISON_INT).any()), (k, 'not stored') + tag
    return out


def assert_same_replay(a, b, tag):
    """Two replay launches wrote the same bits."""
    for key in ('x', 'err', 'kappa', 'dqcmd', 'status', 'k_done', 'x_final', 'p_final'):
        assert (a[key] is None) == (b[key] is None) and (a[key] is None or same_bits(a[key], b[key])), (key,) + tuple(tag)


# ---------------------------------------------------------------------------------------------- single step
def step_recipe(rng, m, n, lanes, method, k0, scale, bw, anneal, steps, default_twin=False, **estimator):
    """`steps` steps from k0 of a bank of T = 64 // L + 3 filters (two blocks, the second ragged) on the inputs of tools/fuzz_step.py: every
    step starts from the ORACLE's state and command of the step before, and a filter that went non-finite starts afresh.  The first item
    is dict(T, gain, desired, x0); then per step dict(k, f, f_old, dq, X_in, P_in -- the state going in --, X, P, kappa, cmd --
    BlockFilter.step's and control_law's results at `estimator` (fpi_threshold, fpi_epoch_max, reg, anneal_span) --, finite (T,), and
    teeth: with default_twin, how far X is from a filter in the same state that steps with the default reg and anneal_span)."""
    from oracle import rmckf_block
    L = abs(lanes) or DEFAULT_LANES[(m, n)]
    T = 64 // L + 3
    gain = float(rng.uniform(0.05, 0.6))
    desired = 128 + 10 * rng.standard_normal(m)
    J = rng.standard_normal((T, m, n)) * 50
    x0 = J.reshape(T, m * n)
    fresh = lambda t: rmckf_block.BlockFilter(m, n, x0[t], method, bw, anneal, K_MAX, **estimator)     # noqa: E731
    filt = [fresh(t) for t in range(T)]
    f_old, dq = 128 + 20 * rng.standard_normal((T, m)), np.zeros((T, n))
    yield dict(T=T, gain=gain, desired=desired, x0=x0)
    for k in range(k0, k0 + steps):
        f = f_old + np.einsum('tmn,tn->tm', J, dq) * 0.05 + scale * rng.standard_t(2.0, size=(T, m))
        st = dict(k=k, f=f, f_old=f_old, dq=dq, X_in=np.stack([fl.X.ravel() for fl in filt]), P_in=np.stack([fl.P for fl in filt]),
                  X=np.zeros((T, m * n)), P=np.zeros((T, m, n, n)), cmd=np.zeros((T, n)), kappa=np.zeros((T, m)), finite=np.ones(T, bool), teeth=0.0)
        for t in range(T):
            twin = copy.deepcopy(filt[t]) if default_twin else None
            with np.errstate(all='ignore'):
                st['kappa'][t] = filt[t].step(f[t] - f_old[t], dq[t], k)
                st['finite'][t] = np.all(np.isfinite(filt[t].X))
            if not st['finite'][t]:                                                         # restart this filter on both sides
                filt[t] = fresh(t)
                filt[t].first = False
                continue
            st['X'][t], st['P'][t] = filt[t].X.ravel(), filt[t].P
            st['cmd'][t] = rmckf_block.control_law(filt[t].X, f[t] - desired, st['kappa'][t], gain)
            if default_twin:
                twin.reg, twin.anneal_span = cs.REG, cs.ANNEAL_SPAN
                with np.errstate(all='ignore'):
                    twin.step(f[t] - f_old[t], dq[t], k)
                st['teeth'] = max(st['teeth'], rel(twin.X, filt[t].X))
        yield st
        f_old, dq = f, np.clip(st['cmd'], -5, 5)


def assert_step(bank, st, desired, worst, routes, tag, fresh=False, put=cuda):
    """One step of step_recipe on the FilterBank `bank` -- from the oracle's state unless `fresh`, into poisoned outputs -- at STEP_GATES; the
    deviations go to every route of `routes` in `worst`.  put: how an input array gets onto the device (an arena's window, say)."""
    if not fresh:
        bank.X.copy_(cuda(st['X_in']))
        bank.P.copy_(cuda(st['P_in']).reshape(bank.P.shape))
    for buf in (bank.dq, bank.err, bank.kappa):
        buf.fill_(float('nan'))
    bank.status.fill_(POISON_INT)
    cmd, err, kappa, status = (o.cpu().numpy().copy() for o in bank.step(put(st['f']), put(st['f_old']), put(st['dq']), st['k']))
    got = {'X': bank.X.cpu().numpy(), 'P': bank.P.cpu().numpy().reshape(st['P'].shape), 'dq': cmd, 'kappa': kappa}
    assert same_bits(err, st['f'] - desired), ('err', st['k']) + tuple(tag)                 # one subtraction: the same bits
    assert np.array_equal(status == 0, st['finite']) and set(status.tolist()) <= {0, 1}, (st['k'], status.tolist()) + tuple(tag)
    for t in np.flatnonzero(st['finite']):
        for key, tol in STEP_GATES:
            d = rel(got[key][t], st['cmd' if key == 'dq' else key][t])
            for route in routes:
                worst.note(route, key, d)
            assert d <= tol, (key, d, st['k'], int(t)) + tuple(tag)


# ---------------------------------------------------------------------------------------------- the grid entry point (per-trial parameters)
def config(method, annealing=False):
    cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))         # the reference's configuration
    cfg['estimator']['method'] = method
    cfg['estimator']['estimator_params']['annealing'] = annealing
    return cfg


def setup(uvs, method, E, annealing=False, alpha=1.5):
    """Config, plan, start poses and noise (device, [K][m][E]) of E trials of the alpha cell, plant, and a parameter-block factory."""
    cfg = uvs.batch.load_config(config(method, annealing))
    plan = uvs.batch.plan_trials(cfg, [alpha], E)
    ex, p = cfg['experiments'], cfg['estimator']['estimator_params']
    K = len(uvs.engine.loop_clock(ex['dt'], ex['t_max']))
    noise = uvs.batch.device_noise(cfg, plan, 0, E, K).contiguous()
    ps = uvs.SyntheticPlant.ur10(ex['desired_f']).to_struct()

    def fp(lanes=0, kernel_bw=p['kernel_bw'], gain=ex['ibvs_gain'], desired=ex['desired_f'], segments=0, fpi_threshold=p['fpi_threshold']):
        f = uvs.engine.make_params(8, 6, method, kernel_bw, annealing, ex['dt'], ex['t_max'], gain, desired, True, lanes, None, fpi_threshold, p['fpi_epoch_max'])
        f.reserved = segments << 8
        return f
    return cfg, plan, cuda(plan.q_start), noise, ps, fp


def host(out, keys=STREAMS):
    return {k: out[k].cpu().numpy() for k in keys + ('stats', 'status', 'k_done') if out.get(k) is not None}


def assert_same_bits(got, lo, ref, what):
    """Trials [lo, lo + E) of the grid launch ``got`` against the uniform launch ``ref`` of E trials: status, k_done, stats and every stream up to k_done
    (rows at and after k_done are unspecified)."""
    E = len(ref['status'])
    assert np.array_equal(got['status'][lo:lo + E], ref['status']), what
    assert np.array_equal(got['k_done'][lo:lo + E], ref['k_done']), what
    assert set(ref['status'].tolist()) <= {0, 1}, what                              # no mark left behind
    ok = ref['status'] == 0
    assert np.array_equal(got['stats'][lo:lo + E][ok], ref['stats'][ok]), what      # (a FAILed trial's statistics are discarded)
    K = ref['err'].shape[0] if 'err' in ref else 0
    logged = np.arange(K)[:, None] < ref['k_done'][None, :]                         # (K, E)
    for key in STREAMS:
        if key in ref:
            a, b = got[key][:, :, lo:lo + E], ref[key]
            same = (a == b) | (np.isnan(a) & np.isnan(b))
            assert same[np.broadcast_to(logged[:, None, :], same.shape)].all(), (what, key)
