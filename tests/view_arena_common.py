"""Arenas for the view contract of libuvs_rmckf (tests/test_gpu_view_bounds.py, tests/test_view_arena_host.py): every stream of an entry point
is a strided view, and a launch stores inside the views of its outputs and reads inside the views of its inputs, whichever store path the
launcher picks from the strides.

arena() carves a [trial][step][comp] window out of ONE allocation with at least GUARD_BYTES on either side -- the largest burst a single
wavefront issues on any path is the record path's 32 records of 384 B = 12 KB, so a whole wavefront's overshoot in either direction stays
inside our own allocation -- and assert_only_the_window_changed() compares every byte the window does not address with a copy taken before
the launch.  The kinds are named for the launcher predicate they flip; closed_x_path / wide_x_path / replay_path restate those predicates
(the library has no query for the store path) and CELLS lists which (kind, T, lanes, method) reaches which (entry point, path, raggedness).

No GPU code here; torch is imported inside the functions and everything works on CPU tensors."""
import collections
import itertools

import numpy as np

GUARD_BYTES = 16384
POISON_INT = -7                                                   # gpu_harness.POISON_INT (asserted equal by the host test)
KINDS = ('kct', 'kct_pitch_even', 'kct_pitch_odd', 'kct_base8', 'ktc', 'ktc_slice', 'ktc_base8', 'tkc', 'tkc_slice')
Geometry = collections.namedtuple('Geometry', 'offset st sk sc numel')     # in elements; offset: of the window's first element in `whole`


def guard_elements(itemsize):
    return -(-GUARD_BYTES // itemsize)


def geometry(T, K, comp, kind, itemsize=8):
    """Where the [trial][step][comp] window of `kind` lies in its allocation, in elements: the offset of element (0, 0, 0), the trial, step
    and component strides, and the size of the allocation (guards included)."""
    g = guard_elements(itemsize)
    if kind in ('kct', 'kct_base8'):                              # dense trial-fastest rows; base8: the base off by one element
        off, st, sk, sc, body = int(kind == 'kct_base8'), 1, comp * T, T, K * comp * T
    elif kind in ('kct_pitch_even', 'kct_pitch_odd'):             # rows pitched at T + 6 / T + 5, one extra step row
        pitch = T + (6 if kind == 'kct_pitch_even' else 5)
        off, st, sk, sc, body = 0, 1, comp * pitch, pitch, (K + 1) * comp * pitch
    elif kind in ('ktc', 'ktc_base8'):                            # dense records
        off, st, sk, sc, body = int(kind == 'ktc_base8'), comp, T * comp, 1, K * T * comp
    elif kind == 'ktc_slice':                                     # records of trials [3, 3 + T) of T + 8
        off, st, sk, sc, body = 3 * comp, comp, (T + 8) * comp, 1, K * (T + 8) * comp
    elif kind == 'tkc':
        off, st, sk, sc, body = 0, K * comp, comp, 1, T * K * comp
    elif kind == 'tkc_slice':                                     # trials [2, 2 + T) and K of K + 1 rows of [T + 4][K + 1][comp]
        off, st, sk, sc, body = 2 * (K + 1) * comp, (K + 1) * comp, comp, 1, (T + 4) * (K + 1) * comp
    else:
        raise ValueError(f'unknown view kind {kind!r}; known: {KINDS}')
    return Geometry(g + off, st, sk, sc, g + body + (off if kind.endswith('base8') else 0) + g)


def _poison(dtype):
    return float('nan') if dtype.is_floating_point else POISON_INT


def arena(T, K, comp, kind, dtype=None, device='cpu', fill=None):
    """(whole, window, before): one allocation filled with NaN (integers: POISON_INT), the [trial][step][comp] as_strided window of `kind`
    into it -- holding `fill` (T, K, comp), an input, when given -- and a clone of `whole` taken after the fill."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    geo = geometry(T, K, comp, kind, torch.empty((), dtype=dtype).element_size())
    whole = torch.full((geo.numel,), _poison(dtype), dtype=dtype, device=device)
    assert whole.data_ptr() % 16 == 0, 'the allocator hands out 16-byte aligned memory: the kinds count on it'
    window = whole.as_strided((T, K, comp), (geo.st, geo.sk, geo.sc), geo.offset)
    if fill is not None:
        window.copy_(torch.as_tensor(np.array(fill, order='C')).reshape(T, K, comp).to(device=device, dtype=dtype))     # (a copy: the inputs are read-only)
    return whole, window, whole.clone()


def byte_arena(nbytes, device='cpu', align=256):
    """(whole, window, before) of uint8: `nbytes` bytes at an `align`-aligned address between two guards filled with 0xA5."""
    import torch
    whole = torch.full((GUARD_BYTES + align + nbytes + GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=device)
    lead = GUARD_BYTES + (-(whole.data_ptr() + GUARD_BYTES)) % align
    window = whole[lead:lead + nbytes]
    assert window.data_ptr() % align == 0
    return whole, window, whole.clone()


def _as_int(t):
    import torch
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def strays(whole, window, before):
    """Element offsets into `whole` (sorted, a numpy array) of what differs from `before`, compared as integers, outside `window`
    (None: an input arena, the whole buffer)."""
    import torch
    changed = _as_int(whole) != _as_int(before)
    if window is not None:
        inside = torch.zeros(whole.numel(), dtype=torch.bool, device=whole.device)
        inside.as_strided(window.shape, window.stride(), window.storage_offset() - whole.storage_offset()).fill_(True)
        changed &= ~inside
    return torch.nonzero(changed).flatten().cpu().numpy()


def assert_only_the_window_changed(whole, window, before, tag):
    """Every byte of `whole` that `window` does not address equals `before` (window None: every byte)."""
    idx = strays(whole, window, before)
    assert idx.size == 0, (f'{idx.size} elements changed outside the view' if window is not None else f'{idx.size} elements of an input changed',
                           'first offsets into the allocation', idx[:8].tolist(), 'last', int(idx[-1]), 'window at',
                           None if window is None else (window.storage_offset(), tuple(window.stride()), tuple(window.shape))) + tuple(tag)


# ---------------------------------------------------------------------------------------------- the launchers' predicates, restated
def _facts(view):
    """(byte offset of the base modulo 16, st, sk, sc) of a Geometry (in an allocation that starts 16-byte aligned, 8-byte elements) or a tensor
    in [trial][step][comp] order."""
    if isinstance(view, Geometry):
        return (view.offset * 8) % 16, view.st, view.sk, view.sc
    return view.data_ptr() % 16, view.stride(0), view.stride(1), view.stride(2)


def closed_x_path(m, n, lanes_used, method, plant_kind, per_trial, strict, T, view):
    """The X-store instantiation of a closed-loop launch: 'records' | 'pairs' | 'plain'.  csrc/tu_closed_tuned.inc, launch2: lines 40-55 (the
    XREC / XPAIR instantiations exist at (8,6), two lanes, KF / IMCC-KF, DH plant, uniform parameters; `aligned` line 41, `records` line 42,
    `pairs` line 46), after line 16-22 (UVS_OPT_STRICT_PINV takes the CERT instantiation, which has neither) -- the segmented kernels (lines
    25-35) are RMCKF's and MCKF's, which have neither anyway.  lanes_used: what uvs_rmckf_closed_loop_lanes answers (the four-lane small-batch
    kernels of lanes_per_filter = 0 are EMU2 instantiations: plain)."""
    base16, st, sk, sc = _facts(view)
    if not ((m, n, lanes_used) == (8, 6, 2) and method in ('KF', 'IMCCKF') and plant_kind == 'dh' and not per_trial and not strict):
        return 'plain'
    aligned = base16 == 0 and sk % 2 == 0
    if aligned and sc == 1 and st == m * n:
        return 'records'
    if aligned and st == 1 and sc % 2 == 0 and T % 2 == 0:
        return 'pairs'
    return 'plain'


def wide_x_path(L, T, view):
    """(32,7): 'records' | 'plain'.  csrc/tu_closed_wide.hip, launch_wide, line 11 (`rec`); closed_wide (lines 28-29) instantiates L = 8 and
    16, L = 32 is the generic template (uvs_rmckf.hip, plan_closed_loop: Route::kWide for L 8 / 16 only)."""
    base16, st, sk, sc = _facts(view)
    return 'records' if L in (8, 16) and sc == 1 and st == 32 * 7 and T % (64 // L) == 0 and base16 == 0 and sk % 2 == 0 else 'plain'


def replay_path(method, lanes, want, T, x_view, err_view, shape=(8, 6)):
    """uvs_rmckf_replay_f64 (uvs_rmckf.hip, lines 402-417) and csrc/tu_replay_tuned.hip: 'records' (replay_rows, `rec`, lines 35-39) |
    'rowgroups' (lines 40-43: KF / RMCKF at lanes_per_filter 0) | 'lanegroups' (lines 44-46) | 'control' (replay_rows_cmd, lines 26-31: KF /
    RMCKF, lanes_per_filter 0, X, err and dqcmd wanted) -- and what is left: 'twolane' (replay_tuned, lines 11-19: L = 2, which is what
    lanes_per_filter 0 resolves to at both shapes) | 'generic'."""
    xo, eo, cmd = 'x' in want, 'err' in want, 'dqcmd' in want
    if shape == (8, 6) and not cmd and lanes in (0, 4):
        if xo and eo and T % 16 == 0:
            (xb, xt, xk, xc), (eb, et, ek, ec) = _facts(x_view), _facts(err_view)
            if xc == 1 and xt == 48 and ec == 1 and et == 8 and xk % 2 == 0 and ek % 2 == 0 and xb == 0 and eb == 0:
                return 'records'
        return 'rowgroups' if lanes == 0 and method in ('GMCKF', 'KF') else 'lanegroups'
    if shape == (8, 6) and cmd and xo and eo and lanes == 0 and method in ('GMCKF', 'KF'):
        return 'control'
    return 'twolane' if lanes in (0, 2) else 'generic'


def raggedness(T, per_wavefront):
    """'whole' wavefronts | one 'single' partial wavefront | a 'ragged_even' / 'ragged_odd' last wavefront after whole ones, by T's parity."""
    if T % per_wavefront == 0:
        return 'whole'
    return 'single' if T < per_wavefront else ('ragged_odd' if T % 2 else 'ragged_even')


# ---------------------------------------------------------------------------------------------- the coverage table
CLOSED_K, WIDE_K, REPLAY_K = 60, 80, 12                            # steps of the 'dh86' and 'wide' cases (closed_shapes_common) and of the replays
CLOSED_T, WIDE_T, REPLAY_T = (64, 70, 69, 2), (4, 8), (48, 64, 35, 65)
METHODS = ('GMCKF', 'KF', 'IMCCKF', 'MCKF')
XREC = ('KF', 'IMCCKF')                                           # the estimators with XREC / XPAIR instantiations
WIDE_METHODS = ('GMCKF', 'KF', 'IMCCKF')                          # closed_wide has no MCKF kernel
WIDE_KINDS = ('kct_pitch_odd', 'ktc_slice', 'ktc_base8', 'tkc_slice')
REPLAY_KINDS = ('kct', 'kct_pitch_odd', 'ktc', 'ktc_slice', 'ktc_base8', 'tkc_slice')
REPLAY_WANTS = (('x', 'err'), ('x',), ('x', 'err', 'kappa', 'dqcmd'))
_REC_KINDS, _PAIR_KINDS = ('ktc', 'ktc_slice'), ('kct', 'kct_pitch_even')
_PLAIN_KINDS = tuple(k for k in KINDS if k not in _REC_KINDS + _PAIR_KINDS)


def _x(*axes):
    return [c for c in itertools.product(*((a,) if isinstance(a, (str, int)) else a for a in axes))]


# (entry point, path, raggedness) -> [(kind, T, lanes_per_filter, method)] ('replay': (kind, T, lanes_per_filter, method, want)): the
# combinations tests/test_gpu_view_bounds.py runs in that cell; `kind` is the kind of the X stream (replay: of X and err).
# 'closed': 'dh86', 32 trials per two-lane wavefront (lanes_per_filter 0: the four-lane small-batch kernels, 16): T = 64 whole, 70 ragged_even,
# 69 ragged_odd, 2 single.  'wide': trials per wavefront 64 / L; 'replay': (8,6), against the 16 trials of a four-lane wavefront.
# Cells the launchers cannot reach: ('closed', 'pairs', 'ragged_odd') -- XPAIR needs an even T; ('wide', 'records', anything but 'whole') and
# ('replay', 'records', anything but 'whole') -- `rec` needs whole wavefronts.
CELLS = {}
for _T, _rag in zip(CLOSED_T, ('whole', 'ragged_even', 'ragged_odd', 'single')):
    CELLS[('closed', 'records', _rag)] = _x(_REC_KINDS, _T, 2, XREC)
    if _T % 2 == 0:
        CELLS[('closed', 'pairs', _rag)] = _x(_PAIR_KINDS, _T, 2, XREC)
    CELLS[('closed', 'plain', _rag)] = (_x(_PLAIN_KINDS, _T, 2, XREC) + (_x(_PAIR_KINDS, _T, 2, XREC) if _T % 2 else []) +
                                       _x(KINDS, _T, 2, ('GMCKF', 'MCKF')) + _x(KINDS, _T, 0, METHODS))
CELLS[('wide', 'records', 'whole')] = _x('ktc_slice', 8, 8, WIDE_METHODS) + _x('ktc_slice', WIDE_T, 16, WIDE_METHODS)
CELLS[('wide', 'plain', 'whole')] = (_x(('kct_pitch_odd', 'ktc_base8', 'tkc_slice'), 8, 8, WIDE_METHODS) +
                                     _x(('kct_pitch_odd', 'ktc_base8', 'tkc_slice'), WIDE_T, 16, WIDE_METHODS) + _x(WIDE_KINDS, WIDE_T, 32, WIDE_METHODS))
CELLS[('wide', 'plain', 'single')] = _x(WIDE_KINDS, 4, 8, WIDE_METHODS)
_FULL = REPLAY_WANTS[2]
for _Ts, _rag in (((48, 64), 'whole'), ((35, 65), 'ragged_odd')):
    _nocmd = REPLAY_WANTS[:2]
    if _rag == 'whole':
        CELLS[('replay', 'records', _rag)] = _x(_REC_KINDS, _Ts, (0, 4), METHODS, (REPLAY_WANTS[0],))
        _rest = [k for k in REPLAY_KINDS if k not in _REC_KINDS]
        CELLS[('replay', 'rowgroups', _rag)] = _x(_rest, _Ts, 0, ('GMCKF', 'KF'), (REPLAY_WANTS[0],)) + _x(REPLAY_KINDS, _Ts, 0, ('GMCKF', 'KF'), (REPLAY_WANTS[1],))
        CELLS[('replay', 'lanegroups', _rag)] = (_x(_rest, _Ts, 0, ('IMCCKF', 'MCKF'), (REPLAY_WANTS[0],)) + _x(REPLAY_KINDS, _Ts, 0, ('IMCCKF', 'MCKF'), (REPLAY_WANTS[1],)) +
                                                 _x(_rest, _Ts, 4, METHODS, (REPLAY_WANTS[0],)) + _x(REPLAY_KINDS, _Ts, 4, METHODS, (REPLAY_WANTS[1],)))
    else:
        CELLS[('replay', 'rowgroups', _rag)] = _x(REPLAY_KINDS, _Ts, 0, ('GMCKF', 'KF'), _nocmd)
        CELLS[('replay', 'lanegroups', _rag)] = _x(REPLAY_KINDS, _Ts, 0, ('IMCCKF', 'MCKF'), _nocmd) + _x(REPLAY_KINDS, _Ts, 4, METHODS, _nocmd)
    CELLS[('replay', 'control', _rag)] = _x(REPLAY_KINDS, _Ts, 0, ('GMCKF', 'KF'), (_FULL,))
    CELLS[('replay', 'twolane', _rag)] = _x(REPLAY_KINDS, _Ts, 0, ('IMCCKF', 'MCKF'), (_FULL,)) + _x(REPLAY_KINDS, _Ts, 2, METHODS, REPLAY_WANTS)
    CELLS[('replay', 'generic', _rag)] = _x(REPLAY_KINDS, _Ts, 4, METHODS, (_FULL,))
UNREACHABLE = ([('closed', 'pairs', 'ragged_odd')] + [('wide', 'records', r) for r in ('ragged_even', 'ragged_odd', 'single')] +
               [('replay', 'records', r) for r in ('ragged_even', 'ragged_odd', 'single')])


def lanes_used(entry, lanes):
    """What lanes_per_filter resolves to on the closed-loop routes of CELLS: 'closed' 0 -> the four-lane small-batch kernels."""
    return (lanes or 4) if entry == 'closed' else lanes


def predicted(entry, combo):
    """(path, raggedness) the predictors give the combination `combo` of the entry point `entry`."""
    kind, T, lanes, method = combo[:4]
    if entry == 'closed':
        L = lanes_used(entry, lanes)
        return closed_x_path(8, 6, L, method, 'dh', False, False, T, geometry(T, CLOSED_K, 48, kind)), raggedness(T, 64 // L)
    if entry == 'wide':
        return wide_x_path(lanes, T, geometry(T, WIDE_K, 224, kind)), raggedness(T, 64 // lanes)
    path = replay_path(method, lanes, combo[4], T, geometry(T, REPLAY_K, 48, kind), geometry(T, REPLAY_K, 8, kind))
    return path, raggedness(T, 16)


def universe(entry):
    """Every combination of the issue's axes for an entry point: CELLS holds each exactly once."""
    if entry == 'closed':
        return _x(KINDS, CLOSED_T, (2, 0), METHODS)
    if entry == 'wide':
        return _x(WIDE_KINDS, WIDE_T, (8, 16, 32), WIDE_METHODS)
    return _x(REPLAY_KINDS, REPLAY_T, (0, 2, 4), METHODS, REPLAY_WANTS)


def cells_of(entry):
    return [(key[1], key[2], combo) for key, combos in CELLS.items() if key[0] == entry for combo in combos]


# ---------------------------------------------------------------------------------------------- FAIL placement (NaN noise samples)
# trial -> the step at which its noise turns NaN: one trial mid-wavefront at step 17, one at step 0 (k_done = 0, nothing logged), and every
# trial of the ragged last two-lane wavefront of T = 70 at step 2 (the wavefront-wide exit)
FAIL_PLAN = {10: 17, 40: 0, 64: 2, 65: 2, 66: 2, 67: 2, 68: 2, 69: 2}


def inject_fails(noise, plan=FAIL_PLAN):
    """A copy of noise (T, K, m) with one NaN sample per planned trial: the trial FAILs at that step with k_done = step."""
    noise = np.array(noise)
    for t, k in plan.items():
        noise[t, k, (t + k) % noise.shape[2]] = np.nan
    return noise
