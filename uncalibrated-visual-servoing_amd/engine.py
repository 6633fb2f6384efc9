"""Typed Python front of the C ABI: builds ``uvs_filter_params``, owns nothing but torch tensors on the GPU,
and launches the HIP kernels on torch's current stream.  No numpy arithmetic of the estimator lives here --
if the library or the GPU is missing these calls raise.

Buffer layout.  Per-step streams are allocated *trial-fastest*: ``[step][component][trial]`` (``layout='kct'``).
With one filter per lane (lanes_per_filter = 1) consecutive lanes then touch consecutive doubles, so every
wavefront load/store of a stream component is one contiguous 512-byte segment.  ``layout='ktc'``
(``[step][trial][component]``) suits the variants where several lanes share a filter; ``'tkc'`` is the
reference's per-trial record order.  The kernels take strides, so all three work everywhere.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FilterParams, View, NULL_VIEW

METHOD_CODES = {'ANALYTICAL': 1, 'KF': 2, 'MCKF': 3, 'IMCCKF': 4, 'GMCKF': 5}
REG = 0.001 ** 2            # experiment.py:280
ANNEAL_SPAN = 100.0         # experiment.py:271


def loop_clock(t_s, t_max):
    """Times at which the reference loop body runs: the clock starts at t_s (ur10_simulation.py:57) and advances by
    t_s per iteration while t < t_max (experiment.py:125), accumulated in floating point exactly like the simulator stub."""
    ts, t = [], 0.0 + t_s
    while t < t_max:
        ts.append(t)
        t += t_s
    return np.array(ts)


def make_params(m, n, method='GMCKF', kernel_bw=10.0, annealing=False, t_s=0.05, t_max=15.0, gain=0.2, desired=None,
                initial_guess=True, lanes=0, steps=None, fpi_threshold=0.1, fpi_epoch_max=1000):
    code = METHOD_CODES[method] if isinstance(method, str) else int(getattr(method, 'value', method))
    fp = FilterParams()
    fp.m, fp.n, fp.method, fp.annealing = m, n, code, int(bool(annealing))
    fp.k_max = int(t_max / t_s)                                     # experiment.py:120
    fp.steps = len(loop_clock(t_s, t_max)) if steps is None else int(steps)
    fp.initial_guess, fp.lanes_per_filter = int(bool(initial_guess)), int(lanes)
    fp.kernel_bw, fp.anneal_span, fp.gain, fp.dt, fp.reg = float(kernel_bw), ANNEAL_SPAN, float(gain), float(t_s), REG
    fp.fpi_threshold, fp.fpi_epoch_max = float(fpi_threshold), int(fpi_epoch_max)
    if m > _lib.UVS_MAX_M or n > _lib.UVS_MAX_N:
        raise ValueError('(m, n) exceeds UVS_MAX_M / UVS_MAX_N')
    if desired is not None:
        for i, v in enumerate(np.asarray(desired, float).ravel()):
            fp.desired[i] = v
    return fp


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.UvsLibraryError('no GPU visible: the RMCKF path runs only on the HIP library (no CPU fallback)')
    return torch


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


_DIMS = {'kct': (2, 0, 1), 'ktc': (1, 0, 2), 'tkc': (0, 1, 2)}    # layout -> the tensor axes that play (trial, step, comp): THE layout table


def _shape(T, K, comp, layout):
    """Tensor shape of a [trial][step][comp] stream in ``layout``."""
    return tuple(size for _, size in sorted(zip(_DIMS[layout], (T, K, comp))))


def current_device(device=None):
    """``device`` ('cuda', 'cuda:1', a torch.device; None = 'cuda') as an INDEXED torch.device: one without an index names the current device."""
    torch = _torch()
    dev = torch.device('cuda' if device is None else device)
    return dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())


def alloc_stream(T, K, comp, layout='kct', device='cuda', zero=False):
    """fp64 tensor for a [trial][step][comp] stream in the requested physical layout.

    Experiment knob UVS_ROW_PAD=<trials>: pitch trial-fastest rows at T + pad (the [:, :, :T] view is returned; every entry point takes
    strides).  With dense rows of a power-of-two T every (step, component) row starts in the same 256-byte slot of the address interleave
    and two of the eight slots drain 17 % slower on MI355X; walking the slots from row to row measured -1 % (config 3), -2 % (IMCC-KF),
    +/-0 (headline) and +8 % (replay) on one box -- DESIGN.md appendix A.1 -- so dense rows stay the default."""
    torch = _torch()
    pad = int(os.environ.get('UVS_ROW_PAD', '0')) if layout == 'kct' else 0
    tensor = (torch.zeros if zero else torch.empty)(_shape(T + pad, K, comp, layout), dtype=torch.float64, device=device)
    return tensor.narrow(_DIMS[layout][0], 0, T) if pad else tensor


def stream_view(tensor, layout='kct'):
    return NULL_VIEW if tensor is None else _lib.view_of(tensor, _DIMS[layout])


def _flat(tensor):
    """uvs_view of a per-trial (T, comp) tensor (no step axis), NULL_VIEW for None."""
    return NULL_VIEW if tensor is None else View(tensor.data_ptr(), tensor.stride(0), 0, tensor.stride(1))


def as_tkc(tensor, layout='kct'):
    """Logical [trial][step][comp] view (no copy) of a stream tensor."""
    return tensor.permute(_DIMS[layout])


def supported_lanes(m, n):
    buf = (C.c_int32 * 16)()
    cnt = _lib.lib().uvs_supported_lanes(m, n, buf, 16)
    return [buf[i] for i in range(min(cnt, 16))]


_WORKSPACES = {}


def workspace(fp, plant_struct, T, device):
    """(pointer, bytes) of the scratch buffer uvs_rmckf_closed_loop_ws_f64 wants for this launch -- (None, 0) when it wants none.  One
    buffer per (indexed) device and stream, grown on demand and kept: the library allocates nothing itself."""
    need = int(_lib.lib().uvs_rmckf_closed_loop_workspace_bytes(C.byref(fp), C.byref(plant_struct), T))
    if need == 0:
        return None, 0
    torch = _torch()
    device = current_device(device)                                # 'cuda', None and 'cuda:0' are one workspace
    key = (device, torch.cuda.current_stream().cuda_stream)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < need:
        buf = _WORKSPACES[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf.data_ptr(), need


def hand_over_fallbacks(fp, plant_struct, T, device=None):
    """Work items of the LAST segmented launch of this (fp, plant, T) on this stream that ran out their spin budget and recomputed their trial
    from step 0 (uvs_rmckf_closed_loop_fallback_offset): 0 on a healthy launch, None when the launch is not segmented.  Synchronises."""
    torch = _torch()
    off = int(_lib.lib().uvs_rmckf_closed_loop_fallback_offset(C.byref(fp), C.byref(plant_struct), T))
    if off == 0:
        return None
    buf = _WORKSPACES.get((current_device(device), torch.cuda.current_stream().cuda_stream))
    if buf is None:
        return None
    return int(buf[off:off + 4].view(torch.int32).item())


def launch_closed_loop(fp, plant_struct, T, *args, device=None):
    """uvs_rmckf_closed_loop_ws_f64 on torch's current stream with this process's cached workspace: ``args`` are the views / pointers of
    uvs_rmckf_closed_loop_f64 between ``T`` and ``stream``, in the header's order.  Returns the library's return code."""
    ws, ws_bytes = workspace(fp, plant_struct, T, device)
    return _lib.lib().uvs_rmckf_closed_loop_ws_f64(C.byref(fp), C.byref(plant_struct), T, *args, ws, ws_bytes, _stream())


TRIAL_PARAM_KEYS = ('kernel_bw', 'gain', 'reg', 'fpi_threshold', 'desired', 'source')


def trial_params_struct(trial_params, T, m, device):
    """uvs_trial_params over the tensors of ``trial_params`` (closed_loop's argument of that name), after checking their dtypes, shapes and device."""
    import torch
    unknown = set(trial_params) - set(TRIAL_PARAM_KEYS)
    if unknown:
        raise ValueError(f'trial_params: unknown keys {sorted(unknown)}; known: {TRIAL_PARAM_KEYS}')
    tp = _lib.TrialParams(None, None, None, None, NULL_VIEW, None)
    for key, value in trial_params.items():
        if value is None:
            continue
        shape, dtype = ((T, m), torch.float64) if key == 'desired' else ((T,), torch.int32 if key == 'source' else torch.float64)
        if tuple(value.shape) != shape or value.dtype != dtype or value.device != device or not value.is_contiguous():
            raise ValueError(f'trial_params[{key!r}]: a contiguous {dtype} tensor of shape {shape} on {device} is needed, got '
                             f'{value.dtype} {tuple(value.shape)} on {value.device}')
        if key == 'desired':
            tp.desired = View(value.data_ptr(), value.stride(0), 0, value.stride(1))
        else:
            setattr(tp, key, value.data_ptr())
    return tp


def _outputs(fp, T, dev, head, want, layout, head_layout, reuse, final_state=None):
    """The dict a closed-loop launch of T trials writes: the per-step streams ``head`` ('x' or 'j', m*n per step, in ``head_layout``), 'err', 'q', 'f', 'dq'
    (in ``layout``; None unless in ``want``), the per-trial 'stats', 'status', 'k_done' and -- unless ``final_state`` is None -- 'x_final' / 'p_final'
    (None when False).  ``reuse``: a dict this function returned for at least T trials, narrowed to T instead of allocating."""
    torch = _torch()
    K, m, n = fp.steps, fp.m, fp.n
    out = {}
    for key, comp in ((head, m * n), ('err', m), ('q', n), ('f', m), ('dq', n)):
        lay = head_layout if key == head else layout
        if key not in want:
            out[key] = None
        elif reuse is not None:
            out[key] = reuse[key].narrow(_DIMS[lay][0], 0, T)
        else:
            out[key] = alloc_stream(T, K, comp, lay, dev)          # rows at and after k_done are unspecified
    for key, shape, dtype in (('stats', (T, 3), torch.float64), ('status', (T,), torch.int32), ('k_done', (T,), torch.int32)):
        out[key] = reuse[key][:T] if reuse is not None else torch.zeros(shape, dtype=dtype, device=dev)
    if final_state is not None:
        out['x_final'] = torch.empty((T, m * n), dtype=torch.float64, device=dev) if final_state else None
        out['p_final'] = torch.empty((T, m * n * n), dtype=torch.float64, device=dev) if final_state else None
    return out


def closed_loop(fp, plant_struct, q_start, noise=None, x0=None, want=('x', 'err', 'q'), layout='kct', final_state=False, x_layout=None, reuse=None,
                trial_params=None):
    """Launch T closed-loop trials.  ``q_start``: (T, n) cuda tensor; ``noise``: stream tensor in ``layout`` or None;
    ``x0``: (T, m*n) cuda tensor when fp.initial_guess == 0.  Returns a dict of output tensors (streams in ``layout``).
    ``x_layout``: another layout for the X stream alone.  The default -- X trial-fastest like every stream -- is what the kernels are tuned for (since round 6
    the (8,6) KF / IMCC-KF kernels write it as 16-byte pairs of consecutive trials when T is even).  'ktc' (per-trial records) is faster still for KF on
    batches above 16 384 trials (two lanes per filter; bench.py `other_estimators.KF.x_records`: up to - 10 %, box-dependent) and level with the default for
    IMCC-KF.  Only there: RMCKF and MCKF keep their strided stores whatever the view, and smaller batches run on the four-lane kernels, for which 'ktc' is an
    uncoalesced, slower path.
    ``reuse``: the dict an earlier call with at least as many trials returned -- its tensors are written again ([..., :T] of the streams,
    [:T] of the per-trial arrays) instead of allocating new ones (batch.run_sweep: cell after cell through one set of buffers).
    ``trial_params``: per-trial estimator parameters, ONE launch for a whole hyperparameter grid (uvs_rmckf_closed_loop_grid_f64; (8,6), DH plant, two
    lanes per filter): a dict with any of 'kernel_bw', 'gain', 'reg', 'fpi_threshold' ((T,) fp64 cuda tensors), 'desired' ((T, m)) and 'source' ((T,)
    int32: trial t reads q_start / noise / x0 of trial source[t]; its values must index the trials those tensors hold -- they are not checked on the
    device).  With 'source' T is len(source) and q_start / noise / x0 may hold fewer trials.  A trial's results are bit-identical to those of a uniform
    launch with its values.  None (the default) is the uniform call."""
    x_layout = x_layout or layout
    torch = _torch()
    T = q_start.shape[0]
    if trial_params is not None and trial_params.get('source') is not None:
        T = trial_params['source'].shape[0]
    dev = q_start.device
    out = _outputs(fp, T, dev, 'x', want, layout, x_layout, reuse, final_state)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)           # around the launch only:
    ws, ws_bytes = workspace(fp, plant_struct, T, dev)
    args = (_flat(q_start), stream_view(noise, layout), _flat(x0),
            stream_view(out['x'], x_layout), stream_view(out['err'], layout), stream_view(out['q'], layout),
            stream_view(out['f'], layout), stream_view(out['dq'], layout),
            out['stats'].data_ptr(), out['status'].data_ptr(), out['k_done'].data_ptr(),
            _flat(out['x_final']), _flat(out['p_final']), ws, ws_bytes, _stream())
    tp = trial_params_struct(trial_params, T, fp.m, dev) if trial_params is not None else None
    start.record()                                                                                     # allocation and the workspace lookup are not kernel time
    if tp is not None:
        rc = _lib.lib().uvs_rmckf_closed_loop_grid_f64(C.byref(fp), C.byref(plant_struct), T, C.byref(tp), *args)
    else:
        rc = _lib.lib().uvs_rmckf_closed_loop_ws_f64(C.byref(fp), C.byref(plant_struct), T, *args)
    stop.record()
    _lib.check(rc)
    out['events'] = (start, stop)
    return out


def analytical_closed_loop(fp, plant_struct, q_start, noise=None, want=('err', 'q'), layout='kct', reuse=None):
    """Launch T closed-loop trials of the calibrated IBVS baseline (Method.ANALYTICAL, uvs_analytical_closed_loop_f64): the interaction matrix
    is computed from the plant at every step instead of estimated.  Arguments and the returned dict as for ``closed_loop``, with the stream
    ``'j'`` (J_feature the control law used, m*n per step) in place of ``'x'``; ``fp.method`` must be ANALYTICAL (make_params(..., 'ANALYTICAL'))."""
    torch = _torch()
    T, dev = q_start.shape[0], q_start.device
    out = _outputs(fp, T, dev, 'j', want, layout, layout, reuse)
    out['x'] = None
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = _lib.lib().uvs_analytical_closed_loop_f64(
        C.byref(fp), C.byref(plant_struct), T, _flat(q_start), stream_view(noise, layout),
        stream_view(out['j'], layout), stream_view(out['err'], layout), stream_view(out['q'], layout), stream_view(out['f'], layout),
        stream_view(out['dq'], layout), out['stats'].data_ptr(), out['status'].data_ptr(), out['k_done'].data_ptr(), _stream())
    stop.record()
    _lib.check(rc)
    out['events'] = (start, stop)
    return out


def replay(fp, f, dq, x0, want=('x', 'err', 'kappa', 'dqcmd'), layout='kct', final_state=False, in_layout=None):
    """Open-loop replay.  ``f``: stream tensor with K+1 steps, ``dq``: K steps, ``x0``: (T, m*n).  ``layout``: physical layout of the
    output streams and, unless ``in_layout`` says otherwise, of ``f`` / ``dq``."""
    in_layout = in_layout or layout
    torch = _torch()
    T, K, m, n = x0.shape[0], fp.steps, fp.m, fp.n
    dev = x0.device
    out = {}
    for key, comp in (('x', m * n), ('err', m), ('kappa', m), ('dqcmd', n)):
        out[key] = alloc_stream(T, K, comp, layout, dev) if key in want else None      # rows at and after k_done are unspecified
    out['status'] = torch.zeros(T, dtype=torch.int32, device=dev)
    out['k_done'] = torch.zeros(T, dtype=torch.int32, device=dev)
    out['x_final'] = torch.empty((T, m * n), dtype=torch.float64, device=dev) if final_state else None
    out['p_final'] = torch.empty((T, m * n * n), dtype=torch.float64, device=dev) if final_state else None
    rc = _lib.lib().uvs_rmckf_replay_f64(
        C.byref(fp), T, stream_view(f, in_layout), stream_view(dq, in_layout), _flat(x0),
        stream_view(out['x'], layout), stream_view(out['err'], layout), stream_view(out['kappa'], layout),
        stream_view(out['dqcmd'], layout), out['status'].data_ptr(), out['k_done'].data_ptr(),
        _flat(out['x_final']), _flat(out['p_final']), _stream())
    _lib.check(rc)
    return out


def replay_f32(fp, f, dq, x0, want=('x', 'err'), layout='kct'):
    """Single-precision estimator-only replay (uvs_rmckf_replay_f32: a measured lower-precision variant, never the parity path).
    ``f`` (K + 1 steps), ``dq`` (K steps): fp32 stream tensors in ``layout``; ``x0``: (T, m*n) fp32."""
    torch = _torch()
    assert f.dtype == dq.dtype == x0.dtype == torch.float32
    T, K, m, n = x0.shape[0], fp.steps, fp.m, fp.n
    dev = x0.device
    out = {'x': torch.empty(_shape(T, K, m * n, layout), dtype=torch.float32, device=dev) if 'x' in want else None,
           'err': torch.empty(_shape(T, K, m, layout), dtype=torch.float32, device=dev) if 'err' in want else None,
           'status': torch.zeros(T, dtype=torch.int32, device=dev), 'k_done': torch.zeros(T, dtype=torch.int32, device=dev)}
    rc = _lib.lib().uvs_rmckf_replay_f32(C.byref(fp), T, stream_view(f, layout), stream_view(dq, layout), _flat(x0),
                                         stream_view(out['x'], layout), stream_view(out['err'], layout), out['status'].data_ptr(), out['k_done'].data_ptr(), _stream())
    _lib.check(rc)
    return out


def _frames_arg(frames):
    """(tensor, T) of a uint8 frame batch the detector kernel can read in place: on the device or in pinned host memory, (T, H, W, 3) or one
    (H, W, 3) frame, rows and pixels dense.  The frame stride is free (a padded batch is a view of a wider buffer)."""
    torch = _torch()
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError('frames: a torch uint8 tensor (T, 256, 256, 3) or (256, 256, 3)')
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f'frames: (T, 256, 256, 3) RGB, got {tuple(frames.shape)}')
    if not (frames.is_cuda or frames.is_pinned()):
        raise ValueError('frames must be on the device or in pinned host memory: the kernel reads them in place (no hidden copy)')
    if frames.shape[0] and tuple(frames.stride()[1:]) != (frames.shape[2] * 3, 3, 1):
        raise ValueError('frames: rows and pixels must be dense (only the frame stride is free)')
    return frames, frames.shape[0]


def detect_circles(frames, n_colours=4, noise=None, out=None, pixels=None):
    """Centre-of-mass circle detectors (utils.py:11-166: n_colours 1 = detectGreenCircle, 3 = detectRGBCircles, 4 = detect4Circles) of a
    batch of camera frames in one launch on the current stream.  ``frames``: torch uint8 (T, 256, 256, 3) or one (256, 256, 3) frame,
    unflipped as the sensor hands them over, on the device or pinned.  ``noise`` (T, 2 n_colours) fp64 is added to the features in the same
    launch (experiment.py:135); ``pixels`` (T, n_colours) int32 receives the mask sizes.  Returns ``out``: (T, 2 n_colours) fp64 on the
    device unless the caller passes its own (device or pinned) tensor.  A colour that is not in a frame gives NaN, like the reference."""
    from . import _vision
    torch = _torch()
    frames, T = _frames_arg(frames)
    m = 2 * int(n_colours)

    def operand(t, name, dtype, cols):
        if t is None:
            return None
        if t.dtype != dtype or tuple(t.shape) != (T, cols) or not t.is_contiguous() or not (t.is_cuda or t.is_pinned()):
            raise ValueError(f'{name}: contiguous {dtype} tensor ({T}, {cols}) on the device or pinned')
        return t.data_ptr()

    if out is None:
        out = torch.empty((T, m), dtype=torch.float64, device=frames.device if frames.is_cuda else current_device())
    if T == 0:
        return out
    rc = _vision.lib().uvs_detect_circles_u8(T, frames.data_ptr(), frames.stride(0) if T > 1 else frames.shape[1] * frames.shape[2] * 3,
                                             frames.shape[1], frames.shape[2], int(n_colours), operand(noise, 'noise', torch.float64, m),
                                             operand(out, 'out', torch.float64, m), operand(pixels, 'pixels', torch.int32, int(n_colours)),
                                             _stream())
    _vision.check(rc)
    return out


# ---------------------------------------------------------------------------------------------------------------- synthetic camera
def _operand(t, name, dtype, shape, optional=False):
    """data_ptr of a contiguous device-or-pinned tensor of the given dtype and shape (None for an optional one that is absent)."""
    if t is None and optional:
        return None
    torch = _torch()
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or not (t.is_cuda or t.is_pinned()):
        raise ValueError(f'{name}: contiguous {dtype} tensor {tuple(shape)} on the device or pinned')
    return t.data_ptr()


def _camera(plant, radius):
    from . import _vision
    return plant if isinstance(plant, _vision.Camera) else plant.to_camera(radius)


def _device_of(*tensors):
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return current_device()


def camera_project(plant, q_prev, dq=None, dt=0.0, radius=None, q_out=None, out=None, cameras=None, camera_index=None, target_motion=None,
                   motion_window=None, k=0):
    """Disc projection of T trials on the current stream (uvs_camera_project_f64).  ``plant``: a ``SyntheticPlant`` (with ``radius`` in metres,
    default plant.DISC_RADIUS) or the ``uvs_camera`` struct of ``SyntheticPlant.to_camera``.  ``q_prev`` (T, n) fp64; with ``dq`` (T, n) the joints
    are q_prev + dq * dt, written to ``q_out`` (T, n) when given.  Returns ``out``: (T, n_points, 3) rows (u, v, r) in pixels; r = -1 for a point
    that is not in front of the camera.
    ``cameras`` (what ``camera_scenes`` returns or takes) and ``camera_index`` ((T,) integers, host or device): trial t is projected by its
    own camera (uvs_camera_project_scenes_f64) -- with an index ``cameras[camera_index[t]]``, without one the one camera there is, or
    ``cameras[t]`` of T -- and ``plant`` only gives the shape.  Trial t has the bits of the call on its camera; a trial whose device-side
    index names no camera is left unwritten.  None (the default) is the call without the arguments.
    ``target_motion`` ((n_points, 3) or (T, n_points, 3) world metres per step, or what ``target_motions`` returns), ``motion_window``
    (None, (2,) or (T, 2) integers (k_on, k_off)) and the step ``k``: trial t's discs where step k of its motion has taken them
    (uvs_camera_project_moving_f64; the rule is ``plant.target_at``'s, bit for bit).  Without ``cameras`` the nominal camera is packed as
    the one scene.  None is the call without the arguments, through the entry point it always used."""
    from . import _vision, plant as plant_mod
    if cameras is None and camera_index is not None:
        raise ValueError('camera_project: camera_index without cameras')
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    motion = _check_target_motion(target_motion, motion_window, getattr(q_prev, 'shape', (0,))[0], cam.n_points, 'camera_project')
    k = _check_step(k, 'camera_project')
    if motion is not None and cameras is None:
        cameras = [cam]
    if cameras is not None:
        _check_cameras(cameras, camera_index, getattr(q_prev, 'shape', (0,))[0], cam.n_points, cam.n_joints, 'camera_project')
    torch = _torch()
    T, n = q_prev.shape[0], cam.n_joints
    if out is None:
        out = torch.empty((T, cam.n_points, 3), dtype=torch.float64, device=_device_of(q_prev))
    rest = (T, _operand(q_prev, 'q_prev', torch.float64, (T, n)), _operand(dq, 'dq', torch.float64, (T, n), True), float(dt),
            _operand(q_out, 'q_out', torch.float64, (T, n), True), _operand(out, 'out', torch.float64, (T, cam.n_points, 3)), _stream())
    if cameras is None:
        rc = _vision.lib().uvs_camera_project_f64(C.byref(cam), *rest)
    else:
        scenes, _keep, _keep_index = _scene_operand(cameras, camera_index, T, cam.n_points, n, radius, _device_of(q_prev), 'camera_project')
        if motion is None:
            rc = _vision.lib().uvs_camera_project_scenes_f64(*scenes, cam.n_points, *rest)
        else:
            mot, _keep_motion = _motion_operand(motion, _device_of(q_prev))
            rc = _vision.lib().uvs_camera_project_moving_f64(*scenes, mot, cam.n_points, *rest[:4], k, *rest[4:])
    _vision.check(rc)
    return out


def _jacobian_scene(who, plant, T, radius, cameras, camera_index, target_motion, motion_window, tensors):
    """The refusals camera_jacobian and camera_jacobian_score share, all on the host alone and before any device work, then the operands:
    (n_points, the scene triple, the motion pointer or None, tensors to keep alive).  Without ``cameras`` the camera of ``plant`` is packed
    as the one scene.  ``tensors``: (name, tensor or None) pairs that must be fp64 (k_done: int32) tensors on the device."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import plant as plant_mod
    if cameras is None and camera_index is not None:
        raise ValueError(f'{who}: camera_index without cameras')
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    if cam.n_joints != 6:
        raise ValueError(f'{who}: the image Jacobian kernels are built for the six-joint arms of this project, not for {cam.n_joints} joints')
    motion = _check_target_motion(target_motion, motion_window, T, cam.n_points, who)
    if cameras is None:
        cameras = [cam]
    _check_cameras(cameras, camera_index, T, cam.n_points, cam.n_joints, who)
    for name, t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f'{who}: {name} is a tensor on the device')
    dev = tensors[0][1].device
    scenes, keep, keep_index = _scene_operand(cameras, camera_index, T, cam.n_points, cam.n_joints, radius, dev, who)
    mot = None if motion is None else _motion_operand(motion, dev)
    return cam.n_points, scenes, None if mot is None else mot[0], (keep, keep_index, mot)


def camera_jacobian(plant, q, *, k=0, radius=None, cameras=None, camera_index=None, target_motion=None, motion_window=None, out=None):
    """The TRUE image Jacobian dh/dq of the synthetic camera on the current stream (uvs_camera_jacobian_f64; the rule:
    ``plant.projection_jacobian``), in pixels per radian -- no t_s in it; an estimator's X converges to fp.dt times it.  h is the (u, v)
    row ``camera_project`` gives.  ``q`` (T, 6) fp64 on the device gives (T, m, 6), the Jacobian of trial t's scene at q[t] and step ``k``;
    ``q`` (K, T, 6) -- a 'q' log -- gives (K, T, m, 6), row r at step ``k`` + r.  ``plant``, ``radius``, ``cameras`` / ``camera_index`` and
    ``target_motion`` / ``motion_window`` are ``camera_project``'s: the scene of every trial, and where step k of its target's motion has
    taken its points (``plant.target_at``).  Without ``cameras`` the camera of ``plant`` is the one scene.  A trial whose device-side index
    names no camera gets NaNs.  ``out``: the tensor to fill, of the result's shape."""
    from . import _vision
    k = _check_step(k, 'camera_jacobian')
    shape = tuple(getattr(q, 'shape', ()))
    if len(shape) not in (2, 3) or shape[-1] != 6:
        raise ValueError(f'camera_jacobian: q is (T, 6) or (K, T, 6) joints, got {shape}')
    rows, T = (1, shape[0]) if len(shape) == 2 else shape[:2]
    if k + rows > 2 ** 31 - 1:
        raise ValueError(f'camera_jacobian: k + the rows of q must stay below 2^31, got {k} + {rows}')
    npts, scenes, mot, _keep = _jacobian_scene('camera_jacobian', plant, T, radius, cameras, camera_index, target_motion, motion_window,
                                               (('q', q), ('out', out)))
    torch, dev = _torch(), q.device
    result = shape[:-1] + (2 * npts, 6)
    if out is None:
        out = torch.empty(result, dtype=torch.float64, device=dev)
    _vision.check(_vision.lib().uvs_camera_jacobian_f64(*scenes, mot, npts, T, rows, k, _operand(q, 'q', torch.float64, shape),
                                                        _operand(out, 'out', torch.float64, result), _stream()))
    return out


SCORE_KEYS = ('rel_err', 'cosine', 'scale', 'shape_err', 'step_ratio')


def camera_jacobian_score(x, q, plant, dt, *, dq=None, k_done=None, radius=None, cameras=None, camera_index=None, target_motion=None,
                          motion_window=None):
    """Score a stream of Jacobian estimates against the true image Jacobian, on the current stream (uvs_camera_jacobian_score_f64; the
    rule: ``plant.jacobian_score`` and ``plant.score_ratios``).  ``x`` (K, T, m 6) and ``q`` (K, T, 6): the 'x' and 'q' logs of
    ``camera_closed_loop``; ``dt``: fp.dt -- X is scored against Js = dt * ``camera_jacobian``(q), what the estimators' measurement model
    makes it converge to; ``dq`` (K, T, 6) or None: the 'dq' log; ``k_done`` (T,) int32 or None: rows k >= k_done[t] of the logs are
    unspecified, are not read, and score NaN.  The scene arguments are ``camera_jacobian``'s, with step k for row k.  So
        out = camera_closed_loop(fp, plant, q0, noise, fused=True, want=ESTIMATOR_CAMERA_LOGS)
        score = camera_jacobian_score(plant=plant, dt=fp.dt, **{k: out[k] for k in ('x', 'q', 'dq', 'k_done')})
    Returns a dict of (K, T) tensors -- 'rel_err' = |X - Js| / |Js|; 'cosine'; 'scale' = the s minimising |X - s Js|; 'shape_err' = the
    sine of the angle between them; 'step_ratio' = (X dq) . (Js dq) / |X dq|^2, the share of the displacement X promises that the plant
    delivers (NaN without ``dq``, or where X dq == 0) -- and 'sums' (K, T, 6): nx2, nj2, dot, diff2, xd_xd, xd_jd as the kernel wrote them."""
    from . import _vision, plant as plant_mod
    shape = tuple(getattr(q, 'shape', ()))
    if len(shape) != 3 or shape[-1] != 6:
        raise ValueError(f'camera_jacobian_score: q is the (K, T, 6) log of the joints, got {shape}')
    K, T = shape[:2]
    if isinstance(dt, bool) or not isinstance(dt, (int, float, np.integer, np.floating)):
        raise ValueError(f'camera_jacobian_score: dt is the control period, a number, got {dt!r}')
    npts, scenes, mot, _keep = _jacobian_scene('camera_jacobian_score', plant, T, radius, cameras, camera_index, target_motion, motion_window,
                                               (('q', q), ('x', x), ('dq', dq), ('k_done', k_done)))
    torch, dev = _torch(), q.device
    sums = torch.empty((K, T, 6), dtype=torch.float64, device=dev)
    _vision.check(_vision.lib().uvs_camera_jacobian_score_f64(
        *scenes, mot, npts, T, K, float(dt), _operand(x, 'x', torch.float64, (K, T, 2 * npts * 6)), _operand(q, 'q', torch.float64, shape),
        _operand(dq, 'dq', torch.float64, shape, True), _operand(k_done, 'k_done', torch.int32, (T,), True), sums.data_ptr(), _stream()))
    out = plant_mod.score_ratios(sums, torch)
    if dq is None:
        out['step_ratio'] = torch.full_like(out['step_ratio'], float('nan'))
    return dict(out, sums=sums)


def _discs_arg(discs, n_colours):
    torch = _torch()
    if not torch.is_tensor(discs) or discs.dim() != 3 or tuple(discs.shape[1:]) != (int(n_colours), 3):
        raise ValueError(f'discs: a torch fp64 tensor (T, {int(n_colours)}, 3) of rows (u, v, r)')
    return discs.shape[0], _operand(discs, 'discs', torch.float64, discs.shape)


def _check_occluders(spec, T, k=0, shade=32, who='occluders'):
    """What can be said of an occluder operand on the host alone, before any device work: ValueError, or the operand -- None, the caller's
    own packed device (or pinned) int32 tensor (T, n_occ, 8), or a checked host int32 array (T, n_occ, 8)."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import plant as plant_mod
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < 2 ** 31:
        raise ValueError(f'{who}: k is a step count, an integer >= 0, got {k!r}')
    if isinstance(shade, bool) or not isinstance(shade, (int, np.integer)) or not 0 <= shade < 250:
        raise ValueError(f'{who}: shade must be an integer 0 .. 249 (250 and above would enter a mask of the detectors), got {shade!r}')
    if spec is None:
        return None
    if torch.is_tensor(spec) and (spec.is_cuda or spec.is_pinned()):
        if spec.dtype != torch.int32 or spec.dim() != 3 or spec.shape[0] != T or spec.shape[2] != 8 or not spec.is_contiguous():
            raise ValueError(f'{who}: a packed tensor is contiguous int32 ({T}, n_occ, 8), got {spec.dtype} {tuple(spec.shape)}')
        if spec.shape[1] > plant_mod.MAX_OCCLUDERS:
            raise ValueError(f'{who}: at most {plant_mod.MAX_OCCLUDERS} per trial, got {spec.shape[1]}')
        return spec
    return plant_mod.occluder_array(spec.numpy() if torch.is_tensor(spec) else spec, T).astype(np.int32)


def occluders(spec, T, device=None):
    """Pack occluders for the kernels (uvs_occluder of include/uvs_vision.h): ``spec`` is a (T, n_occ, 8) or (n_occ, 8) integer array-like of
    rows (x, y, w, h, vx, vy, k_on, k_off) -- ``plant.OCCLUDER_FIELDS``; the second form is broadcast over the trials -- with n_occ <= 4.
    Returns a contiguous int32 tensor (T, n_occ, 8) on ``device``.  Indexing per scenario is the caller's, by gathering on the host or with
    torch: the C ABI has no index operand."""
    host = _check_occluders(spec, T)
    torch = _torch()
    if host is None:
        raise ValueError('occluders: nothing to pack')
    dev = current_device(device)
    return host.to(dev) if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host)).to(dev)


def _occluder_operand(checked, dev):
    """(pointer or None, n_occ, tensor to keep alive) of what _check_occluders returned."""
    torch = _torch()
    t = checked if torch.is_tensor(checked) else torch.from_numpy(np.ascontiguousarray(checked)).to(dev)
    return (t.data_ptr() if t.numel() else None), t.shape[1], t


def _check_occluder_colours(spec, checked, T, n_colours, who='occluder_colours'):
    """What can be said of the occluders' paints on the host alone, before any device work: ValueError, or the operand -- None, the
    caller's own packed device (or pinned) int32 tensor (T, n_occ), or a checked host int32 array (T, n_occ).  ``checked``: what
    ``_check_occluders`` returned for the same call (None: there are no occluders to paint, a ValueError)."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import plant as plant_mod
    if spec is None:
        return None
    n_occ = None if checked is None else checked.shape[1]
    if torch.is_tensor(spec) and (spec.is_cuda or spec.is_pinned()):
        if n_occ is None:
            raise ValueError(f'{who}: occluder_colours without occluders: a paint belongs to a rectangle')
        if spec.dtype != torch.int32 or tuple(spec.shape) != (T, n_occ) or not spec.is_contiguous():
            raise ValueError(f'{who}: a packed tensor of paints is contiguous int32 ({T}, {n_occ}), got {spec.dtype} {tuple(spec.shape)}')
        return spec                                                  # its values are the device's to read: anything but a disc is opaque
    try:
        return plant_mod.occluder_colour_array(spec.numpy() if torch.is_tensor(spec) else spec, n_occ, int(n_colours), T).astype(np.int32)
    except ValueError as exc:
        raise ValueError(f'{who}: {exc}') from exc


def _paint_operand(checked, dev):
    """(pointer or None, tensor to keep alive) of what _check_occluder_colours returned (not None)."""
    torch = _torch()
    t = checked if torch.is_tensor(checked) else torch.from_numpy(np.ascontiguousarray(checked)).to(dev)
    return (t.data_ptr() if t.numel() else None), t


def render_discs(discs, n_colours=4, background=96, out=None, occluders=None, k=0, shade=32, occluder_colours=None):
    """Rasterise ``discs`` (T, n_colours, 3) fp64 rows (u, v, r) into camera frames on the current stream (uvs_render_discs_u8; the pixel rule
    is ``plant.render_discs``'s, byte for byte).  Returns ``out``: uint8 (T, 256, 256, 3), unflipped as the detectors expect them, on the device
    unless the caller passes its own device or pinned tensor -- whose frame stride is free (bytes between frames are not written).
    ``occluders`` (what ``occluders()`` takes or returns), the step ``k`` and ``shade``: the frames with those rectangles in front
    (uvs_render_discs_occluded_u8; ``plant.render_discs(..., occluders, k, shade)`` byte for byte).  None is the call above.
    ``occluder_colours``: the occluders' paints, (n_occ,) or (T, n_occ) integers or a packed int32 tensor (T, n_occ): a rectangle painted
    p shows disc p's colour, -1 is opaque (uvs_render_discs_painted_u8; ``plant.render_discs(..., occluder_colours=)`` byte for byte).
    None is the call without the argument, through the entry point it always used."""
    from . import _vision
    checked = _check_occluders(occluders, getattr(discs, 'shape', (0,))[0], k, shade, 'render_discs')
    paints = _check_occluder_colours(occluder_colours, checked, getattr(discs, 'shape', (0,))[0], n_colours, 'render_discs')
    torch = _torch()
    T, ptr = _discs_arg(discs, n_colours)
    if out is None:
        out = torch.empty((T, _vision.SIDE, _vision.SIDE, 3), dtype=torch.uint8, device=_device_of(discs))
    frames, Tf = _frames_arg(out)
    if Tf != T or tuple(frames.shape[1:3]) != (_vision.SIDE, _vision.SIDE):
        raise ValueError(f'out: ({T}, 256, 256, 3) uint8, got {tuple(out.shape)}')
    stride = frames.stride(0) if T > 1 else _vision.SIDE * _vision.SIDE * 3
    if checked is None:
        rc = _vision.lib().uvs_render_discs_u8(T, ptr, int(n_colours), int(background), frames.data_ptr(), stride, _stream())
    else:
        occ, n_occ, _keep = _occluder_operand(checked, _device_of(discs))
        if paints is None:
            rc = _vision.lib().uvs_render_discs_occluded_u8(T, ptr, int(n_colours), int(background), occ, n_occ, int(k), int(shade),
                                                            frames.data_ptr(), stride, _stream())
        else:
            paint, _keep_paint = _paint_operand(paints, _device_of(discs))
            rc = _vision.lib().uvs_render_discs_painted_u8(T, ptr, int(n_colours), int(background), occ, paint, n_occ, int(k), int(shade),
                                                           frames.data_ptr(), stride, _stream())
    _vision.check(rc)
    return out


def disc_features(discs, n_colours=4, noise=None, out=None, pixels=None, occluders=None, k=0, occluder_colours=None):
    """The frame-free detector (uvs_disc_features_f64): what ``detect_circles(render_discs(discs))`` returns, bit for bit, in one launch that
    never writes a frame.  Arguments and result as ``detect_circles`` with ``discs`` (T, n_colours, 3) in place of the frames.  With
    ``occluders`` at step ``k`` (uvs_disc_features_occluded_f64) it is ``detect_circles(render_discs(discs, occluders=..., k=k))``, and with
    ``occluder_colours``, their paints as ``render_discs`` takes them (uvs_disc_features_painted_f64), that of the painted frames."""
    from . import _vision
    checked = _check_occluders(occluders, getattr(discs, 'shape', (0,))[0], k, who='disc_features')
    paints = _check_occluder_colours(occluder_colours, checked, getattr(discs, 'shape', (0,))[0], n_colours, 'disc_features')
    torch = _torch()
    T, ptr = _discs_arg(discs, n_colours)
    m = 2 * int(n_colours)
    if out is None:
        out = torch.empty((T, m), dtype=torch.float64, device=_device_of(discs))
    rest = (_operand(noise, 'noise', torch.float64, (T, m), True), _operand(out, 'out', torch.float64, (T, m)),
            _operand(pixels, 'pixels', torch.int32, (T, int(n_colours)), True), _stream())
    if checked is None:
        rc = _vision.lib().uvs_disc_features_f64(T, ptr, int(n_colours), *rest)
    else:
        occ, n_occ, _keep = _occluder_operand(checked, _device_of(discs))
        if paints is None:
            rc = _vision.lib().uvs_disc_features_occluded_f64(T, ptr, int(n_colours), occ, n_occ, int(k), *rest)
        else:
            paint, _keep_paint = _paint_operand(paints, _device_of(discs))
            rc = _vision.lib().uvs_disc_features_painted_f64(T, ptr, int(n_colours), occ, paint, n_occ, int(k), *rest)
    _vision.check(rc)
    return out


def camera_features(plant, q_prev, dq=None, dt=0.0, radius=None, noise=None, q_out=None, out=None, pixels=None, discs=None, occluders=None, k=0,
                    occluder_colours=None, cameras=None, camera_index=None, target_motion=None, motion_window=None):
    """``camera_project`` and ``disc_features`` in one launch (uvs_camera_features_f64), bit-identical to the two in a row: joints in, noisy
    detected features (T, 2 n_points) out.  ``discs`` (T, n_points, 3) receives the projection when given.  ``occluders`` at step ``k``:
    uvs_camera_features_occluded_f64, the two occluded calls in a row; with ``occluder_colours`` uvs_camera_features_painted_f64, the two
    painted ones.
    ``cameras`` / ``camera_index`` (as ``camera_project`` takes them): trial t on its own camera, with or without occluders and their
    colours, in one launch (uvs_camera_features_scenes_f64); ``plant`` only gives the shape.  None is the call without the arguments.
    ``target_motion`` / ``motion_window`` (as ``camera_project`` takes them): the detection of the frame with trial t's discs where step
    ``k`` of its motion has taken them (uvs_camera_features_moving_f64), with or without cameras, occluders and their colours; without
    ``cameras`` the nominal camera is packed as the one scene.  None is the call without the arguments."""
    from . import _vision, plant as plant_mod
    if cameras is None and camera_index is not None:
        raise ValueError('camera_features: camera_index without cameras')
    checked = _check_occluders(occluders, getattr(q_prev, 'shape', (0,))[0], k, who='camera_features')
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    paints = _check_occluder_colours(occluder_colours, checked, getattr(q_prev, 'shape', (0,))[0], cam.n_points, 'camera_features')
    motion = _check_target_motion(target_motion, motion_window, getattr(q_prev, 'shape', (0,))[0], cam.n_points, 'camera_features')
    if motion is not None and cameras is None:
        cameras = [cam]
    if cameras is not None:
        _check_cameras(cameras, camera_index, getattr(q_prev, 'shape', (0,))[0], cam.n_points, cam.n_joints, 'camera_features')
    torch = _torch()
    T, n, npts = q_prev.shape[0], cam.n_joints, cam.n_points
    if out is None:
        out = torch.empty((T, 2 * npts), dtype=torch.float64, device=_device_of(q_prev))
    joints = (C.byref(cam), T, _operand(q_prev, 'q_prev', torch.float64, (T, n)), _operand(dq, 'dq', torch.float64, (T, n), True), float(dt),
              _operand(q_out, 'q_out', torch.float64, (T, n), True))
    rest = (_operand(noise, 'noise', torch.float64, (T, 2 * npts), True), _operand(out, 'out', torch.float64, (T, 2 * npts)),
            _operand(pixels, 'pixels', torch.int32, (T, npts), True), _operand(discs, 'discs', torch.float64, (T, npts, 3), True), _stream())
    if cameras is not None:
        dev = _device_of(q_prev)
        scenes, _keep, _keep_index = _scene_operand(cameras, camera_index, T, npts, n, radius, dev, 'camera_features')
        occ, n_occ, _keep_occ = (None, 0, None) if checked is None else _occluder_operand(checked, dev)
        paint, _keep_paint = (None, None) if paints is None else _paint_operand(paints, dev)
        if motion is None:
            rc = _vision.lib().uvs_camera_features_scenes_f64(*scenes, npts, *joints[1:], occ, paint, n_occ, int(k), *rest)
        else:
            mot, _keep_motion = _motion_operand(motion, dev)
            rc = _vision.lib().uvs_camera_features_moving_f64(*scenes, mot, npts, *joints[1:], occ, paint, n_occ, int(k), *rest)
    elif checked is None:
        rc = _vision.lib().uvs_camera_features_f64(*joints, *rest)
    else:
        occ, n_occ, _keep = _occluder_operand(checked, _device_of(q_prev))
        if paints is None:
            rc = _vision.lib().uvs_camera_features_occluded_f64(*joints, occ, n_occ, int(k), *rest)
        else:
            paint, _keep_paint = _paint_operand(paints, _device_of(q_prev))
            rc = _vision.lib().uvs_camera_features_painted_f64(*joints, occ, paint, n_occ, int(k), *rest)
    _vision.check(rc)
    return out


def _check_hold(hold, who='camera_closed_loop'):
    """``hold`` as the other integers are checked, on the host alone: an int >= 0 (below 2^31)."""
    if isinstance(hold, bool) or not isinstance(hold, (int, np.integer)) or not 0 <= hold < 2 ** 31:
        raise ValueError(f'{who}: hold is a number of steps, an integer >= 0, got {hold!r}')
    return int(hold)


def hold_features(f, f_prev, pixels, miss, hold, k, held=None):
    """Hold a lost disc's last detection, one step of T trials on the current stream (uvs_hold_features_f64; ``plant.hold_features`` states
    the rule, and this is it bit for bit).  ``f`` (T, 2 n_points) fp64: the row ``camera_features(..., pixels=pixels, k=k)`` has just
    written, rewritten IN PLACE where a pair is held; ``f_prev`` (T, 2 n_points): the reported row of step k - 1, or None at k == 0;
    ``pixels`` (T, n_points) int32: the mask counts of step k; ``miss`` (T, 4) int32: the loop's counters, zeros before step 0, updated in
    place (disc j of trial t at [t, j]); ``hold`` >= 0; ``held`` (T, n_points) int32 receives 1 where the disc was held at this step, else 0
    (a new tensor when None).  Returns (f, miss, held)."""
    from . import _vision
    hold = _check_hold(hold, 'hold_features')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < 2 ** 31:
        raise ValueError(f'hold_features: k is a step count, an integer >= 0, got {k!r}')
    if f_prev is None and k >= 1:
        raise ValueError('hold_features: f_prev, the reported row of step k - 1, is needed from step 1 on')
    torch = _torch()
    if not torch.is_tensor(f) or f.dim() != 2 or f.shape[1] % 2:
        raise ValueError('hold_features: f is a torch fp64 tensor (T, 2 n_points)')
    T, npts = f.shape[0], f.shape[1] // 2
    if held is None:
        held = torch.empty((T, npts), dtype=torch.int32, device=_device_of(f))
    rc = _vision.lib().uvs_hold_features_f64(T, npts, hold, int(k), _operand(f_prev, 'f_prev', torch.float64, (T, 2 * npts), True),
                                             _operand(f, 'f', torch.float64, (T, 2 * npts)), _operand(pixels, 'pixels', torch.int32, (T, npts)),
                                             _operand(miss, 'miss', torch.int32, (T, 4)), _operand(held, 'held', torch.int32, (T, npts)), _stream())
    _vision.check(rc)
    return f, miss, held


def believed_models(models, radius=None, device=None):
    """The believed-model operand of the calibrated baseline on a wrong model: ``models`` -- a ``SyntheticPlant``, a ``Camera`` struct, or a
    sequence of either (``plant.miscalibrated`` makes wrong plants) -- packed as the device array of ``uvs_camera`` structs that
    uvs_camera_believed_step_f64 / _loop_f64 / _guess_f64 read: a uint8 tensor (n_believed, sizeof(uvs_camera)).  Pack once and pass the
    tensor as ``believed=`` to as many calls as needed.  ``radius`` as ``SyntheticPlant.to_camera`` (the law does not read it)."""
    from . import _vision, plant as plant_mod
    torch = _torch()
    if isinstance(models, (_vision.Camera, plant_mod.SyntheticPlant)):
        models = [models]
    models = list(models)
    if not models:
        raise ValueError('believed_models: at least one model')
    size = C.sizeof(_vision.Camera)
    host = np.empty((len(models), size), np.uint8)
    for i, model in enumerate(models):
        if not isinstance(model, (_vision.Camera, plant_mod.SyntheticPlant)):
            raise ValueError('believed_models: a SyntheticPlant, a Camera struct, or a sequence of them')
        cam = _camera(model, plant_mod.DISC_RADIUS if radius is None else radius)
        host[i] = np.frombuffer(C.string_at(C.addressof(cam), size), np.uint8)
    return torch.from_numpy(host).to(current_device(device))


def _check_believed(believed, believed_index, T, who):
    """What can be said of a ``believed=`` / ``believed_index=`` pair for T trials on the host alone, before anything is packed or uploaded:
    ValueError, or (n_believed, the index as a host int32 array | the caller's device tensor | None)."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import _vision, plant as plant_mod
    if believed is None:
        raise ValueError(f'{who}: believed_index without believed')
    size = C.sizeof(_vision.Camera)
    if torch.is_tensor(believed):
        if believed.dtype != torch.uint8 or believed.dim() != 2 or believed.shape[1] != size or not believed.is_contiguous():
            raise ValueError(f'{who}: believed is what believed_models returns: a contiguous uint8 tensor (n_believed, {size}) on the device')
        n = believed.shape[0]
    else:
        n = 1 if isinstance(believed, (_vision.Camera, plant_mod.SyntheticPlant)) else len(believed)
    if n < 1:
        raise ValueError(f'{who}: at least one believed model')
    if believed_index is None:
        if n not in (1, T):
            raise ValueError(f'{who}: {n} believed models for {T} trials: one, or one per trial, or pass believed_index')
        return n, None
    if torch.is_tensor(believed_index) and believed_index.is_cuda:   # the kernels FAIL a trial whose index names no model
        return n, believed_index
    host = np.asarray(believed_index.numpy() if torch.is_tensor(believed_index) else believed_index)
    if host.shape != (T,) or host.dtype.kind not in 'iu':
        raise ValueError(f'{who}: believed_index is {T} integers, one per trial')
    if host.size and (host.min() < 0 or host.max() >= n):
        raise ValueError(f'{who}: believed_index must lie in [0, {n}), got {int(host.min())} .. {int(host.max())}')
    return n, np.ascontiguousarray(host, np.int32)


def _believed_operand(believed, believed_index, T, radius, dev, who):
    """(pointer, n_believed, index pointer or None, tensors to keep alive) of a ``believed=`` / ``believed_index=`` pair for T trials; a
    host-side index is checked before it is uploaded."""
    torch = _torch()
    n, index = _check_believed(believed, believed_index, T, who)
    if not torch.is_tensor(believed):
        believed = believed_models(believed, radius, dev)
    if not (believed.is_cuda or believed.is_pinned()):
        raise ValueError(f'{who}: believed is what believed_models returns: a tensor on the device (or pinned)')
    if index is None:
        return believed.data_ptr(), n, None, (believed,)
    if not torch.is_tensor(index):
        index = torch.from_numpy(index).to(dev)
    return believed.data_ptr(), n, _operand(index, 'believed_index', torch.int32, (T,)), (believed, index)


def camera_scenes(models, radius=None, device=None):
    """The scene operand of the pixel loops: the cameras that RENDER the trials' frames, one ``uvs_camera`` struct each, packed like
    ``believed_models`` as a uint8 tensor (n_cams, sizeof(uvs_camera)) on the device -- pack once, pass it as ``cameras=`` to as many calls
    as needed.  ``models``: a ``SyntheticPlant``, a ``Camera`` struct, or a sequence of either (``plant.miscalibrated`` makes variants of a
    plant).  ``radius`` (metres; default plant.DISC_RADIUS) is read by the sensor side, so it may differ per scene: a scalar, one value per
    model, or (n_models, n_points); a ``Camera`` struct keeps its own."""
    from . import _vision, plant as plant_mod
    torch = _torch()
    if isinstance(models, (_vision.Camera, plant_mod.SyntheticPlant)):
        models = [models]
    models = list(models)
    if not models:
        raise ValueError('camera_scenes: at least one model')
    radii = np.asarray(plant_mod.DISC_RADIUS if radius is None else radius, float)
    if radii.ndim and radii.shape[0] != len(models):
        raise ValueError(f'camera_scenes: radius is a scalar or one value (or one row of n_points) per model, got {radii.shape} for {len(models)} models')
    size = C.sizeof(_vision.Camera)
    host = np.empty((len(models), size), np.uint8)
    for i, model in enumerate(models):
        if not isinstance(model, (_vision.Camera, plant_mod.SyntheticPlant)):
            raise ValueError('camera_scenes: a SyntheticPlant, a Camera struct, or a sequence of them')
        cam = _camera(model, radii[i] if radii.ndim else radii)
        host[i] = np.frombuffer(C.string_at(C.addressof(cam), size), np.uint8)
    return torch.from_numpy(host).to(current_device(device))


def _check_cameras(cameras, camera_index, T, n_points, n_joints, who):
    """What can be said of a ``cameras=`` / ``camera_index=`` pair for T output trials of the given shape on the host alone, before anything
    is packed or uploaded: ValueError, or (n_cams, the index as a host int32 array | the caller's device tensor | None)."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import _vision, plant as plant_mod
    if cameras is None:
        raise ValueError(f'{who}: camera_index without cameras')
    if n_joints != 6:
        raise ValueError(f'{who}: the scene kernels are built for the six-joint arms of this project, not for {n_joints} joints')
    size = C.sizeof(_vision.Camera)
    if torch.is_tensor(cameras):
        if cameras.dtype != torch.uint8 or cameras.dim() != 2 or cameras.shape[1] != size or not cameras.is_contiguous():
            raise ValueError(f'{who}: cameras is what camera_scenes returns: a contiguous uint8 tensor (n_cams, {size}) on the device')
        n = cameras.shape[0]
    else:
        models = [cameras] if isinstance(cameras, (_vision.Camera, plant_mod.SyntheticPlant)) else list(cameras)
        for model in models:
            if not isinstance(model, (_vision.Camera, plant_mod.SyntheticPlant)):
                raise ValueError(f'{who}: cameras is a SyntheticPlant, a Camera struct, a sequence of them, or what camera_scenes returns')
            if (model.n_points, model.n_joints) != (n_points, n_joints):
                raise ValueError(f'{who}: a camera of {model.n_points} points and {model.n_joints} joints among the scenes of a loop of '
                                 f'{n_points} points and {n_joints} joints')
        n = len(models)
    if n < 1:
        raise ValueError(f'{who}: at least one camera')
    if camera_index is None:
        if n not in (1, T):
            raise ValueError(f'{who}: {n} cameras for {T} trials: one, or one per trial, or pass camera_index')
        return n, None
    if torch.is_tensor(camera_index) and camera_index.is_cuda:       # the kernels void a trial whose index names no camera
        if tuple(camera_index.shape) != (T,):
            raise ValueError(f'{who}: camera_index is {T} integers, one per output trial')
        return n, camera_index
    host = np.asarray(camera_index.numpy() if torch.is_tensor(camera_index) else camera_index)
    if host.shape != (T,) or host.dtype.kind not in 'iu':
        raise ValueError(f'{who}: camera_index is {T} integers, one per output trial')
    if host.size and (host.min() < 0 or host.max() >= n):
        raise ValueError(f'{who}: camera_index must lie in [0, {n}), got {int(host.min())} .. {int(host.max())}')
    return n, np.ascontiguousarray(host, np.int32)


def _scene_operand(cameras, camera_index, T, n_points, n_joints, radius, dev, who):
    """((pointer, n_cams, index pointer or None), the packed tensor, the index tensor or None) of a ``cameras=`` / ``camera_index=`` pair for
    T output trials; a host-side index is checked before it is uploaded."""
    torch = _torch()
    n, index = _check_cameras(cameras, camera_index, T, n_points, n_joints, who)
    if not torch.is_tensor(cameras):
        cameras = camera_scenes(cameras, radius, dev)
    if not (cameras.is_cuda or cameras.is_pinned()):
        raise ValueError(f'{who}: cameras is what camera_scenes returns: a tensor on the device (or pinned)')
    if index is None:
        return (cameras.data_ptr(), n, None), cameras, None
    if not torch.is_tensor(index):
        index = torch.from_numpy(index).to(dev)
    return (cameras.data_ptr(), n, _operand(index, 'camera_index', torch.int32, (T,))), cameras, index


def _check_target_motion(target_motion, motion_window, T, n_points, who):
    """What can be said of a ``target_motion=`` / ``motion_window=`` pair for T output trials of n_points discs on the host alone, before any
    device work: ValueError, or the operand -- None, the caller's own packed device (or pinned) uint8 tensor (T, 104) (what
    ``target_motions`` returns), or the packed host uint8 array (T, 104) of ``plant.target_motion_array``."""
    import torch                                                     # not _torch(): these refusals need no GPU
    from . import plant as plant_mod
    if target_motion is None:
        if motion_window is not None:
            raise ValueError(f'{who}: motion_window without target_motion: a window belongs to a motion')
        return None
    if torch.is_tensor(target_motion) and target_motion.dtype == torch.uint8:
        if motion_window is not None:
            raise ValueError(f'{who}: a packed target_motion carries its windows: no motion_window next to it')
        if tuple(target_motion.shape) != (T, plant_mod.MOTION_ROW) or not target_motion.is_contiguous():
            raise ValueError(f'{who}: a packed target_motion is what target_motions returns for these trials: a contiguous uint8 tensor '
                             f'({T}, {plant_mod.MOTION_ROW}), got {tuple(target_motion.shape)}')
        if not (target_motion.is_cuda or target_motion.is_pinned()):
            raise ValueError(f'{who}: a packed target_motion is on the device (or pinned)')
        return target_motion
    velocity = target_motion.detach().cpu().numpy() if torch.is_tensor(target_motion) else target_motion
    window = motion_window.detach().cpu().numpy() if torch.is_tensor(motion_window) else motion_window
    try:
        return plant_mod.target_motion_array(velocity, window, int(n_points), int(T))
    except ValueError as exc:
        raise ValueError(f'{who}: {exc}') from exc


def target_motions(velocity, window, n_points, T, device=None):
    """Pack target motions for the kernels (uvs_target_motion of include/uvs_vision.h; the rule: ``plant.target_at``): ``velocity``
    (n_points, 3) or (T, n_points, 3) world metres per step, ``window`` None, (2,) or (T, 2) integers (k_on, k_off) -- the shorter forms
    are broadcast over the trials.  Returns a contiguous uint8 tensor (T, 104) on ``device``: pack once, pass it as ``target_motion=`` to as
    many calls as needed.  Indexed by OUTPUT trial."""
    host = _check_target_motion(velocity, window, T, n_points, 'target_motions')
    torch = _torch()
    if host is None:
        raise ValueError('target_motions: nothing to pack')
    return host if torch.is_tensor(host) else torch.from_numpy(host).to(current_device(device))


def _motion_operand(checked, dev):
    """(pointer, tensor to keep alive) of what _check_target_motion returned (not None)."""
    torch = _torch()
    t = checked if torch.is_tensor(checked) else torch.from_numpy(np.ascontiguousarray(checked)).to(dev)
    return t.data_ptr(), t


MAX_LATENCY = 8                                                     # UVS_CAMERA_MAX_LATENCY of include/uvs_vision.h (plant.MAX_LATENCY)


def _check_latency(latency, T, who, name='latency'):
    """What can be said of a ``latency=`` for T output trials on the host alone, before any device work: ValueError, or the operand --
    None, or a host int32 array (T,) of values in 0 .. MAX_LATENCY.  ``latency``: None, an integer for every trial, or T integers (a
    sequence, an array or an integer tensor, which is brought to the host).  ``name``: what the refusals call the argument
    ('assumed_latency' and 'predict' have the same rule and the same messages)."""
    many = 'latencies' if name == 'latency' else f'{name} values'
    import torch                                                     # not _torch(): these refusals need no GPU
    if latency is None:
        return None
    if torch.is_tensor(latency):
        if latency.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64) or latency.is_complex():
            raise ValueError(f'{who}: {name} is integers, control periods, got {latency.dtype}')
        latency = latency.detach().cpu().numpy()
    try:
        a = np.asarray(latency)
    except Exception as exc:                                         # ragged lists
        raise ValueError(f'{who}: {name} is an integer or ({T},) integers') from exc
    if a.dtype.kind not in 'iu' or a.ndim > 1:
        raise ValueError(f'{who}: {name} is an integer or ({T},) integers, control periods, got {a.dtype} {a.shape}')
    if a.ndim == 1 and a.shape[0] != T:
        raise ValueError(f'{who}: {a.shape[0]} {many} for {T} trials')
    if a.size and (a.min() < 0 or a.max() > MAX_LATENCY):
        raise ValueError(f'{who}: {name} must lie in 0 .. {MAX_LATENCY} control periods, got {int(a.min())} .. {int(a.max())}')
    return np.broadcast_to(a.astype(np.int32), (T,)).copy()


def _latency_operand(checked, dev):
    """(pointer, tensor to keep alive) of what _check_latency returned (not None)."""
    t = _torch().from_numpy(checked).to(dev)
    return t.data_ptr(), t


def _check_step(k, who):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < 2 ** 31:
        raise ValueError(f'{who}: k is a step count, an integer >= 0, got {k!r}')
    return int(k)


def camera_guess(plant, q_start, f0, radius=None, out=None, believed=None, believed_index=None):
    """The analytic initial guess of T trials on the device (uvs_camera_guess_f64): what ``plant.analytic_guess`` returns per trial for the
    joints ``q_start`` (T, 6) and the detected features ``f0`` (T, 2 n_points), both cuda fp64, to about 1e-13 relative (another order of
    operations, not the same bits).  Returns ``out``: (T, 2 n_points * 6).
    ``believed`` (what ``believed_models`` returns or takes) and ``believed_index`` ((T,) integers, host or device): the guess of trial t from
    its own believed model instead (uvs_camera_believed_guess_f64; ``plant`` then only says how many points there are) -- with an index
    ``believed[believed_index[t]]``, without one the one model there is, or ``believed[t]`` of T.  ``f0`` stays what the true camera detects."""
    if believed is None and believed_index is not None:
        raise ValueError('camera_guess: believed_index without believed')
    from . import _vision, plant as plant_mod
    torch = _torch()
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    T, n, m = q_start.shape[0], cam.n_joints, 2 * cam.n_points
    if out is None:
        out = torch.empty((T, m * n), dtype=torch.float64, device=_device_of(q_start, f0))
    if believed is not None:
        models, n_believed, index, _keep = _believed_operand(believed, believed_index, T, radius, _device_of(q_start, f0), 'camera_guess')
        rc = _vision.lib().uvs_camera_believed_guess_f64(T, cam.n_points, models, n_believed, index, _operand(q_start, 'q_start', torch.float64, (T, n)),
                                                         _operand(f0, 'f0', torch.float64, (T, m)), _operand(out, 'out', torch.float64, (T, m * n)),
                                                         _stream())
        _vision.check(rc)
        return out
    rc = _vision.lib().uvs_camera_guess_f64(C.byref(cam), T, _operand(q_start, 'q_start', torch.float64, (T, n)),
                                            _operand(f0, 'f0', torch.float64, (T, m)), _operand(out, 'out', torch.float64, (T, m * n)), _stream())
    _vision.check(rc)
    return out


def camera_analytical_step(plant, q, f, fp, radius=None, dq=None, err=None, j=None, status=None, believed=None, believed_index=None):
    """One step of the calibrated IBVS baseline for T trials on the current stream (uvs_camera_analytical_step_f64): the interaction matrix
    from the model at the joints ``q`` (T, 6) and the DETECTED features ``f`` (T, 2 n_points) -- raw pixels, noise already added -- then
    dq = -gain pinv(J) (f - desired).  ``plant``: a SyntheticPlant or a ``Camera`` struct; ``fp.method`` must be ANALYTICAL.  Returns
    (dq (T, 6), err (T, m), status (T,) int32), written into the tensors given or into new ones; ``j`` (T, m * 6), when given, receives J.
    A trial whose J is not finite has status FAIL and an unspecified dq row.
    ``believed`` / ``believed_index`` (as ``camera_guess`` takes them): the step of trial t on its own believed model
    (uvs_camera_believed_step_f64); ``plant`` then only gives the shape.  With the true model as ``believed`` the bits are the same."""
    if believed is None and believed_index is not None:
        raise ValueError('camera_analytical_step: believed_index without believed')
    from . import _vision, plant as plant_mod
    torch = _torch()
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    T, n, m = q.shape[0], cam.n_joints, 2 * cam.n_points
    dev = _device_of(q, f)
    if dq is None:
        dq = torch.empty((T, n), dtype=torch.float64, device=dev)
    if err is None:
        err = torch.empty((T, m), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(T, dtype=torch.int32, device=dev)
    operands = (_operand(q, 'q', torch.float64, (T, n)), _operand(f, 'f', torch.float64, (T, m)), _operand(dq, 'dq', torch.float64, (T, n)),
                _operand(err, 'err', torch.float64, (T, m)), _operand(j, 'j', torch.float64, (T, m * n), True),
                _operand(status, 'status', torch.int32, (T,)), _stream())
    if believed is not None:
        if fp.m != m or fp.n != n:
            raise ValueError(f'camera_analytical_step: fp is ({fp.m}, {fp.n}) but the camera gives {m} features of {n} joints')
        models, n_believed, index, _keep = _believed_operand(believed, believed_index, T, radius, dev, 'camera_analytical_step')
        rc = _vision.lib().uvs_camera_believed_step_f64(C.byref(fp), T, models, n_believed, index, *operands)
    else:
        rc = _vision.lib().uvs_camera_analytical_step_f64(C.byref(fp), C.byref(cam), T, *operands)
    _vision.check(rc)
    return dq, err, status


CAMERA_LOGS = ('err', 'q', 'f', 'dq', 'kappa')
ANALYTICAL_CAMERA_LOGS = ('err', 'q', 'f', 'dq')                    # the calibrated law has no correntropy weights
ESTIMATOR_CAMERA_LOGS = CAMERA_LOGS + ('x',)                         # the estimators can log the estimate itself: X_k, (K, T, m n)


def _features_step(cam_ref, T, dt, occ, stream, hold=0, npts=0, dev=None, paint=None, scenes=None, motion=None, latency=None, steps=0):
    """The stepwise loops' sensor launch at step k: uvs_camera_features_f64, or its occluded namesake when ``occ`` -- None, or the
    (pointer, n_occ, tensor) of ``_occluder_operand`` -- is given.  Returns f(k, q_prev, dq_prev, q, noise, f, pixels) -> return code.
    With ``hold`` > 0 the step is that launch and uvs_hold_features_f64 behind it on the same stream, on the same rows: the callable then
    takes two more row pointers, f(..., pixels, f_prev, held), and keeps the counters of consecutive held steps (T, 4) itself.
    ``paint``: None, or the (pointer, tensor) of ``_paint_operand`` next to ``occ`` -- the launch is then uvs_camera_features_painted_f64.
    ``scenes``: None, or the (pointer, n_cams, index pointer) of ``_scene_operand`` -- the launch is then uvs_camera_features_scenes_f64 for
    ``npts`` points, with or without ``occ`` and ``paint``, and ``cam_ref`` is not read.
    ``motion``: None, or the pointer of ``_motion_operand`` next to ``scenes`` -- the launch is then uvs_camera_features_moving_f64, which
    takes the motions and the step k.
    ``latency``: None, or the pointer of ``_latency_operand`` for a loop of ``steps`` steps -- the sensor launch then writes the noise-free
    detection and its mask sizes into row k of two logs the callable keeps, (steps, T, 2 npts) and (steps, T, npts), and
    uvs_delay_features_f64 behind it forms the reported row (row max(k - d, 0) plus step k's noise) and its counts into f and pixels;
    the hold launch, if any, follows on those."""
    from . import _vision
    if motion is not None:
        moving = _vision.lib().uvs_camera_features_moving_f64
        occ_ptr, n_occ = (None, 0) if occ is None else occ[:2]
        paint_ptr = None if paint is None else paint[0]
        detect = lambda k, q_prev, dq_prev, q, noise, f, pixels: moving(*scenes, motion, npts, T, q_prev, dq_prev, dt, q, occ_ptr, paint_ptr,   # noqa: E731
                                                                        n_occ, k, noise, f, pixels, None, stream)
    elif scenes is not None:
        per_scene = _vision.lib().uvs_camera_features_scenes_f64
        occ_ptr, n_occ = (None, 0) if occ is None else occ[:2]
        paint_ptr = None if paint is None else paint[0]
        detect = lambda k, q_prev, dq_prev, q, noise, f, pixels: per_scene(*scenes, npts, T, q_prev, dq_prev, dt, q, occ_ptr, paint_ptr, n_occ,   # noqa: E731
                                                                           k, noise, f, pixels, None, stream)
    elif paint is not None:
        painted = _vision.lib().uvs_camera_features_painted_f64
        detect = lambda k, q_prev, dq_prev, q, noise, f, pixels: painted(cam_ref, T, q_prev, dq_prev, dt, q, occ[0], paint[0], occ[1], k, noise,   # noqa: E731
                                                                         f, pixels, None, stream)
    elif occ is None:
        plain = _vision.lib().uvs_camera_features_f64
        detect = lambda k, q_prev, dq_prev, q, noise, f, pixels: plain(cam_ref, T, q_prev, dq_prev, dt, q, noise, f, pixels, None, stream)   # noqa: E731
    else:
        occluded = _vision.lib().uvs_camera_features_occluded_f64
        detect = lambda k, q_prev, dq_prev, q, noise, f, pixels: occluded(cam_ref, T, q_prev, dq_prev, dt, q, occ[0], occ[1], k, noise, f,   # noqa: E731
                                                                          pixels, None, stream)
    if latency is not None:
        torch = _torch()
        sensed = torch.empty((steps, T, 2 * npts), dtype=torch.float64, device=dev)
        counts = torch.zeros((steps, T, npts), dtype=torch.int32, device=dev)
        sense, delay_row = detect, _vision.lib().uvs_delay_features_f64

        def detect(k, q_prev, dq_prev, q, noise, f, pixels):
            rc = sense(k, q_prev, dq_prev, q, None, sensed.data_ptr() + k * sensed.stride(0) * 8, counts.data_ptr() + k * counts.stride(0) * 4)
            return rc if rc else delay_row(T, npts, k, latency, sensed.data_ptr(), counts.data_ptr(), noise, f, pixels, stream)
    if hold == 0:
        return detect
    miss = _torch().zeros((T, 4), dtype=_torch().int32, device=dev)
    hold_row = _vision.lib().uvs_hold_features_f64

    def held_step(k, q_prev, dq_prev, q, noise, f, pixels, f_prev, held):
        rc = detect(k, q_prev, dq_prev, q, noise, f, pixels)
        return rc if rc else hold_row(T, npts, hold, k, f_prev, f, pixels, miss.data_ptr(), held, stream)
    return held_step


# What asks for each flavour of a one-launch pixel loop, highest flavour first: the flavours are a chain, so the entry point of a call is the
# one of the highest flavour anything given asks for (``_vision.ESTIMATOR_LOOPS`` / ``BASELINE_LOOPS`` name them, lowest first).
ESTIMATOR_LOOP_ASKS = ('x', 'predict', 'assumed', 'latency', 'motion', 'scenes', 'paint', 'hold', 'occluders', 'trial_params')
BASELINE_LOOP_ASKS = ('predict', 'assumed', 'latency', 'motion', 'scenes', 'believed')


def _loop_entry(asks, entries, given):
    flavour = max((len(asks) - rank for rank, name in enumerate(asks) if name in given), default=0)
    return entries[flavour]


def _estimator_loop_entry(given):
    """The estimator loop entry point for a call in which the members of ``given`` -- names of ``ESTIMATOR_LOOP_ASKS`` -- are given ('x': in want)."""
    from . import _vision
    return _loop_entry(ESTIMATOR_LOOP_ASKS, _vision.ESTIMATOR_LOOPS, given)


def _baseline_loop_entry(given):
    """The baseline loop entry point for a call in which the members of ``given`` -- names of ``BASELINE_LOOP_ASKS`` -- are given."""
    from . import _vision
    return _loop_entry(BASELINE_LOOP_ASKS, _vision.BASELINE_LOOPS, given)


def _camera_closed_loop_analytical(fp, cam, q_start, noise, fused, want, believed=None, occ=None, hold=0, paint=None, scenes=None, motion=None,
                                   latency=None, assumed=None, predict=None):
    """camera_closed_loop for fp.method == ANALYTICAL: the one launch (fused) or K x (camera features, analytical step) on rows of the logs.
    ``believed``: None, or the (pointer, n_believed, index pointer) of ``_believed_operand`` -- the law then runs on those models.
    ``occ``: None, or the occluder operand of the stepwise loop (the one launch has none).  ``hold`` > 0 (stepwise alone): a third launch per
    step, uvs_hold_features_f64, between the two.  ``paint``: None, or the paint operand next to ``occ`` (stepwise alone).
    ``scenes``: None, or the (pointer, n_cams, index pointer) of ``_scene_operand`` -- every trial's frames come from its own camera
    (stepwise: uvs_camera_features_scenes_f64); ``believed`` is then given, and
    ``cam`` is the shape alone.  ``motion``: None, or the pointer of ``_motion_operand`` next to ``scenes`` -- the sensor side's discs move
    (stepwise: uvs_camera_features_moving_f64); the law's model does not.
    ``latency``: None, or the pointer of ``_latency_operand`` next to ``scenes`` -- the detector is handed the frame of step max(k - d, 0)
    (stepwise: uvs_delay_features_f64 behind the features call); the law's joints are the current ones.
    ``assumed``: None, or the (pointer, int32 tensor) of ``_latency_operand`` for the ASSUMED latencies next to ``scenes`` -- the joints the
    law is handed at step k are those of step max(k - a, 0) (stepwise: per trial that row of the q log, gathered by torch indexing -- a
    copy, no arithmetic).
    ``predict``: None, or the (pointer, int32 tensor) of ``_latency_operand`` for the prediction HORIZONS next to ``scenes`` -- the law is
    handed f^ = f + (h(q_k) - h(q_{max(k - p, 0)})), h the projection of its own model (stepwise: two uvs_camera_project_scenes_f64 calls
    on the law's models, at row k of the q log and at the per-trial gather of rows max(k - p_t, 0), and the two torch operations of the
    rule on the launches' stream).  The f log stays the reported row.
    The one launch is the entry point ``_baseline_loop_entry`` names for the operands given: the highest flavour any of them needs."""
    from . import _vision
    torch = _torch()
    K, m, n, npts = fp.steps, fp.m, fp.n, cam.n_points
    T, dev = q_start.shape[0], q_start.device
    f64 = dict(dtype=torch.float64, device=dev)
    q0 = _operand(q_start, 'q_start', torch.float64, (T, n))
    noise_ptr = _operand(noise, 'noise', torch.float64, (K, T, m), True)
    comps = dict(err=m, q=n, f=m, dq=n)
    if fused:
        log = {key: torch.empty((K, T, comps[key]), **f64) for key in ANALYTICAL_CAMERA_LOGS if key in want}
        ptr = lambda key: log[key].data_ptr() if key in log else None   # noqa: E731
        status, k_done = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(2))
        stats = torch.empty((T, 3), **f64)
        pixels = torch.empty((T, npts), dtype=torch.int32, device=dev)
        first = lambda operand: None if operand is None else operand[0]   # noqa: E731
        given = dict(predict=predict, assumed=assumed, latency=latency, motion=motion, scenes=scenes, believed=believed)
        values = dict(fp=C.byref(fp), cam=C.byref(cam), motion=motion, latency=latency, assumed=first(assumed), predict=first(predict), T=T,
                      q_start=q0, noise=noise_ptr, q_log=ptr('q'), f_log=ptr('f'), dq_log=ptr('dq'), err_log=ptr('err'), status=status.data_ptr(),
                      k_done=k_done.data_ptr(), stats=stats.data_ptr(), pixels=pixels.data_ptr(), stream=_stream())
        values.update(zip(('cams', 'n_cams', 'cam_index'), scenes or (None, 0, None)))
        values.update(zip(('believed', 'n_believed', 'believed_index'), believed or (None, 0, None)))
        _vision.check(_vision.call_loop(_baseline_loop_entry({name for name, operand in given.items() if operand is not None}), values))
        return dict(log, pixels=pixels, status=status, k_done=k_done, stats=stats)
    log = {key: torch.empty((K, T, comp), **f64) for key, comp in comps.items()}
    status_log = torch.zeros((K, T), dtype=torch.int32, device=dev)
    pixel_log = torch.zeros((K, T, npts), dtype=torch.int32, device=dev)
    cam_ref, fp_ref, stream = C.byref(cam), C.byref(fp), _stream()
    features = _features_step(cam_ref, T, fp.dt, occ, stream, hold, npts, dev, paint, scenes, motion, latency, K)
    held_log = torch.zeros((K, T, npts), dtype=torch.int32, device=dev) if hold else None
    if believed is None:
        step = lambda *rows: _vision.lib().uvs_camera_analytical_step_f64(fp_ref, cam_ref, T, *rows)          # noqa: E731
    else:
        step = lambda *rows: _vision.lib().uvs_camera_believed_step_f64(fp_ref, T, *believed, *rows)          # noqa: E731
    row = {key: (t.data_ptr(), t.stride(0) * t.element_size()) for key, t in dict(log, status=status_log, pixels=pixel_log).items()}
    if hold:
        row['held'] = (held_log.data_ptr(), held_log.stride(0) * held_log.element_size())
    at = lambda key, k: row[key][0] + k * row[key][1]                # noqa: E731
    noise_row = 0 if noise is None else noise.stride(0) * 8
    if assumed is not None or predict is not None:
        trials = torch.arange(T, device=dev)
    if assumed is not None:
        told = assumed[1].to(torch.int64)
    if predict is not None:                                          # h of the law's models: zeros stay where a trial has no model (it starts FAILed)
        horizon = predict[1].to(torch.int64)
        h_now, h_then = (torch.zeros((T, npts, 3), **f64) for _ in range(2))
        project = lambda joints, out: _vision.lib().uvs_camera_project_scenes_f64(*believed, npts, T, joints, None, 0.0, None, out.data_ptr(),  # noqa: E731
                                                                                  stream)
    for k in range(K):
        q_prev, dq_prev = (q0, None) if k == 0 else (at('q', k - 1), at('dq', k - 1))
        extra = (None if k == 0 else at('f', k - 1), at('held', k)) if hold else ()
        _vision.check(features(k, q_prev, dq_prev, at('q', k), None if noise is None else noise_ptr + k * noise_row, at('f', k), at('pixels', k),
                               *extra))
        joints = at('q', k)
        if assumed is not None:                                      # the joints the assumed frame shows: row max(k - a_t, 0) of the q log, per trial
            told_q = log['q'][(k - told).clamp_(min=0), trials]
            joints = told_q.data_ptr()
        feats = at('f', k)
        if predict is not None:                                      # f^ = f + (h(q_k) - h(q_{max(k - p_t, 0)})): the difference first, then one add
            shown_q = log['q'][(k - horizon).clamp_(min=0), trials]
            _vision.check(project(at('q', k), h_now))
            _vision.check(project(shown_q.data_ptr(), h_then))
            moved = (h_now[:, :, :2] - h_then[:, :, :2]).reshape(T, m)
            predicted = log['f'][k] + moved
            feats = predicted.data_ptr()
        _vision.check(step(joints, feats, at('dq', k), at('err', k), None, at('status', k), stream))
    return _reduce_camera_logs(fp, log, status_log, pixel_log, want, held_log)


def _reduce_camera_logs(fp, log, status_log, pixel_log, want, held_log=None):
    """k_done, status, pixels and stats of a stepwise pixel loop from its per-step status words and mask sizes -- and, where the loop holds
    lost discs, 'held' from its per-step held flags (K, T, n_points): the steps pixels looks at."""
    torch = _torch()
    K, dev = status_log.shape[0], status_log.device
    failed = status_log != 0
    steps = torch.arange(K, device=dev, dtype=torch.int32)[:, None]
    k_done = torch.where(failed, steps, torch.full_like(steps, K)).amin(0)          # the first FAIL, else K
    status = (k_done < K).to(torch.int32)
    seen = steps <= k_done[None, :]                                  # the failing step's own masks count: an empty one shows as 0
    pixels = torch.where(seen[:, :, None], pixel_log, torch.full_like(pixel_log, 2 ** 31 - 1)).amin(0)
    out = dict({key: t for key, t in log.items() if key in want}, pixels=pixels, status=status, k_done=k_done)
    if held_log is not None:
        out['held'] = torch.where(seen[:, :, None], held_log, torch.zeros_like(held_log)).sum(0, dtype=torch.int32)
    out['stats'] = stats_reduce(log['err'], _loop_times(fp.dt, K), k_done, layout='ktc')
    return out


def _check_camera_trial_params(trial_params, n_in):
    """What can be said of camera_closed_loop's ``trial_params`` on the host alone, before any device work: ValueError, or (the number of
    output trials, 'source' as a checked host int32 array | the caller's device tensor | None)."""
    import torch                                                     # not _torch(): these refusals need no GPU
    if not isinstance(trial_params, dict):
        raise ValueError(f'camera_closed_loop: trial_params is a dict with keys of {TRIAL_PARAM_KEYS}')
    unknown = set(trial_params) - set(TRIAL_PARAM_KEYS)
    if unknown:
        raise ValueError(f'camera_closed_loop: trial_params: unknown keys {sorted(unknown)}; known: {TRIAL_PARAM_KEYS}')
    source = trial_params.get('source')
    if source is None:
        return n_in, None
    if torch.is_tensor(source) and source.is_cuda:                   # the kernel FAILs a trial whose index names no input trial
        if source.dim() != 1:
            raise ValueError("camera_closed_loop: trial_params['source'] is (T,) integers, one per output trial")
        return source.shape[0], source
    host = np.asarray(source.numpy() if torch.is_tensor(source) else source)
    if host.ndim != 1 or host.dtype.kind not in 'iu':
        raise ValueError("camera_closed_loop: trial_params['source'] is (T,) integers, one per output trial")
    if host.size and (host.min() < 0 or host.max() >= n_in):
        raise ValueError(f"camera_closed_loop: trial_params['source'] must lie in [0, {n_in}), the trials q_start holds, got "
                         f'{int(host.min())} .. {int(host.max())}')
    return host.shape[0], np.ascontiguousarray(host, np.int32)


def _camera_trial_params_struct(trial_params, T, n_in, m, dev):
    """(uvs_camera_trial_params over the tensors of ``trial_params``, tensors to keep alive): closed_loop's shapes and dtypes."""
    from . import _vision
    torch = _torch()
    _, source = _check_camera_trial_params(trial_params, n_in)
    tp = _vision.CameraTrialParams(None, None, None, None, None, None, n_in)
    keep = []
    for key, value in trial_params.items():
        if value is None:
            continue
        if key == 'source':
            value = source if torch.is_tensor(source) else torch.from_numpy(source).to(dev)
        shape, dtype = ((T, m), torch.float64) if key == 'desired' else ((T,), torch.int32 if key == 'source' else torch.float64)
        if not torch.is_tensor(value) or tuple(value.shape) != shape or value.dtype != dtype or value.device != dev or not value.is_contiguous():
            raise ValueError(f'camera_closed_loop: trial_params[{key!r}]: a contiguous {dtype} tensor of shape {shape} on {dev} is needed, got '
                             f'{getattr(value, "dtype", type(value))} {tuple(getattr(value, "shape", ()))} on {getattr(value, "device", "the host")}')
        setattr(tp, key, value.data_ptr())
        keep.append(value)
    return tp, keep


def _camera_closed_loop_fused(fp, cam, q_start, noise, x0, guess, want, trial_params=None, occluders=None, hold=0, paints=None, scenes=None,
                              motion=None, latency=None, assumed=None, predict=None):
    """camera_closed_loop(fused=True): at most three launches and no host loop.  ``trial_params``: None, or the dict of camera_closed_loop --
    then q_start, noise and x0 hold the n_in input trials, and T, the number of output trials, is len(source) where there is one.
    ``occluders``: None, or what ``_check_occluders`` returned for the T output trials (there is no 'source' next to them: see
    ``_gather_by_source``).  ``hold`` > 0: the result has 'held'.  ``paints``: None, or what ``_check_occluder_colours`` returned next to
    ``occluders``.  ``scenes``: None, or the (operand, packed cameras, index tensor or None) of
    ``_scene_operand`` for the T output trials (no 'source' next to them either);
    f0 comes from the step-0 frame of every trial's own scene, and x0 is given (camera_closed_loop has made it).
    A fourth member, True, says that the one scene is the NOMINAL camera standing in for a moving launch without ``cameras``: ``cam`` is then
    the model of every trial, and guess='device' may still make x0 from it.
    ``motion``: None, or the (pointer, packed tensor) of ``_motion_operand`` for the T output trials next to ``scenes``; f0 comes from the
    step-0 frame, where s(0) applies.
    ``latency``: None, or the (pointer, int32 tensor) of ``_latency_operand`` for the T output trials next to ``scenes``; f0 still comes
    from the step-0 frame.
    ``assumed``, ``predict``: None, or the (pointer, int32 tensor) of ``_latency_operand`` for the ASSUMED latencies and the prediction
    HORIZONS of the T output trials next to ``scenes``.
    'x' in ``want`` (camera_closed_loop has made ``scenes``): the result has 'x' (K, T, m n): X_k after step k's update, rows k < k_done.
    The launch is the entry point ``_estimator_loop_entry`` names for what is given: the highest flavour any of it asks for, whatever else
    is given or not.  ``motion``, ``latency``, ``assumed``, ``predict`` and 'x' REQUIRE ``scenes``: their entry points take the scene operand
    where the lower ones take ``cam``, and without it the library refuses the call (NULL cams)."""
    from . import _vision
    torch = _torch()
    K, m, n, npts = fp.steps, fp.m, fp.n, cam.n_points
    scene_kw = {} if scenes is None else dict(cameras=scenes[1], camera_index=scenes[2])
    if motion is not None:
        scene_kw['target_motion'] = motion[1]
    n_in, dev = q_start.shape[0], q_start.device
    T = n_in if trial_params is None else _check_camera_trial_params(trial_params, n_in)[0]
    tp, _keep = (None, ()) if trial_params is None else _camera_trial_params_struct(trial_params, T, n_in, m, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    q0 = _operand(q_start, 'q_start', torch.float64, (n_in, n))
    noise_ptr = _operand(noise, 'noise', torch.float64, (K, n_in, m), True)
    f0 = torch.zeros((n_in, m), **f64)
    occ = None if occluders is None else _occluder_operand(occluders, dev)
    paint = None if paints is None else _paint_operand(paints, dev)
    if fp.initial_guess:                                             # the step-0 frame, occluders at k = 0 and their paints included
        camera_features(cam, q_start, out=f0, occluders=None if occ is None else occ[2], occluder_colours=None if paint is None else paint[1],
                        **scene_kw)
        if x0 is None and guess == 'device' and (scenes is None or scenes[3]):
            x0 = camera_guess(cam, q_start, f0)
    if x0 is None:
        raise ValueError("camera_closed_loop: fused=True takes x0, or guess='device' with fp.initial_guess")
    X0 = torch.as_tensor(x0, **f64).reshape(n_in, m * n).contiguous()
    comps = dict(err=m, q=n, f=m, dq=n, kappa=m, x=m * n)
    log = {key: torch.empty((K, T, comps[key]), **f64) for key in ESTIMATOR_CAMERA_LOGS if key in want}
    ptr = lambda key: log[key].data_ptr() if key in log else None   # noqa: E731
    status, k_done = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.empty((T, 3), **f64)
    pixels = torch.empty((T, npts), dtype=torch.int32, device=dev)
    held = torch.empty((T, npts), dtype=torch.int32, device=dev) if hold else None
    first = lambda operand: None if operand is None else operand[0]   # noqa: E731
    given = dict(x='x' in log or None, predict=predict, assumed=assumed, latency=latency, motion=motion, scenes=scenes, paint=paint,
                 hold=hold or None, occluders=occ, trial_params=tp)
    values = dict(fp=C.byref(fp), cam=C.byref(cam), motion=first(motion), latency=first(latency), assumed=first(assumed), predict=first(predict),
                  T=T, tp=None if tp is None else C.byref(tp), occ=first(occ), paint=first(paint), n_occ=0 if occ is None else occ[1], hold=hold,
                  q_start=q0, noise=noise_ptr, x0=X0.data_ptr(), f0=f0.data_ptr(), q_log=ptr('q'), f_log=ptr('f'), dq_log=ptr('dq'),
                  err_log=ptr('err'), kappa_log=ptr('kappa'), x_log=ptr('x'), status=status.data_ptr(), k_done=k_done.data_ptr(),
                  stats=stats.data_ptr(), pixels=pixels.data_ptr(), held=None if held is None else held.data_ptr(), stream=_stream())
    values.update(zip(('cams', 'n_cams', 'cam_index'), (None, 0, None) if scenes is None else scenes[0]))
    _vision.check(_vision.call_loop(_estimator_loop_entry({name for name, operand in given.items() if operand is not None}), values))
    out = dict(log, pixels=pixels, status=status, k_done=k_done, stats=stats)
    return dict(out, held=held) if hold else out


def _gather_by_source(q_start, noise, x0, trial_params):
    """Occluders belong to OUTPUT trials, and with them the step-0 frame, f0 and the initial guess: where 'source' and occluders meet, the
    inputs are gathered by source here (torch, on the device) and the launch runs without an index.  Returns (q_start, noise, x0,
    trial_params without 'source').  'source' was checked on the host, or is the caller's device tensor, whose range is checked here."""
    torch = _torch()
    source = trial_params['source']
    n_in, dev = q_start.shape[0], q_start.device
    index = source.to(torch.int64) if torch.is_tensor(source) else torch.as_tensor(np.asarray(source), dtype=torch.int64)
    index = index.to(dev)
    if index.numel() and bool(((index < 0) | (index >= n_in)).any()):
        raise ValueError(f"camera_closed_loop: trial_params['source'] must lie in [0, {n_in}) next to occluders")
    if x0 is not None:
        x0 = torch.as_tensor(x0, dtype=torch.float64, device=dev).reshape(n_in, -1).index_select(0, index)
    return (q_start.index_select(0, index).contiguous(), None if noise is None else noise.index_select(1, index).contiguous(), x0,
            {key: value for key, value in trial_params.items() if key != 'source'})


def _loop_camera(fp, plant, radius):
    """camera_closed_loop's uvs_camera of ``plant``; ValueError unless its shape is fp's."""
    from . import plant as plant_mod
    cam = _camera(plant, plant_mod.DISC_RADIUS if radius is None else radius)
    if fp.m != 2 * cam.n_points or fp.n != cam.n_joints:
        raise ValueError(f'camera_closed_loop: fp is ({fp.m}, {fp.n}) but the camera gives {2 * cam.n_points} features of {cam.n_joints} joints')
    return cam


def camera_closed_loop(fp, plant, q_start, noise=None, radius=None, x0=None, *, fused=False, guess='host', want=CAMERA_LOGS, believed=None,
                       believed_index=None, trial_params=None, occluders=None, hold=0, occluder_colours=None, cameras=None, camera_index=None,
                       target_motion=None, motion_window=None, latency=None, assumed_latency=None, predict=None):
    """T closed-loop trials THROUGH PIXELS: at every step the features are what the centre-of-mass detector returns for the 256 x 256 frame of the
    plant's discs (pixel quantisation included), not the ideal projection ``closed_loop`` feeds.  ``plant``: a ``SyntheticPlant``; ``radius``: disc
    radius in metres (default plant.DISC_RADIUS); ``q_start`` (T, n) cuda fp64; ``noise`` (K, T, m) cuda fp64 or None; ``x0`` (T, m*n) array-like, or
    None: with fp.initial_guess the analytic guess (plant.analytic_guess) per trial from the noise-free detection at q_start -- which is also
    the first step's f_old (zeros without initial_guess, where x0 must be given).
    Step k is two launches on the current stream and no synchronisation: uvs_camera_features_f64 (q_log[k-1], dq_log[k-1] -> q_log[k], f_log[k])
    and uvs_rmckf_step_f64 (-> dq_log[k], err_log[k], kappa_log[k], status_log[k]), each on rows of the logs, which are plain (K, T, comp)
    tensors.  A disc that leaves the frame gives NaN features, a non-finite X and FAIL at that step, as the reference's loop ends on a NaN
    detection.  Returns a dict: 'err', 'q', 'f', 'dq', 'kappa' (K, T, comp; rows at and after k_done unspecified), 'pixels' (T, n_points) the
    smallest mask per colour over the steps up to and including k_done, 'status', 'k_done' (T,) int32, 'stats' (T, 3).
    ``fused=True`` runs the same loop as ONE launch (uvs_camera_closed_loop_f64: the filter state stays in registers over the K steps) and
    returns the same bits; ``want`` names the logs to return (the others are neither allocated nor written).  ``guess='device'`` computes the
    initial guess with ``camera_guess`` instead of the per-trial host loop, under either value of ``fused``: equal to the host's to about
    1e-13, not in the last bits.  With fused=True a ``Camera`` struct is accepted for ``plant`` when x0 is given or guess='device'.
    ``fp.method == ANALYTICAL`` runs the calibrated IBVS baseline through the same pixels instead of an estimator: fused=True is one launch
    (uvs_camera_analytical_loop_f64), fused=False K x (uvs_camera_features_f64, uvs_camera_analytical_step_f64) with the same reduction, and
    the two return the same bits.  It takes no ``x0`` and no ``guess`` (ValueError), ``want`` is a subset of ('err', 'q', 'f', 'dq') --
    there is no 'kappa' -- and ``plant`` may be a ``Camera`` struct.
    ``believed`` (what ``believed_models`` returns or takes) and ``believed_index`` ((T,) integers, host or device) separate the camera that
    renders the frames -- always ``plant`` -- from the model the control side believes in, per trial: with an index trial t believes in
    ``believed[believed_index[t]]``, without one in the one model there is, or in ``believed[t]`` of T.  With ANALYTICAL the law runs on the
    believed model at every step (fused=True: uvs_camera_believed_loop_f64, one launch; fused=False: K x (uvs_camera_features_f64 on the true
    camera, uvs_camera_believed_step_f64); the same bits, and with the true model as ``believed`` the bits of the call without it).  With an
    estimator the believed models feed the initial guess alone (``camera_guess(believed=...)``) and the estimator's loop is untouched; that
    needs guess='device', and guess='host' or an explicit ``x0`` next to ``believed`` is a ValueError, like ``believed_index`` without
    ``believed`` and a host-side index out of range.
    ``trial_params``: per-trial estimator parameters, ONE launch for a whole hyperparameter grid through pixels
    (uvs_camera_closed_loop_grid_f64): a dict with any of the keys of ``TRIAL_PARAM_KEYS``, in ``closed_loop``'s shapes and dtypes --
    'kernel_bw', 'gain', 'reg', 'fpi_threshold' ((T,) fp64 cuda tensors), 'desired' ((T, m)) and 'source' ((T,) int32 on the device, or host
    integers: trial t reads q_start / noise / x0 and the first f_old of input trial source[t]).  With 'source' T is len(source) and
    ``q_start`` / ``noise`` / ``x0`` hold n_in = q_start.shape[0] trials, over which f0 and the initial guess are computed; every output has
    T trials.  A host-side 'source' outside [0, n_in) is a ValueError; one on the device makes its trial FAIL with k_done = 0, alone.  A
    trial's results are bit-identical to those of the uniform fused call with its values; ``{}`` is that call through the per-trial
    kernel, None (the default) the uniform call itself.  It needs fused=True (the two-launch step has no per-trial flavour) and an
    estimator (not ANALYTICAL), and excludes ``believed``: each a ValueError before any device work.
    ``occluders``: rectangles that slide in front of the discs while the loop runs, per OUTPUT trial -- what ``occluders()`` takes or returns:
    (T, n_occ, 8) or (n_occ, 8) integer rows (x, y, w, h, vx, vy, k_on, k_off), n_occ <= 4 (the rule: include/uvs_vision.h, uvs_occluder;
    ``plant.render_discs`` states it).  The detection of step k is that of the frame with the occluders at step k; f0, the first f_old, and
    with it the initial guess, come from the step-0 frame, occluders at k = 0 included.  fused=False passes k to
    uvs_camera_features_occluded_f64 at every step, for the estimators and for the calibrated and believed baselines alike; fused=True with an
    estimator is ONE launch, uvs_camera_closed_loop_occluded_f64, with or without ``trial_params``, and returns the stepwise loop's bits.
    fused=True with ANALYTICAL and occluders is a ValueError -- use fused=False: the baseline's one-launch loop has no occluders.  A disc
    that is covered completely has an empty mask: NaN features and FAIL at that step, like a disc that leaves the frame.  Next to
    trial_params['source'] the inputs are gathered by source before the launch (an out-of-range index is then a ValueError, also on the
    device), because the step-0 frame belongs to the output trial.
    ``hold``: an integer >= 0, one for the call: the largest number of consecutive steps for which a LOST disc's pair is held -- the rule of
    ``plant.hold_features`` (include/uvs_vision.h, HOLDING a lost disc's last detection).  A disc is lost at step k iff its mask is empty there,
    behind an occluder or out of the frame alike; from step 1 on, and while its run of misses is shorter than ``hold``, the loop reports
    step k - 1's pair again (that step's noise in it, none of step k's) instead of NaN, and the estimator or the law takes it like any
    other.  Once the hold is used up, and at step 0, a lost disc is the NaN pair and FAIL of above.  0 (the default) is the call without
    the argument: its routes, its entry points, its bits.  With hold > 0 the result has 'held' (T, n_points) int32: the steps up to and
    including k_done at which each disc was held ('pixels' still shows the smallest mask, 0 after a hold).  fused=True with an estimator
    is ONE launch (uvs_camera_closed_loop_held_f64), with or without ``occluders`` and ``trial_params``; fused=False is three launches per
    step (uvs_hold_features_f64 between the two) for the estimators and the calibrated and believed baselines alike; the two return the
    same bits.  fused=True with ANALYTICAL and hold > 0 is a ValueError -- use fused=False: the baseline's one-launch loops hold nothing.
    ``occluder_colours``: the PAINT of every occluder, per OUTPUT trial like the occluders -- (n_occ,) or (T, n_occ) integers, or a packed
    int32 tensor (T, n_occ): p in 0 .. n_points - 1 paints the rectangle the colour of disc p, a DISTRACTOR whose pixels enter that
    colour's mask and pull its centroid; -1 leaves it opaque (the rule: ``plant.render_discs(occluder_colours=)``; include/uvs_vision.h).
    The detector never reports a loss for a colour whose distractor is visible, so ``hold`` does not step in there.  f0 and the initial
    guess come from the step-0 frame, painted rectangles included.  None (the default) is the call without the argument.  fused=True with
    an estimator is ONE launch, uvs_camera_closed_loop_painted_f64, with or without ``trial_params`` and for any ``hold``; fused=False
    passes the paints to uvs_camera_features_painted_f64 at every step, for the estimators and the calibrated and believed baselines
    alike; the two return the same bits.  It needs ``occluders`` (ValueError), and fused=True with ANALYTICAL stays the ValueError it is
    for occluders.
    ``cameras`` (what ``camera_scenes`` returns or takes) and ``camera_index`` ((T,) integers per OUTPUT trial, host or device): a SCENE per
    trial -- the camera that renders trial t's frames is ``cameras[camera_index[t]]``, or without an index the one camera there is, or
    ``cameras[t]`` of T -- so that a Monte-Carlo over true cameras (focal length, target positions and sizes, hand-eye geometry) is one
    batch.  None (the default) is the call without the arguments: its routes, its entry points, its bits.  With cameras ``plant`` stays the
    NOMINAL model: it gives the shape.  fused=True with an estimator is ONE launch (uvs_camera_closed_loop_scenes_f64) with any of
    ``trial_params``, ``occluders``, ``occluder_colours`` and ``hold``; fused=False passes the scenes to uvs_camera_features_scenes_f64 at
    every step, for the estimators and for ANALYTICAL alike; the two return the same bits, and trial t has the bits of the call without
    cameras on its own camera.  ANALYTICAL runs the law on ``believed`` / ``believed_index`` if given, otherwise on the trial's own scene
    (fused=True: uvs_camera_believed_loop_scenes_f64; fused=False: uvs_camera_believed_step_f64 behind the scenes' features); with
    occluders or hold > 0 fused=True stays the ValueError it is.  Estimators: f0 and the initial guess come from the step-0 frame of the
    trial's own scene; guess='device' computes the guess on ``believed`` if given, otherwise on the trial's scene
    (uvs_camera_believed_guess_f64); guess='host' without ``x0`` next to cameras is a ValueError.  Next to trial_params['source'] the inputs
    are gathered by source before the launch, as next to occluders.  A trial whose device-side index names no camera FAILs with
    k_done = 0, alone.  ValueErrors before any device work: ``camera_index`` without ``cameras``, a host-side index out of range or of the
    wrong length, a model whose shape is not fp's.
    ``target_motion`` and ``motion_window``: MOVING TARGETS, per OUTPUT trial -- (n_points, 3) or (T, n_points, 3) world velocities in
    metres per step and None, (2,) or (T, 2) integer windows (k_on, k_off), or what ``target_motions`` returns for both.  At step k trial
    t's discs stand where s(k) = clamp(k - k_on, 0, max(k_off - k_on, 0)) steps of its motion have taken them (the rule:
    ``plant.target_at``; include/uvs_vision.h, uvs_target_motion); projection, pixels, occluders, paints and hold follow as they are.  The
    controller does not know the motion: the calibrated law's model -- ``believed``, or the trial's own camera -- and every initial guess
    keep the points where they were.  None (the default) is the call without the arguments: its routes, its entry points, its bits.
    Without ``cameras`` the nominal camera is packed as the one scene.  fused=True with an estimator is ONE launch
    (uvs_camera_closed_loop_moving_f64) with any of ``trial_params``, ``occluders``, ``occluder_colours``, ``hold`` and ``cameras``;
    fused=False passes the motions and k to uvs_camera_features_moving_f64 at every step; the two return the same bits.  f0 and the
    initial guess come from the step-0 frame, where s(0) applies.  ANALYTICAL: fused=True is uvs_camera_believed_loop_moving_f64 (with
    occluders or hold > 0 it stays the ValueError it is), fused=False the moving features call, then uvs_camera_believed_step_f64.  Next
    to trial_params['source'] the inputs are gathered by source before the launch, as next to occluders.  ValueErrors before any device
    work: a wrong shape or dtype, a window without a motion, T rows of motion for a different T, window entries outside int32.
    ``latency``: CAMERA LATENCY, per OUTPUT trial -- an integer, or T integers (a sequence, an array or an integer tensor), each in
    0 .. ``MAX_LATENCY`` control periods.  At step k trial t's detector is handed the frame of step kk = max(k - latency[t], 0) -- the
    joints, occluders, paints and target motion of step kk (the rule: ``plant.delayed_step``; include/uvs_vision.h, CAMERA LATENCY); the
    noise added to that detection is step k's, and the hold rule, the estimator or the law follow on it as they are.  The controller is
    not told: the law's joints are the current q_k, the estimators' regressor is dq_{k-1}.  'f' logs the reported rows, 'pixels' is the
    smallest mask among the detections reported up to and including k_done.  f0 and the initial guess come from the step-0 frame.  None
    (the default) is the call without the argument: its routes, its entry points, its bits; zeros give the same bits through the
    delayed kernels.  Without ``cameras`` the nominal camera is packed as the one scene, as with motion.  fused=True with an estimator is
    ONE launch (uvs_camera_closed_loop_delayed_f64) with any of ``trial_params``, ``occluders``, ``occluder_colours``, ``hold``,
    ``cameras`` and ``target_motion``; with ANALYTICAL it is uvs_camera_believed_loop_delayed_f64 (with occluders or hold > 0 it stays the
    ValueError it is).  fused=False, for the estimators and ANALYTICAL alike, is per step the features call without noise into a log of
    sensed rows, uvs_delay_features_f64, then the hold call and the step as before; the two return the same bits.  Next to
    trial_params['source'] the inputs are gathered by source before the launch, as next to occluders.  ValueErrors before any device
    work, after the refusals above: a value outside 0 .. ``MAX_LATENCY``, a wrong length, non-integers.
    ``assumed_latency``: ASSUMED LATENCY, per OUTPUT trial -- the controller is TOLD a latency a, in the same form and range as ``latency``
    and independent of it: a != latency is the mismatch experiment, and a > 0 without any latency is legal.  Estimators: the regressor
    of step k is the command of step k - 1 - a, or the zero vector where there is none (the rule: ``plant.aligned_regressor_step``;
    include/uvs_vision.h, ASSUMED LATENCY) -- the command that caused f_k - f_{k-1} when the latency is a; the command integrated into
    the joints stays dq_{k-1}.  ANALYTICAL (calibrated or believed): the joints the law is handed are q_{max(k - a, 0)}
    (``plant.delayed_step(k, a)``), so its Jacobian, depths and interaction matrix are those of the pose the assumed frame shows; the
    features stay the reported row, the 'q' log stays current.  None (the default) is the call without the argument: its routes, its
    entry points, its bits; zeros give the same bits through the aligned kernels.  It combines with everything ``latency`` combines
    with, in the same way: fused=True is ONE launch (uvs_camera_closed_loop_aligned_f64, or uvs_camera_believed_loop_aligned_f64 for
    ANALYTICAL, where occluders or hold > 0 stay the ValueError they are); fused=False hands the step call, per trial, row k - 1 - a of
    the 'dq' log (or zeros) as dq_prev, or row max(k - a, 0) of the 'q' log as joints, gathered by torch indexing; the two return the
    same bits.  Next to trial_params['source'] it is by output trial.  ValueErrors before any device work, after the refusals above,
    latency's included: the same as for ``latency``, naming assumed_latency.
    ``predict``: FEATURE PREDICTION, per OUTPUT trial -- a prediction HORIZON p, in the same form and range as ``latency`` and independent
    of it and of ``assumed_latency``: p != latency is the mismatch experiment, and p > 0 without any latency is legal.  The control law
    acts on the reported row advanced over the last p commands (the steps: ``plant.prediction_steps``; include/uvs_vision.h, FEATURE
    PREDICTION).  Estimators: err = (f + X_k s) - desired after the update, s the sum of those commands newest first; z, kappa, the 'f'
    log and the regressor are untouched.  ANALYTICAL: the law is handed f + (h(q_k) - h(q_{max(k - p, 0)})), h the (u, v) of
    ``camera_project`` on its own model -- the believed model of the trial, else its scene, else the nominal camera.  The 'err' log and
    the stats are on the PREDICTED error, so they are not comparable across p; the 'f' log stays the reported row.  None (the default)
    is the call without the argument: its routes, its entry points, its bits; zeros give the same bits through the predicted kernels.
    fused=True is ONE launch (uvs_camera_closed_loop_predicted_f64, or uvs_camera_believed_loop_predicted_f64 for ANALYTICAL, where
    occluders or hold > 0 stay the ValueError they are) and combines with everything ``assumed_latency`` combines with, in the same way.
    fused=False: ANALYTICAL projects the law's models at rows k and max(k - p, 0) of the 'q' log and applies the rule's two torch
    operations per step, with the one launch's bits; the estimators refuse (ValueError 'predict needs fused=True': the two-launch step
    forms err inside libuvs_rmckf.so).  Next to trial_params['source'] it is by output trial.  ValueErrors before any device work, after
    assumed_latency's: the same as for ``latency``, naming predict.
    ``'x'`` in ``want`` (``ESTIMATOR_CAMERA_LOGS`` is ``CAMERA_LOGS + ('x',)``; ``CAMERA_LOGS`` stays the default): THE ESTIMATE AS A LOG, for
    the estimators -- the result has 'x' (K, T, m n): row k is X_k, the matrix after step k's update, the one step k's control law (and
    prediction) read; element i n + j is X[i][j], the layout of ``x0``; rows at and after k_done are unspecified, like those of 'err'.
    fused=True is ONE launch through uvs_camera_closed_loop_logged_f64, whatever else is given: the nominal camera stands in as the one
    scene, exactly as for ``latency`` without ``cameras`` (six joints, or a ValueError), and ``x0`` / ``guess`` are handled as on that
    route.  fused=False copies the step kernel's X tensor into row k after every step call; the two return the same bits.  ANALYTICAL has
    no 'x': the ValueError it always was.  Without 'x' every call takes the route and the entry point it always took.
    ``camera_jacobian_score`` takes the result: ``camera_jacobian_score(plant=plant, dt=fp.dt, **{k: out[k] for k in ('x', 'q', 'dq',
    'k_done')})``."""
    from . import _vision, plant as plant_mod
    if guess not in ('host', 'device'):
        raise ValueError("camera_closed_loop: guess is 'host' or 'device'")
    if cameras is None and camera_index is not None:
        raise ValueError('camera_closed_loop: camera_index without cameras')
    analytical = fp.method == _lib.METHOD_ANALYTICAL
    if cameras is not None:
        n_out = getattr(q_start, 'shape', (0,))[0]
        if isinstance(trial_params, dict) and trial_params.get('source') is not None:
            n_out = _check_camera_trial_params(trial_params, q_start.shape[0])[0]
        _check_cameras(cameras, camera_index, n_out, fp.m // 2, fp.n, 'camera_closed_loop')
        if not analytical and x0 is None and guess == 'host':
            raise ValueError("camera_closed_loop: next to cameras the host has no per-trial kinematics for the initial guess: pass x0, or "
                             "guess='device'")
    hold = _check_hold(hold)
    if hold and analytical and fused:
        raise ValueError('camera_closed_loop: the calibrated baseline has no one-launch loop that holds a lost disc: use fused=False')
    if occluders is not None:
        if analytical and fused:
            raise ValueError('camera_closed_loop: the calibrated baseline has no one-launch loop with occluders: use fused=False')
        n_out = q_start.shape[0]
        if isinstance(trial_params, dict) and trial_params.get('source') is not None:
            n_out = _check_camera_trial_params(trial_params, q_start.shape[0])[0]
        occluders = _check_occluders(occluders, n_out, who='camera_closed_loop: occluders')
    paints = _check_occluder_colours(occluder_colours, occluders, None if occluders is None else occluders.shape[0], fp.m // 2,
                                     'camera_closed_loop')
    n_out = getattr(q_start, 'shape', (0,))[0]
    if isinstance(trial_params, dict) and trial_params.get('source') is not None and (target_motion is not None or motion_window is not None):
        n_out = _check_camera_trial_params(trial_params, q_start.shape[0])[0]
    motion = _check_target_motion(target_motion, motion_window, n_out, fp.m // 2, 'camera_closed_loop')
    nominal = motion is not None and cameras is None                 # the nominal camera stands in as the one scene of a moving launch
    if nominal and fp.n != 6:
        raise ValueError(f'camera_closed_loop: the moving-target kernels are built for the six-joint arms of this project, not for {fp.n} joints')
    if trial_params is not None:
        if not fused:
            raise ValueError('camera_closed_loop: trial_params needs fused=True: the two-launch step kernel has no per-trial flavour')
        if analytical:
            raise ValueError('camera_closed_loop: trial_params are estimator parameters: the calibrated baseline (ANALYTICAL) takes none')
        if believed is not None or believed_index is not None:
            raise ValueError('camera_closed_loop: trial_params and believed models do not combine')
        _check_camera_trial_params(trial_params, q_start.shape[0])
    if believed is None and believed_index is not None:
        raise ValueError('camera_closed_loop: believed_index without believed')
    if believed is not None and not analytical:
        if x0 is not None or guess != 'device':
            raise ValueError("camera_closed_loop: with an estimator the believed models feed the device's initial guess alone: "
                             "guess='device' and no x0")
        if not fp.initial_guess:
            raise ValueError('camera_closed_loop: believed models need fp.initial_guess (they feed the analytic initial guess)')
    if believed is not None:                                         # a host-side index out of range is refused here, before any device work
        _check_believed(believed, believed_index, q_start.shape[0], 'camera_closed_loop')
    if analytical:                                                   # refused on the arguments alone, before anything is looked at
        if x0 is not None or guess != 'host':
            raise ValueError('camera_closed_loop: the calibrated baseline estimates nothing: it takes no x0 and no guess')
        want = ANALYTICAL_CAMERA_LOGS if want is CAMERA_LOGS else tuple(want)
        unknown = [key for key in want if key not in ANALYTICAL_CAMERA_LOGS]
        if unknown:
            raise ValueError(f'camera_closed_loop: the calibrated baseline logs {ANALYTICAL_CAMERA_LOGS}, it has no {unknown}')
    n_out = getattr(q_start, 'shape', (0,))[0]
    checked = []                                                     # each None, or (T,) int32 on the host, by output trial
    for name, value in (('latency', latency), ('assumed_latency', assumed_latency), ('predict', predict)):
        if value is not None and trial_params is not None and trial_params.get('source') is not None:
            n_out = _check_camera_trial_params(trial_params, q_start.shape[0])[0]
        checked.append(_check_latency(value, n_out, 'camera_closed_loop', name))
    delays, tolds, horizons = checked
    if horizons is not None and not analytical and not fused:
        raise ValueError('camera_closed_loop: predict needs fused=True: the two-launch step kernel forms the error the law acts on itself')
    if (delays is not None or tolds is not None or horizons is not None) and cameras is None and not nominal:   # the nominal camera stands in as the one scene here too
        if fp.n != 6:
            raise ValueError(f'camera_closed_loop: the camera-latency kernels are built for the six-joint arms of this project, not for {fp.n} joints')
        nominal = True
    want_x = not analytical and 'x' in tuple(want)                   # the estimate itself as a log: X_k of every step
    if want_x and fused and cameras is None and not nominal:         # the one-launch X log is a scenes kernel: the nominal camera stands in here too
        if fp.n != 6:
            raise ValueError(f"camera_closed_loop: the kernels that log 'x' are built for the six-joint arms of this project, not for {fp.n} joints")
        nominal = True
    if fused and not getattr(q_start, 'is_cuda', False):
        raise ValueError('camera_closed_loop: q_start must be on the device (the logs are allocated next to it)')
    torch = _torch()
    if (occluders is not None or cameras is not None or motion is not None or delays is not None or tolds is not None or horizons is not None) \
            and trial_params is not None \
            and trial_params.get('source') is not None:
        q_start, noise, x0, trial_params = _gather_by_source(q_start, noise, x0, trial_params)
    K, m, n = fp.steps, fp.m, fp.n
    T, dev = q_start.shape[0], q_start.device
    if K < 1 or T < 1:
        raise ValueError('camera_closed_loop: at least one step (fp.steps) and one trial')
    if not q_start.is_cuda:
        raise ValueError('camera_closed_loop: q_start must be on the device (the logs are allocated next to it)')
    scenes, scene_kw = None, {}                                      # the scene operand of the T output trials, and what the calls below take
    if nominal:
        cameras = [_loop_camera(fp, plant, radius)]
    if cameras is not None:
        scenes = _scene_operand(cameras, camera_index, T, m // 2, n, radius, dev, 'camera_closed_loop') + (nominal,)
        scene_kw = dict(cameras=scenes[1], camera_index=scenes[2])
    mot = None if motion is None else _motion_operand(motion, dev)   # (pointer, packed tensor) of the T output trials
    if mot is not None:
        scene_kw['target_motion'] = mot[1]
    lat = None if delays is None else _latency_operand(delays, dev)  # (pointer, int32 tensor) of the T output trials
    told = None if tolds is None else _latency_operand(tolds, dev)   # likewise, the assumed latencies
    ahead = None if horizons is None else _latency_operand(horizons, dev)   # likewise, the prediction horizons
    if analytical:
        cam = _loop_camera(fp, plant, radius)
        occ = None if occluders is None else _occluder_operand(occluders, dev)
        paint = None if paints is None else _paint_operand(paints, dev)
        if believed is None and scenes is None:
            return _camera_closed_loop_analytical(fp, cam, q_start, noise, fused, want, occ=occ, hold=hold, paint=paint)
        if believed is None:                                         # the calibrated law on every trial's own scene
            operand = scenes[0]
        else:
            *operand, _keep = _believed_operand(believed, believed_index, T, radius, dev, 'camera_closed_loop')
        return _camera_closed_loop_analytical(fp, cam, q_start, noise, fused, want, tuple(operand), occ=occ, hold=hold, paint=paint,
                                              scenes=None if scenes is None else scenes[0], motion=None if mot is None else mot[0],
                                              latency=None if lat is None else lat[0], assumed=told, predict=ahead)
    if believed is not None or (scenes is not None and not nominal and x0 is None):  # an estimator that starts from a model in memory: the believed one, or
        cam = _loop_camera(fp, plant, radius)                        # its own scene; the rest is the x0= path
        if not fp.initial_guess:
            raise ValueError('camera_closed_loop: x0 is needed when fp.initial_guess is 0 (the reference draws it unseeded, experiment.py:117)')
        models, index = (believed, believed_index) if believed is not None else (scenes[1], scenes[2])
        x0 = camera_guess(cam, q_start, camera_features(cam, q_start, occluders=occluders, occluder_colours=paints, **scene_kw), radius=radius,
                          believed=models, believed_index=index)
    if fused and (x0 is not None or guess == 'device' or not fp.initial_guess):
        cam = _loop_camera(fp, plant, radius)
        return _camera_closed_loop_fused(fp, cam, q_start, noise, x0, guess, tuple(want), trial_params, occluders, hold, paints, scenes, mot, lat, told, ahead)
    if not isinstance(plant, plant_mod.SyntheticPlant):
        raise ValueError('camera_closed_loop: plant must be a SyntheticPlant (the analytic initial guess needs its host kinematics)')
    cam = _loop_camera(fp, plant, radius)
    npts = cam.n_points
    q0 = _operand(q_start, 'q_start', torch.float64, (T, n))
    noise_ptr = _operand(noise, 'noise', torch.float64, (K, T, m), True)
    f64 = dict(dtype=torch.float64, device=dev)
    f0 = torch.zeros((T, m), **f64)
    occ = None if occluders is None else _occluder_operand(occluders, dev)
    paint = None if paints is None else _paint_operand(paints, dev)
    if fp.initial_guess:                                             # the step-0 frame, occluders at k = 0 and their paints included
        camera_features(cam, q_start, out=f0, occluders=None if occ is None else occ[2], occluder_colours=None if paint is None else paint[1],
                        **scene_kw)
        if x0 is None and guess == 'device':
            x0 = camera_guess(cam, q_start, f0)
        if x0 is None:
            f_host, q_host = f0.cpu().numpy(), q_start.cpu().numpy()
            x0 = np.empty((T, m * n))
            robot = plant_mod.SyntheticRobot(plant, fp.dt)
            for t in range(T):
                robot.start(q_host[t])
                x0[t] = plant_mod.analytic_guess(robot, f_host[t], (plant_mod.RESOLUTION, plant_mod.RESOLUTION), m, n)
    if x0 is None:
        raise ValueError('camera_closed_loop: x0 is needed when fp.initial_guess is 0 (the reference draws it unseeded, experiment.py:117)')
    X = torch.as_tensor(x0, **f64).reshape(T, m * n).clone()
    if fused:                                                        # the host guess is in hand: the rest is the one launch
        return _camera_closed_loop_fused(fp, cam, q_start, noise, X, guess, tuple(want), trial_params, None if occ is None else occ[2], hold,
                                         None if paint is None else paint[1], scenes, mot, lat, told, ahead)
    P = torch.eye(n, **f64).repeat(T, m, 1, 1).contiguous()          # P = I (experiment.py:73)
    log = {key: torch.empty((K, T, comp), **f64) for key, comp in (('err', m), ('q', n), ('f', m), ('dq', n), ('kappa', m))}
    x_log = torch.empty((K, T, m * n), **f64) if want_x else None    # row k: the step kernel's X after step k
    status_log = torch.zeros((K, T), dtype=torch.int32, device=dev)
    pixel_log = torch.zeros((K, T, npts), dtype=torch.int32, device=dev)
    dq_zero = torch.zeros((T, n), **f64)
    step = _lib.lib().uvs_rmckf_step_f64
    cam_ref, fp_ref, stream = C.byref(cam), C.byref(fp), _stream()
    features = _features_step(cam_ref, T, fp.dt, occ, stream, hold, npts, dev, paint, None if scenes is None else scenes[0],
                              None if mot is None else mot[0], None if lat is None else lat[0], K)
    held_log = torch.zeros((K, T, npts), dtype=torch.int32, device=dev) if hold else None
    row = {key: (t.data_ptr(), t.stride(0) * t.element_size()) for key, t in dict(log, status=status_log, pixels=pixel_log).items()}
    if hold:
        row['held'] = (held_log.data_ptr(), held_log.stride(0) * held_log.element_size())
    at = lambda key, k: row[key][0] + k * row[key][1]                # noqa: E731
    noise_row = 0 if noise is None else noise.stride(0) * 8
    if told is not None:
        assumed, trials = told[1].to(torch.int64), torch.arange(T, device=dev)
    for k in range(K):
        q_prev, dq_prev, f_old = (q0, None, f0.data_ptr()) if k == 0 else (at('q', k - 1), at('dq', k - 1), at('f', k - 1))
        extra = (None if k == 0 else f_old, at('held', k)) if hold else ()
        _vision.check(features(k, q_prev, dq_prev, at('q', k), None if noise is None else noise_ptr + k * noise_row, at('f', k), at('pixels', k),
                               *extra))
        regressor = dq_zero.data_ptr() if k == 0 else dq_prev
        if told is not None and k > 0:                               # per trial row k - 1 - a_t of the dq log, or the zero row: a copy
            rows = k - 1 - assumed
            told_dq = torch.where((rows >= 0)[:, None], log['dq'][rows.clamp(min=0), trials], dq_zero)
            regressor = told_dq.data_ptr()
        _lib.check(step(fp_ref, T, X.data_ptr(), P.data_ptr(), at('f', k), f_old, regressor, int(k == 0), k,
                        at('dq', k), at('err', k), at('kappa', k), at('status', k), stream))
        if x_log is not None:
            x_log[k].copy_(X)
    if x_log is not None:
        log['x'] = x_log
    return _reduce_camera_logs(fp, log, status_log, pixel_log, want, held_log)


def _loop_times(t_s, K):
    """The first K times of ``loop_clock``: t_s accumulated in floating point."""
    ts, t = [], 0.0 + t_s
    for _ in range(K):
        ts.append(t)
        t += t_s
    return np.array(ts)


class FilterBank:
    """T estimators whose state (X, P) stays in HBM between ``step`` calls: the drop-in used when the robot is external."""

    def __init__(self, fp, T=1, x0=None, device='cuda'):
        torch = _torch()
        self.fp, self.T = fp, T
        m, n = fp.m, fp.n
        self.X = torch.zeros((T, m * n), dtype=torch.float64, device=device)
        if x0 is not None:
            self.X.copy_(torch.as_tensor(np.asarray(x0, float).reshape(T, m * n)))
        self.P = torch.eye(n, dtype=torch.float64, device=device).repeat(T, m, 1, 1).contiguous()   # P = I (experiment.py:73)
        self.dq = torch.zeros((T, n), dtype=torch.float64, device=device)
        self.err = torch.zeros((T, m), dtype=torch.float64, device=device)
        self.kappa = torch.ones((T, m), dtype=torch.float64, device=device)
        self.status = torch.zeros(T, dtype=torch.int32, device=device)
        self.first = True
        self._host = None
        self._image, self._f_last = None, None                      # step_image's own records; the features its next call takes as f_old

    def _host_io(self):
        """Pinned host records the step kernel reads and writes in place (zero-copy: hipHostMalloc memory is mapped into the device's address
        space at the same address): two input records [f | f_old] and two output records [dq | err | kappa], status words, used alternately so
        that call k reads the command of call k - 1 as its regressor.  numpy views are made once."""
        torch = _torch()
        m, n, T = self.fp.m, self.fp.n, self.T
        pin = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype).pin_memory()      # noqa: E731
        h = dict(f=pin(2, T, m), f_old=pin(2, T, m), dq=pin(2, T, n), err=pin(2, T, m), kappa=pin(2, T, m), status=pin(2, T, dtype=torch.int32))
        h['np'] = {k_: v.numpy() for k_, v in h.items()}
        ptr = {k_: [v[i].data_ptr() for i in (0, 1)] for k_, v in h.items() if k_ != 'np'}
        fn = _lib.lib().uvs_rmckf_step_f64
        fpref = C.byref(self.fp)
        # everything of the call that does not change from step to step, per parity
        h['call'] = [lambda first, k, dq_prev, stream, i=i: fn(fpref, self.T, self.X.data_ptr(), self.P.data_ptr(), ptr['f'][i], ptr['f_old'][i],
                                                                dq_prev, first, k, ptr['dq'][i], ptr['err'][i], ptr['kappa'][i],
                                                                ptr['status'][i], stream) for i in (0, 1)]
        h['ptr'], h['calls'] = ptr, 0
        return h

    def step_host(self, f, f_old, k, dq_prev=None):
        """The drop-in step for a caller whose data lives on the HOST (Experiment.run() with an external robot, experiment.py:166-312): ``f``,
        ``f_old`` (T, m) array-likes; ``dq_prev`` (T, n) or None = the command the previous call returned (zero on the first).  No device copy
        in either direction and no allocation: the kernel reads the inputs from and writes its outputs to pinned host memory; one launch, one
        stream synchronisation.  Returns numpy views (dq (T, n), err (T, m), kappa (T, m), status (T,)) that stay valid until the next call
        but one; X and P stay in HBM."""
        h = self._host
        if h is None:
            h = self._host = self._host_io()
        i = h['calls'] & 1
        views = h['np']
        views['f'][i][...] = f
        views['f_old'][i][...] = f_old
        if dq_prev is not None:
            views['dq'][1 - i][...] = dq_prev
        stream = _torch().cuda.current_stream()
        _lib.check(h['call'][i](int(self.first), int(k), h['ptr']['dq'][1 - i], C.c_void_p(stream.cuda_stream)))
        self.first = False
        h['calls'] += 1
        stream.synchronize()
        return views['dq'][i], views['err'][i], views['kappa'][i], views['status'][i]

    def set_features(self, f0):
        """The features in hand before the first ``step_image`` call -- the reference's ``f`` ahead of its loop: zeros, or the initial-guess
        detection (experiment.py:76, :89).  The first call's f_old (experiment.py:128)."""
        self._f_last = np.broadcast_to(np.asarray(f0, float), (self.T, self.fp.m)).copy()

    def _image_io(self):
        """What ``step_image`` adds to the pinned records of ``_host_io``: a frame buffer for callers that hand over numpy arrays, two noise
        records, and the detector call of each parity with everything that does not change from step to step."""
        from . import _vision
        torch = _torch()
        m, T = self.fp.m, self.T
        if m // 2 not in _vision.N_COLOURS or m % 2:
            raise ValueError(f'step_image: m = {m} features are not those of a circle detector (2, 6 or 8)')
        h = self._host
        noise = torch.zeros((2, T, m), dtype=torch.float64).pin_memory()
        fn = _vision.lib().uvs_detect_circles_u8
        img = dict(frames=None, shape=(T, _vision.SIDE, _vision.SIDE, 3), stride=_vision.SIDE * _vision.SIDE * 3,
                   noise=noise, noise_np=noise.numpy(), noise_ptr=[noise[i].data_ptr() for i in (0, 1)])
        img['call'] = [lambda src, stride, noise_ptr, stream, i=i: fn(T, src, stride, _vision.SIDE, _vision.SIDE, m // 2, noise_ptr,
                                                                      h['ptr']['f'][i], None, stream) for i in (0, 1)]
        img['check'] = _vision.check
        if self._f_last is None:
            self.set_features(np.zeros(m))
        return img

    def step_image(self, frames, k, noise=None, dq_prev=None):
        """The fused live step: detector and estimator of one loop iteration (experiment.py:127-312) as two launches on one stream and one
        synchronisation.  ``frames``: (T, 256, 256, 3) uint8 -- a numpy array (copied into a pinned buffer this bank owns) or a torch tensor
        that is pinned or on the device (read in place); one (256, 256, 3) frame when T = 1.  ``noise`` (T, m) array-like or None is added to
        the detection on the device.  The detector writes f into this call's pinned input record; f_old is the f of the previous
        ``step_image`` call, noise included (experiment.py:128), and on the first call what ``set_features`` was given (default zeros).
        Returns numpy views (dq, err, kappa, status, f) with the lifetime of ``step_host``'s."""
        h = self._host
        if h is None:
            h = self._host = self._host_io()
        img = self._image
        if img is None:
            img = self._image = self._image_io()
        i = h['calls'] & 1
        views = h['np']
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise ValueError('step_image: frames must be uint8')
            if img['frames'] is None:                                # allocated once, on the first numpy frame
                img['frames'] = _torch().zeros(img['shape'], dtype=_torch().uint8).pin_memory()
                img['frames_np'] = img['frames'].numpy()
            img['frames_np'][...] = frames.reshape(img['shape'])
            src, stride = img['frames'].data_ptr(), img['stride']
        else:
            frames, T = _frames_arg(frames)
            if tuple(frames.shape) != img['shape']:
                raise ValueError(f'step_image: frames {tuple(frames.shape)} for a bank of {self.T} filters, expected {img["shape"]}')
            src, stride = frames.data_ptr(), (frames.stride(0) if T > 1 else img['stride'])
        noise_ptr = None
        if noise is not None:
            img['noise_np'][i][...] = noise
            noise_ptr = img['noise_ptr'][i]
        views['f_old'][i][...] = self._f_last
        if dq_prev is not None:
            views['dq'][1 - i][...] = dq_prev
        stream = _torch().cuda.current_stream()
        handle = C.c_void_p(stream.cuda_stream)
        img['check'](img['call'][i](src, stride, noise_ptr, handle))
        _lib.check(h['call'][i](int(self.first), int(k), h['ptr']['dq'][1 - i], handle))
        self.first = False
        h['calls'] += 1
        stream.synchronize()
        self._f_last = views['f'][i]
        return views['dq'][i], views['err'][i], views['kappa'][i], views['status'][i], views['f'][i]

    def step(self, f, f_old, dq_prev, k):
        """f, f_old: (T, m), dq_prev: (T, n) cuda fp64 tensors.  Updates X, P in place; returns (dq, err, kappa, status)."""
        f, f_old, dq_prev = f.contiguous(), f_old.contiguous(), dq_prev.contiguous()
        rc = _lib.lib().uvs_rmckf_step_f64(C.byref(self.fp), self.T, self.X.data_ptr(), self.P.data_ptr(), f.data_ptr(),
                                           f_old.data_ptr(), dq_prev.data_ptr(), int(self.first), int(k), self.dq.data_ptr(),
                                           self.err.data_ptr(), self.kappa.data_ptr(), self.status.data_ptr(), _stream())
        _lib.check(rc)
        self.first = False
        return self.dq, self.err, self.kappa, self.status


def stats_reduce(err, t, k_done=None, layout='kct'):
    """Per-trial ||ISE||, ||IAE||, ||ITAE|| (results/plot_errorbar.m:39-84) of an error stream tensor."""
    torch = _torch()
    e = as_tkc(err, layout)
    T, K, m = e.shape
    stats = torch.empty((T, 3), dtype=torch.float64, device=err.device)
    t_dev = torch.as_tensor(np.asarray(t, float), device=err.device)
    rc = _lib.lib().uvs_stats_reduce_f64(T, K, m, stream_view(err, layout), t_dev.data_ptr(),
                                         None if k_done is None else k_done.data_ptr(), stats.data_ptr(), _stream())
    _lib.check(rc)
    return stats
