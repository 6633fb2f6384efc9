"""ctypes binding of libuvs_vision.so (include/uvs_vision.h): the circle detectors of the live route and the synthetic camera on the device.

Like ``_lib``: no CPU fallback.  If the HIP library is missing or fails to load, ``lib()`` raises ``UvsLibraryError`` -- the device route
never substitutes the numpy detectors of ``utils``.
"""
import ctypes as C
import os
import subprocess

from ._lib import UvsError, UvsLibraryError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libuvs_vision.so')
CSRC = os.path.join(HERE, 'csrc_vision')

SIDE = 256                                                          # UVS_VISION_SIDE
N_COLOURS = (1, 3, 4)                                               # green | red, green, blue | red, green, blue, pink

MAX_JOINTS, MAX_POINTS = 8, 4                                       # UVS_CAMERA_MAX_JOINTS, UVS_CAMERA_MAX_POINTS
MAX_OCCLUDERS = 4                                                   # UVS_CAMERA_MAX_OCCLUDERS


class Camera(C.Structure):
    """uvs_camera of include/uvs_vision.h (plant.SyntheticPlant.to_camera fills it)."""
    _fields_ = [('n_joints', C.c_int32), ('n_points', C.c_int32),
                ('theta_offset', C.c_double * MAX_JOINTS), ('d', C.c_double * MAX_JOINTS), ('a', C.c_double * MAX_JOINTS),
                ('cos_alpha', C.c_double * MAX_JOINTS), ('sin_alpha', C.c_double * MAX_JOINTS),
                ('points', (C.c_double * 3) * MAX_POINTS), ('focal', C.c_double), ('center', C.c_double),
                ('radius', C.c_double * MAX_POINTS)]


class CameraTrialParams(C.Structure):
    """uvs_camera_trial_params of include/uvs_vision.h: device pointers (None = fp's value, or trial t for 'source') and n_in."""
    _fields_ = [('kernel_bw', C.c_void_p), ('gain', C.c_void_p), ('reg', C.c_void_p), ('fpi_threshold', C.c_void_p),
                ('desired', C.c_void_p), ('source', C.c_void_p), ('n_in', C.c_int64)]


class Occluder(C.Structure):
    """uvs_occluder of include/uvs_vision.h: eight int32, the row layout of the (T, n_occ, 8) tensor ``engine.occluders`` packs."""
    _fields_ = [(name, C.c_int32) for name in ('x', 'y', 'w', 'h', 'vx', 'vy', 'k_on', 'k_off')]


class TargetMotion(C.Structure):
    """uvs_target_motion of include/uvs_vision.h: the row layout of the (T, 104) uint8 tensor ``plant.target_motion_array`` packs."""
    _fields_ = [('v', (C.c_double * 3) * MAX_POINTS), ('k_on', C.c_int32), ('k_off', C.c_int32)]


# name -> (restype, argtypes); every symbol include/uvs_vision.h declares
_VP, _I64, _I32, _F64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
_CAM = C.POINTER(Camera)
SYMBOLS = {
    'uvs_vision_version': (C.c_char_p, []),
    'uvs_vision_last_error': (C.c_char_p, []),
    'uvs_detect_circles_u8': (C.c_int, [_I64, _VP, _I64, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    'uvs_camera_project_f64': (C.c_int, [_CAM, _I64, _VP, _VP, _F64, _VP, _VP, _VP]),
    'uvs_render_discs_u8': (C.c_int, [_I64, _VP, _I32, _I32, _VP, _I64, _VP]),
    'uvs_disc_features_f64': (C.c_int, [_I64, _VP, _I32, _VP, _VP, _VP, _VP]),
    'uvs_camera_features_f64': (C.c_int, [_CAM, _I64, _VP, _VP, _F64, _VP, _VP, _VP, _VP, _VP, _VP]),
    # the three above with the occluder operand (occ: device int32 [T][n_occ][8] or None, n_occ, k; the rasteriser's shade after it)
    'uvs_render_discs_occluded_u8': (C.c_int, [_I64, _VP, _I32, _I32, _VP, _I32, _I32, _I32, _VP, _I64, _VP]),
    'uvs_disc_features_occluded_f64': (C.c_int, [_I64, _VP, _I32, _VP, _I32, _I32, _VP, _VP, _VP, _VP]),
    'uvs_camera_features_occluded_f64': (C.c_int, [_CAM, _I64, _VP, _VP, _F64, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    # the three occluded calls with the paints (device int32 [T][n_occ] or None) directly after occ
    'uvs_render_discs_painted_u8': (C.c_int, [_I64, _VP, _I32, _I32, _VP, _VP, _I32, _I32, _I32, _VP, _I64, _VP]),
    'uvs_disc_features_painted_f64': (C.c_int, [_I64, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP]),
    'uvs_camera_features_painted_f64': (C.c_int, [_CAM, _I64, _VP, _VP, _F64, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    # T, n_points, hold, k, f_prev_row, f_row, pixels_row, miss, held_row, stream
    'uvs_hold_features_f64': (C.c_int, [_I64, _I32, _I32, _I32] + [_VP] * 6),
    'uvs_camera_guess_f64': (C.c_int, [_CAM, _I64, _VP, _VP, _VP, _VP]),
    # fp, cam, T, q, f, dq_out, err_out, j_out, status, stream
    'uvs_camera_analytical_step_f64': (C.c_int, [_VP, _CAM, _I64] + [_VP] * 7),
    # the believed operand is (believed: device array of Camera, n_believed, believed_index: device int32 [T] or None)
    # fp, T, believed operand, q, f, dq_out, err_out, j_out, status, stream
    'uvs_camera_believed_step_f64': (C.c_int, [_VP, _I64, _VP, _I64, _VP] + [_VP] * 7),
    # T, n_points, believed operand, q_start, f0, x0_out, stream
    'uvs_camera_believed_guess_f64': (C.c_int, [_I64, _I32, _VP, _I64, _VP] + [_VP] * 4),
    # the scene operand is (cams: device array of Camera, n_cams, cam_index: device int32 [T] or None): it stands where the namesake has cam
    # scene operand, n_points, T, q_prev, dq, dt, q_out, discs_out, stream
    'uvs_camera_project_scenes_f64': (C.c_int, [_VP, _I64, _VP, _I32, _I64, _VP, _VP, _F64, _VP, _VP, _VP]),
    # scene operand, n_points, T, q_prev, dq, dt, q_out, occ, paint, n_occ, k, noise, f_out, pixels_out, discs_out, stream
    'uvs_camera_features_scenes_f64': (C.c_int, [_VP, _I64, _VP, _I32, _I64, _VP, _VP, _F64, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    # moving targets: the two scenes calls with motion (device array of TargetMotion [T] or None) directly after the scene operand; the
    # project call, which has no k, takes it after dt
    'uvs_camera_project_moving_f64': (C.c_int, [_VP, _I64, _VP, _VP, _I32, _I64, _VP, _VP, _F64, _I32, _VP, _VP, _VP]),
    'uvs_camera_features_moving_f64': (C.c_int, [_VP, _I64, _VP, _VP, _I32, _I64, _VP, _VP, _F64, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP,
                                                 _VP]),
    # T, n_points, k, latency, sensed_log, count_log, noise_row, f_row, pixels_row, stream
    'uvs_delay_features_f64': (C.c_int, [_I64, _I32, _I32] + [_VP] * 7),
    # the true image Jacobian: scene operand, motion, n_points, T, rows, k0, q, j_out, stream
    'uvs_camera_jacobian_f64': (C.c_int, [_VP, _I64, _VP, _VP, _I32, _I64, _I64, _I32, _VP, _VP, _VP]),
    # an X stream scored against it: scene operand, motion, n_points, T, K, dt, x_log, q_log, dq_log, k_done, score, stream
    'uvs_camera_jacobian_score_f64': (C.c_int, [_VP, _I64, _VP, _VP, _I32, _I64, _I64, _F64, _VP, _VP, _VP, _VP, _VP, _VP]),
}

# The one-launch pixel loops.  A family's entry points are a chain of flavours, each the previous one plus operands (csrc_vision/
# camera_loop_device.hpp, camera_analytical_device.hpp): entry point f of a family takes, in this order, the operands of its table whose
# (first, last) flavours enclose f.  Pointers are device pointers or None; fp and tp are structs passed with byref, cam a Camera likewise;
# (cams, n_cams, cam_index) is the scene operand, which stands where the lower flavours have cam; (believed, n_believed, believed_index)
# the believed operand.
ESTIMATOR_LOOPS = tuple('uvs_camera_closed_loop_' + flavour + 'f64' for flavour in (
    '', 'grid_', 'occluded_', 'held_', 'painted_', 'scenes_', 'moving_', 'delayed_', 'aligned_', 'predicted_', 'logged_'))
ESTIMATOR_LOOP_OPERANDS = (
    ('fp', _VP, 0, 10), ('cam', _CAM, 0, 4), ('cams', _VP, 5, 10), ('n_cams', _I64, 5, 10), ('cam_index', _VP, 5, 10), ('motion', _VP, 6, 10),
    ('latency', _VP, 7, 10), ('assumed', _VP, 8, 10), ('predict', _VP, 9, 10), ('T', _I64, 0, 10), ('tp', _VP, 1, 10), ('occ', _VP, 2, 10),
    ('paint', _VP, 4, 10), ('n_occ', _I32, 2, 10), ('hold', _I32, 3, 10), ('q_start', _VP, 0, 10), ('noise', _VP, 0, 10), ('x0', _VP, 0, 10),
    ('f0', _VP, 0, 10), ('q_log', _VP, 0, 10), ('f_log', _VP, 0, 10), ('dq_log', _VP, 0, 10), ('err_log', _VP, 0, 10), ('kappa_log', _VP, 0, 10),
    ('x_log', _VP, 10, 10), ('status', _VP, 0, 10), ('k_done', _VP, 0, 10), ('stats', _VP, 0, 10), ('pixels', _VP, 0, 10), ('held', _VP, 3, 10),
    ('stream', _VP, 0, 10))
BASELINE_LOOPS = ('uvs_camera_analytical_loop_f64',) + tuple('uvs_camera_believed_loop_' + flavour + 'f64' for flavour in (
    '', 'scenes_', 'moving_', 'delayed_', 'aligned_', 'predicted_'))
BASELINE_LOOP_OPERANDS = (
    ('fp', _VP, 0, 6), ('cam', _CAM, 0, 1), ('cams', _VP, 2, 6), ('n_cams', _I64, 2, 6), ('cam_index', _VP, 2, 6), ('motion', _VP, 3, 6),
    ('latency', _VP, 4, 6), ('assumed', _VP, 5, 6), ('predict', _VP, 6, 6), ('T', _I64, 0, 6), ('believed', _VP, 1, 6), ('n_believed', _I64, 1, 6),
    ('believed_index', _VP, 1, 6), ('q_start', _VP, 0, 6), ('noise', _VP, 0, 6), ('q_log', _VP, 0, 6), ('f_log', _VP, 0, 6), ('dq_log', _VP, 0, 6),
    ('err_log', _VP, 0, 6), ('status', _VP, 0, 6), ('k_done', _VP, 0, 6), ('stats', _VP, 0, 6), ('pixels', _VP, 0, 6), ('stream', _VP, 0, 6))
LOOP_OPERANDS = {}                                                  # entry point -> the names of its operands, in the order of its prototype
for _names, _table in ((ESTIMATOR_LOOPS, ESTIMATOR_LOOP_OPERANDS), (BASELINE_LOOPS, BASELINE_LOOP_OPERANDS)):
    for _flavour, _name in enumerate(_names):
        _taken = [row for row in _table if row[2] <= _flavour <= row[3]]
        LOOP_OPERANDS[_name] = tuple(row[0] for row in _taken)
        SYMBOLS[_name] = (C.c_int, [row[1] for row in _taken])

_lib = None


def build(force=False):
    """Compile libuvs_vision.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.run(['make', '-j', str(min(os.cpu_count() or 4, 16)), '-C', CSRC], check=True)        # twenty translation units, one rule each
    return LIB_PATH


def lib():
    """The loaded library with typed entry points; raises UvsLibraryError when it cannot be loaded."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise UvsLibraryError(f'{LIB_PATH} is missing: run `make -C {CSRC}` (or __graft_entry__.build()); '
                                  'there is no CPU fallback for the device detectors')
        try:
            import torch  # noqa: F401  (first, so that one HIP runtime serves torch and this library: see _lib.lib)
            handle = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise UvsLibraryError(f'cannot load {LIB_PATH}: {exc}') from exc
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def call_loop(name, values):
    """Loop entry point ``name`` on the operands it takes, picked by name from ``values`` (a dict that may hold more); its return code."""
    return getattr(lib(), name)(*(values[operand] for operand in LOOP_OPERANDS[name]))


class UvsVisionError(UvsError):
    def __init__(self, code, text):
        RuntimeError.__init__(self, f'libuvs_vision error {code}: {text}')
        self.code = code


def check(code):
    if code != 0:
        raise UvsVisionError(code, lib().uvs_vision_last_error().decode())
