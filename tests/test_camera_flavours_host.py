"""CPU-only tests of how the one-launch pixel loops' 18 entry points are described and chosen in Python: the rows of ``_vision.SYMBOLS`` that
``_vision.ESTIMATOR_LOOP_OPERANDS`` and ``BASELINE_LOOP_OPERANDS`` generate, against the prototypes of include/uvs_vision.h, and the two
choosers of engine.py against the dispatch ladders they replaced, written out here.  Neither test loads a library."""
import ctypes
import itertools
import os
import re

from conftest import ROOT

CTYPE = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}


def test_generated_rows_are_the_headers_prototypes():
    """Each of the 18 rows has the prototype's number of arguments, its int64_t / int32_t / double where the header has them and a pointer
    where it has one, and names its operands as the header does: the call sites pick the arguments by these names."""
    import uvs_amd
    vision = uvs_amd._vision
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    entries = vision.ESTIMATOR_LOOPS + vision.BASELINE_LOOPS
    assert len(vision.ESTIMATOR_LOOPS) == 11 and len(vision.BASELINE_LOOPS) == 7 and len(set(entries)) == 18
    for fn in entries:
        args, (restype, types) = declared(fn), vision.SYMBOLS[fn]
        assert restype is ctypes.c_int and len(types) == len(args) == len(vision.LOOP_OPERANDS[fn]), fn
        for arg, ctype, operand in zip(args, types, vision.LOOP_OPERANDS[fn]):
            if '*' in arg:
                assert ctype is ctypes.c_void_p or ctype is ctypes.POINTER(vision.Camera), (fn, arg)
            else:
                assert ctype is CTYPE[arg.split()[0]], (fn, arg)
            assert arg.split()[-1].lstrip('*') == operand, (fn, arg)


def old_estimator_ladder(x, predict, assumed, latency, motion, scenes, paint, hold, occluders, trial_params):
    if x:
        return 'uvs_camera_closed_loop_logged_f64'
    elif predict:
        return 'uvs_camera_closed_loop_predicted_f64'
    elif assumed:
        return 'uvs_camera_closed_loop_aligned_f64'
    elif latency:
        return 'uvs_camera_closed_loop_delayed_f64'
    elif motion:
        return 'uvs_camera_closed_loop_moving_f64'
    elif scenes:
        return 'uvs_camera_closed_loop_scenes_f64'
    elif paint:
        return 'uvs_camera_closed_loop_painted_f64'
    elif hold:
        return 'uvs_camera_closed_loop_held_f64'
    elif occluders:
        return 'uvs_camera_closed_loop_occluded_f64'
    elif trial_params:
        return 'uvs_camera_closed_loop_grid_f64'
    return 'uvs_camera_closed_loop_f64'


def old_baseline_ladder(predict, assumed, latency, motion, scenes, believed):
    if predict:
        return 'uvs_camera_believed_loop_predicted_f64'
    elif assumed:
        return 'uvs_camera_believed_loop_aligned_f64'
    elif latency:
        return 'uvs_camera_believed_loop_delayed_f64'
    elif motion:
        return 'uvs_camera_believed_loop_moving_f64'
    elif scenes:
        return 'uvs_camera_believed_loop_scenes_f64'
    elif not believed:
        return 'uvs_camera_analytical_loop_f64'
    return 'uvs_camera_believed_loop_f64'


def test_the_choosers_make_the_old_ladders_choices():
    """Every combination of given and absent operands -- 2^10 for the estimators, 'x' in want among them, and 2^6 for the baseline."""
    import uvs_amd
    engine = uvs_amd.engine
    for ladder, chooser, names in ((old_estimator_ladder, engine._estimator_loop_entry, engine.ESTIMATOR_LOOP_ASKS),
                                   (old_baseline_ladder, engine._baseline_loop_entry, engine.BASELINE_LOOP_ASKS)):
        assert names == ladder.__code__.co_varnames[:ladder.__code__.co_argcount]
        seen = set()
        for flags in itertools.product((False, True), repeat=len(names)):
            given = {name for name, flag in zip(names, flags) if flag}
            assert chooser(given) == ladder(*flags), given
            seen.add(chooser(given))
        assert len(seen) == len(names) + 1, 'every flavour is reached'
