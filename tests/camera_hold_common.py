"""Scenes and restatements shared by tests/test_camera_hold_host.py (CPU) and tests/test_gpu_camera_hold.py (GPU): holding a lost disc's last
detection through the pixel loops (include/uvs_vision.h: uvs_camera_closed_loop_held_f64, uvs_hold_features_f64; plant.hold_features is the
rule).

The scenes are occluder rows over the discs of ONE fixed start pose, Q_START.  With gain = 0 the arm never moves, so the discs stay where
``SyntheticPlant.discs(Q_START)`` puts them and the step at which a mask is empty follows from plant.render_discs alone: the CPU file asserts,
from host frames, that every scene is the cover schedule its name says, and the GPU file holds the loops to those schedules."""
import numpy as np

import camera_common as cc
import camera_occluders_common as oc

K = oc.K                                                             # 12 steps, the K of the grid and occluder tests
Q_START = cc.Q_GOAL + np.array([0.02, -0.03, 0.025, 0.01, -0.02, 0.015])
RED, GREEN = 0, 1
RESET_HOLD = 3                                                       # the longer of the two covers of 'twice'


def box_around(disc, margin=4):
    """(x, y, w, h) of a square that contains the disc's whole box of the pixel rule, and ``margin`` more pixels."""
    u, v, r = disc
    half = int(np.ceil(r)) + margin
    return int(np.floor(u)) - half, int(np.floor(v)) - half, 2 * half + 1, 2 * half + 1


def scenes(discs):
    """name -> occluder rows over ``discs`` (4, 3), the discs of the pose the loop stays at."""
    x, y, w, h = box_around(discs[RED])
    red_still = (x, y, w, h, 0, 0)
    green_still = box_around(discs[GREEN]) + (0, 0)
    return {
        'red_run': [(x, y - 48, w, h + 16, 0, 8, 0, oc.INT32_MAX)],  # a rectangle taller than red that slides down over it, 8 rows a step
        'step0': [red_still + oc.ALWAYS],                            # red is empty in the step-0 frame: no hold can help
        'twice': [red_still + (2, 4), red_still + (6, 6 + RESET_HOLD)],              # two covers, detections in between: the counter must reset
        'two_discs': [red_still + (3, 6), green_still + (4, 8)],     # overlapping, different step ranges
    }


def host_schedule(uvs, discs, rows, steps=K):
    """(steps, 4) mask counts of the static ``discs`` behind ``rows``, step by step, from host frames and the reference's thresholds."""
    return np.stack([cc.host_counts(uvs.plant.render_discs(discs, 4, occluders=rows, k=k)) for k in range(steps)])


def runs(counts):
    """The runs of zeros in one disc's counts over the steps: [(first step, length), ...]."""
    out, k = [], 0
    counts = [int(c) for c in counts]
    while k < len(counts):
        if counts[k] == 0:
            first = k
            while k < len(counts) and counts[k] == 0:
                k += 1
            out.append((first, k - first))
        else:
            k += 1
    return out


def hold_restated(f, f_prev, pixels, miss, hold):
    """The rule once more, in plain Python over lists and by another route than plant.hold_features: disc by disc.
    Returns (f, miss, held) as nested lists."""
    f = [list(row) for row in np.asarray(f, float).tolist()]
    miss = [list(row) for row in np.asarray(miss).tolist()]
    held = [[0] * len(row) for row in miss]
    for t, row in enumerate(np.asarray(pixels).tolist()):
        for j, count in enumerate(row):
            if count != 0:
                miss[t][j] = 0
                continue
            if f_prev is None or not miss[t][j] < hold:
                continue
            f[t][2 * j], f[t][2 * j + 1] = float(f_prev[t][2 * j]), float(f_prev[t][2 * j + 1])
            miss[t][j] += 1
            held[t][j] = 1
    return f, miss, held


def outcome(counts, hold):
    """What the rule makes of a (steps, n) cover schedule when nothing else FAILs: (k_done, held per disc up to and including k_done)."""
    steps, n = np.asarray(counts).shape
    miss, held = [0] * n, [0] * n
    for k in range(steps):
        failed = False
        for j in range(n):
            if counts[k][j] != 0:
                miss[j] = 0
            elif k >= 1 and miss[j] < hold:
                miss[j] += 1
                held[j] += 1
            else:
                failed = True
        if failed:
            return k, held
    return steps, held


# ------------------------------------------------------------------------------------------------------------- the moving arm's bars
def wide_bar():
    """One row: a full-height bar 48 px wide -- twice a disc's diameter at the start poses of the loop tests (about 23 px; 17 px at the
    goal) -- that moves right 13 px a step from the left edge, where no disc starts: it crosses the discs during the transient and empties
    each mask for two or three steps."""
    return (0, 0, 48, cc.SIDE, 13, 0, 0, oc.INT32_MAX)


def counter_bar():
    """One row: a full-height bar 30 px wide that moves LEFT 12 px a step from column 226: next to wide_bar it empties other discs over
    other step ranges."""
    return (226, 0, 30, cc.SIDE, -12, 0, 0, oc.INT32_MAX)
