"""Scenes shared by tests/test_camera_occluders_host.py (CPU) and tests/test_gpu_camera_occluders.py (GPU): occluders -- rows
(x, y, w, h, vx, vy, k_on, k_off) of include/uvs_vision.h's uvs_occluder, columns and FLIPPED rows -- over the static scenes of camera_common
that matter here, the extremes of the integer rule, and the bar that sweeps the frame while a loop runs.  The CPU file asserts, from host
frames, that every scene is the case its name says; the GPU file holds the kernels to plant.render_discs on them."""
import numpy as np

import camera_common as cc

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
K = 12
ALWAYS = (0, INT32_MAX)
NEVER = (0, 0, 0, 0, 0, 0, 0, 0)                                     # no size and no steps: pads a set to four rows
STATIC_SCENES = ('overlap_four', 'clip_corner', 'whole_frame', 'fixture_0')
STEPS = (0, 1, K - 1)                                                # the steps the static scenes are rendered at


def scene(name):
    n, discs = cc.edge_scenes()[name]
    assert n == 4
    return np.asarray(discs, float)


def still(x, y, w, h):
    return (int(x), int(y), int(w), int(h), 0, 0) + ALWAYS


def targets(discs):
    """(first, second): the disc the partial covers aim at -- green, or red where the scene draws no green (whole_frame) -- and red."""
    return (discs[1] if discs[1][2] >= 0 else discs[0]), discs[0]


def slack_column(disc):
    """A column of the disc's box that the rule gives no pixel (the slack of disc_box) and that the clip left in the box, or None:
    (column, +1 | -1 for the side of the box it is on)."""
    (x0, x1), _ = cc.disc_box(disc)
    u, _, r = disc
    if x1 == int(np.floor(u + r + 1.0)) and x1 <= cc.SIDE - 1 and not cc.rule_mask(disc)[:, x1].any():
        return x1, +1
    if x0 == int(np.ceil(u - r - 1.0)) and x0 >= 0 and not cc.rule_mask(disc)[:, x0].any():
        return x0, -1
    return None


def static_covers(discs):
    """name -> list of occluder rows (1 .. 4) for one static scene; every row is still and always active."""
    first, red = targets(discs)
    u, v, r = first
    left, top, size = int(np.floor(u - r)) - 2, int(np.floor(v - r)) - 2, int(np.ceil(2 * r)) + 5
    half = still(left, top, int(np.floor(u)) - left + 1, size)      # columns up to floor(u): the left half
    upper = still(left, top, size, int(np.floor(v)) - top + 1)
    ru, rv, rr = red
    whole_red = still(np.floor(ru - rr) - 1, np.floor(rv - rr) - 1, np.ceil(2 * rr) + 3, np.ceil(2 * rr) + 3)
    mid_u, mid_v = (discs[0][0] + discs[1][0]) / 2, (discs[0][1] + discs[1][1]) / 2
    covers = {
        'half': [half],
        'red_entirely': [whole_red],
        'two_overlapping': [half, upper],
        'disc_overlap': [still(np.floor(mid_u) - 4, np.floor(mid_v) - 4, 9, 9)],
        'four': [half, still(discs[2][0] - 1, discs[2][1] - 30, 3, 60), upper, still(discs[3][0] - 30, discs[3][1], 60, 2)],
    }
    slack = slack_column(first)
    if slack is not None:                                            # meets the box in its slack column only: the box's rows, two columns outward
        column, side = slack
        (_, _), (y0, y1) = cc.disc_box(first)
        covers['slack_column'] = [still(column if side > 0 else column - 1, y0, 2, y1 - y0 + 1)]
    return covers


def extremes():
    """name -> one occluder row: the corners of the integer rule.  To be evaluated at every step of STEPS."""
    return {
        'min_x_max_vx': (INT32_MIN, 10, INT32_MAX, 40, INT32_MAX, 0) + ALWAYS,      # k = 1: x_k = -1; k = K - 1: far off the right side
        'max_w': (-5, 100, INT32_MAX, 20, 0, 0) + ALWAYS,
        'max_w_max_x': (INT32_MAX, 100, INT32_MAX, 20, 0, 0) + ALWAYS,               # x + w - 1 is past int32
        'max_h_moving_up': (120, 250, 30, INT32_MAX, 0, -20) + ALWAYS,
        'negative_w': (100, 100, -3, 50, 0, 0) + ALWAYS,
        'negative_h': (100, 100, 50, -3, 0, 0) + ALWAYS,
        'zero_w': (100, 100, 0, 50, 0, 0) + ALWAYS,
        'on_equals_off': (100, 100, 50, 50, 0, 0, 1, 1),
        'off_before_on': (100, 100, 50, 50, 0, 0, 5, 1),
        'one_step_only': (100, 100, 50, 50, 0, 0, 1, 2),
        'off_left': (-20, 100, 20, 50, 0, 0) + ALWAYS,                              # last column -1
        'off_right': (256, 100, 20, 50, 0, 0) + ALWAYS,
        'off_top': (100, -20, 50, 20, 0, 0) + ALWAYS,
        'off_bottom': (100, 256, 50, 20, 0, 0) + ALWAYS,
        'one_column_left': (-19, 0, 20, 256, 0, 0) + ALWAYS,                        # column 0 alone
        'corner_pixel': (255, 255, 9, 9, 0, 0) + ALWAYS,
        'whole_frame': (INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, 1, 2),   # k = 1: from (-1, -1) on
    }


def rects_restated(row, k):
    """The rule once more, in plain Python integers and by another route than plant.occluder_rects: the set of covered columns and the set
    of covered flipped rows, by membership over the 256 frame indices."""
    x, y, w, h, vx, vy, k_on, k_off = (int(v) for v in row)
    if not (k_on <= k and k < k_off) or w <= 0 or h <= 0:
        return (), ()
    xk, yk = x + vx * k, y + vy * k
    cols = tuple(j for j in range(cc.SIDE) if xk <= j <= xk + w - 1)
    rows = tuple(i for i in range(cc.SIDE) if yk <= i <= yk + h - 1)
    return (cols, rows) if cols and rows else ((), ())


def padded(rows, n=4):
    """(n, 8) int64: the rows, then occluders that never cover anything."""
    rows = [tuple(int(v) for v in r) for r in rows]
    assert len(rows) <= n
    return np.array(rows + [NEVER] * (n - len(rows)), np.int64).reshape(n, 8)


def static_batch(name):
    """(names, discs (T, 4, 3), occluders (T, 4, 8)) of one static scene: a trial per cover set, then a trial per extreme."""
    discs = scene(name)
    sets = dict(static_covers(discs))
    sets.update({'extreme_' + key: [row] for key, row in extremes().items()})
    names = list(sets)
    return names, np.broadcast_to(discs, (len(names), 4, 3)).copy(), np.stack([padded(sets[key]) for key in names])


# ------------------------------------------------------------------------------------------------------------- the loops' occluders
BAR_W, BAR_X0, BAR_V = 12, 60, 12                                    # the sweeping bar: 12 px wide, full height, a width per step


def sweeping_bar(k_on=0, k_off=INT32_MAX):
    """One row: columns [60 + 12 k, 71 + 12 k], every row -- over K = 12 steps it passes every column from 60 to 203 exactly once."""
    return (BAR_X0, 0, BAR_W, cc.SIDE, BAR_V, 0, k_on, k_off)


def half_cover(desired, pair=1):
    """One still row over the left half of the green disc where the servo wants it (feature pair 1; pair 0 of a one-disc camera), 29 px
    high around it."""
    u, v = desired[2 * pair], desired[2 * pair + 1]
    return still(np.floor(u) - 14, np.floor(v) - 14, 15, 29)


def covered_counts(uvs, discs, occluders, k):
    """(solo, covered, with): mask sizes per colour of the discs alone each, of the scene, and of the scene behind the occluders at step k."""
    solo = []
    for c in range(4):
        alone = cc.pad([])
        alone[c] = discs[c]
        solo.append(cc.host_counts(uvs.plant.render_discs(alone))[c])
    return np.array(solo), cc.host_counts(uvs.plant.render_discs(discs)), cc.host_counts(uvs.plant.render_discs(discs, occluders=occluders, k=k))
