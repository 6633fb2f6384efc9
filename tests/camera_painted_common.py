"""Scenes shared by tests/test_camera_painted_host.py (CPU) and tests/test_gpu_camera_painted.py (GPU): occluders that carry a PAINT -- a disc's
colour: distractors -- over the static scenes of the occluder suite and a few scenes whose discs draw nothing; the owner rule restated pixel
by pixel in plain Python; and the rectangles the loops run behind.  A paint set is (rows, paints): occluder rows of uvs_occluder and one
paint per row (a disc index, or OPAQUE)."""
import numpy as np

import camera_common as cc
import camera_occluders_common as oc

OPAQUE = -1
K = oc.K
SCENES = {name: 4 for name in oc.STATIC_SCENES}
SCENES.update({'not_drawn': 4, 'outside': 4, 'green_alone': 1, 'green_alone_absent': 1, 'rgb': 3, 'rgb_blue_absent': 3})   # (e) and (i)
COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 0, 255))


def scene(name):
    n, discs = cc.edge_scenes()[name]
    assert n == SCENES[name]
    return n, np.asarray(discs, float)


def target(discs):
    """(index, disc) of the disc the paints aim at: green, or the first disc where there is no green or it draws nothing."""
    i = 1 if len(discs) > 1 and discs[1][2] >= 0 else 0
    return i, discs[i]


def free_block(lo, hi):
    """A 64-index block that [lo, hi] does not touch (the last such one), or None."""
    for b in (3, 2, 1, 0):
        if hi < 64 * b or lo > 64 * b + 63:
            return b
    return None


def lone_block_rect(disc):
    """(f): an 11 x 9 rectangle wholly inside one 64-index block of columns and one of rows, neither touched by the disc's box."""
    (x0, x1), (y0, y1) = cc.disc_box(disc) if disc[2] >= 0 and np.all(np.isfinite(disc)) else ((100, 120), (100, 120))
    bx, by = free_block(x0, x1), free_block(y0, y1)
    bx, by = 3 if bx is None else bx, 0 if by is None else by
    return oc.still(64 * bx + 20, 64 * by + 30, 11, 9)


def paint_sets(discs):
    """name -> (rows, paints) for one static scene of n = len(discs) colours: the patterns (a) .. (h) of the suite's list."""
    n = len(discs)
    c, disc = target(discs)
    other = (c + 1) % n if n > 1 else OPAQUE
    u, v, r = (float(x) if np.isfinite(x) else 100.0 for x in disc)
    r = max(r, 6.0) if r < 1e3 else 8.0
    left, top, size = int(np.floor(u - r)) - 2, int(np.floor(v - r)) - 2, int(np.ceil(2 * r)) + 5
    half = oc.still(left, top, int(np.floor(u)) - left + 1, size)    # the left half of the target, as in the occluder suite
    upper = oc.still(left, top, size, int(np.floor(v)) - top + 1)
    sets = {
        'a_disjoint': ([oc.still(10, 200, 9, 7)], [c]),
        'b_over_its_own_disc': ([half], [c]),
        'c_over_another_disc': ([half], [other]),
        'd_opaque_in_front_of_painted': ([half, upper], [c, OPAQUE]),
        'd_painted_in_front_of_opaque': ([half, upper], [OPAQUE, c]),
        'd_two_paints_in_two_orders': ([upper, half], [other, c]),
        'f_lone_block': ([lone_block_rect(disc)], [c]),
        'g_four_of_one_colour': ([half, upper, oc.still(left + 3, top + 3, size, 4), oc.still(left + 5, top - 2, 4, size + 9)], [c] * 4),
        'g_four_mixed': ([half, upper, oc.still(left + 3, top + 3, size, 4), oc.still(left + 5, top - 2, 4, size + 9)], [c, other, OPAQUE, c]),
        'h_clipped_at_every_edge': ([oc.still(-5, 100, 10, 10), oc.still(250, 90, 10, 10), oc.still(100, -5, 10, 10), oc.still(90, 250, 10, 10)],
                                    [c] * 4),
        'h_one_pixel': ([oc.still(77, 33, 1, 1)], [c]),
        'h_whole_frame': ([oc.still(0, 0, 256, 256)], [c]),
        'h_whole_frame_behind_opaque': ([oc.still(-3, -3, 300, 300), upper], [c, OPAQUE]),
        'e_every_colour': ([oc.still(20 + 50 * p, 40 + 45 * p, 8 + p, 5 + 2 * p) for p in range(min(n, 4))], list(range(min(n, 4)))),
        'all_opaque': ([half, upper], [OPAQUE, OPAQUE]),
    }
    sets.update({'extreme_' + key: ([row], [c]) for key, row in oc.extremes().items()})
    return sets


def padded_paints(paints, n=4):
    return np.array(list(paints) + [OPAQUE] * (n - len(paints)), np.int64)


def static_batch(name):
    """(names, n_colours, discs (T, n, 3), occluders (T, 4, 8), paints (T, 4)) of one scene: a trial per paint set."""
    n, discs = scene(name)
    sets = paint_sets(discs)
    names = list(sets)
    return (names, n, np.broadcast_to(discs, (len(names), n, 3)).copy(), np.stack([oc.padded(sets[key][0]) for key in names]),
            np.stack([padded_paints(sets[key][1]) for key in names]))


def owners_restated(discs, rows, paints, k):
    """The owner rule, pixel by pixel in plain Python: (256, 256) lists [flipped row][column] of ('rect', o), ('disc', c) or None.  A pixel
    belongs to the highest-index active rectangle that contains it, otherwise to the topmost (highest-index) disc that the pixel rule
    gives it, otherwise to nobody.  Rectangles by membership of plain integers; discs by the rule's own rounded expression."""
    rects = []
    for row in rows:
        x, y, w, h, vx, vy, k_on, k_off = (int(a) for a in row)
        active = k_on <= k < k_off and w > 0 and h > 0
        rects.append((x + vx * k, y + vy * k, w, h) if active else None)
    masks = [cc.rule_mask(d) for d in np.asarray(discs, float)]
    out = [[None] * cc.SIDE for _ in range(cc.SIDE)]
    for i in range(cc.SIDE):
        for j in range(cc.SIDE):
            owner = None
            for c, mask in enumerate(masks):
                if mask[i, j]:
                    owner = ('disc', c)
            for o, rect in enumerate(rects):
                if rect is not None and rect[0] <= j <= rect[0] + rect[2] - 1 and rect[1] <= i <= rect[1] + rect[3] - 1:
                    owner = ('rect', o)
            out[i][j] = owner
    return out


def frame_restated(discs, rows, paints, k, background=96, shade=32):
    """uint8 (256, 256, 3), unflipped: the frame of the owner rule."""
    n = len(discs)
    colour = lambda p: COLOURS[1 if n == 1 else p]                   # noqa: E731
    frame = np.empty((cc.SIDE, cc.SIDE, 3), np.uint8)
    for i, line in enumerate(owners_restated(discs, rows, paints, k)):
        for j, owner in enumerate(line):
            if owner is None:
                px = (background,) * 3
            elif owner[0] == 'disc':
                px = colour(owner[1])
            else:
                p = int(paints[owner[1]])
                px = (shade,) * 3 if p == OPAQUE else colour(p)
            frame[cc.SIDE - 1 - i, j] = px
    return frame


def counts(frame, n):
    """Mask sizes per feature pair of an n-colour camera from a host frame."""
    four = cc.host_counts(frame)
    return four[..., 1:2] if n == 1 else four[..., :n]


# ------------------------------------------------------------------------------------------------------------- the loops' rectangles
def painted_bar(paint):
    """The occluder suite's sweeping bar, a quarter of the frame high so that a painted one leaves the discs' rows alone at times:
    columns [60 + 12 k, 71 + 12 k] -- 12 px per step in the occluder suite -- here 1 px per step, rows 100 .. 179."""
    return [(118, 100, 6, 80, 1, 0) + oc.ALWAYS], [paint]


def still_distractor(paint, x=212, y=20, w=13, h=11):
    """A still rectangle in a 64-index block of columns (3) and of rows (0) that no disc of the servo's scene touches."""
    return [oc.still(x, y, w, h)], [paint]
