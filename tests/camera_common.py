"""Scenes and helpers shared by tests/test_camera_host.py (CPU) and tests/test_gpu_camera.py (GPU): discs (u, v, r) in pixels of the flipped
frame, colour order red, green, blue, pink."""
import os

import numpy as np

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'detect_circles.npz'))
ORDER = ('red', 'green', 'blue', 'pink')
SIDE, DENSE = 256, 256 * 256 * 3
NAN = float('nan')
Q_GOAL = np.array([0.0, -np.pi / 8, np.pi / 2 + np.pi / 8, 0.0, -np.pi / 2, 0.0])       # SyntheticPlant.ur10()'s goal pose


def fixture_discs(unsoftened_only=False):
    """(scenes, 4, 3) discs of tests/golden/detect_circles.npz and the indices of the scenes they come from."""
    idx = [i for i in range(len(G['f4'])) if not (unsoftened_only and G['soften'][i])]
    return np.stack([np.stack([G['cu'][i], G['cv'][i], G['radius'][i]], axis=1) for i in idx]), idx


def squares(disc):
    """(d2, r2): the rounded squared distance of every pixel (flipped row i, column j) to the disc's centre, and the rounded r^2."""
    u, v, r = disc
    grid = np.arange(SIDE, dtype=float)
    dx, dy = grid[None, :] - u, grid[:, None] - v
    return dx * dx + dy * dy, r * r


def closest_to_rim(discs):
    """min over discs and pixels of |d^2 - r^2|: 0 means a pixel sits exactly on a rim (where `hypot <= r` and `d^2 <= r^2` may part)."""
    best = np.inf
    for disc in np.asarray(discs, float).reshape(-1, 3):
        if disc[2] >= 0 and np.all(np.isfinite(disc)):
            d2, r2 = squares(disc)
            best = min(best, float(np.abs(d2 - r2).min()))
    return best


def pad(rows, n=4):
    """n discs: the given ones, then discs that draw nothing (r = -1)."""
    rows = [tuple(map(float, r)) for r in rows]
    return np.array(rows + [(0.0, 0.0, -1.0)] * (n - len(rows)))


def edge_scenes():
    """name -> (n_colours, (n_colours, 3) discs): the edge cases of the pixel rule, of clipping and of the painter's order."""
    s = {
        'clip_left': (4, pad([(-2.5, 100.3, 7.0), (40.0, 200.0, 5.5)])),
        'clip_right': (4, pad([(254.2, 60.7, 8.0), (100.0, 100.0, 4.0)])),
        'clip_top': (4, pad([(80.4, 1.3, 9.0)])),
        'clip_bottom': (4, pad([(90.1, 255.6, 6.3), (10.0, 10.0, 5.0), (200.0, 30.0, 4.5)])),
        'clip_corner': (4, pad([(253.9, 254.4, 10.2), (1.2, 0.7, 6.1), (255.0, 0.0, 3.0), (0.0, 255.0, 3.0)])),
        'outside': (4, pad([(300.0, 100.0, 8.0), (100.0, -40.0, 8.0), (-9.1, -9.1, 8.0), (128.0, 128.0, 7.0)])),
        'overlap_two': (4, pad([(100.0, 100.0, 12.0), (108.5, 104.25, 9.0)])),
        'overlap_four': (4, pad([(120.0, 120.0, 14.0), (128.3, 121.1, 11.0), (124.7, 129.9, 10.0), (126.0, 124.0, 5.0)])),
        'covered': (4, pad([(60.0, 60.0, 4.0), (60.5, 60.5, 9.0), (200.0, 200.0, 6.0), (30.0, 220.0, 6.0)])),     # red wholly under green: NaN pair
        'point_on_lattice': (4, pad([(17.0, 33.0, 0.0), (41.0, 37.0, 0.0), (255.0, 255.0, 0.0), (0.0, 0.0, 0.0)])),
        'point_off_lattice': (4, pad([(17.5, 33.0, 0.0), (41.0, 37.25, 0.0), (100.0, 100.0, 6.0)])),
        'r5_integer_centre': (4, pad([(50.0, 60.0, 5.0), (150.0, 160.0, 5.0)])),
        'not_drawn': (4, pad([(100.0, 100.0, -1.0), (NAN, 50.0, 6.0), (50.0, NAN, 6.0), (70.0, 70.0, NAN)])),
        'whole_frame': (4, pad([(128.0, 128.0, 400.0)])),
        'whole_frame_under': (4, pad([(128.0, 128.0, 400.0), (33.3, 41.9, 7.7), (200.2, 180.8, 9.1), (90.0, 210.0, 6.0)])),
        'green_alone': (1, pad([(133.7, 99.2, 8.4)], 1)),
        'green_alone_clipped': (1, pad([(2.0, 253.0, 8.4)], 1)),
        'green_alone_absent': (1, pad([(128.0, 128.0, -1.0)], 1)),
        'rgb': (3, pad([(60.2, 70.9, 7.1), (130.5, 64.4, 8.8), (190.6, 200.3, 6.6)], 3)),
        'rgb_blue_absent': (3, pad([(60.2, 70.9, 7.1), (130.5, 64.4, 8.8)], 3)),
        'rgb_overlap': (3, pad([(100.0, 100.0, 9.0), (104.0, 103.0, 9.0), (108.0, 100.0, 9.0)], 3)),
    }
    fixture, idx = fixture_discs()
    for disc, i in zip(fixture, idx):
        s[f'fixture_{i}'] = (4, disc)
        s[f'fixture_{i}_rgb'] = (3, disc[:3])
        s[f'fixture_{i}_green'] = (1, disc[1:2])
    return s


def batches():
    """n_colours -> (names, (T, n_colours, 3) discs): every scene above, grouped into one batch per colour count."""
    out = {}
    for name, (n, disc) in edge_scenes().items():
        out.setdefault(n, ([], []))
        out[n][0].append(name)
        out[n][1].append(disc)
    return {n: (names, np.stack(discs)) for n, (names, discs) in out.items()}


def host_counts(img):
    """Mask sizes of red, green, blue, pink by the reference's integer thresholds (utils.py:15-24, :130-144)."""
    r, g, b = (img[..., ch].astype(int) for ch in range(3))
    lo, hi = (lambda x: x < 250), (lambda x: x > 250)
    masks = (hi(r) & lo(g) & lo(b), lo(r) & hi(g) & lo(b), lo(r) & lo(g) & hi(b), hi(r) & lo(g) & hi(b))
    return np.stack([mk.sum(axis=(-2, -1)) for mk in masks], axis=-1)
