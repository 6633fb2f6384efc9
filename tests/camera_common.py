"""Scenes and helpers shared by tests/test_camera_host.py (CPU), tests/test_gpu_camera.py, tests/test_gpu_camera_scenes.py and
tests/test_gpu_camera_loop.py (GPU): discs (u, v, r) in pixels of the flipped frame, colour order red, green, blue, pink; plants whose camera
shows a given scene; numpy mirrors of the kernels' bounding box; the bit-for-bit comparison of two closed-loop outputs."""
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
    s.update(huge_scenes())
    fixture, idx = fixture_discs()
    for disc, i in zip(fixture, idx):
        s[f'fixture_{i}'] = (4, disc)
        s[f'fixture_{i}_rgb'] = (3, disc[:3])
        s[f'fixture_{i}_green'] = (1, disc[1:2])
    return s


INF = float('inf')
RED, GREEN = (40.0, 200.0, 7.5), (200.3, 50.2, 9.5)                # ordinary discs to go under or over a huge one
THREE = [(60.2, 70.9, 7.1), (130.5, 64.4, 8.8), (190.6, 200.3, 6.6)]
RIM_BEYOND_2_54 = {'right': (2.0 ** 55, 128.0, 2.0 ** 55 - 200.0), 'left': (-2.0 ** 55, 128.0, 2.0 ** 55 + 100.0),
                   'below': (128.0, 2.0 ** 56, 2.0 ** 56 - 100.0)}


def huge_scenes():
    """name -> (n_colours, discs): discs far larger than the frame, and non-finite ones.  Above 1e9 `may_cover` (vision_device.hpp) stops
    reading a disc's box; beyond 2^54 doubles next to the centre are more than a pixel apart, so a box taken from centre -+ r -+ 1 would
    lose pixels of the rule: such discs get the whole frame as their box (disc_box below)."""
    s = {
        'huge_1e12': (4, pad([(128.0, 128.0, 1e12)])),
        'huge_off_centre': (4, pad([(1e15, 3e14, 2e15)])),
        'inf_radius': (4, pad([(100.0, 100.0, INF)])),
        'inf_all': (4, pad([(INF, INF, INF)])),
        'inf_radius_minus_inf_u': (4, pad([(-INF, 5.0, INF)])),
        'inf_u_small_radius': (4, pad([(INF, 100.0, 5.0)])),
        'below_1e9': (4, pad([(5e8, 128.0, 5e8 - 100.0)])),
        'below_1e9_over_red': (4, pad([RED, (5e8, 128.0, 5e8 - 100.0)])),
    }
    for name, disc in (('above_1e9', (3e9, 128.0, 3e9)), ('above_1e9_rim', (3e9, 128.0, 2.9999999e9))):
        s[name] = (4, pad([disc]))
        s[name + '_over_red'] = (4, pad([RED, disc]))               # `may_cover`'s branch for operands >= 1e9 decides red's counts
    for name, disc in RIM_BEYOND_2_54.items():
        s[f'rim_2_54_{name}'] = (4, pad([disc]))
        s[f'rim_2_54_{name}_green_alone'] = (1, pad([disc], 1))
        s[f'rim_2_54_{name}_under_green'] = (4, pad([disc, GREEN]))
        s[f'rim_2_54_{name}_pink_over_three'] = (4, pad(THREE + [disc]))
    return s


def pixel_range(centre, r, slack=1.0):
    """numpy mirror of pixel_range (vision_device.hpp): the inclusive index range [lo, hi] of [centre - r - slack, centre + r + slack]
    clipped to the frame.  fmax / fmin drop a NaN operand, as in the kernel."""
    with np.errstate(invalid='ignore', over='ignore'):
        centre, r, slack = np.float64(centre), np.float64(r), np.float64(slack)
        lo = np.fmin(np.fmax(np.ceil(centre - r - slack), 0.0), float(SIDE))
        hi = np.fmax(np.fmin(np.floor(centre + r + slack), float(SIDE - 1)), -1.0)
    return int(lo), int(hi)


def disc_box(disc, guarded=True):
    """numpy mirror of disc_box (vision_device.hpp): ((x0, x1), (y0, y1)), one pixel of slack for a disc with |u|, |v| and r below 1e9 and
    the whole frame (slack = inf) for any other.  ``guarded=False`` is the box with one pixel of slack whatever the disc."""
    u, v, r = (np.float64(x) for x in disc)
    slack = 1.0 if not guarded or (abs(u) < 1e9 and abs(v) < 1e9 and r < 1e9) else np.inf
    return pixel_range(u, r, slack), pixel_range(v, r, slack)


def rule_mask(disc):
    """(256, 256) bool, [flipped row i, column j]: the pixels the contract's rule gives one disc (plant.render_discs' own expression)."""
    with np.errstate(invalid='ignore', over='ignore'):
        d2, r2 = squares(disc)
        return (d2 <= r2) & bool(disc[2] >= 0)


def pixels_outside_box(disc, guarded=True):
    """Number of pixels the rule gives ``disc`` that lie outside its box."""
    mask = rule_mask(disc)
    (x0, x1), (y0, y1) = disc_box(disc, guarded)
    inside = np.zeros_like(mask)
    inside[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
    return int(np.sum(mask & ~inside))


# ------------------------------------------------------------------------------------------------------------- scenes through a camera
JITTER = 2e-3                                                       # rad: see test_jitter_varies_the_masks_and_keeps_the_scenes (test_camera_host.py)
GRAZING_PC = (0.3, 0.2, 1e-6)                                       # metres in the camera frame at Q_GOAL: a point that grazes the focal plane


def scene_plant(uvs, discs):
    """(plant, radius) for an (n, 3) scene of finite discs: plant.discs(Q_GOAL, radius) is the scene (to about 1e-13 px).  A row with
    r < 0 becomes a point behind the camera, for which the projection itself returns r = -1."""
    discs = np.asarray(discs, float)
    assert np.all(np.isfinite(discs))
    plant = uvs.SyntheticPlant.ur10(desired_f=tuple(discs[:, :2].ravel()))
    pose = plant.fkine_all(Q_GOAL)[-1]
    radius = discs[:, 2] * pose[2, 3] / plant.focal
    for i in np.flatnonzero(discs[:, 2] < 0):
        plant.points[i] = pose[:3, 3] + pose[:3, :3] @ np.array([0.01, 0.02, -0.3])
        radius[i] = 0.024
    return plant, radius


def grazing_plant(uvs):
    """(plant, radius): the red point at GRAZING_PC -- depth 1e-6 m, so u, v and r are some 1e7 px -- with a physical radius equal to its
    distance from the optical axis: its rim then passes through the principal point whatever the depth.  Three ordinary discs beside it."""
    plant, radius = scene_plant(uvs, [(0.0, 0.0, 1.0)] + THREE)
    pose = plant.fkine_all(Q_GOAL)[-1]
    plant.points[0] = pose[:3, 3] + pose[:3, :3] @ np.array(GRAZING_PC)
    radius[0] = np.hypot(GRAZING_PC[0], GRAZING_PC[1])
    return plant, radius


def camera_scene_names():
    """The scenes of tests/test_gpu_camera_scenes.py: every finite scene of edge_scenes that is no fixture scene, and 'grazing'.  The discs of
    huge_scenes are not among them: no camera of metre-sized links projects 2^55 px to a fraction of a pixel; they go to the kernels as discs."""
    huge = huge_scenes()
    return [name for name, (_, disc) in edge_scenes().items()
            if not name.startswith('fixture_') and name not in huge and np.all(np.isfinite(disc))] + ['grazing']


def camera_scene(uvs, name):
    """(n_colours, plant, radius) of one of camera_scene_names()."""
    if name == 'grazing':
        return (4,) + grazing_plant(uvs)
    n, disc = edge_scenes()[name]
    return (n,) + scene_plant(uvs, disc)


def scene_joints(T, name):
    """(T, 6) start poses: trial 0 is Q_GOAL exactly, the others Q_GOAL plus a seeded jitter of +-JITTER rad."""
    seed = int.from_bytes(name.encode(), 'little') % (1 << 32)
    q = Q_GOAL + np.random.default_rng(seed).uniform(-JITTER, JITTER, (T, 6))
    q[0] = Q_GOAL
    return q


CONSTANT_COUNTS = ('whole_frame', 'green_alone_absent')             # scenes whose mask sizes cannot depend on the pose
EMPTY_MASK = ('clip_left', 'clip_right', 'clip_top', 'clip_bottom', 'outside', 'overlap_two', 'covered', 'point_off_lattice',
              'r5_integer_centre', 'whole_frame', 'green_alone_absent', 'rgb_blue_absent')      # some colour has no pixel: FAIL at step 0


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


# ------------------------------------------------------------------------------------------------------------- comparing loop outputs
LOGS = ('err', 'q', 'f', 'dq', 'kappa')


def bits(t):
    """int64 view of an fp64 tensor / array on the host: equality of bits, NaN payloads included."""
    a = t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64)


def assert_same_bits(got, want, K, where, trials=None, want_trials=None):
    """Every specified value of ``got`` equals that of ``want`` bit for bit; ``trials`` / ``want_trials`` pair up the trials to compare."""
    import torch
    T = got['status'].shape[0]
    trials = list(range(T)) if trials is None else trials
    want_trials = trials if want_trials is None else want_trials
    k_done = got['k_done'].cpu().numpy()
    assert np.array_equal(k_done[trials], want['k_done'].cpu().numpy()[want_trials]), (where, 'k_done')
    assert torch.equal(got['status'].cpu()[trials], want['status'].cpu()[want_trials]), (where, 'status')
    assert torch.equal(got['pixels'].cpu()[trials], want['pixels'].cpu()[want_trials]), (where, 'pixels')
    assert np.array_equal(bits(got['stats'])[trials], bits(want['stats'])[want_trials]), (where, 'stats')
    for key in LOGS:
        if key not in got:
            continue
        a, b = bits(got[key]), bits(want[key])
        assert a.shape[0] == K and a.shape[2] == b.shape[2], (where, key)
        for t, tw in zip(trials, want_trials):
            rows = min(K, k_done[t] + 1) if key in ('q', 'f') else k_done[t]
            assert np.array_equal(a[:rows, t], b[:rows, tw]), (where, key, t)
