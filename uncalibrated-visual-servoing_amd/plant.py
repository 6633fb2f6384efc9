"""Synthetic plants for closed-loop Monte-Carlo runs: a DH serial arm carrying a pinhole camera.

The reference talks to an external CoppeliaSim process (ur10_simulation.py RPC methods); what it computes
locally is the UR10 DH forward kinematics and geometric Jacobian (ur10_simulation.py:97-139, 204-211).
``SyntheticPlant`` keeps exactly those kinematics and closes the loop with a pinhole camera on the last frame
looking at fixed world points.  The same description is (a) handed to the HIP kernels
as a ``uvs_plant`` struct, where the plant runs inside the closed-loop kernel, and (b) evaluated on the host
by ``SyntheticRobot``, the duck-typed robot that ``Experiment`` drives.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _lib

RESOLUTION = 256
FOV_DEG = 65.0
DISC_RADIUS = 0.024                     # metres: 8.01 px at SyntheticPlant.ur10()'s goal pose (CameraRobot)
DISC_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 0, 255))       # red, green, blue, pink (utils.py:126-166)


def focal_length(resolution=RESOLUTION, fov_deg=FOV_DEG):
    return resolution / (2 * np.tan(0.5 * np.deg2rad(fov_deg)))            # experiment.py:97


def camera_pose(T):
    """[x, y, z, roll, pitch, yaw] of a homogeneous camera transform, as UR10Simulation.computePose returns it
    (ur10_simulation.py:151-163): position, then the angles utils.quat2euler extracts from the simulator's scalar-first
    quaternion -- R = Rz(yaw) Ry(pitch) Rx(roll), i.e. roll = atan2(R21, R22), pitch = asin(-R20), yaw = atan2(R10, R00)
    (the reference's own commented-out matrix form, ur10_simulation.py:158-160)."""
    T = np.asarray(T, float)
    pose = np.empty(6)
    pose[:3] = T[:3, 3]
    pose[3] = np.arctan2(T[2, 1], T[2, 2])
    pose[4] = np.arcsin(np.clip(-T[2, 0], -1.0, 1.0))
    pose[5] = np.arctan2(T[1, 0], T[0, 0])
    return pose


MAX_OCCLUDERS = 4                       # UVS_CAMERA_MAX_OCCLUDERS
OCCLUDER_FIELDS = ('x', 'y', 'w', 'h', 'vx', 'vy', 'k_on', 'k_off')         # uvs_occluder of include/uvs_vision.h: eight int32
NO_RECT = (1, 0, 1, 0)                  # a rectangle that covers nothing: x0 > x1


def occluder_array(occluders, T=None):
    """``occluders`` as an int64 host array (T, n_occ, 8) of ``OCCLUDER_FIELDS`` rows whose values are int32: from (n_occ, 8) -- every trial
    the same -- or (T, n_occ, 8) integers.  ValueError for anything else, more than ``MAX_OCCLUDERS`` rows, or a T that does not match."""
    try:
        a = np.asarray(occluders)
    except Exception as exc:                                         # ragged lists
        raise ValueError(f'occluders: (n_occ, 8) or (T, n_occ, 8) integers, rows of {OCCLUDER_FIELDS}') from exc
    if a.size == 0 and a.ndim in (1, 2) and a.shape[-1] in (0, 8):   # [] and np.empty((0, 8)): no occluder
        a = np.zeros((0, 8), np.int64)
    if a.dtype.kind not in 'iu' or a.ndim not in (2, 3) or a.shape[-1] != 8:
        raise ValueError(f'occluders: (n_occ, 8) or (T, n_occ, 8) integers, rows of {OCCLUDER_FIELDS}, got {a.dtype} {a.shape}')
    if a.shape[-2] > MAX_OCCLUDERS:
        raise ValueError(f'occluders: at most {MAX_OCCLUDERS} per trial, got {a.shape[-2]}')
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError('occluders: every field is an int32')
    a = a.astype(np.int64)
    if a.ndim == 2:
        a = np.broadcast_to(a, (1 if T is None else T,) + a.shape)
    elif T is not None and a.shape[0] != T:
        raise ValueError(f'occluders: {a.shape[0]} trials of occluders for {T} trials')
    return np.ascontiguousarray(a)


def occluder_rects(occluders, k):
    """The rule of uvs_occluder (include/uvs_vision.h) in Python-int arithmetic: for (n_occ, 8) rows of ``OCCLUDER_FIELDS`` the list of the
    clipped inclusive rectangles (x0, x1, y0, y1) at step ``k`` -- columns and FLIPPED rows.  An occluder is active iff k_on <= k < k_off,
    w > 0 and h > 0, and then covers columns [x + vx k, x + vx k + w - 1] and flipped rows [y + vy k, y + vy k + h - 1], clipped to the
    frame.  One that covers nothing is returned as ``NO_RECT``: x0 > x1."""
    k = int(k)
    if k < 0:
        raise ValueError('k must be >= 0')
    out = []
    for row in np.asarray(occluders).reshape(-1, 8).tolist():
        x, y, w, h, vx, vy, k_on, k_off = (int(v) for v in row)
        rect = NO_RECT
        if k_on <= k < k_off and w > 0 and h > 0:
            xk, yk = x + vx * k, y + vy * k
            x0, x1, y0, y1 = max(xk, 0), min(xk + w - 1, RESOLUTION - 1), max(yk, 0), min(yk + h - 1, RESOLUTION - 1)
            if x0 <= x1 and y0 <= y1:
                rect = (x0, x1, y0, y1)
        out.append(rect)
    return out


OPAQUE = -1                             # the paint of an occluder that takes no disc's colour


def occluder_colour_array(occluder_colours, n_occ, n_colours, T=None):
    """``occluder_colours`` -- the PAINT of every occluder -- as an int64 host array (T, n_occ): from (n_occ,) -- every trial the same -- or
    (T, n_occ) integers.  A value p in 0 .. n_colours - 1 paints the rectangle the colour of disc p (n_colours == 1: 0 is the green one),
    ``OPAQUE`` (-1) leaves it the opaque occluder it was.  ValueError for any other value, for anything that is not such an array, for a
    length that is not ``n_occ`` (None: the caller has no occluders), or for a T that does not match."""
    if n_occ is None:
        raise ValueError('occluder_colours without occluders: a paint belongs to a rectangle')
    try:
        a = np.asarray(occluder_colours)
    except Exception as exc:                                         # ragged lists
        raise ValueError('occluder_colours: (n_occ,) or (T, n_occ) integers') from exc
    if a.size == 0 and a.ndim == 1:                                  # []: no occluder to paint
        a = np.zeros((0,), np.int64)
    if a.dtype.kind not in 'iu' or a.ndim not in (1, 2):
        raise ValueError(f'occluder_colours: (n_occ,) or (T, n_occ) integers, got {a.dtype} {a.shape}')
    if a.shape[-1] != n_occ:
        raise ValueError(f'occluder_colours: {a.shape[-1]} paints for {n_occ} occluders')
    if a.size and (a.min() < OPAQUE or a.max() >= n_colours):
        raise ValueError(f'occluder_colours: every value is {OPAQUE} (opaque) or a disc 0 .. {n_colours - 1}')
    a = a.astype(np.int64)
    if a.ndim == 1:
        a = np.broadcast_to(a, (1 if T is None else T,) + a.shape)
    elif T is not None and a.shape[0] != T:
        raise ValueError(f'occluder_colours: {a.shape[0]} trials of paints for {T} trials')
    return np.ascontiguousarray(a)


def render_discs(discs, n_colours=4, background=96, occluders=None, k=0, shade=32, occluder_colours=None):
    """Camera frames of coloured discs: the numpy statement of the pixel rule uvs_render_discs_u8 (include/uvs_vision.h) is held to.
    ``discs``: (n_colours, 3) or (T, n_colours, 3) rows (u, v, r) in pixels of the flipped frame (u right, v down), colour order red,
    green, blue, pink (n_colours == 1: the green disc).  Pixel (flipped row i, column j) belongs to disc c iff r_c >= 0 and
    fl(fl(dx * dx) + fl(dy * dy)) <= fl(r_c * r_c) with dx = j - u_c, dy = i - v_c; a NaN gives nothing; a later disc overwrites an earlier
    one; everything else is ``background``.  A disc is drawn as a circle (no perspective-correct ellipse).
    ``occluders``: None, or (n_occ, 8) / (T, n_occ, 8) integer rows of ``OCCLUDER_FIELDS`` -- rectangles in front of the discs at step ``k``
    (``occluder_rects``): a covered pixel belongs to no disc and is ``shade`` (0 .. 249) in all three channels; the covered set is the union.
    This function is the statement of that rule too (uvs_render_discs_occluded_u8 and the occluded detectors are held to it).
    ``occluder_colours``: None, or the PAINT of every occluder (``occluder_colour_array``: (n_occ,) or (T, n_occ) integers).  Rectangle o' is
    in front of rectangle o when o' > o, and all are in front of every disc: a pixel belongs to the highest-index active rectangle that
    contains it, else to the topmost disc, else to the background.  A rectangle painted p shows ``DISC_COLOURS`` of disc p -- a DISTRACTOR:
    its pixels enter that colour's mask -- and an ``OPAQUE`` one shows ``shade``.  None, or all opaque, is the union of above.
    Returns uint8 (256, 256, 3) or (T, 256, 256, 3), UNFLIPPED as the sensor hands frames over (flipped row i is row 255 - i)."""
    discs = np.asarray(discs, float)
    if n_colours not in (1, 3, 4) or discs.shape[-2:] != (n_colours, 3) or discs.ndim not in (2, 3):
        raise ValueError(f'discs: (n_colours, 3) or (T, n_colours, 3) with n_colours in (1, 3, 4), got {discs.shape} for n_colours = {n_colours}')
    if not 0 <= background < 250:
        raise ValueError('background must be 0 .. 249: 250 and above would enter a mask of the detectors')
    batch = discs.reshape((-1,) + discs.shape[-2:])
    if occluders is not None:
        if not 0 <= shade < 250:
            raise ValueError('shade must be 0 .. 249: 250 and above would enter a mask of the detectors')
        occluders = occluder_array(occluders, len(batch))
        rects = [occluder_rects(rows, k) for rows in occluders]     # refuses k < 0
    if occluder_colours is not None:
        paints = occluder_colour_array(occluder_colours, None if occluders is None else occluders.shape[1], n_colours, len(batch))
    grid = np.arange(RESOLUTION, dtype=float)
    frames = np.full((len(batch), RESOLUTION, RESOLUTION, 3), background, np.uint8)
    with np.errstate(invalid='ignore', over='ignore'):
        for t, (frame, scene) in enumerate(zip(frames, batch)):
            for c, (u, v, r) in enumerate(scene):
                if not r >= 0:
                    continue
                dx, dy = grid[None, :] - u, grid[:, None] - v
                frame[(dx * dx + dy * dy) <= r * r] = DISC_COLOURS[1 if n_colours == 1 else c]
            if occluders is not None:
                for o, (x0, x1, y0, y1) in enumerate(rects[t]):      # NO_RECT: an empty slice; a later rectangle overwrites an earlier one
                    p = OPAQUE if occluder_colours is None else int(paints[t, o])
                    frame[y0:y1 + 1, x0:x1 + 1] = shade if p == OPAQUE else DISC_COLOURS[1 if n_colours == 1 else p]
    frames = frames[:, ::-1].copy()
    return frames[0] if discs.ndim == 2 else frames


def hold_features(f, f_prev, pixels, miss, hold):
    """Hold a lost disc's last detection: the numpy statement of the rule uvs_camera_closed_loop_held_f64 and uvs_hold_features_f64
    (include/uvs_vision.h) are held to, for ONE step of T trials.  ``f`` (T, 2 n_points): the detector's row of step k, noise included;
    ``f_prev`` (T, 2 n_points): the REPORTED row of step k - 1 (what this function returned then), or None at step 0; ``pixels``
    (T, n_points) integers: the mask counts of step k; ``miss`` (T, n_points) integers: the counters, zeros before step 0; ``hold`` >= 0:
    the largest number of consecutive steps for which a pair may be held.
    Disc j is lost iff pixels[j] == 0 -- the count decides, never the pair.  Detected: miss[j] = 0 and the pair is f's.  Lost, not step 0
    and miss[j] < hold: the pair is f_prev's (that step's noise in it, none of this step's), miss[j] += 1, held[j] = 1.  Lost otherwise:
    the pair stays f's (NaN, which FAILs the trial at this step).
    Returns new arrays (f, miss, held); the arguments are not written."""
    if isinstance(hold, bool) or not isinstance(hold, (int, np.integer)) or hold < 0:
        raise ValueError(f'hold is a number of steps, an integer >= 0, got {hold!r}')
    f, pixels, miss = np.array(f, float), np.asarray(pixels), np.array(miss)
    if f.ndim != 2 or pixels.shape != (f.shape[0], f.shape[1] // 2) or miss.shape != pixels.shape or f.shape[1] % 2:
        raise ValueError(f'f (T, 2 n_points), pixels and miss (T, n_points), got {f.shape}, {pixels.shape}, {miss.shape}')
    if pixels.dtype.kind not in 'iu' or miss.dtype.kind not in 'iu':
        raise ValueError('pixels and miss are integers')
    lost = pixels == 0
    held = lost & (miss < hold) if f_prev is not None else np.zeros_like(lost)
    if held.any():
        f_prev = np.asarray(f_prev, float)
        if f_prev.shape != f.shape:
            raise ValueError(f'f_prev has the shape of f, got {f_prev.shape} for {f.shape}')
        pairs = np.repeat(held, 2, axis=1)
        f[pairs] = f_prev[pairs]
    miss = np.where(held, miss + 1, np.where(lost, miss, 0)).astype(miss.dtype)
    return f, miss, held.astype(np.int32)


def analytic_guess(robot, f, resolution, m, n):
    """X0 for an external robot (experiment.py:94-114), evaluated once on the host from the robot's own kinematics."""
    depth = robot.computeZ(m // 2)
    focal = resolution[0] / (2 * np.tan(0.5 * np.deg2rad(robot.perspective_angle)))
    Ji = np.zeros((m, 6))
    for i in range(m // 2):
        u, v = f[2 * i], f[2 * i + 1]
        Ji[2 * i] = [-focal / depth[i], 0.0, u / depth[i], u * v / focal, -(focal ** 2 + u ** 2) / focal, v]
        Ji[2 * i + 1] = [0.0, -focal / depth[i], v / depth[i], (focal ** 2 + v ** 2) / focal, -u * v / focal, -u]
    return (Ji @ np.kron(np.eye(2), robot.getCameraRotation().T) @ robot.jacobian()).reshape(m * n)


@dataclass
class SyntheticPlant:
    theta_offset: np.ndarray
    d: np.ndarray
    a: np.ndarray
    alpha: np.ndarray
    points: np.ndarray                      # (n_points, 3) world coordinates
    focal: float = field(default_factory=focal_length)
    center: float = RESOLUTION / 2
    fov_deg: float = FOV_DEG

    # ---------------------------------------------------------------- constructors
    @classmethod
    def ur10(cls, desired_f=(149.0, 145.0, 125.0, 121.0, 101.0, 145.0, 125.0, 169.0), q_goal=None):
        """UR10 chain of ur10_simulation.py:100-105; discs on the floor that project onto ``desired_f`` (config.json:9)
        from the straight-down pose used by the reference's tests/*.py."""
        half = np.pi / 2
        plant = cls(theta_offset=np.array([0.0, -half, 0.0, -half, 0.0, np.pi]),
                    d=np.array([0.128, 0.0, 0.0, 0.1639, 0.1157, 0.0922]),
                    a=np.array([0.0, 0.6127, 0.5716, 0.0, 0.0, 0.0]),
                    alpha=np.array([-half, 0.0, 0.0, -half, half, 0.0]),
                    points=np.zeros((len(desired_f) // 2, 3)))
        q_goal = np.array([0.0, -np.pi / 8, half + np.pi / 8, 0.0, -half, 0.0]) if q_goal is None else np.asarray(q_goal, float)
        T = plant.fkine_all(q_goal)[-1]
        depth = T[2, 3]
        for i in range(len(desired_f) // 2):
            ray = np.array([(desired_f[2 * i] - plant.center) / plant.focal * depth,
                            (desired_f[2 * i + 1] - plant.center) / plant.focal * depth, depth])
            plant.points[i] = T[:3, 3] + T[:3, :3] @ ray
        return plant

    # ---------------------------------------------------------------- host kinematics
    @property
    def n_joints(self):
        return len(self.d)

    @property
    def n_points(self):
        return len(self.points)

    def link(self, i, theta):
        c, s = np.cos(theta), np.sin(theta)
        ca, sa = np.cos(self.alpha[i]), np.sin(self.alpha[i])
        rz = np.array([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, self.d[i]], [0.0, 0.0, 0.0, 1.0]])
        rx = np.array([[1.0, 0.0, 0.0, self.a[i]], [0.0, ca, -sa, 0.0], [0.0, sa, ca, 0.0], [0.0, 0.0, 0.0, 1.0]])
        return rz @ rx                                              # ur10_simulation.py:204-211

    def fkine_all(self, q):
        Ts, T = [], None
        for i in range(self.n_joints):
            A = self.link(i, q[i] + self.theta_offset[i])
            T = A if T is None else T @ A
            Ts.append(T)
        return Ts

    def jacobian(self, Ts):
        p_e = Ts[-1][:3, 3]
        z, p, cols = np.array([0.0, 0.0, 1.0]), np.zeros(3), []
        for T in Ts:
            cols.append(np.concatenate([np.cross(z, p_e - p), z]))  # ur10_simulation.py:132-137
            z, p = T[:3, 2], T[:3, 3]
        return np.stack(cols, axis=1)

    def camera_pose_batch(self, q):
        """camera_pose(fkine(q)) for a whole array of joint vectors, q of shape (..., n) -> (..., 6): the same link products as
        ``link`` / ``fkine_all`` (ur10_simulation.py:97-110, 204-211) evaluated with stacked 4 x 4 matrices, for the sinks that log the
        camera pose of every step of every trial (results.csv / Parquet, main.py:160-165)."""
        q = np.asarray(q, float)
        T = None
        for i in range(self.n_joints):
            th = q[..., i] + self.theta_offset[i]
            c, s = np.cos(th), np.sin(th)
            ca, sa = np.cos(self.alpha[i]), np.sin(self.alpha[i])
            A = np.zeros(q.shape[:-1] + (4, 4))
            A[..., 0, 0], A[..., 0, 1], A[..., 0, 2], A[..., 0, 3] = c, -s * ca, s * sa, self.a[i] * c
            A[..., 1, 0], A[..., 1, 1], A[..., 1, 2], A[..., 1, 3] = s, c * ca, -c * sa, self.a[i] * s
            A[..., 2, 1], A[..., 2, 2], A[..., 2, 3] = sa, ca, self.d[i]
            A[..., 3, 3] = 1.0
            T = A if T is None else T @ A
        pose = np.empty(q.shape[:-1] + (6,))
        pose[..., :3] = T[..., :3, 3]
        pose[..., 3] = np.arctan2(T[..., 2, 1], T[..., 2, 2])
        pose[..., 4] = np.arcsin(np.clip(-T[..., 2, 0], -1.0, 1.0))
        pose[..., 5] = np.arctan2(T[..., 1, 0], T[..., 0, 0])
        return pose

    def project(self, T):
        R, t = T[:3, :3], T[:3, 3]
        f = np.empty(2 * self.n_points)
        for i, w in enumerate(self.points):
            pc = R.T @ (w - t)
            f[2 * i] = self.center + self.focal * pc[0] / pc[2]
            f[2 * i + 1] = self.center + self.focal * pc[1] / pc[2]
        return f

    def features(self, q):
        return self.project(self.fkine_all(q)[-1])

    def discs(self, q, radius=DISC_RADIUS):
        """(n_points, 3) rows (u, v, r) in pixels of the discs of physical ``radius`` (metres; a scalar or one per point) around the world
        points, seen from the camera at joints ``q``: the numpy statement uvs_camera_project_f64 is held to.  u, v as ``project``;
        r = focal * radius / depth along the optical axis, -1 for a point that is not in front of the camera (depth <= 0 or not finite)."""
        T = self.fkine_all(q)[-1]
        R, t = T[:3, :3], T[:3, 3]
        radius = np.broadcast_to(np.asarray(radius, float), (self.n_points,))
        out = np.empty((self.n_points, 3))
        with np.errstate(all='ignore'):
            for i, w in enumerate(self.points):
                pc = R.T @ (w - t)
                out[i, 0] = self.center + self.focal * pc[0] / pc[2]
                out[i, 1] = self.center + self.focal * pc[1] / pc[2]
                out[i, 2] = self.focal * radius[i] / pc[2] if pc[2] > 0 and np.isfinite(pc[2]) else -1.0
        return out

    # ---------------------------------------------------------------- device description
    def to_struct(self):
        n, npts = self.n_joints, self.n_points
        if n > _lib.UVS_MAX_N or npts > _lib.UVS_MAX_POINTS:
            raise ValueError('plant exceeds UVS_MAX_N / UVS_MAX_POINTS')
        s = _lib.Plant()
        s.n_joints, s.n_points = n, npts
        for i in range(n):
            s.theta_offset[i], s.d[i], s.a[i] = self.theta_offset[i], self.d[i], self.a[i]
            s.cos_alpha[i], s.sin_alpha[i] = np.cos(self.alpha[i]), np.sin(self.alpha[i])
        for i in range(npts):
            for c in range(3):
                s.points[i][c] = self.points[i][c]
        s.focal, s.center = self.focal, self.center
        s.kind = _lib.PLANT_DH_PINHOLE
        return s


    def to_camera(self, radius=DISC_RADIUS):
        """The ``uvs_camera`` struct of include/uvs_vision.h for discs of physical ``radius`` (metres; a scalar or one per point)."""
        from . import _vision
        n, npts = self.n_joints, self.n_points
        if n > _vision.MAX_JOINTS or npts not in _vision.N_COLOURS:
            raise ValueError('camera: at most 8 joints and 1, 3 or 4 points')
        s = _vision.Camera()
        s.n_joints, s.n_points = n, npts
        for i in range(n):
            s.theta_offset[i], s.d[i], s.a[i] = self.theta_offset[i], self.d[i], self.a[i]
            s.cos_alpha[i], s.sin_alpha[i] = np.cos(self.alpha[i]), np.sin(self.alpha[i])
        radius = np.broadcast_to(np.asarray(radius, float), (npts,))
        for i in range(npts):
            for c in range(3):
                s.points[i][c] = self.points[i][c]
            s.radius[i] = radius[i]
        s.focal, s.center = self.focal, self.center
        return s


def miscalibrated(plant, focal_scale=1.0, point_offset=(0.0, 0.0, 0.0), joint_offset=0.0, link_scale=1.0):
    """A new ``SyntheticPlant``: what a controller BELIEVES about ``plant`` when its calibration is off.  ``focal_scale`` multiplies the focal
    length (the intrinsics); ``point_offset`` -- (3,) or (n_points, 3) metres -- moves the world points (the depth assumption);
    ``joint_offset`` -- a scalar or one value per joint, radians -- is added to the encoder zeros ``theta_offset`` (the last joint's is a
    camera roll); ``link_scale`` multiplies ``d`` and ``a`` (link and hand-eye lengths).  ``fov_deg`` follows the new focal length, because
    ``analytic_guess`` derives its focal length from the robot's ``perspective_angle``; with ``focal_scale == 1`` it is kept as it is, and with
    all defaults the result equals ``plant`` field for field.  The result is an ordinary plant: hand it to ``engine.believed_models``, or
    to a ``SyntheticRobot`` for the numpy side."""
    focal = plant.focal * focal_scale
    fov_deg = plant.fov_deg if focal_scale == 1.0 else float(np.rad2deg(2.0 * np.arctan(plant.center / focal)))
    return SyntheticPlant(theta_offset=np.asarray(plant.theta_offset, float) + np.asarray(joint_offset, float),
                          d=np.asarray(plant.d, float) * link_scale, a=np.asarray(plant.a, float) * link_scale,
                          alpha=np.array(plant.alpha, float),
                          points=np.asarray(plant.points, float) + np.asarray(point_offset, float),
                          focal=focal, center=plant.center, fov_deg=fov_deg)


MOTION_WINDOW = (0, 2 ** 31 - 1)        # a target that moves from step 0 on, for as long as the loop runs
MOTION_ROW = 104                        # sizeof(uvs_target_motion): twelve doubles v[4][3], then int32 k_on, k_off


def motion_steps(k, window=MOTION_WINDOW):
    """s(k) of uvs_target_motion (include/uvs_vision.h): the steps a target has moved at step ``k`` >= 0 under the window (k_on, k_off),
    clamp(k - k_on, 0, max(k_off - k_on, 0)), in Python integers -- nothing overflows, whatever the int32 fields hold."""
    k, (k_on, k_off) = int(k), (int(w) for w in window)
    if k < 0:
        raise ValueError('k must be >= 0')
    return min(max(k - k_on, 0), max(k_off - k_on, 0))


def target_at(plant, velocity, k, window=MOTION_WINDOW):
    """A new ``SyntheticPlant``: ``plant`` with its world points where step ``k`` of a motion has taken them -- the numpy statement of the
    rule of uvs_target_motion (include/uvs_vision.h) that every moving-target kernel is held to.  ``velocity`` (n_points, 3): world metres
    per step of every disc; ``window`` (k_on, k_off), one for all discs.  With s = ``motion_steps(k, window)``: if s == 0 the points are
    the plant's own, bits untouched, with no arithmetic at all (a -0.0 stays -0.0, a velocity that is not finite moves nothing);
    otherwise, per coordinate, points + float64(s) * velocity: one rounded multiply, then one rounded add.  One plant and a scalar ``k``:
    not vectorised over trials."""
    velocity = np.asarray(velocity, np.float64)
    points = np.array(plant.points, np.float64)
    if velocity.shape != points.shape:
        raise ValueError(f'velocity: {points.shape} world metres per step, one row per disc, got {velocity.shape}')
    s = motion_steps(k, window)
    if s != 0:
        with np.errstate(all='ignore'):
            step = np.float64(s) * velocity
            points = points + step
    return SyntheticPlant(theta_offset=np.array(plant.theta_offset, float), d=np.array(plant.d, float), a=np.array(plant.a, float),
                          alpha=np.array(plant.alpha, float), points=points, focal=plant.focal, center=plant.center, fov_deg=plant.fov_deg)


def target_motion_array(velocity, window, n_points, T=None):
    """``velocity`` and ``window`` as the packed rows of uvs_target_motion (include/uvs_vision.h): a uint8 host array (T, ``MOTION_ROW``),
    row t = twelve float64 v[4][3] (rows from n_points on are zeros), then int32 k_on, k_off.  ``velocity``: (n_points, 3) -- every trial
    the same -- or (T, n_points, 3) reals, NaN and inf allowed (the device rule is total); ``window``: None (``MOTION_WINDOW``), (2,) or
    (T, 2) integers that are int32.  ValueError for anything else, or for T rows of either that do not match each other or ``T``."""
    try:
        v = np.asarray(velocity)
    except Exception as exc:                                         # ragged lists
        raise ValueError(f'target_motion: ({n_points}, 3) or (T, {n_points}, 3) reals, world metres per step') from exc
    if v.dtype.kind not in 'fiu' or v.ndim not in (2, 3) or v.shape[-2:] != (n_points, 3):
        raise ValueError(f'target_motion: ({n_points}, 3) or (T, {n_points}, 3) reals, world metres per step, got {v.dtype} {v.shape}')
    try:
        w = np.asarray(MOTION_WINDOW if window is None else window)
    except Exception as exc:
        raise ValueError('motion_window: (2,) or (T, 2) integers (k_on, k_off)') from exc
    if w.dtype.kind not in 'iu' or w.ndim not in (1, 2) or w.shape[-1] != 2:
        raise ValueError(f'motion_window: (2,) or (T, 2) integers (k_on, k_off), got {w.dtype} {w.shape}')
    if w.size and (w.min() < -2 ** 31 or w.max() > 2 ** 31 - 1):
        raise ValueError('motion_window: k_on and k_off are int32')
    rows = {a.shape[0] for a, nd in ((v, 3), (w, 2)) if a.ndim == nd}
    if T is not None:
        rows.add(T)
    if len(rows) > 1:
        raise ValueError(f'target_motion: {sorted(rows)} trials of velocities, windows and trials do not match')
    T = rows.pop() if rows else 1
    out = np.zeros((T, MOTION_ROW), np.uint8)
    vel = np.zeros((T, 4, 3), np.float64)
    vel[:, :n_points] = v.astype(np.float64)
    out[:, :96] = vel.reshape(T, 12).view(np.uint8)
    out[:, 96:] = np.ascontiguousarray(np.broadcast_to(w.astype(np.int32), (T, 2))).view(np.uint8)
    return out


MAX_LATENCY = 8                         # UVS_CAMERA_MAX_LATENCY: control periods between the pose a frame shows and the command from it


def delayed_step(k, d):
    """The step whose frame the detector is handed at step ``k`` >= 0 by a camera of latency ``d`` -- the numpy statement of the rule of
    include/uvs_vision.h (CAMERA LATENCY) that every delayed kernel is held to: kk = max(k - clamp(d, 0, MAX_LATENCY), 0), in Python
    integers.  The rule is total: a negative latency is none, a huge one is ``MAX_LATENCY``.  The frame of step kk shows joints q_kk,
    occluders, paints and target motion at kk; the noise added to its detection is that of step k; the delay line is primed with the
    step-0 frame."""
    k, d = int(k), int(d)
    if k < 0:
        raise ValueError('k must be >= 0')
    return max(k - min(max(d, 0), MAX_LATENCY), 0)


def aligned_regressor_step(k, a):
    """The step whose command is the estimator's regressor at step ``k`` >= 0 when the controller assumes a camera latency ``a``, or -1
    for "the zero vector" -- the numpy statement of the rule of include/uvs_vision.h (ASSUMED LATENCY) that every aligned kernel is held
    to: k - 1 - clamp(a, 0, MAX_LATENCY) where that is >= 0, in Python integers.  At latency d the difference f_k - f_{k-1} the
    estimator sees was caused by the command of step k - 1 - d; an assumed latency pairs it with that command.  Only the regressor moves:
    the command integrated into the joints stays dq_{k-1}.  The zero vector goes through the update with h = 0 that step 0 always ran.
    The law's counterpart is ``delayed_step(k, a)``: the step whose joints the calibrated or believed law is handed."""
    k, a = int(k), int(a)
    if k < 0:
        raise ValueError('k must be >= 0')
    return max(k - 1 - min(max(a, 0), MAX_LATENCY), -1)


def prediction_steps(k, p):
    """The steps whose commands the feature predictor sums at step ``k`` >= 0 with a prediction horizon ``p``, newest first -- the numpy
    statement of the rule of include/uvs_vision.h (FEATURE PREDICTION) that every predicted kernel is held to:
    k - 1, k - 2, ..., max(k - clamp(p, 0, MAX_LATENCY), 0), in Python integers; the empty list for p <= 0 or k == 0.  The estimators
    advance the reported feature row by X_k times the sum of those commands; the calibrated or believed law by h(q_k) - h(q_j), j the
    LAST step listed (or k itself where the list is empty).  For k < p the frame shown is frame 0: the missing terms are dropped."""
    k, p = int(k), int(p)
    if k < 0:
        raise ValueError('k must be >= 0')
    return list(range(k - 1, max(k - min(max(p, 0), MAX_LATENCY), 0) - 1, -1))


def projection_jacobian(plant, q, points=None):
    """The TRUE image Jacobian dh/dq of ``plant`` at joints ``q`` (6,), (2 n_points, 6) in pixels per radian -- no t_s in it: the numpy
    statement of the rule uvs_camera_jacobian_f64 (include/uvs_vision.h) is held to.  h = ``plant.features``; ``points`` (n_points, 3)
    replaces the plant's world points (a moved target: ``target_at(...).points``).  With T6 = fkine(q), R and c its rotation and origin,
    [v_j; w_j] column j of ``SyntheticPlant.jacobian`` and p = R^T (w - c) for a world point w:
        dp/dq_j = -R^T (w_j x (w - c) + v_j)
        du/dq_j = focal (dp_x / p_z - p_x dp_z / p_z^2), dv/dq_j likewise with p_y.
    That is the interaction row at the CENTRED pixels with the depth ALONG THE OPTICAL AXIS applied to the camera-frame twist;
    ``analytic_guess`` (uncentred pixels, the camera-disc distance, no t_s) is not this matrix.  What an estimator's X converges to is
    t_s times it: z = X dq with dq a velocity and q += dq t_s."""
    q = np.asarray(q, float)
    Ts = plant.fkine_all(q)
    R, c = Ts[-1][:3, :3], Ts[-1][:3, 3]
    Jg = plant.jacobian(Ts)
    points = np.asarray(plant.points if points is None else points, float)
    out = np.empty((2 * len(points), plant.n_joints))
    with np.errstate(all='ignore'):
        for i, w in enumerate(points):
            p = R.T @ (w - c)
            for j in range(plant.n_joints):
                dp = -R.T @ (np.cross(Jg[3:, j], w - c) + Jg[:3, j])
                out[2 * i, j] = plant.focal * (dp[0] / p[2] - p[0] * dp[2] / p[2] ** 2)
                out[2 * i + 1, j] = plant.focal * (dp[1] / p[2] - p[1] * dp[2] / p[2] ** 2)
    return out


SCORE_SUMS = ('nx2', 'nj2', 'dot', 'diff2', 'xd_xd', 'xd_jd')


def jacobian_score(X, Js, dq=None):
    """The six sums uvs_camera_jacobian_score_f64 (include/uvs_vision.h) is held to, for an estimate ``X`` against a scaled true Jacobian
    ``Js`` = t_s * ``projection_jacobian``: (..., m, n) arrays, or (..., m n) for X as the logs hold it; ``dq`` (..., n) or None.  Returns
    (..., 6) in the order of ``SCORE_SUMS``: nx2 = sum X^2, nj2 = sum Js^2, dot = sum X Js, diff2 = sum (X - Js)^2, each over (i, j) in
    row-major order from 0.0; xd_xd = |X dq|^2 and xd_jd = (X dq) . (Js dq), 0.0 without ``dq``.  ``score_ratios`` turns them into
    rel_err, cosine, scale, shape_err and step_ratio."""
    Js = np.asarray(Js, float)
    m, n = Js.shape[-2:]
    X = np.asarray(X, float)
    X = X.reshape(X.shape[:-1] + (m, n)) if X.shape[-1] == m * n and X.shape[-2:] != (m, n) else X
    X, Js = np.broadcast_arrays(X, Js)
    out = np.zeros(X.shape[:-2] + (6,))
    with np.errstate(all='ignore'):
        for i in range(m):
            for j in range(n):
                x, js = X[..., i, j], Js[..., i, j]
                out[..., 0] += x * x
                out[..., 1] += js * js
                out[..., 2] += x * js
                out[..., 3] += (x - js) * (x - js)
        if dq is not None:
            dq = np.asarray(dq, float)
            xd, jd = np.zeros(X.shape[:-1]), np.zeros(X.shape[:-1])
            for j in range(n):
                xd += X[..., :, j] * dq[..., None, j]
                jd += Js[..., :, j] * dq[..., None, j]
            for i in range(m):
                out[..., 4] += xd[..., i] * xd[..., i]
                out[..., 5] += xd[..., i] * jd[..., i]
    return out


def score_ratios(sums, xp=np):
    """What the six sums say, as a dict of arrays of the leading shape (``xp``: numpy, or torch for tensors): rel_err = sqrt(diff2 / nj2);
    cosine = dot / sqrt(nx2 nj2); scale = dot / nj2, the s that minimises |X - s Js|; shape_err = sqrt(max(nx2 nj2 - dot^2, 0) /
    (nx2 nj2)), the sine of the angle between them; step_ratio = xd_jd / xd_xd, the share of the displacement X promises for dq that the
    plant delivers (NaN where dq was not given or X dq == 0)."""
    nx2, nj2, dot, diff2, xd_xd, xd_jd = (sums[..., i] for i in range(6))
    with np.errstate(all='ignore'):                              # 0 / 0 is the NaN it should be
        both = nx2 * nj2
        gap = both - dot * dot
        gap = xp.where(gap < 0, xp.zeros_like(gap), gap)         # keeps a NaN a NaN
        return {'rel_err': xp.sqrt(diff2 / nj2), 'cosine': dot / xp.sqrt(both), 'scale': dot / nj2, 'shape_err': xp.sqrt(gap / both),
                'step_ratio': xd_jd / xd_xd}


class LinearPlant:
    """Consistent linearised camera f = f0 + J (q - q0) for shapes without a DH model (BASELINE config 5: m = 32, n = 7;
    a 7-joint arm would be redundant for a 6-DoF camera pose and leave the feature Jacobian rank 6).  J, f0, q0 are uploaded
    once and referenced by device pointer from the ``uvs_plant`` struct."""

    def __init__(self, jacobian, f0, q0):
        self.J = np.ascontiguousarray(jacobian, float)
        self.f0, self.q0 = np.ascontiguousarray(f0, float), np.ascontiguousarray(q0, float)
        self._dev = None

    @classmethod
    def random(cls, m=32, n=7, seed=0):
        rng = np.random.default_rng(seed)
        u, _ = np.linalg.qr(rng.normal(size=(m, n)))
        v, _ = np.linalg.qr(rng.normal(size=(n, n)))
        sv = np.geomspace(400.0, 20.0, n)                            # spread like the UR10 interaction matrix (cond ~ 20)
        return cls((u * sv) @ v.T, rng.uniform(90.0, 170.0, m), rng.uniform(-1.0, 1.0, n))

    @property
    def n_joints(self):
        return self.J.shape[1]

    def features(self, q):
        return self.f0 + self.J @ (np.asarray(q, float) - self.q0)

    def to_struct(self, device='cuda'):
        import torch
        if self._dev is None:
            self._dev = [torch.as_tensor(a, device=device) for a in (self.J.ravel(), self.f0, self.q0)]
        s = _lib.Plant()
        s.n_joints, s.n_points, s.kind = self.J.shape[1], self.J.shape[0] // 2, _lib.PLANT_LINEAR
        s.lin_jacobian, s.lin_f0, s.lin_q0 = (t.data_ptr() for t in self._dev)
        return s


class _Clock:
    def __init__(self):
        self.t = 0.0

    def getSimulationTime(self):
        return self.t


class SyntheticRobot:
    """The robot duck-type ``Experiment.run`` expects, backed by a ``SyntheticPlant``: kinematic joints
    (a commanded target is reached in one ``step()``), ``start`` advances the clock once (ur10_simulation.py:57)."""

    def __init__(self, plant=None, dt=0.05, logger=None, visualization=False):
        self.plant = SyntheticPlant.ur10() if plant is None else plant
        self.dt = dt
        self.perspective_angle = self.plant.fov_deg
        self.sim = _Clock()
        self.q = np.zeros(self.plant.n_joints)
        self.q_target = self.q.copy()
        self._Ts = self.plant.fkine_all(self.q)

    def start(self, q=None):
        if q is not None:
            self.q = np.array(q, float)
        self.q_target = self.q.copy()
        self.sim.t = 0.0
        self._Ts = self.plant.fkine_all(self.q)
        self.step()

    def stop(self):
        pass

    def step(self):
        self.q = self.q_target.copy()
        self.sim.t += self.dt

    def getJointsPos(self):
        return self.q

    def setJointsPos(self, q):
        self.q_target = np.array(q, float)

    def fkine(self, recalculate=False, all_transforms=False):
        if recalculate:
            self._Ts = self.plant.fkine_all(self.q)
        return tuple(self._Ts[::-1]) if all_transforms else self._Ts[-1]

    def jacobian(self, recalculate_fkine=False):
        if recalculate_fkine:
            self._Ts = self.plant.fkine_all(self.q)
        return self.plant.jacobian(self._Ts)

    def getCameraRotation(self, recalculate_fkine=False):
        return self.fkine(recalculate_fkine)[:3, :3]

    def getCameraPosition(self, recalculate_fkine=False):
        return self.fkine(recalculate_fkine)[:3, 3]

    def computePose(self, recalculate_fkine=False):
        return camera_pose(self.fkine(True))

    def computeZ(self, n=1, recalculate_fkine=False):
        cam = self.getCameraPosition(recalculate_fkine)
        return np.array([np.linalg.norm(cam - w) for w in self.plant.points[:n]])

    def getCameraImage(self):
        return self, (RESOLUTION, RESOLUTION)

    def features(self):
        return self.plant.project(self.fkine(True))


class CameraRobot:
    """A robot that carries a camera: the duck-type of ``SyntheticRobot`` (to which everything but the camera is delegated) whose
    ``getCameraImage()`` returns a real frame -- uint8 (256, 256, 3), unflipped, the plant's discs drawn by ``render_discs`` at their
    projected centres and radii -- so that ``Experiment`` detects its features from pixels, on the host or (perception='device') on the GPU.
    Deliberately NOT a ``SyntheticRobot``: ``Experiment.run()`` sends those down the plant-in-kernel route, and this robot has to take the
    external-robot route.  ``radius``: physical disc radius in metres; the default 0.024 m measures 8.01 px at ``SyntheticPlant.ur10()``'s
    goal pose (depth 0.602 m, focal 200.9 px).  A disc is drawn as a circle, not as the ellipse a tilted camera would see.
    ``occluders``: None, or (n_occ, 8) integer rows of ``OCCLUDER_FIELDS``, drawn in ``shade`` at the robot's step count ``k`` -- 0 from
    ``start()`` on, one more with every ``step()`` after it, so that the loop's guess image and its first image are both the step-0 frame,
    as in ``engine.camera_closed_loop(occluders=...)``.  ``occluder_colours``: None, or (n_occ,) paints of those occluders
    (``occluder_colour_array``): a painted one is a distractor of that disc's colour.
    ``target_motion``: None, or (n_points, 3) world velocities in metres per step, with ``motion_window`` (k_on, k_off) or None
    (``MOTION_WINDOW``): the discs stand where step ``k`` of that motion has taken them (``target_at``), so ``discs()`` and
    ``getCameraImage()`` show the frames ``engine.camera_closed_loop(target_motion=...)`` detects.  The robot's own kinematics -- what
    the calibrated law reads -- keep the plant's points: the controller does not know the target's motion.
    ``latency``: an integer 0 .. ``MAX_LATENCY``, the camera's latency in control periods: at step ``k`` ``discs()`` and
    ``getCameraImage()`` show the frame of step ``delayed_step(k, latency)`` -- the joints, occluders, paints and target motion of that
    step -- rendered on demand from the joints kept since ``start()``.  The robot's own joints, what the encoders report, are the
    current ones.  0 (the default) is the robot without the argument."""

    def __init__(self, plant=None, radius=DISC_RADIUS, dt=0.05, background=96, occluders=None, shade=32, occluder_colours=None,
                 target_motion=None, motion_window=None, latency=0):
        self._robot = SyntheticRobot(plant, dt)
        self.radius, self.background, self.shade = radius, background, shade
        self.occluders = None if occluders is None else occluder_array(occluders, 1)[0]
        self.occluder_colours = None
        if occluder_colours is not None:
            self.occluder_colours = occluder_colour_array(occluder_colours, None if occluders is None else len(self.occluders),
                                                          self._robot.plant.n_points, 1)[0]
        if not 0 <= shade < 250:
            raise ValueError('shade must be 0 .. 249: 250 and above would enter a mask of the detectors')
        if target_motion is None and motion_window is not None:
            raise ValueError('motion_window without target_motion: a window belongs to a motion')
        self.target_motion, self.motion_window = None, MOTION_WINDOW
        if target_motion is not None:
            npts = self._robot.plant.n_points
            target_motion_array(target_motion, motion_window, npts, 1)          # its refusals
            self.target_motion = np.array(target_motion, np.float64).reshape(npts, 3)
            if motion_window is not None:
                self.motion_window = tuple(int(w) for w in np.asarray(motion_window).reshape(2))
        if isinstance(latency, bool) or not isinstance(latency, (int, np.integer)) or not 0 <= latency <= MAX_LATENCY:
            raise ValueError(f'latency is an integer 0 .. {MAX_LATENCY} control periods, got {latency!r}')
        self.latency = int(latency)
        self._shown = []                                            # the joints of the last latency + 1 steps, the current ones last
        self.k = 0

    def __getattr__(self, name):                                    # everything but the camera: the synthetic robot's
        if name == '_robot':
            raise AttributeError(name)
        return getattr(self._robot, name)

    def start(self, q=None):
        self._robot.start(q)
        self.k = 0
        self._shown = [np.array(self._robot.q, np.float64)]

    def step(self):
        self._robot.step()
        self.k += 1
        self._shown = (self._shown + [np.array(self._robot.q, np.float64)])[-(self.latency + 1):]

    def _frame_step(self):
        """(step, joints) of the frame the camera shows now: ``delayed_step(k, latency)`` and the joints kept from it."""
        kk = delayed_step(self.k, self.latency)
        if kk == self.k or not self._shown:                         # no latency, or a robot that was never started: the current joints
            return self.k, self._robot.q
        return kk, self._shown[-1 - (self.k - kk)]

    def discs(self):
        kk, q = self._frame_step()
        if self.target_motion is not None:
            return target_at(self._robot.plant, self.target_motion, kk, self.motion_window).discs(q, self.radius)
        return self._robot.plant.discs(q, self.radius)

    def getCameraImage(self):
        frame = render_discs(self.discs(), self._robot.plant.n_points, self.background, self.occluders, self._frame_step()[0], self.shade,
                             self.occluder_colours)
        return frame, (RESOLUTION, RESOLUTION)
