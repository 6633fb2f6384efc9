"""numpy restatement of the calibrated IBVS baseline through pixels ON A WRONG MODEL, one trial at a time: the checker of
uvs_camera_believed_step_f64 / uvs_camera_believed_loop_f64.  It is tests/camera_analytical_ref.run with two changes: the sensor (``detect``:
disc projection, rasteriser, host detector) is on the TRUE plant, and ``step`` (the image Jacobian from analytic_guess, numpy's pinv) is on
the BELIEVED plant and its SyntheticRobot.  The joints are the true ones: the arm moves as commanded, whatever the controller believes.
With ``believed_plant is true_plant`` it returns exactly the arrays of camera_analytical_ref.run."""
import numpy as np

import uvs_amd
from camera_analytical_ref import detect, step  # noqa: F401  (step: the believed step of one trial, for the GPU tests)


def run(true_plant, believed_plant, q_start, noise, desired, dt, gain, steps, radius=uvs_amd.plant.DISC_RADIUS):
    """One trial.  Arguments and result as camera_analytical_ref.run (without ``ideal``), ``j`` being the believed interaction matrix."""
    K, m = int(steps), 2 * true_plant.n_points
    assert believed_plant.n_points == true_plant.n_points and believed_plant.n_joints == true_plant.n_joints
    robot = uvs_amd.SyntheticRobot(believed_plant, dt)
    out = dict(err=np.zeros((K, m)), f=np.zeros((K, m)), q=np.zeros((K, 6)), dq=np.zeros((K, 6)), j=np.zeros((K, m * 6)),
               discs=np.zeros((K, true_plant.n_points, 3)), masks=np.zeros((K, true_plant.n_points), int))
    acc = np.zeros((3, m))
    q, t = np.array(q_start, float), 0.0 + dt
    status, k_done = 0, K
    for k in range(K):
        f, out['discs'][k], out['masks'][k] = detect(true_plant, q, radius)
        if noise is not None:
            f = f + noise[k]
        out['q'][k], out['f'][k] = q, f
        J, err, dq = step(believed_plant, robot, q, f, desired, gain)
        if dq is None:
            status, k_done = 1, k
            break
        out['err'][k], out['dq'][k], out['j'][k] = err, dq, J.reshape(-1)
        acc += np.stack([err * err, np.abs(err), t * np.abs(err)])
        q = q + dq * dt
        t += dt
    return dict(out, status=status, k_done=k_done, stats=np.sqrt((acc ** 2).sum(axis=1)))
