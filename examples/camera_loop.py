#!/usr/bin/env python3
"""What does the camera's pixel grid do to the estimators?  The same small batch of closed-loop trials twice: through engine.closed_loop, which
feeds the estimator the ideal projections of the discs plus noise, and through engine.camera_closed_loop, which feeds it what the centre-of-mass
detector returns for the 256 x 256 frame of those discs (the reference's live route) plus the same noise.  Prints the median ISE / IAE / ITAE of
both, side by side, and the smallest colour mask the detector ever saw.
--fused runs the pixel loop as one launch with the initial guess computed on the device (engine.camera_closed_loop(fused=True, guess='device')).
--baseline answers the question the reference's experiment asks -- what does not knowing the Jacobian cost? -- through pixels: the chosen
estimator and the calibrated control law (Method.ANALYTICAL, fp.method == ANALYTICAL) on the same starts and the same noise, paired trial by
trial over the trials both ran to the end, with the FAIL count of each.
--miscalibration asks what each side loses when the model is WRONG -- the experiment that motivates uncalibrated visual servoing.  A ladder
of miscalibration levels (LEVELS below: the signed fraction of a focal length 20 % long, discs believed 5 cm aside and 20 cm lower, encoder
zeros off by up to 0.1 rad, links 3 % short; a negative level errs the other way) times the trials is ONE launch per side: the calibrated law on every trial's believed model
(engine.camera_closed_loop(believed=..., believed_index=...)), and the estimator started from the analytic guess of that same wrong model, on the
same starts and the same noise at every level.  Prints the median ISE / IAE / ITAE per level over the trials neither side FAILed.
--grid asks which kernel bandwidth and which gain survive pixel quantisation: kernel_bw x gain (GRID_BANDWIDTHS x GRID_GAINS below) over the SAME
starts and the same noise is ONE launch (engine.camera_closed_loop(fused=True, trial_params=...) with a 'source' index, so the inputs are
uploaded once, not once per cell).  Prints the median ISE / IAE / ITAE per cell over the trials that ran to the end, and the FAIL count.
--occlusion asks who survives a real outlier: a 12 px bar of full height crosses the frame at constant speed while the servo runs
(engine.camera_closed_loop(occluders=...)); a disc behind it loses a side of its mask and its centroid jumps.  GMCKF, KF and the calibrated law
(stepwise) on the same starts and noise; prints the median ISE / IAE / ITAE and the FAIL count without and with the bar.
--occlusion --hold N asks the question the narrow bar could not: who survives a FULL occlusion?  The bar is 28 px wide -- a disc is about 17 px
across at the goal -- and crosses the discs during the transient, so every mask is empty for a few steps.  Without a hold every trial FAILs
there; with engine.camera_closed_loop(hold=N) a lost disc's last detection is reported again for up to N steps (df = 0 while dq != 0, then a
jump: the outlier the correntropy estimators exist for).  KF, MCKF, IMCC-KF, GMCKF (one launch each) and the calibrated law (stepwise) on the
same starts and noise; prints the FAIL count at hold = 0 beside the median ISE / IAE / ITAE, the FAIL count and the held steps at hold = N.
--distractor asks about the outlier a colour threshold is best known for: something else in the scene has the target's colour.  A still
6 x 6 px rectangle of the green disc's colour sits 20 px from green's goal position (engine.camera_closed_loop(occluders=, occluder_colours=)):
its pixels enter green's mask and pull the centroid towards it, by an amount that grows as the disc shrinks or is covered -- and the detector
never reports a loss.  KF, MCKF, IMCC-KF, GMCKF (one launch each) and the calibrated law (stepwise) on the same starts and noise; prints the
median ISE / IAE / ITAE and the FAIL count without and with the distractor.  With --occlusion --hold N the wide bar of above crosses the
frame as well, behind the distractor, and lost discs are held: green, whose distractor stays visible, is never lost.
--scenes N asks the question an UNCALIBRATED method exists for: what if the scene itself is not the nominal one?  N true scenes drawn around
the nominal plant (plant.miscalibrated, seeded: focal length +-10 %, targets +-2 cm, camera roll +-3 degrees, links +-2 %) times the trials is
ONE launch per method (engine.camera_closed_loop(cameras=..., camera_index=...)): every trial's frames come from its own camera.  KF, MCKF,
IMCC-KF and GMCKF start from the nominal model's guess, next to the calibrated law on the nominal model and on the truth.  Prints the median
ISE / IAE / ITAE over the trials that ran to the end, the FAIL count and the FAILs of the worst scene.
--moving asks the classic servoing question: can the loop TRACK?  After the servo has converged the target moves for a window of steps
(MOVING_WINDOW below, every disc with the same seeded world velocity of MOVING_SPEED metres per step in the floor plane, one direction per
motion) and then stops (engine.camera_closed_loop(target_motion=..., motion_window=...)): N_MOTIONS motions x the trials in ONE launch per
method.  While the target moves, the features move and dq does not explain it -- the estimators' measurement model is broken at every step
-- and the calibrated law's depths go stale: its model of the points stays where it was.  The chosen estimator, KF and the calibrated law on
the same starts and noise; prints the median ISE / IAE / ITAE, the FAIL count, and the median feature error at the window's last step and
at the last step of the run (re-convergence).
--latency asks the textbook robustness question of visual servoing: what if the frame is old?  LATENCIES control periods between the pose a
frame shows and the command computed from it (engine.camera_closed_loop(latency=...)), each x the trials over the same starts and noise in
ONE launch per method: the estimators pair f_k - f_{k-1} with a regressor that is d steps too new, and the calibrated law feeds an
interaction matrix at the current joints the features of the pose d steps ago.  Nobody is told the latency.  The chosen estimator, KF and
the calibrated law; prints the median ISE / IAE / ITAE, the FAIL count and the median feature error at the last step, per latency.
--latency --told tells the controller: LATENCIES x ASSUMED assumed latencies x the trials in ONE launch per method
(engine.camera_closed_loop(latency=, assumed_latency=)) -- the estimators' regressor becomes the command of step k - 1 - a, the law's joints
those of step max(k - a, 0) -- told (a > 0) and untold (a = 0) on the same starts and noise.  Prints the median ISE and the FAILs with their
median k_done per (d, a) cell: the diagonal is what telling recovers, the rest how wrong the assumed latency may be.
--latency --predict lets the control law predict the features over the latency: LATENCIES x HORIZONS prediction horizons x the trials in
ONE launch per method (engine.camera_closed_loop(latency=, assumed_latency=, predict=)), every controller told the true latency (a = d) --
the estimators' law acts on f + X_k (dq_{k-1} + ... + dq_{k-p}), the calibrated law on f + (h(q_k) - h(q_{k-p})).  Prints per (d, p) cell
the FAIL count, the median ISE as returned -- it is on the PREDICTED error, so it is not comparable across p -- and a "true" ISE recomputed
from the q log with engine.camera_features at the logged joints against the target, which is.
--score looks at the product itself, the Jacobian estimate: KF, MCKF, IMCC-KF and GMCKF log X_k (engine.camera_closed_loop(want=
ESTIMATOR_CAMERA_LOGS)) and engine.camera_jacobian_score scores every X_k against t_s times the TRUE image Jacobian of the trial's scene at
q_k (engine.camera_jacobian), on the device.  Twice on the same starts and noise: from the reference's analytic guess, and from
x0 = t_s * camera_jacobian(q_start), the correctly scaled start.  Prints per estimator the ISE of both and, at steps 0, 1, 5, 20, 100 and
K - 1, the median over the trials of scale (the s that minimises |X - s t_s J|), cosine, rel_err and step_ratio (the share of the
displacement X promises for dq_k that the plant delivers).  --latency (every trial at latency 2, told), --moving and --scenes N combine
with it: the truth is then the moved target's, or the trial's own scene's.
usage: examples/camera_loop.py [--method GMCKF] [--trials 64] [--sigma 0.3] [--radius 0.024] [--seed 0] [--fused] [--baseline] [--miscalibration]
       [--grid] [--occlusion [--hold N]] [--distractor [--occlusion --hold N]] [--scenes N] [--moving] [--latency [--told | --predict]]
       [--score [--latency] [--moving] [--scenes N]]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (-1.0, -0.5, 0.0, 0.5, 1.0)                                  # fraction of the full miscalibration below, either way; 0 is the true model
JOINT_OFFSETS = np.array([0.03, -0.02, 0.04, -0.03, 0.02, 0.1])      # radians; the last one is a camera roll


def believed_plant(uvs, plant, level):
    """The model believed at miscalibration ``level``: every knob of plant.miscalibrated moved by that fraction of its full value."""
    return uvs.plant.miscalibrated(plant, focal_scale=1.0 + 0.2 * level, point_offset=level * np.array([0.05, -0.05, -0.2]),
                                   joint_offset=level * JOINT_OFFSETS, link_scale=1.0 - 0.03 * level)


def miscalibration_table(uvs, method='GMCKF', trials=64, sigma=0.3, radius=None, seed=0, levels=LEVELS):
    """The robustness table as a list of lines: levels x trials in one launch per side."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True)
    fp_cal = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, desired)
    n, K = len(levels), fp.steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    q0_d = torch.as_tensor(np.tile(q0, (n, 1)), device='cuda')       # the same starts and the same noise at every level
    noise_d = torch.as_tensor(np.tile(noise, (1, n, 1)), device='cuda')
    believed = uvs.engine.believed_models([believed_plant(uvs, plant, level) for level in levels], radius)
    index = np.repeat(np.arange(n, dtype=np.int32), trials)
    kw = dict(radius=radius, fused=True, want=(), believed=believed, believed_index=index)
    calibrated = uvs.engine.camera_closed_loop(fp_cal, plant, q0_d, noise_d, **kw)
    estimator = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, guess='device', **kw)
    torch.cuda.synchronize()
    lines = [f'miscalibration ladder, {n} levels x {trials} trials of {K} steps in one launch per side, white noise {sigma} px; '
             'median over the trials neither side FAILed',
             f'{"level":>6s}{"focal":>7s}{"paired":>8s}   {"ANALYTICAL on the wrong model":^36s}{"FAIL":>6s}   {method + " started from it":^36s}{"FAIL":>6s}',
             f'{"":21s}   {"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}   {"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}']
    for i, level in enumerate(levels):
        rows = slice(i * trials, (i + 1) * trials)
        ok_cal, ok_est = ((out['status'][rows] == 0).cpu().numpy() for out in (calibrated, estimator))
        both = ok_cal & ok_est
        med = [np.median(out['stats'][rows].cpu().numpy()[both], axis=0) if both.any() else np.full(3, np.nan) for out in (calibrated, estimator)]
        lines.append(f'{level:6.2f}{1.0 + 0.2 * level:7.2f}{int(both.sum()):>8d}   {med[0][0]:12.3f}{med[0][1]:12.3f}{med[0][2]:12.3f}{int((~ok_cal).sum()):>6d}'
                     f'   {med[1][0]:12.3f}{med[1][1]:12.3f}{med[1][2]:12.3f}{int((~ok_est).sum()):>6d}')
    return lines


GRID_BANDWIDTHS = (1.0, 2.0, 3.5, 5.0, 7.5, 10.0, 15.0, 20.0)         # sigma_0, pixels
GRID_GAINS = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5)


def grid_table(uvs, method='GMCKF', trials=16, sigma=0.3, radius=None, seed=0, bandwidths=GRID_BANDWIDTHS, gains=GRID_GAINS):
    """The kernel_bw x gain table through pixels as a list of lines: cells x trials in one launch."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    fp = uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True)
    K = fp.steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    cells = [(bw, gain) for bw in bandwidths for gain in gains]
    T = len(cells) * trials
    tp = {'kernel_bw': torch.as_tensor(np.repeat([c[0] for c in cells], trials), device='cuda'),
          'gain': torch.as_tensor(np.repeat([c[1] for c in cells], trials), device='cuda'),
          'source': np.arange(T) % trials}                            # cell c is the output trials [c trials, (c + 1) trials), all reading the same inputs
    out = uvs.engine.camera_closed_loop(fp, plant, torch.as_tensor(q0, device='cuda'), torch.as_tensor(noise, device='cuda'), radius=radius,
                                        fused=True, guess='device', want=(), trial_params=tp)
    torch.cuda.synchronize()
    status, stats = out['status'].cpu().numpy().reshape(len(cells), trials), out['stats'].cpu().numpy().reshape(len(cells), trials, 3)
    lines = [f'{method} through pixels, kernel_bw x gain: {len(cells)} cells x {trials} trials of {K} steps in one launch, white noise {sigma} px, '
             'the same starts and noise in every cell; median over the trials that ran to the end',
             f'{"kernel_bw":>10s}{"gain":>7s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"FAIL":>6s}']
    for c, (bw, gain) in enumerate(cells):
        ok = status[c] == 0
        med = np.median(stats[c][ok], axis=0) if ok.any() else np.full(3, np.nan)
        lines.append(f'{bw:10.2f}{gain:7.2f}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~ok).sum()):>6d}')
    medians = np.array([np.median(stats[c][status[c] == 0], axis=0) if (status[c] == 0).any() else np.full(3, np.inf) for c in range(len(cells))])
    for i, name in enumerate(('ISE', 'IAE', 'ITAE')):
        best = int(np.argmin(medians[:, i]))
        lines.append(f'smallest median {name}: kernel_bw {cells[best][0]:g}, gain {cells[best][1]:g}')
    return lines


BAR = (-12, 0, 12, 256, 1, 0, 0, 2 ** 31 - 1)                         # x, y, w, h, vx, vy, k_on, k_off: a 12 px bar of full height, 1 px per step


def occlusion_table(uvs, trials=64, sigma=0.3, radius=None, seed=0, bar=BAR):
    """The occlusion table as a list of lines: GMCKF, KF (one launch each) and the calibrated law (stepwise: its one-launch loop has no
    occluders) on the same starts and noise, without and with the bar crossing the frame while the servo runs."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    fps = {method: uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True) for method in ('GMCKF', 'KF', 'ANALYTICAL')}
    K = fps['GMCKF'].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    q0_d = torch.as_tensor(q0, device='cuda')
    noise_d = torch.as_tensor(rng.standard_normal((K, trials, 8)) * sigma, device='cuda')
    occluders = uvs.engine.occluders([bar], trials)
    lines = [f'a {bar[2]} px bar of full height crossing the frame at {bar[4]} px per step, {trials} trials of {K} steps, white noise {sigma} px; '
             'median over the trials that ran to the end',
             f'{"":28s}{"without the bar":^36s}{"FAIL":>6s}   {"behind the bar":^36s}{"FAIL":>6s}{"mask":>6s}',
             f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}   {"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}{"min":>6s}']
    for method, fp in fps.items():
        kw = dict(radius=radius, want=()) if method == 'ANALYTICAL' else dict(radius=radius, fused=True, guess='device', want=())
        row = f'{method + (" (calibrated, stepwise)" if method == "ANALYTICAL" else ""):28s}'
        for occ in (None, occluders):
            out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, occluders=occ, **kw)
            torch.cuda.synchronize()
            done = (out['status'] == 0).cpu().numpy()
            med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
            row += f'{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>6d}' + ('   ' if occ is None else f'{int(out["pixels"].min()):>6d}')
        lines.append(row)
    return lines


WIDE_BAR = (20, 0, 28, 256, 2, 0, 0, 2 ** 31 - 1)                     # a 28 px bar of full height, 2 px per step: over the discs in steps 20 .. 70


def hold_table(uvs, hold, trials=64, sigma=0.3, radius=None, seed=0, bar=WIDE_BAR):
    """The full-occlusion table as a list of lines: the four estimators (one launch each) and the calibrated law (stepwise) behind a bar wider
    than a disc, on the same starts and noise, with hold = 0 and with hold = ``hold``."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = ('KF', 'MCKF', 'IMCCKF', 'GMCKF', 'ANALYTICAL')
    fps = {method: uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True) for method in methods}
    K = fps['GMCKF'].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    q0_d = torch.as_tensor(q0, device='cuda')
    noise_d = torch.as_tensor(rng.standard_normal((K, trials, 8)) * sigma, device='cuda')
    occluders = uvs.engine.occluders([bar], trials)
    lines = [f'a {bar[2]} px bar of full height crossing the frame at {bar[4]} px per step from column {bar[0]}, {trials} trials of {K} steps, '
             f'white noise {sigma} px; median over the trials that ran to the end',
             f'{"":28s}{"hold = 0":>10s}   {"hold = " + str(hold):^36s}{"FAIL":>6s}{"held":>8s}{"most":>9s}',
             f'{"":28s}{"FAIL":>10s}   {"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}{"steps":>8s}{"per disc":>9s}']
    for method, fp in fps.items():
        kw = dict(radius=radius, want=()) if method == 'ANALYTICAL' else dict(radius=radius, fused=True, guess='device', want=())
        unheld = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, occluders=occluders, **kw)
        out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, occluders=occluders, hold=hold, **kw)
        torch.cuda.synchronize()
        done = (out['status'] == 0).cpu().numpy()
        med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
        held = out['held'].cpu().numpy()
        lines.append(f'{method + (" (stepwise)" if method == "ANALYTICAL" else ""):28s}{int((unheld["status"] != 0).sum()):>10d}   '
                     f'{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>6d}{int(held.sum()):>8d}{int(held.max()):>9d}')
    return lines


DISTRACTOR = (139, 100, 6, 6, 0, 0, 0, 2 ** 31 - 1)                   # still, 20 px from green's goal position (125, 121), beside its disc
GREEN = 1


def distractor_table(uvs, trials=64, sigma=0.3, radius=None, seed=0, rect=DISTRACTOR, bar=None, hold=0):
    """The distractor table as a list of lines: the four estimators (one launch each) and the calibrated law (stepwise) on the same starts
    and noise, with the rectangle opaque and with it painted green.  ``bar``: an opaque occluder behind the rectangle, or None; ``hold``."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = ('KF', 'MCKF', 'IMCCKF', 'GMCKF', 'ANALYTICAL')
    fps = {method: uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True) for method in methods}
    K = fps['GMCKF'].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    q0_d = torch.as_tensor(q0, device='cuda')
    noise_d = torch.as_tensor(rng.standard_normal((K, trials, 8)) * sigma, device='cuda')
    rows = ([] if bar is None else [bar]) + [rect]                    # the rectangle last: in front of the bar
    occluders = uvs.engine.occluders(rows, trials)
    paints = {'opaque': [-1] * len(rows), 'green': [-1] * (len(rows) - 1) + [GREEN]}
    behind = '' if bar is None else f', in front of a {bar[2]} px opaque bar at {bar[4]} px per step, hold = {hold}'
    lines = [f'a still {rect[2]} x {rect[3]} px rectangle at ({rect[0]}, {rect[1]}){behind}, {trials} trials of {K} steps, white noise {sigma} px; '
             'median over the trials that ran to the end',
             f'{"":28s}{"the rectangle opaque":^36s}{"FAIL":>6s}   {"painted green: a distractor":^36s}{"FAIL":>6s}{"green":>7s}',
             f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}   {"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"":6s}{"held":>7s}']
    for method, fp in fps.items():
        kw = dict(radius=radius, want=()) if method == 'ANALYTICAL' else dict(radius=radius, fused=True, guess='device', want=())
        row = f'{method + (" (calibrated, stepwise)" if method == "ANALYTICAL" else ""):28s}'
        for name in ('opaque', 'green'):
            out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, occluders=occluders, occluder_colours=paints[name], hold=hold, **kw)
            torch.cuda.synchronize()
            done = (out['status'] == 0).cpu().numpy()
            med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
            row += f'{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>6d}'
            row += '   ' if name == 'opaque' else (f'{int(out["held"][:, GREEN].sum()):>7d}' if hold else f'{"-":>7s}')
        lines.append(row)
    return lines


def scene_plants(uvs, plant, n, seed):
    """n plausible true scenes around ``plant``, seeded: focal length +-10 %, every target +-2 cm, camera roll +-3 degrees, links +-2 %."""
    rng = np.random.default_rng(seed + 1000)
    roll = np.zeros(6)
    out = []
    for _ in range(n):
        roll[5] = np.deg2rad(rng.uniform(-3.0, 3.0))
        out.append(uvs.plant.miscalibrated(plant, focal_scale=rng.uniform(0.9, 1.1), point_offset=rng.uniform(-0.02, 0.02, (plant.n_points, 3)),
                                           joint_offset=roll.copy(), link_scale=rng.uniform(0.98, 1.02)))
    return out


def scenes_table(uvs, n_scenes, trials=64, sigma=0.3, radius=None, seed=0):
    """The Monte-Carlo over TRUE scenes as a list of lines: n_scenes x trials in ONE launch per method
    (engine.camera_closed_loop(cameras=..., camera_index=...)).  The four estimators start from the NOMINAL model's analytic guess -- they
    do not know the scene -- next to the calibrated law on the nominal model (wrong in every scene) and on the truth of every trial."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    nominal = uvs.SyntheticPlant.ur10(desired)
    methods = ('KF', 'MCKF', 'IMCCKF', 'GMCKF', 'ANALYTICAL')
    fps = {method: uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True) for method in methods}
    K = fps['GMCKF'].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    q0_d = torch.as_tensor(np.tile(q0, (n_scenes, 1)), device='cuda')            # the same starts and the same noise in every scene
    noise_d = torch.as_tensor(np.tile(noise, (1, n_scenes, 1)), device='cuda')
    cameras = uvs.engine.camera_scenes(scene_plants(uvs, nominal, n_scenes, seed), radius)
    index = np.repeat(np.arange(n_scenes, dtype=np.int32), trials)
    kw = dict(radius=radius, fused=True, want=(), cameras=cameras, camera_index=index)
    lines = [f'{n_scenes} true scenes (focal +-10 %, targets +-2 cm, camera roll +-3 deg, links +-2 %) x {trials} trials of {K} steps in one launch '
             f'per method, white noise {sigma} px; median over the trials that ran to the end',
             f'{"":44s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"FAIL":>8s}{"worst scene":>13s}',
             f'{"":44s}{"":36s}{"":8s}{"FAILs":>13s}']
    runs = [(method + ', started from the nominal guess', fps[method], dict(guess='device', believed=nominal)) for method in methods[:4]]
    runs += [('ANALYTICAL on the nominal model', fps['ANALYTICAL'], dict(believed=nominal)), ('ANALYTICAL on the truth', fps['ANALYTICAL'], dict())]
    for name, fp, more in runs:
        out = uvs.engine.camera_closed_loop(fp, nominal, q0_d, noise_d, **kw, **more)
        torch.cuda.synchronize()
        done = (out['status'] == 0).cpu().numpy()
        med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
        worst = int((~done).reshape(n_scenes, trials).sum(axis=1).max())
        lines.append(f'{name:44s}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>8d}{worst:>13d}')
    return lines


MOVING_WINDOW = (150, 200)                                            # steps: the target moves after the servo has converged, then stops
MOVING_SPEED = 0.001                                                 # metres per step: 5 cm over the window, some 17 px at the goal
N_MOTIONS = 8


def moving_velocities(n_motions, n_points, seed, speed=MOVING_SPEED):
    """(n_motions, n_points, 3) world velocities: per motion one seeded direction in the floor plane, the same for every disc."""
    angle = np.random.default_rng(seed + 2000).uniform(0.0, 2.0 * np.pi, n_motions)
    v = np.stack([speed * np.cos(angle), speed * np.sin(angle), np.zeros(n_motions)], axis=1)
    return np.repeat(v[:, None, :], n_points, axis=1)


def moving_table(uvs, method='GMCKF', trials=64, sigma=0.3, radius=None, seed=0, n_motions=N_MOTIONS, window=MOVING_WINDOW):
    """The tracking table as a list of lines: n_motions x trials in ONE launch per method (engine.camera_closed_loop(target_motion=,
    motion_window=)).  No finding is drawn here: the table is what the experiment prints."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = tuple(dict.fromkeys((method, 'KF', 'ANALYTICAL')))
    fps = {name: uvs.engine.make_params(8, 6, name, 10.0, False, 0.05, 15.0, 0.2, desired, True) for name in methods}
    K = fps[method].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    q0_d = torch.as_tensor(np.tile(q0, (n_motions, 1)), device='cuda')           # the same starts and the same noise under every motion
    noise_d = torch.as_tensor(np.tile(noise, (1, n_motions, 1)), device='cuda')
    T = n_motions * trials
    motions = uvs.engine.target_motions(np.repeat(moving_velocities(n_motions, 4, seed), trials, axis=0), window, 4, T)
    at = (min(window[1], K) - 1, K - 1)
    lines = [f'{n_motions} target motions ({MOVING_SPEED * 1e3:g} mm per step in the floor plane during steps {window[0]} .. {window[1] - 1}) x {trials} '
             f'trials of {K} steps in one launch per method, white noise {sigma} px; median over the trials that ran to the end',
             f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"FAIL":>8s}{"|err| at step " + str(at[0]):>20s}{"|err| at step " + str(at[1]):>20s}']
    for name, fp in fps.items():
        kw = dict(radius=radius, fused=True, want=('err',), target_motion=motions)
        if name != 'ANALYTICAL':
            kw['guess'] = 'device'
        for label, more in ((name + ', still target', dict(kw, target_motion=None)), (name + ', moving target', kw)):
            out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, **more)
            torch.cuda.synchronize()
            done = (out['status'] == 0).cpu().numpy()
            med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
            err = out['err'].cpu().numpy()
            norms = [np.median(np.linalg.norm(err[k][done], axis=1)) if done.any() else np.nan for k in at]
            lines.append(f'{label:28s}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>8d}{norms[0]:20.3f}{norms[1]:20.3f}')
    return lines


LATENCIES = (0, 1, 2, 3, 4)                                          # control periods


def latency_table(uvs, method='GMCKF', trials=64, sigma=0.3, radius=None, seed=0, latencies=LATENCIES):
    """The latency table as a list of lines: len(latencies) x trials in ONE launch per method (engine.camera_closed_loop(latency=)).  No
    finding is drawn here: the table is what the experiment prints."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = tuple(dict.fromkeys((method, 'KF', 'ANALYTICAL')))
    fps = {name: uvs.engine.make_params(8, 6, name, 10.0, False, 0.05, 15.0, 0.2, desired, True) for name in methods}
    K = fps[method].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    n = len(latencies)
    q0_d = torch.as_tensor(np.tile(q0, (n, 1)), device='cuda')       # the same starts and the same noise at every latency
    noise_d = torch.as_tensor(np.tile(noise, (1, n, 1)), device='cuda')
    latency = np.repeat(np.array(latencies, np.int64), trials)
    lines = [f'{n} camera latencies x {trials} trials of {K} steps in one launch per method, white noise {sigma} px; median over the trials that '
             f'ran to the end',
             f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"FAIL":>8s}{"|err| at step " + str(K - 1):>20s}']
    for name, fp in fps.items():
        kw = dict(radius=radius, fused=True, want=('err',), latency=latency)
        if name != 'ANALYTICAL':
            kw['guess'] = 'device'
        out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, **kw)
        torch.cuda.synchronize()
        status, stats, last = out['status'].cpu().numpy(), out['stats'].cpu().numpy(), out['err'][K - 1].cpu().numpy()
        for c, d in enumerate(latencies):
            rows = slice(c * trials, (c + 1) * trials)
            done = status[rows] == 0
            med = np.median(stats[rows][done], axis=0) if done.any() else np.full(3, np.nan)
            norm = np.median(np.linalg.norm(last[rows][done], axis=1)) if done.any() else np.nan
            lines.append(f'{name + ", latency " + str(d):28s}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~done).sum()):>8d}{norm:20.3f}')
    return lines


ASSUMED = (0, 1, 2, 3, 4)                                            # control periods the controller is told


def told_table(uvs, method='GMCKF', trials=64, sigma=0.3, radius=None, seed=0, latencies=LATENCIES, assumed=ASSUMED):
    """The true-latency x assumed-latency grid as a list of lines: len(latencies) x len(assumed) x trials in ONE launch per method
    (engine.camera_closed_loop(latency=, assumed_latency=)), over the same starts and noise in every cell; a = 0 is the controller that is
    not told.  Per (d, a) cell the median ISE over the trials that ran to the end and, after the slash, the trials that did not with their
    median k_done.  No finding is drawn here: the table is what the experiment prints."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = tuple(dict.fromkeys((method, 'KF', 'ANALYTICAL')))
    fps = {name: uvs.engine.make_params(8, 6, name, 10.0, False, 0.05, 15.0, 0.2, desired, True) for name in methods}
    K = fps[method].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    cells = [(d, a) for d in latencies for a in assumed]
    n = len(cells)
    q0_d = torch.as_tensor(np.tile(q0, (n, 1)), device='cuda')       # the same starts and the same noise in every cell
    noise_d = torch.as_tensor(np.tile(noise, (1, n, 1)), device='cuda')
    latency = np.repeat(np.array([d for d, _ in cells], np.int64), trials)
    told = np.repeat(np.array([a for _, a in cells], np.int64), trials)
    lines = [f'{len(latencies)} camera latencies x {len(assumed)} assumed latencies x {trials} trials of {K} steps in one launch per method, '
             f'white noise {sigma} px; per cell: median ISE over the trials that ran to the end / FAILs (their median k_done)']
    for name, fp in fps.items():
        kw = dict(radius=radius, fused=True, want=('err',), latency=latency, assumed_latency=told)
        if name != 'ANALYTICAL':
            kw['guess'] = 'device'
        out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, **kw)
        torch.cuda.synchronize()
        status, stats, k_done = out['status'].cpu().numpy(), out['stats'].cpu().numpy(), out['k_done'].cpu().numpy()
        lines.append(f'{name + ": latency | told":26s}' + ''.join(f'{"a = " + str(a):>22s}' for a in assumed))
        for i, d in enumerate(latencies):
            row = f'{"d = " + str(d):26s}'
            for j in range(len(assumed)):
                c = i * len(assumed) + j
                rows = slice(c * trials, (c + 1) * trials)
                done = status[rows] == 0
                ise = np.median(stats[rows][done, 0]) if done.any() else np.nan
                fails = f'{int((~done).sum())}' + (f' ({int(np.median(k_done[rows][~done]))})' if (~done).any() else '')
                row += f'{ise:14.3f} /{fails:>6s}'
            lines.append(row)
    return lines


HORIZONS = (0, 1, 2, 3, 4)                                           # control periods the law predicts over


def predicted_table(uvs, method='GMCKF', trials=64, sigma=0.3, radius=None, seed=0, latencies=LATENCIES, horizons=HORIZONS):
    """The true-latency x prediction-horizon grid as a list of lines: len(latencies) x len(horizons) x trials in ONE launch per method
    (engine.camera_closed_loop(latency=, assumed_latency=, predict=)), over the same starts and noise in every cell; every controller is
    told the true latency (a = d), p = 0 is the controller that does not predict.  Per (d, p) cell: the trials that FAILed / the median
    ISE as returned, which is on the predicted error and so not comparable across p / the median "true" ISE, recomputed from the q log
    with engine.camera_features at the logged joints (no noise, no latency) against the target by the same sums -- both medians over the
    trials that ran to the end.  No finding is drawn here: the table is what the experiment prints."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = tuple(dict.fromkeys((method, 'KF', 'ANALYTICAL')))
    fps = {name: uvs.engine.make_params(8, 6, name, 10.0, False, 0.05, 15.0, 0.2, desired, True) for name in methods}
    K = fps[method].steps
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    noise = rng.standard_normal((K, trials, 8)) * sigma
    cells = [(d, p) for d in latencies for p in horizons]
    n = len(cells)
    q0_d = torch.as_tensor(np.tile(q0, (n, 1)), device='cuda')       # the same starts and the same noise in every cell
    noise_d = torch.as_tensor(np.tile(noise, (1, n, 1)), device='cuda')
    latency = np.repeat(np.array([d for d, _ in cells], np.int64), trials)
    ahead = np.repeat(np.array([p for _, p in cells], np.int64), trials)
    target = torch.as_tensor(desired, device='cuda')
    lines = [f'{len(latencies)} camera latencies x {len(horizons)} prediction horizons x {trials} trials of {K} steps in one launch per method, '
             f'white noise {sigma} px, every controller told its latency (a = d); per cell: FAILs / median ISE as returned (on the predicted '
             f'error) / median true ISE (from the q log), over the trials that ran to the end']
    for name, fp in fps.items():
        kw = dict(radius=radius, fused=True, want=('err', 'q'), latency=latency, assumed_latency=latency, predict=ahead)
        if name != 'ANALYTICAL':
            kw['guess'] = 'device'
        out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, **kw)
        sums = torch.zeros((n * trials, 8), dtype=torch.float64, device='cuda')
        for k in range(K):                                           # the features the camera would show at the logged joints, without noise
            err = uvs.engine.camera_features(plant, out['q'][k], radius=radius) - target
            sums += err * err
        true_ise = sums.norm(dim=1).cpu().numpy()                    # the norm over the features of the per-feature sums, as the stats are
        torch.cuda.synchronize()
        status, stats = out['status'].cpu().numpy(), out['stats'].cpu().numpy()
        lines.append(f'{name + ": latency | horizon":28s}' + ''.join(f'{"p = " + str(p):>30s}' for p in horizons))
        for i, d in enumerate(latencies):
            row = f'{"d = " + str(d):28s}'
            for j in range(len(horizons)):
                c = i * len(horizons) + j
                rows = slice(c * trials, (c + 1) * trials)
                done = status[rows] == 0
                ise = np.median(stats[rows][done, 0]) if done.any() else np.nan
                true = np.median(true_ise[rows][done]) if done.any() else np.nan
                row += f'{int((~done).sum()):4d} /{ise:11.1f} /{true:11.1f}'
            lines.append(row)
    return lines


SCORE_STEPS = (0, 1, 5, 20, 100)                                     # and K - 1
SCORE_LATENCY = 2                                                    # --score --latency: control periods, told to the controller


def score_table(uvs, trials=64, sigma=0.3, radius=None, seed=0, latency=False, moving=False, n_scenes=0):
    """The Jacobian-estimate table as a list of lines: the four estimators from the reference's guess and from the correctly scaled start
    x0 = t_s * camera_jacobian(q_start), on the same starts and noise, one launch each, X_k logged and scored on the device.  No finding is
    drawn here: the table is what the experiment prints."""
    import torch
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    plant = uvs.SyntheticPlant.ur10(desired)
    methods = ('KF', 'MCKF', 'IMCCKF', 'GMCKF')
    fps = {method: uvs.engine.make_params(8, 6, method, 10.0, False, 0.05, 15.0, 0.2, desired, True) for method in methods}
    K, dt = fps['GMCKF'].steps, fps['GMCKF'].dt
    rng = np.random.default_rng(seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (trials, 1))
    q0[:, :2] += rng.uniform(-0.1, 0.0, (trials, 2))
    q0_d = torch.as_tensor(q0, device='cuda')
    noise_d = torch.as_tensor(rng.standard_normal((K, trials, 8)) * sigma, device='cuda')
    truth, what = {}, []                                             # the scene arguments the loop and the score share
    if n_scenes:
        truth.update(cameras=uvs.engine.camera_scenes(scene_plants(uvs, plant, n_scenes, seed), radius),
                     camera_index=np.arange(trials, dtype=np.int32) % n_scenes)
        what.append(f'{n_scenes} true scenes')
    if moving:
        velocity = np.repeat(moving_velocities(1, 4, seed), trials, axis=0)
        truth.update(target_motion=uvs.engine.target_motions(velocity, MOVING_WINDOW, 4, trials))
        what.append(f'the target moves during steps {MOVING_WINDOW[0]} .. {MOVING_WINDOW[1] - 1}')
    more = dict(latency=SCORE_LATENCY, assumed_latency=SCORE_LATENCY) if latency else {}
    if latency:
        what.append(f'camera latency {SCORE_LATENCY}, told')
    steps = tuple(k for k in SCORE_STEPS if k < K - 1) + (K - 1,)
    scaled = dt * uvs.engine.camera_jacobian(plant, q0_d, radius=radius, **truth)
    starts = (("the reference's guess", dict(guess='device', **(dict(believed=plant) if n_scenes else {}))),
              ('x0 = t_s J(q_start)', dict(x0=scaled.reshape(trials, -1))))
    lines = [f'{trials} trials of {K} steps, white noise {sigma} px' + ''.join(', ' + w for w in what) + '; X_k scored against t_s times the true image '
             f'Jacobian at q_k; median over the trials whose row is due',
             f'{"":36s}{"ISE":>10s}{"FAIL":>6s}  ' + ''.join(f'{"step " + str(k):>31s}' for k in steps),
             f'{"":36s}{"":16s}  ' + ''.join(f'{"scale  cos  rel_err  ratio":>31s}' for _ in steps)]
    for method in methods:
        for label, start in starts:
            out = uvs.engine.camera_closed_loop(fps[method], plant, q0_d, noise_d, radius=radius, fused=True, want=uvs.engine.ESTIMATOR_CAMERA_LOGS,
                                                **start, **truth, **more)
            score = uvs.engine.camera_jacobian_score(plant=plant, dt=dt, radius=radius, **{k: out[k] for k in ('x', 'q', 'dq', 'k_done')}, **truth)
            torch.cuda.synchronize()
            done = (out['status'] == 0).cpu().numpy()
            ise = np.median(out['stats'].cpu().numpy()[done, 0]) if done.any() else np.nan
            cells = []
            for k in steps:
                med = [float(np.nanmedian(score[key][k].cpu().numpy())) for key in ('scale', 'cosine', 'rel_err', 'step_ratio')]
                cells.append(f'{med[0]:10.3f}{med[1]:7.3f}{med[2]:8.3f}{med[3]:6.2f}')
            lines.append(f'{method + ", " + label:36s}{ise:10.3f}{int((~done).sum()):>6d}  ' + ''.join(cells))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='GMCKF', choices=('KF', 'MCKF', 'IMCCKF', 'GMCKF'))
    ap.add_argument('--trials', type=int, default=64)
    ap.add_argument('--sigma', type=float, default=0.3, help='standard deviation of the white measurement noise, pixels')
    ap.add_argument('--radius', type=float, default=None, help='physical disc radius in metres (default plant.DISC_RADIUS: about 8 px at the goal)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--fused', action='store_true', help='the pixel loop as one launch, initial guess on the device, no log returned')
    ap.add_argument('--baseline', action='store_true', help='pair the estimator with the calibrated law (ANALYTICAL) through the same pixels')
    ap.add_argument('--miscalibration', action='store_true', help='a ladder of wrong models x trials in one launch per side, and nothing else')
    ap.add_argument('--grid', action='store_true', help='kernel_bw x gain over the same starts and noise in one launch, and nothing else')
    ap.add_argument('--occlusion', action='store_true', help='a bar crosses the frame while the servo runs: GMCKF, KF and the calibrated law, and nothing else')
    ap.add_argument('--hold', type=int, default=0, metavar='N',
                    help='with --occlusion: a bar wider than a disc, and a lost disc keeps its last detection for up to N steps (0: the narrow bar)')
    ap.add_argument('--distractor', action='store_true',
                    help='a still rectangle of the green disc\'s colour near its goal: the estimators and the calibrated law, and nothing else '
                         '(with --occlusion --hold N: in front of the wide bar, lost discs held)')
    ap.add_argument('--scenes', type=int, default=0, metavar='N',
                    help='N seeded true scenes x the trials in one launch per method: the estimators and the calibrated law, and nothing else')
    ap.add_argument('--moving', action='store_true',
                    help='the target moves for a window of steps after convergence: the estimator, KF and the calibrated law, and nothing else')
    ap.add_argument('--latency', action='store_true',
                    help='camera latencies 0 .. 4 x the trials in one launch per method: the estimator, KF and the calibrated law, and nothing else')
    ap.add_argument('--told', action='store_true',
                    help='with --latency: the controller is told a latency -- latencies 0 .. 4 x assumed latencies 0 .. 4 x the trials in one '
                         'launch per method, told and untold on the same starts and noise')
    ap.add_argument('--score', action='store_true',
                    help="the four estimators' X_k scored against the true image Jacobian, from the reference's guess and from the correctly scaled "
                         'start; combines with --latency, --moving and --scenes N, and nothing else')
    ap.add_argument('--predict', action='store_true',
                    help='with --latency: the law predicts the features over the latency -- latencies 0 .. 4 x prediction horizons 0 .. 4 x the '
                         'trials in one launch per method, every controller told its latency; FAILs, the ISE as returned and a true ISE from the q log')
    args = ap.parse_args()
    import torch
    import uvs_amd as uvs
    if args.hold and not args.occlusion:
        ap.error('--hold goes with --occlusion')
    if args.told and not args.latency:
        ap.error('--told goes with --latency')
    if args.predict and (not args.latency or args.told):
        ap.error('--predict goes with --latency, and not with --told')
    if args.score:
        if args.told or args.predict:
            ap.error('--score combines with --latency, --moving and --scenes N')
        print('\n'.join(score_table(uvs, args.trials, args.sigma, args.radius, args.seed, args.latency, args.moving, args.scenes)))
        return
    if args.latency and args.predict:
        print('\n'.join(predicted_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.latency and args.told:
        print('\n'.join(told_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.latency:
        print('\n'.join(latency_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.moving:
        print('\n'.join(moving_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.scenes:
        print('\n'.join(scenes_table(uvs, args.scenes, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.distractor:
        if args.occlusion and not args.hold:
            ap.error('--distractor --occlusion needs --hold N: the wide bar empties every mask')
        print('\n'.join(distractor_table(uvs, args.trials, args.sigma, args.radius, args.seed, bar=WIDE_BAR if args.occlusion else None,
                                          hold=args.hold)))
        return
    if args.occlusion and args.hold:
        print('\n'.join(hold_table(uvs, args.hold, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.occlusion:
        print('\n'.join(occlusion_table(uvs, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.grid:
        print('\n'.join(grid_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    if args.miscalibration:
        print('\n'.join(miscalibration_table(uvs, args.method, args.trials, args.sigma, args.radius, args.seed)))
        return
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])                   # config.json:9
    plant = uvs.SyntheticPlant.ur10(desired)
    fp = uvs.engine.make_params(8, 6, args.method, 10.0, False, 0.05, 15.0, 0.2, desired, True)
    T, K = args.trials, fp.steps
    rng = np.random.default_rng(args.seed)
    q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))          # config.json:8, jittered like the reference's driver
    q0[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    noise = rng.standard_normal((K, T, 8)) * args.sigma
    q0_d, noise_d = torch.as_tensor(q0, device='cuda'), torch.as_tensor(noise, device='cuda')
    ideal = uvs.engine.closed_loop(fp, plant.to_struct(), q0_d, noise_d.permute(0, 2, 1).contiguous(), want=('err',))
    if args.fused:
        pixels = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, radius=args.radius, fused=True, guess='device', want=())
    else:
        pixels = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise_d, radius=args.radius)
    torch.cuda.synchronize()
    print(f'{args.method}, {T} trials of {K} steps, white noise {args.sigma} px; median over the trials that ran to the end')
    print(f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"SUCCESS":>10s}')
    for name, out in (('ideal projections', ideal), ('through 256 x 256 pixels', pixels)):
        done = (out['status'] == 0).cpu().numpy()
        med = np.median(out['stats'].cpu().numpy()[done], axis=0) if done.any() else np.full(3, np.nan)
        print(f'{name:28s}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int(done.sum()):>7d}/{T}')
    print(f'smallest colour mask over all steps of all trials: {int(pixels["pixels"].min())} pixels')
    if args.baseline:
        fp_cal = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, desired)
        calibrated = uvs.engine.camera_closed_loop(fp_cal, plant, q0_d, noise_d, radius=args.radius, fused=args.fused, want=())
        torch.cuda.synchronize()
        ok_est, ok_cal = (pixels['status'] == 0).cpu().numpy(), (calibrated['status'] == 0).cpu().numpy()
        both = ok_est & ok_cal
        print(f'through pixels, paired: median over the {int(both.sum())} trials both ran to the end')
        print(f'{"":28s}{"ISE":>12s}{"IAE":>12s}{"ITAE":>12s}{"FAIL":>10s}')
        for name, out, ok in ((args.method, pixels, ok_est), ('ANALYTICAL (calibrated)', calibrated, ok_cal)):
            med = np.median(out['stats'].cpu().numpy()[both], axis=0) if both.any() else np.full(3, np.nan)
            print(f'{name:28s}{med[0]:12.3f}{med[1]:12.3f}{med[2]:12.3f}{int((~ok).sum()):>7d}/{T}')
        if both.any():
            ratio = np.median(pixels['stats'].cpu().numpy()[both] / calibrated['stats'].cpu().numpy()[both], axis=0)
            print(f'{"median of the paired ratios":28s}{ratio[0]:12.4f}{ratio[1]:12.4f}{ratio[2]:12.4f}')


if __name__ == '__main__':
    main()
