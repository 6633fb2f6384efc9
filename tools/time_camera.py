#!/usr/bin/env python3
"""Time the synthetic camera on the device, in one run on one GPU box:
  (a) engine.render_discs followed by engine.detect_circles, frames resident in HBM, at T = 1, 64 and 4 096;
  (b) engine.disc_features on the same discs: the frame-free detector, which moves no frame;
  (c) engine.camera_features: projection and frame-free detection in one launch, from the joints;
  (d) engine.camera_closed_loop at T = 1 024, K = 299 (two launches per step), wall clock, and next to it engine.closed_loop on the same
      trials as context -- ideal features, plant in the kernel: a different computation, not a gate.  The loop is timed twice: as called
      (the analytic initial guess of every trial is host work inside the call) and with x0 handed in (the loop alone);
  (e) camera_closed_loop(fused=True) -- the same loop as one launch -- with x0 handed in, against (d) "the loop alone", also at T = 64 and 4 096;
  (f) camera_closed_loop(fused=True, guess='device') as called, against (d) as called;
  (g) (e) with want=(): no log is allocated or written.
      (e)-(g) and their (d) counterparts are host-clock times around synchronised calls, taken in alternating blocks in the same process.
(a)-(c) are HIP-event times around the launches, taken in alternating blocks so that all three see the same machine state; every figure is
the median of 250 iterations after a warm-up, with the 10th and 90th percentile.  The acceptance condition is (b) below (a) at every T.
Writes profiles/camera_device.txt (or the path given).  usage: tools/time_camera.py [out.txt]
With --analytical only the calibrated baseline's pixel loop is timed, into profiles/camera_analytical.txt (or the path given):
  (h) camera_closed_loop with fp.method == ANALYTICAL, fused=False: K x (camera features, analytical step);
  (i) the same with fused=True: one launch;
  (e) the fused GMCKF loop with x0 handed in, as context;
      at T = 1 024, K = 299, white noise 0.3 px, host clock around synchronised calls in alternating blocks of one process; (h) and (i) at
      T = 64 as well.  The acceptance condition is (i) below (h) at both sizes; (i) against (e) is reported, not gated.  Also the paired
      ISE / IAE / ITAE medians of ANALYTICAL and GMCKF through pixels on the same starts and noise.
usage: tools/time_camera.py --analytical [out.txt]
With --believed only the calibrated baseline on a per-trial believed model is timed, into profiles/camera_believed.txt (or the path given):
  (j) camera_closed_loop with fp.method == ANALYTICAL and believed models mixed over the trials through an index, fused=False:
      K x (camera features on the true camera, believed step);
  (k) the same with fused=True: one launch;
  (i) the calibrated one launch of --analytical, in the same run;
      method and sizes as --analytical.  The acceptance condition is (k) below (j) at both sizes; (k) against (i) -- what reading the model
      from LDS per trial costs -- is reported, not gated.  Then the robustness table of examples/camera_loop.py --miscalibration.
usage: tools/time_camera.py --believed [out.txt]
With --grid only the per-trial pixel loop is timed, into profiles/camera_grid.txt (or the path given): GMCKF, K = 299, white noise 0.3 px,
64 cells (8 bandwidths x 8 gains) x 16 trials = 1 024 output trials over the same 16 starts and noise rows;
  (j) the grid as 64 uniform fused launches of 16 trials, one per cell, synchronised once at the end;
  (k) the grid as ONE launch: camera_closed_loop(fused=True, trial_params=...) with 'source';
  (e) the uniform fused launch of 1 024 trials, x0 handed in -- with this library and, given --parent-lib=PATH (a libuvs_vision.so built
      from the parent commit, loaded next to this one), with that one in turn;
  (l) (e)'s trials through the per-trial kernel, every trial with fp's own kernel_bw and gain: what the kernel flavour costs, apart from
      what the grid's other bandwidths and gains make the estimator do;
      host clock around synchronised calls, alternating blocks of one process.  The acceptance condition is (k) below (j); (e) new against
      (e) parent and (k) / (e) are reported next to the parent's own spread.  Every cell of (k) is checked against its launch of (j), bit
      for bit, before anything is timed.  Then the table of examples/camera_loop.py --grid.
usage: tools/time_camera.py --grid [--parent-lib=PATH] [out.txt]
With --occluded only the occluded pixel loop is timed, into profiles/camera_occluded.txt (or the path given): GMCKF, 1 024 trials x 299
steps, white noise 0.3 px, x0 handed in, medians of 20 with p10-p90;
  (e) the uniform fused launch -- with this library and, given --parent-lib=PATH, with the parent's in turn;
  (m) (e)'s trials through camera_occluded_kernel with n_occ = 0: what the kernel flavour costs;
  (n) the sweeping bar of examples/camera_loop.py --occlusion on every trial, one launch;
  (o) (n) stepwise: K x (occluded camera features, estimator step).
      The acceptance condition is (n) below (o); (e) new against (e) parent is reported next to the parent's own spread; (m) / (e) and
      (n) / (m) are reported, not gated.  (m) is checked against (e) and (n) against (o), bit for bit, before anything is timed.  Then the
      table of examples/camera_loop.py --occlusion.
usage: tools/time_camera.py --occluded [--parent-lib=PATH] [out.txt]
With --held only the pixel loop that holds a lost disc's last detection is timed, into profiles/camera_hold.txt (or the path given): GMCKF,
1 024 trials x 299 steps, white noise 0.3 px, x0 handed in, medians of 20 with p10-p90;
  (n) the 12 px bar of --occluded through camera_occluded_kernel -- with this library and, given --parent-lib=PATH, with the parent's in
      turn: the existing kernel was not to move (the gate is its resource figures; the time is the evidence);
  (p) (n)'s trials through camera_held_kernel with hold = 0: what the kernel flavour costs;
  (q) the wide bar of examples/camera_loop.py --occlusion --hold on every trial with hold = 30, one launch;
  (r) (q) stepwise: K x (occluded camera features, hold, estimator step), three launches a step.
      The acceptance condition is (q) below (r); (n) new against (n) parent is reported next to the parent's own spread; (p) / (n) and
      (q) / (n) are reported, not gated.  (n) is checked against the parent's (n), (p) against (n) and (q) against (r), bit for bit,
      before anything is timed.  Then the table of examples/camera_loop.py --occlusion --hold 30.
usage: tools/time_camera.py --held [--parent-lib=PATH] [out.txt]
With --painted only the pixel loop behind painted occluders (distractors) is timed, into profiles/camera_painted.txt (or the path given):
GMCKF, 1 024 trials x 299 steps, white noise 0.3 px, x0 handed in, medians of 20 with p10-p90;
  (e) the uniform fused launch, (n) the 12 px bar of --occluded through camera_occluded_kernel and (q) the wide bar of --held with
      hold = 30 through camera_held_kernel -- each with this library and, given --parent-lib=PATH, with the parent's TWICE (two entries of
      the same alternating blocks): the existing kernels were not to move.  A figure passes when it is no slower than the slower of the two
      parent runs by more than the two parent runs differ; the outputs must be bit-identical;
  (s) (q)'s trials through camera_painted_kernel with paint = NULL: what the kernel flavour costs;
  (t) (q) with a still distractor of green's colour in front of the bar on every trial (examples/camera_loop.py --distractor --occlusion
      --hold 30), one launch;
  (u) (t) stepwise: K x (painted camera features, hold, estimator step), three launches a step.
      (s), (t), (u) are reported, not gated.  (s) is checked against (q) and (t) against (u), bit for bit, before anything is timed.  Then
      the tables of examples/camera_loop.py --distractor and --distractor --occlusion --hold 30.
usage: tools/time_camera.py --painted [--parent-lib=PATH] [out.txt]
With --scenes only the scene-per-trial pixel loops are timed, into profiles/camera_scenes_timing.txt (or the path given): GMCKF, 1 024
trials x 299 steps, white noise 0.3 px, x0 handed in, medians of 20 with p10-p90;
  (e), (n), (q) as under --painted, gated against two runs of the parent's library by the same rule: the existing kernels were not to move;
  (v) (e)'s trials through camera_scene_kernel with n_cams = 1: what the kernel flavour costs;
  (w) 16 scenes (examples/camera_loop.py --scenes) x 64 trials in ONE launch, (x) the same as 16 uniform launches of 64 trials, one per
      scene, (z) (w) stepwise: K x (scene features, estimator step);
  (k) the believed baseline loop on the nominal model, (y) its trials through scene_baseline_loop_kernel with n_cams = 1, (y16) the
      baseline over the 16 scenes in one launch.
      (v) .. (y16) are reported, not gated.  (v) is checked against (e), (w) against (x) and (z), (y) against (k), bit for bit, before
      anything is timed.  Then the table of examples/camera_loop.py --scenes 8.
usage: tools/time_camera.py --scenes [--parent-lib=PATH] [out.txt]
With --moving only the moving-target pixel loops are timed, into profiles/camera_moving_timing.txt (or the path given): GMCKF, 1 024 trials
x 299 steps, white noise 0.3 px, x0 handed in, medians of 20 with p10-p90;
  (e), (n), (q), (v), (w) as under --scenes, gated against two runs of the parent's library by the same rule: the existing kernels were
      not to move;
  (mv) (v)'s trials through moving_target_kernel with motion = NULL: what the kernel flavour costs;
  (mw) 16 motions (examples/camera_loop.py --moving) x 64 trials in ONE launch, (mx) the same as 16 launches of 64 trials, one per motion,
      (mz) (mw) stepwise: K x (moving features, estimator step);
  (y) the scenes baseline loop on the nominal camera, (my) its trials through moving_baseline_kernel with motion = NULL, (my16) the baseline
      over the 16 motions in one launch.
      (mv) .. (my16) are reported, not gated.  (mv) is checked against (v), (mw) against (mx) and (mz), (my) against (y), bit for bit,
      before anything is timed.  Then the table of examples/camera_loop.py --moving.
usage: tools/time_camera.py --moving [--parent-lib=PATH] [out.txt]

With --delayed only the camera-latency pixel loops are timed, into profiles/camera_latency_timing.txt (or the path given): GMCKF, 1 024 trials
x 299 steps, white noise 0.3 px --
  (e), (n), (q), (v), (w), (mv), (mw) of the sections above, each against the parent's library when --parent-lib names it (gated);
  (dv) (mv)'s trials through delayed_frames_kernel with latency = NULL: what the kernel flavour costs;
  (dw) 5 latencies (examples/camera_loop.py --latency) x 64 trials in ONE launch, (dx) the same as 5 launches of 64 trials, one per latency,
      (dz) (dw) stepwise: K x (features without noise, delay, estimator step);
  (my) the moving baseline loop with motion = NULL, (dy) its trials through delayed_baseline_kernel with latency = NULL, (dy5) the baseline
      over the 5 latencies x 64 trials in one launch
      -- (dv) is asserted to have the bits of (mv), (dw) those of (dx) and (dz) trial for trial, (dy) those of (my), before anything is timed.
      Then the table of examples/camera_loop.py --latency.
usage: tools/time_camera.py --delayed [--parent-lib=PATH] [out.txt]

With --aligned only the assumed-latency pixel loops are timed, into profiles/camera_aligned_timing.txt (or the path given): GMCKF, 1 024 trials
x 299 steps, white noise 0.3 px --
  (dv) the delayed loop with latency = NULL, (dy) the delayed baseline loop with latency = NULL, each also through the parent's library,
      twice, when --parent-lib names it;
  (av) (dv)'s trials through aligned_frames_kernel with latency = assumed = NULL, (ay) (dy)'s through aligned_baseline_kernel: against the
      parent's (dv) and (dy) by the rule of DESIGN.md 4.20 -- no slower than the slower parent run by more than the parent runs differ;
  (aw) 5 latencies x 5 assumed latencies (examples/camera_loop.py --latency --told) x 64 trials in ONE launch, (ax) the same as 25 launches
      of 64 trials, one per cell, (az) (aw) stepwise: K x (features without noise, delay, gather of the regressor, estimator step);
  (ay25) the baseline over the 25 cells x 64 trials in one launch
      -- (av) is asserted to have the bits of (dv), (ay) those of (dy), (aw) those of (ax) and (az) trial for trial, before anything is timed.
      Then the table of examples/camera_loop.py --latency --told.
usage: tools/time_camera.py --aligned [--parent-lib=PATH] [out.txt]

With --predicted only the feature-prediction pixel loops are timed, into profiles/camera_predicted_timing.txt (or the path given): GMCKF,
1 024 trials x 299 steps, white noise 0.3 px --
  (av) the aligned loop with latency = assumed = NULL, (ay) the aligned baseline loop likewise, each also through the parent's library,
      twice, when --parent-lib names it;
  (pv) (av)'s trials through predicted_frames_kernel with latency = assumed = predict = NULL, (py) (ay)'s through predicted_baseline_kernel:
      the ratio against the parent's (av) and (ay) is printed next to the parent's own two-run spread; nothing is gated;
  (a4) the aligned loop at d = a = 4, (p4) the predicted loop at d = a = p = 4, (ay4) and (py4) the baseline's likewise;
  (pw) 5 latencies x 5 horizons (examples/camera_loop.py --latency --predict) x 64 trials in ONE launch, (px) the same as 25 launches of
      64 trials, one per cell; (py25) the baseline over the 25 cells in one launch, (pz25) that stepwise
      -- (pv) is asserted to have the bits of (av), (py) those of (ay), (pw) those of (px) trial for trial, (py25) those of (pz25), before
      anything is timed.  Then the table of examples/camera_loop.py --latency --predict.
usage: tools/time_camera.py --predicted [--parent-lib=PATH] [out.txt]

--score: the X log, the true image Jacobian and the score, into profiles/camera_score.txt
  (pv) the predicted loop with every optional operand NULL, 1 024 trials x 299 steps, through the C ABI -- with this library and, given
      --parent-lib=PATH, with the parent's, twice;
  (lv) the same trials through logged_frames_kernel with x_log = NULL: the price of the text; (lx) the same with the log: the price of
      117 MB of stores from wavefront 0 -- (lv) is asserted to have the bits of (pv), (lx) those too in every other output, before anything
      is timed; each ratio is printed next to the parent's own two-run spread; nothing is gated;
  (cj) engine.camera_jacobian over the q log of (lx), (cs) engine.camera_jacobian_score over its x, q and dq logs: HIP events around the
      calls, alternating blocks, with the bytes each moves.  Then the table of examples/camera_loop.py --score.
usage: tools/time_camera.py --score [--parent-lib=PATH] [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uvs_amd as uvs  # noqa: E402
import torch  # noqa: E402

ANALYTICAL, BELIEVED, GRID = '--analytical' in sys.argv[1:], '--believed' in sys.argv[1:], '--grid' in sys.argv[1:]
OCCLUDED, HELD, PAINTED = '--occluded' in sys.argv[1:], '--held' in sys.argv[1:], '--painted' in sys.argv[1:]
SCENES = '--scenes' in sys.argv[1:]
MOVING = '--moving' in sys.argv[1:]
DELAYED = '--delayed' in sys.argv[1:]
ALIGNED = '--aligned' in sys.argv[1:]
PREDICTED = '--predicted' in sys.argv[1:]
SCORE = '--score' in sys.argv[1:]
PARENT_LIB = next((a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('--parent-lib=')), None)
ARGV = [a for a in sys.argv[1:] if a not in ('--analytical', '--believed', '--grid', '--occluded', '--held', '--painted', '--scenes', '--moving', '--delayed', '--aligned', '--predicted', '--score') and not a.startswith('--parent-lib=')]
OUT = ARGV[0] if ARGV else os.path.join(ROOT, 'profiles', 'camera_score.txt' if SCORE else 'camera_predicted_timing.txt' if PREDICTED else 'camera_aligned_timing.txt' if ALIGNED else 'camera_latency_timing.txt' if DELAYED else 'camera_moving_timing.txt' if MOVING else 'camera_scenes_timing.txt' if SCENES else 'camera_painted.txt' if PAINTED else 'camera_hold.txt' if HELD else 'camera_occluded.txt' if OCCLUDED else 'camera_grid.txt' if GRID else 'camera_believed.txt' if BELIEVED else
                                        'camera_analytical.txt' if ANALYTICAL else 'camera_device.txt')
ROUNDS, BLOCK, WARM = 5, 50, 20                      # 250 timed iterations per figure, in 5 alternating blocks
Q_GOAL = np.array([0.0, -np.pi / 8, np.pi / 2 + np.pi / 8, 0.0, -np.pi / 2, 0.0])
DESIRED = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
lines = []


def say(text=''):
    print(text, flush=True)
    lines.append(text)


def stats(us):
    us = np.asarray(us)
    return float(np.median(us)), float(np.percentile(us, 10)), float(np.percentile(us, 90))


def fmt(us):
    med, lo, hi = stats(us)
    return f'{med:10.1f} us   (p10 {lo:.1f}, p90 {hi:.1f}, n = {len(us)})'


def alternate(fns, rounds=ROUNDS, block=BLOCK, warm=WARM):
    """HIP-event time of every call of every function, in alternating blocks."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            for _ in range(block):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                events[name].append((e0, e1))
        torch.cuda.synchronize()
    return {name: [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev] for name, ev in events.items()}


def wall(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def wall_alternate(fns, rounds=5, block=4):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name] += wall(fn, block)[:]
    return ms


def fmt_ms(ms):
    med, lo, hi = stats(ms)
    return f'median {med:9.2f} ms   (p10 {lo:.2f}, p90 {hi:.2f}, n = {len(ms)})'


def analytical_section():
    """(h), (i), (e): see the module docstring."""
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K = 299
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fp_cal = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K and fp_cal.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --analytical on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# K = {K}, white noise 0.3 px; host clock around synchronised calls, alternating blocks in one process, allocation of the logs included')
    ok = True
    for T, rounds, block in ((1024, 5, 4), (64, 5, 4)):
        q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
        q0[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
        q0_d = torch.as_tensor(q0, device='cuda')
        noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
        x0_d = uvs.engine.camera_guess(plant, q0_d, uvs.engine.camera_features(plant, q0_d))
        stepwise, fused = loop(fp_cal, plant, q0_d, noise), loop(fp_cal, plant, q0_d, noise, fused=True)
        gmckf = loop(fp, plant, q0_d, noise, x0=x0_d, fused=True)
        torch.cuda.synchronize()
        same = all(torch.equal(fused[key].view(torch.int64), stepwise[key].view(torch.int64)) for key in ('err', 'q', 'f', 'dq', 'stats'))
        same = same and all(torch.equal(fused[key], stepwise[key]) for key in ('status', 'k_done', 'pixels'))
        assert same, 'the one launch and the stepwise loop of the calibrated law disagree'
        fns = {'h': lambda: loop(fp_cal, plant, q0_d, noise), 'i': lambda: loop(fp_cal, plant, q0_d, noise, fused=True)}
        if T == 1024:
            fns['e'] = lambda: loop(fp, plant, q0_d, noise, x0=x0_d, fused=True)
        ms = wall_alternate(fns, rounds=rounds, block=block)
        h_med, i_med = float(np.median(ms['h'])), float(np.median(ms['i']))
        ok = ok and i_med < h_med
        say()
        say(f'T = {T}')
        say(f'  (h) ANALYTICAL, stepwise: K x (camera features, analytical step)   {fmt_ms(ms["h"])}   = {h_med / K * 1e3:.1f} us per step')
        say(f'  (i) ANALYTICAL, fused=True: one launch                             {fmt_ms(ms["i"])}   = {i_med / K * 1e3:.1f} us per step')
        say(f'  (i) / (h) = {i_med / h_med:.4f}: (i) is {"BELOW" if i_med < h_med else "NOT below"} (h); logs, stats, status, k_done, pixels bit-identical')
        if 'e' in ms:
            e_med = float(np.median(ms['e']))
            say(f'  (e) GMCKF, fused=True, x0 handed in (context)                      {fmt_ms(ms["e"])}   = {e_med / K * 1e3:.1f} us per step')
            say(f'  (i) / (e) = {i_med / e_med:.4f} (reported, not gated)')
        ok_cal, ok_est = (fused['status'] == 0).cpu().numpy(), (gmckf['status'] == 0).cpu().numpy()
        both = ok_cal & ok_est
        med_cal, med_est = (np.median(out['stats'].cpu().numpy()[both], axis=0).round(3).tolist() for out in (fused, gmckf))
        say(f'  through pixels, paired over the {int(both.sum())} of {T} trials both ran to the end (FAIL: ANALYTICAL {int((~ok_cal).sum())}, '
            f'GMCKF {int((~ok_est).sum())}); smallest mask {int(fused["pixels"].min())} px')
        say(f'    median ISE / IAE / ITAE   ANALYTICAL {med_cal}   GMCKF {med_est}')
    say()
    say(f'acceptance: (i) below (h) at both sizes: {"yes" if ok else "NO"}')
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def believed_section():
    """(j), (k), (i): see the module docstring."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K = 299
    fp_cal = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp_cal.steps == K
    loop = uvs.engine.camera_closed_loop
    believed = uvs.engine.believed_models([example.believed_plant(uvs, plant, level) for level in example.LEVELS])
    say(f'# tools/time_camera.py --believed on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# K = {K}, white noise 0.3 px; host clock around synchronised calls, alternating blocks in one process, allocation of the logs included')
    say(f'# believed models: the {len(example.LEVELS)} levels of examples/camera_loop.py --miscalibration, mixed over the trials through a device index')
    ok = True
    for T, rounds, block in ((1024, 5, 4), (64, 5, 4)):
        q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
        q0[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
        q0_d = torch.as_tensor(q0, device='cuda')
        noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
        index = torch.as_tensor((np.arange(T) % believed.shape[0]).astype(np.int32), device='cuda')
        kw = dict(believed=believed, believed_index=index)
        stepwise, fused = loop(fp_cal, plant, q0_d, noise, **kw), loop(fp_cal, plant, q0_d, noise, fused=True, **kw)
        torch.cuda.synchronize()
        k_done = fused['k_done'].cpu().numpy()
        same = all(torch.equal(fused[key], stepwise[key]) for key in ('status', 'k_done', 'pixels')) \
            and torch.equal(fused['stats'].view(torch.int64), stepwise['stats'].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq'):                          # the specified rows: q, f up to and including k_done, dq, err before it
            rows = torch.arange(K, device='cuda')[:, None] < (fused['k_done'][None, :] + (1 if key in ('q', 'f') else 0))
            a, b = (out[key].view(torch.int64)[rows] for out in (fused, stepwise))
            same = same and torch.equal(a, b)
        assert same, 'the one launch and the stepwise loop on the believed models disagree'
        ms = wall_alternate({'j': lambda: loop(fp_cal, plant, q0_d, noise, **kw), 'k': lambda: loop(fp_cal, plant, q0_d, noise, fused=True, **kw),
                             'i': lambda: loop(fp_cal, plant, q0_d, noise, fused=True)}, rounds=rounds, block=block)
        j_med, k_med, i_med = (float(np.median(ms[key])) for key in 'jki')
        ok = ok and k_med < j_med
        say()
        say(f'T = {T}   ({int((k_done == K).sum())} of {T} trials ran to the end on their believed models)')
        say(f'  (j) believed, stepwise: K x (camera features, believed step)   {fmt_ms(ms["j"])}   = {j_med / K * 1e3:.1f} us per step')
        say(f'  (k) believed, fused=True: one launch                           {fmt_ms(ms["k"])}   = {k_med / K * 1e3:.1f} us per step')
        say(f'  (i) calibrated, fused=True: one launch (row (i) of --analytical) {fmt_ms(ms["i"])}   = {i_med / K * 1e3:.1f} us per step')
        say(f'  (k) / (j) = {k_med / j_med:.4f}: (k) is {"BELOW" if k_med < j_med else "NOT below"} (j); specified log rows, stats, status, k_done, pixels '
            'bit-identical')
        say(f'  (k) / (i) = {k_med / i_med:.4f} (reported, not gated: the model per trial from LDS against the model in scalar registers)')
    say()
    say(f'acceptance: (k) below (j) at both sizes: {"yes" if ok else "NO"}')
    say()
    say('# examples/camera_loop.py --miscalibration (its defaults)')
    for line in example.miscalibration_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def grid_section():
    """(j), (k), (e): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, E = 299, 16
    bandwidths, gains = example.GRID_BANDWIDTHS, example.GRID_GAINS
    cells = [(bw, gain) for bw in bandwidths for gain in gains]
    T = len(cells) * E
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    assert fp.steps == K and T == 1024
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --grid on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, K = {K}, white noise 0.3 px; {len(cells)} cells (kernel_bw {list(bandwidths)} x gain {list(gains)}) x {E} trials = {T} output '
        'trials over the same starts and noise')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included')

    def starts(n):
        q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (n, 1))
        q[:, :2] += rng.uniform(-0.1, 0.0, (n, 2))
        q_d = torch.as_tensor(q, device='cuda')
        return q_d, torch.as_tensor(rng.standard_normal((K, n, 8)) * 0.3, device='cuda'), \
            uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))

    q_in, noise_in, x0_in = starts(E)
    q_all, noise_all, x0_all = starts(T)
    tp = {'kernel_bw': torch.as_tensor(np.repeat([c[0] for c in cells], E), device='cuda'),
          'gain': torch.as_tensor(np.repeat([c[1] for c in cells], E), device='cuda'),
          'source': torch.as_tensor((np.arange(T) % E).astype(np.int32), device='cuda')}
    fps = []
    for bw, gain in cells:
        one = type(fp).from_buffer_copy(fp)
        one.kernel_bw, one.gain = bw, gain
        fps.append(one)

    def run_j():
        return [loop(one, plant, q_in, noise_in, x0=x0_in, fused=True) for one in fps]

    def run_k():
        return loop(fp, plant, q_in, noise_in, x0=x0_in, fused=True, trial_params=tp)

    def run_e():
        return loop(fp, plant, q_all, noise_all, x0=x0_all, fused=True)

    tp_same = {'kernel_bw': torch.full((T,), fp.kernel_bw, dtype=torch.float64, device='cuda'),
               'gain': torch.full((T,), fp.gain, dtype=torch.float64, device='cuda'),
               'source': torch.arange(T, dtype=torch.int32, device='cuda')}

    def run_l():
        return loop(fp, plant, q_all, noise_all, x0=x0_all, fused=True, trial_params=tp_same)

    per_cell, one_launch = run_j(), run_k()
    torch.cuda.synchronize()
    for c, want in enumerate(per_cell):
        rows = slice(c * E, (c + 1) * E)
        done = want['k_done']
        same = all(torch.equal(one_launch[key][rows], want[key]) for key in ('status', 'k_done', 'pixels')) \
            and torch.equal(one_launch['stats'][rows].view(torch.int64), want['stats'].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
            same = same and torch.equal(one_launch[key][:, rows].view(torch.int64)[spec], want[key].view(torch.int64)[spec])
        assert same, f'cell {cells[c]} of the one launch and its uniform launch disagree'
    uniform_all, same_all = run_e(), run_l()
    torch.cuda.synchronize()
    assert all(torch.equal(same_all[key].view(torch.int64), uniform_all[key].view(torch.int64)) for key in ('err', 'q', 'f', 'dq', 'kappa', 'stats'))
    fns = {'j': run_j, 'k': run_k, 'e': run_e, 'l': run_l}
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def run_e_parent():
            mine, uvs._vision._lib = uvs._vision._lib, parent
            try:
                return run_e()
            finally:
                uvs._vision._lib = mine

        new, old = run_e(), run_e_parent()
        torch.cuda.synchronize()
        assert all(torch.equal(new[key].view(torch.int64), old[key].view(torch.int64)) for key in ('err', 'q', 'f', 'dq', 'kappa', 'stats'))
        fns['e_parent'] = run_e_parent
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    spread = lambda v: (np.percentile(v, 90) - np.percentile(v, 10)) / np.median(v)   # noqa: E731
    say()
    say(f'  (j) {len(cells)} uniform fused launches of {E} trials, one per cell   {fmt_ms(ms["j"])}   = {med["j"] / len(cells):.2f} ms per cell')
    say(f'  (k) the grid in ONE launch (trial_params with source)       {fmt_ms(ms["k"])}')
    say(f'  (e) uniform fused launch of {T} trials, this library        {fmt_ms(ms["e"])}')
    if 'e_parent' in ms:
        say(f'  (e) the same with the parent\'s library                      {fmt_ms(ms["e_parent"])}')
        say(f'  (e) new / (e) parent = {med["e"] / med["e_parent"]:.4f}; the parent\'s own p10-p90 spread is {spread(ms["e_parent"]) * 100:.2f} % of its median, '
            f'this library\'s {spread(ms["e"]) * 100:.2f} %; the outputs of the two are bit-identical')
    say(f'  (k) / (j) = {med["k"] / med["j"]:.4f}: (k) is {"BELOW" if med["k"] < med["j"] else "NOT below"} (j); every cell of (k) has the bits of '
        'its launch of (j)')
    say(f'  (l) (e)\'s trials through the per-trial kernel, fp\'s values    {fmt_ms(ms["l"])}')
    say(f'  (k) / (e) = {med["k"] / med["e"]:.4f} (reported, not gated);  (l) / (e) = {med["l"] / med["e"]:.4f}: the kernel flavour alone, same trials, same bits')
    careful = lambda out: int((out['k_done'] < K).sum())             # noqa: E731
    say(f'  trials that FAILed: (k) {careful(one_launch)}, (e) {careful(uniform_all)}')
    say()
    say(f'acceptance: (k) below (j): {"yes" if med["k"] < med["j"] else "NO"}')
    say()
    say('# examples/camera_loop.py --grid (its defaults)')
    for line in example.grid_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def occluded_section():
    """(e), (m), (n), (o): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T = 299, 1024
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --occluded on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in; the sweeping bar: rows {example.BAR} of (x, y, w, h, vx, vy, k_on, k_off)')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    none, bar = uvs.engine.occluders(np.zeros((T, 0, 8), np.int64), T), uvs.engine.occluders([example.BAR], T)
    fns = {'e': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True),
           'm': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=none),
           'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'o': lambda: loop(fp, plant, q_d, noise, x0=x0, occluders=bar)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()
    logs = ('err', 'q', 'f', 'dq', 'kappa', 'stats')

    def same(a, b):
        done = a['k_done']
        ok = all(torch.equal(a[key], b[key]) for key in ('status', 'k_done', 'pixels')) and torch.equal(a['stats'].view(torch.int64), b['stats'].view(torch.int64))
        for key in logs[:5]:                                         # the specified rows: q, f up to and including k_done, the others before it
            spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
            ok = ok and torch.equal(a[key].view(torch.int64)[spec], b[key].view(torch.int64)[spec])
        return ok

    assert same(first['m'], first['e']), 'the occluded kernel without occluders and the uniform kernel disagree'
    assert same(first['n'], first['o']), 'the one launch and the stepwise loop behind the bar disagree'
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def run_e_parent():
            mine, uvs._vision._lib = uvs._vision._lib, parent
            try:
                return fns['e']()
            finally:
                uvs._vision._lib = mine

        old = run_e_parent()
        torch.cuda.synchronize()
        assert same(first['e'], old), 'this library and the parent disagree on the uniform launch'
        fns['e_parent'] = run_e_parent
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    spread = lambda v: (np.percentile(v, 90) - np.percentile(v, 10)) / np.median(v)   # noqa: E731
    say()
    say(f'  (e) uniform fused launch, this library                          {fmt_ms(ms["e"])}   = {med["e"] / K * 1e3:.1f} us per step')
    if 'e_parent' in ms:
        say(f'  (e) the same with the parent\'s library                          {fmt_ms(ms["e_parent"])}')
        say(f'  (e) new / (e) parent = {med["e"] / med["e_parent"]:.4f}; the parent\'s own p10-p90 spread is {spread(ms["e_parent"]) * 100:.2f} % of its median, '
            f'this library\'s {spread(ms["e"]) * 100:.2f} %; the outputs of the two are bit-identical')
    say(f'  (m) (e)\'s trials through camera_occluded_kernel, n_occ = 0        {fmt_ms(ms["m"])}')
    say(f'  (n) the sweeping bar on every trial, one launch                  {fmt_ms(ms["n"])}   = {med["n"] / K * 1e3:.1f} us per step')
    say(f'  (o) (n) stepwise: K x (occluded camera features, estimator step) {fmt_ms(ms["o"])}   = {med["o"] / K * 1e3:.1f} us per step')
    say(f'  (n) / (o) = {med["n"] / med["o"]:.4f}: (n) is {"BELOW" if med["n"] < med["o"] else "NOT below"} (o); specified log rows, stats, status, k_done, '
        'pixels bit-identical')
    say(f'  (m) / (e) = {med["m"] / med["e"]:.4f}, (n) / (m) = {med["n"] / med["m"]:.4f} (reported, not gated); (m) has the bits of (e)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (e) {failed(first["e"])}, (n) {failed(first["n"])}; smallest mask behind the bar {int(first["n"]["pixels"].min())} px')
    say()
    say(f'acceptance: (n) below (o): {"yes" if med["n"] < med["o"] else "NO"}')
    say()
    say('# examples/camera_loop.py --occlusion (its defaults)')
    for line in example.occlusion_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def held_section():
    """(n), (p), (q), (r): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, HOLD = 299, 1024, 30
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --held on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in; rows of (x, y, w, h, vx, vy, k_on, k_off): the 12 px bar '
        f'{example.BAR}, the wide bar {example.WIDE_BAR}; hold = {HOLD}')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    bar, wide = uvs.engine.occluders([example.BAR], T), uvs.engine.occluders([example.WIDE_BAR], T)
    held_entry = uvs._vision.lib().uvs_camera_closed_loop_held_f64

    def run_p():
        """(n)'s call through the held entry point with hold = 0 (engine.camera_closed_loop(hold=0) takes the occluded route), with (n)'s allocations."""
        cam = plant.to_camera(uvs.plant.DISC_RADIUS)
        f64 = dict(dtype=torch.float64, device='cuda')
        f0 = torch.zeros((T, 8), **f64)
        uvs.engine.camera_features(cam, q_d, out=f0, occluders=bar)
        log = {key: torch.empty((K, T, comp), **f64) for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8), ('kappa', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats_t, pixels, held = torch.empty((T, 3), **f64), *(torch.empty((T, 4), dtype=torch.int32, device='cuda') for _ in range(2))
        uvs._vision.check(held_entry(ctypes.byref(fp), ctypes.byref(cam), T, None, bar.data_ptr(), bar.shape[1], 0, q_d.data_ptr(), noise.data_ptr(),
                                     x0.data_ptr(), f0.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(), log['dq'].data_ptr(),
                                     log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats_t.data_ptr(),
                                     pixels.data_ptr(), held.data_ptr(), uvs.engine._stream()))
        return dict(log, pixels=pixels, status=status, k_done=k_done, stats=stats_t, held=held)

    fns = {'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'p': run_p,
           'q': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, hold=HOLD),
           'r': lambda: loop(fp, plant, q_d, noise, x0=x0, occluders=wide, hold=HOLD)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b):
        done = a['k_done']
        ok = all(torch.equal(a[key], b[key]) for key in ('status', 'k_done', 'pixels')) and torch.equal(a['stats'].view(torch.int64), b['stats'].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
            ok = ok and torch.equal(a[key].view(torch.int64)[spec], b[key].view(torch.int64)[spec])
        return ok

    assert same(first['p'], first['n']) and int(first['p']['held'].sum()) == 0, 'the held kernel with hold = 0 and the occluded kernel disagree'
    assert same(first['q'], first['r']) and torch.equal(first['q']['held'], first['r']['held']), 'the one launch and the stepwise loop disagree'
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def run_n_parent():
            mine, uvs._vision._lib = uvs._vision._lib, parent
            try:
                return fns['n']()
            finally:
                uvs._vision._lib = mine

        old = run_n_parent()
        torch.cuda.synchronize()
        assert same(first['n'], old), 'this library and the parent disagree on the occluded launch'
        fns['n_parent'] = run_n_parent
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    spread = lambda v: (np.percentile(v, 90) - np.percentile(v, 10)) / np.median(v)   # noqa: E731
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say()
    say(f'  (n) the 12 px bar, camera_occluded_kernel, this library           {fmt_ms(ms["n"])}   = {med["n"] / K * 1e3:.1f} us per step')
    if 'n_parent' in ms:
        say(f'  (n) the same with the parent\'s library                           {fmt_ms(ms["n_parent"])}')
        say(f'  (n) new / (n) parent = {med["n"] / med["n_parent"]:.4f}; the parent\'s own p10-p90 spread is {spread(ms["n_parent"]) * 100:.2f} % of its median, '
            f'this library\'s {spread(ms["n"]) * 100:.2f} %; the outputs of the two are bit-identical')
    say(f'  (p) (n)\'s trials through camera_held_kernel, hold = 0             {fmt_ms(ms["p"])}')
    say(f'  (q) the wide bar, hold = {HOLD}, one launch                           {fmt_ms(ms["q"])}   = {med["q"] / K * 1e3:.1f} us per step')
    say(f'  (r) (q) stepwise: K x (occluded features, hold, estimator step)   {fmt_ms(ms["r"])}   = {med["r"] / K * 1e3:.1f} us per step')
    say(f'  (q) / (r) = {med["q"] / med["r"]:.4f}: (q) is {"BELOW" if med["q"] < med["r"] else "NOT below"} (r); specified log rows, stats, status, k_done, '
        'pixels, held bit-identical')
    say(f'  (p) / (n) = {med["p"] / med["n"]:.4f}, (q) / (n) = {med["q"] / med["n"]:.4f} (reported, not gated); (p) has the bits of (n)')
    say(f'  trials that FAILed: (n) {failed(first["n"])}, (q) {failed(first["q"])}; held steps in (q): {int(first["q"]["held"].sum())} over {T} trials, '
        f'at most {int(first["q"]["held"].max())} per disc; the wide bar without a hold FAILs '
        f'{failed(loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, want=()))}')
    say()
    say(f'acceptance: (q) below (r): {"yes" if med["q"] < med["r"] else "NO"}')
    say()
    say(f'# examples/camera_loop.py --occlusion --hold {HOLD} (its defaults)')
    for line in example.hold_table(uvs, HOLD):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def painted_section():
    """(e), (n), (q) against the parent's; (s), (t), (u): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, HOLD = 299, 1024, 30
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --painted on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in; rows of (x, y, w, h, vx, vy, k_on, k_off): the 12 px bar '
        f'{example.BAR}, the wide bar {example.WIDE_BAR}, the distractor {example.DISTRACTOR} painted green; hold = {HOLD}')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    bar, wide = uvs.engine.occluders([example.BAR], T), uvs.engine.occluders([example.WIDE_BAR], T)
    both = uvs.engine.occluders([example.WIDE_BAR, example.DISTRACTOR], T)
    paints = torch.as_tensor(np.tile(np.array([-1, example.GREEN], np.int32), (T, 1)), device='cuda')
    painted_entry = uvs._vision.lib().uvs_camera_closed_loop_painted_f64

    def run_s():
        """(q)'s call through the painted entry point with paint = NULL (engine.camera_closed_loop without paints takes the held route)."""
        cam = plant.to_camera(uvs.plant.DISC_RADIUS)
        f64 = dict(dtype=torch.float64, device='cuda')
        f0 = torch.zeros((T, 8), **f64)
        uvs.engine.camera_features(cam, q_d, out=f0, occluders=wide)
        log = {key: torch.empty((K, T, comp), **f64) for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8), ('kappa', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats_t, pixels, held = torch.empty((T, 3), **f64), *(torch.empty((T, 4), dtype=torch.int32, device='cuda') for _ in range(2))
        uvs._vision.check(painted_entry(ctypes.byref(fp), ctypes.byref(cam), T, None, wide.data_ptr(), None, wide.shape[1], HOLD, q_d.data_ptr(),
                                        noise.data_ptr(), x0.data_ptr(), f0.data_ptr(), log['q'].data_ptr(), log['f'].data_ptr(),
                                        log['dq'].data_ptr(), log['err'].data_ptr(), log['kappa'].data_ptr(), status.data_ptr(), k_done.data_ptr(),
                                        stats_t.data_ptr(), pixels.data_ptr(), held.data_ptr(), uvs.engine._stream()))
        return dict(log, pixels=pixels, status=status, k_done=k_done, stats=stats_t, held=held)

    fns = {'e': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True),
           'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'q': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, hold=HOLD),
           's': run_s,
           't': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=both, occluder_colours=paints, hold=HOLD),
           'u': lambda: loop(fp, plant, q_d, noise, x0=x0, occluders=both, occluder_colours=paints, hold=HOLD)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b):
        done = a['k_done']
        ok = all(torch.equal(a[key], b[key]) for key in ('status', 'k_done', 'pixels')) and torch.equal(a['stats'].view(torch.int64), b['stats'].view(torch.int64))
        ok = ok and ('held' in a) == ('held' in b) and ('held' not in a or torch.equal(a['held'], b['held']))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
            ok = ok and torch.equal(a[key].view(torch.int64)[spec], b[key].view(torch.int64)[spec])
        return ok

    assert same(first['s'], first['q']), 'the painted kernel with paint = NULL and the held kernel disagree'
    assert same(first['t'], first['u']), 'the one launch and the stepwise loop disagree'
    assert not torch.equal(first['t']['f'].view(torch.int64), first['q']['f'].view(torch.int64)), 'the distractor moves no feature'
    gated = ('e', 'n', 'q')
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in gated:
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say()
    what = {'e': 'the uniform fused launch, camera_loop_kernel', 'n': 'the 12 px bar, camera_occluded_kernel', 'q': f'the wide bar, hold = {HOLD}, camera_held_kernel'}
    passed = True
    for name in gated:
        say(f'  ({name}) {what[name]:48s} this library   {fmt_ms(ms[name])}   = {med[name] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[name + '_parent_a'], med[name + '_parent_b']
            say(f'  ({name}) {"":48s} the parent\'s, 1  {fmt_ms(ms[name + "_parent_a"])}')
            say(f'  ({name}) {"":48s} the parent\'s, 2  {fmt_ms(ms[name + "_parent_b"])}')
            ok = med[name] <= max(a, b) + abs(a - b)
            passed = passed and ok
            say(f'  ({name}) new / slower parent run = {med[name] / max(a, b):.4f}; the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %: '
                f'{"passes" if ok else "DOES NOT pass"}; outputs bit-identical')
    say(f'  (s) (q)\'s trials through camera_painted_kernel, paint = NULL        {fmt_ms(ms["s"])}')
    say(f'  (t) (q) with a still distractor on every trial, one launch         {fmt_ms(ms["t"])}   = {med["t"] / K * 1e3:.1f} us per step')
    say(f'  (u) (t) stepwise: K x (painted features, hold, estimator step)     {fmt_ms(ms["u"])}   = {med["u"] / K * 1e3:.1f} us per step')
    say(f'  (s) / (q) = {med["s"] / med["q"]:.4f}, (t) / (q) = {med["t"] / med["q"]:.4f}, (t) / (u) = {med["t"] / med["u"]:.4f} (reported, not gated); '
        '(s) has the bits of (q), (t) those of (u)')
    say(f'  trials that FAILed: (q) {failed(first["q"])}, (t) {failed(first["t"])}; held steps of green: (q) {int(first["q"]["held"][:, 1].sum())}, '
        f'(t) {int(first["t"]["held"][:, 1].sum())}; smallest green mask: (q) {int(first["q"]["pixels"][:, 1].min())}, (t) {int(first["t"]["pixels"][:, 1].min())}')
    say()
    if PARENT_LIB is not None:
        say(f'gate: (e), (n), (q) against two runs of the parent\'s library: {"pass" if passed else "DO NOT pass"}')
        say()
    say('# examples/camera_loop.py --distractor (its defaults)')
    for line in example.distractor_table(uvs):
        say(line)
    say()
    say(f'# examples/camera_loop.py --distractor --occlusion --hold {HOLD}')
    for line in example.distractor_table(uvs, bar=example.WIDE_BAR, hold=HOLD):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def scenes_section():
    """(e), (n), (q) against the parent's; (v) .. (z): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, HOLD, N_SCENES = 299, 1024, 30, 16
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --scenes on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess); the 12 px bar {example.BAR}, the wide '
        f'bar {example.WIDE_BAR} with hold = {HOLD}; {N_SCENES} scenes of examples/camera_loop.py --scenes (seed 0) x {T // N_SCENES} trials')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    bar, wide = uvs.engine.occluders([example.BAR], T), uvs.engine.occluders([example.WIDE_BAR], T)
    one = uvs.engine.camera_scenes(plant)
    scene_plants = example.scene_plants(uvs, plant, N_SCENES, 0)
    scenes = uvs.engine.camera_scenes(scene_plants)
    per = T // N_SCENES
    index = torch.as_tensor(np.repeat(np.arange(N_SCENES, dtype=np.int32), per), device='cuda')
    nominal = uvs.engine.believed_models(plant)
    parts = [(c, slice(c * per, (c + 1) * per)) for c in range(N_SCENES)]
    cut = {c: (q_d[rows].contiguous(), noise[:, rows].contiguous(), x0[rows].contiguous()) for c, rows in parts}

    def run_x():
        return [loop(fp, scene_plants[c], *cut[c][:2], x0=cut[c][2], fused=True) for c, _ in parts]

    fns = {'e': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True),
           'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'q': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, hold=HOLD),
           'v': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=one),
           'w': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=scenes, camera_index=index),
           'x': run_x,
           'z': lambda: loop(fp, plant, q_d, noise, x0=x0, cameras=scenes, camera_index=index),
           'k': lambda: loop(fa, plant, q_d, noise, fused=True, believed=nominal),
           'y': lambda: loop(fa, plant, q_d, noise, fused=True, believed=nominal, cameras=one),
           'y16': lambda: loop(fa, plant, q_d, noise, fused=True, believed=nominal, cameras=scenes, camera_index=index)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b, rows=slice(None), rows_b=slice(None)):
        done = a['k_done'][rows]
        ok = all(torch.equal(a[key][rows], b[key][rows_b]) for key in ('status', 'k_done', 'pixels'))
        ok = ok and torch.equal(a['stats'][rows].view(torch.int64), b['stats'][rows_b].view(torch.int64))
        ok = ok and ('held' in a) == ('held' in b) and ('held' not in a or torch.equal(a['held'][rows], b['held'][rows_b]))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            if key in a:
                spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
                ok = ok and torch.equal(a[key][:, rows].view(torch.int64)[spec], b[key][:, rows_b].view(torch.int64)[spec])
        return ok

    assert same(first['v'], first['e']), 'the scenes kernel on the one nominal camera and the uniform kernel disagree'
    assert same(first['w'], first['z']), 'the one launch and the stepwise loop disagree'
    assert same(first['y'], first['k']), 'the scenes baseline on the one nominal camera and the believed loop disagree'
    for c, rows in parts:
        assert same(first['w'], first['x'][c], rows), f'scene {c}: the one launch and the launch per scene disagree'
    gated = ('e', 'n', 'q')
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in gated:
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'e': 'the uniform fused launch, camera_loop_kernel', 'n': 'the 12 px bar, camera_occluded_kernel', 'q': f'the wide bar, hold = {HOLD}, camera_held_kernel'}
    passed = True
    for name in gated:
        say(f'  ({name}) {what[name]:48s} this library   {fmt_ms(ms[name])}   = {med[name] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[name + '_parent_a'], med[name + '_parent_b']
            say(f'  ({name}) {"":48s} the parent\'s, 1  {fmt_ms(ms[name + "_parent_a"])}')
            say(f'  ({name}) {"":48s} the parent\'s, 2  {fmt_ms(ms[name + "_parent_b"])}')
            ok = med[name] <= max(a, b) + abs(a - b)
            passed = passed and ok
            say(f'  ({name}) new / slower parent run = {med[name] / max(a, b):.4f}; the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %: '
                f'{"passes" if ok else "DOES NOT pass"}; outputs bit-identical')
    say(f'  (v) (e)\'s trials through camera_scene_kernel, n_cams = 1                  {fmt_ms(ms["v"])}   = {med["v"] / K * 1e3:.1f} us per step')
    say(f'  (w) {N_SCENES} scenes x {per} trials, one launch                                   {fmt_ms(ms["w"])}   = {med["w"] / K * 1e3:.1f} us per step')
    say(f'  (x) the same as {N_SCENES} uniform launches of {per} trials, one per scene             {fmt_ms(ms["x"])}')
    say(f'  (z) (w) stepwise: K x (scene features, estimator step)                    {fmt_ms(ms["z"])}   = {med["z"] / K * 1e3:.1f} us per step')
    say(f'  (k) the believed baseline loop, camera_believed_loop_kernel               {fmt_ms(ms["k"])}')
    say(f'  (y) (k)\'s trials through scene_baseline_loop_kernel, n_cams = 1           {fmt_ms(ms["y"])}')
    say(f'  (y16) the baseline on the nominal model over the {N_SCENES} scenes, one launch       {fmt_ms(ms["y16"])}')
    say(f'  (v) / (e) = {med["v"] / med["e"]:.4f}, (w) / (x) = {med["w"] / med["x"]:.4f}, (w) / (z) = {med["w"] / med["z"]:.4f}, (y) / (k) = '
        f'{med["y"] / med["k"]:.4f} (reported, not gated); (v) has the bits of (e), (w) those of (x) and of (z), (y) those of (k)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (e) {failed(first["e"])}, (w) {failed(first["w"])}, (k) {failed(first["k"])}, (y16) {failed(first["y16"])}')
    say()
    if PARENT_LIB is not None:
        say(f'gate: (e), (n), (q) against two runs of the parent\'s library: {"pass" if passed else "DO NOT pass"}')
        say()
    say('# examples/camera_loop.py --scenes 8 (its defaults)')
    for line in example.scenes_table(uvs, 8):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def moving_section():
    """(e), (n), (q), (v), (w) against the parent's; (mv) .. (my16): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, HOLD, N = 299, 1024, 30, 16
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --moving on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess); the 12 px bar {example.BAR}, the wide '
        f'bar {example.WIDE_BAR} with hold = {HOLD}; {N} scenes of examples/camera_loop.py --scenes (seed 0) and {N} motions of --moving '
        f'(seed 0, {example.MOVING_SPEED} m per step in the window {example.MOVING_WINDOW}) x {T // N} trials')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    bar, wide = uvs.engine.occluders([example.BAR], T), uvs.engine.occluders([example.WIDE_BAR], T)
    one = uvs.engine.camera_scenes(plant)
    scenes = uvs.engine.camera_scenes(example.scene_plants(uvs, plant, N, 0))
    per = T // N
    index = torch.as_tensor(np.repeat(np.arange(N, dtype=np.int32), per), device='cuda')
    nominal = uvs.engine.believed_models(plant)
    velocities = example.moving_velocities(N, 4, 0)
    motions = uvs.engine.target_motions(np.repeat(velocities, per, axis=0), example.MOVING_WINDOW, 4, T)
    parts = [(c, slice(c * per, (c + 1) * per)) for c in range(N)]
    cut = {c: (q_d[rows].contiguous(), noise[:, rows].contiguous(), x0[rows].contiguous(), motions[rows].contiguous()) for c, rows in parts}
    cam = plant.to_camera(uvs.plant.DISC_RADIUS)
    scene_one = (one.data_ptr(), 1, None), one, None, True           # the nominal camera as the one scene
    no_motion = (None, None)                                         # the moving entry points with motion = NULL

    def run_mx():
        return [loop(fp, plant, *cut[c][:2], x0=cut[c][2], fused=True, target_motion=cut[c][3]) for c, _ in parts]

    def run_my_null():                                               # the same call through uvs_camera_believed_loop_moving_f64, motion = NULL
        import ctypes as C
        out = {key: torch.empty((K, T, comp), dtype=torch.float64, device='cuda') for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.empty((T, 3), dtype=torch.float64, device='cuda'), torch.empty((T, 4), dtype=torch.int32, device='cuda')
        uvs._vision.check(uvs._vision.lib().uvs_camera_believed_loop_moving_f64(
            C.byref(fa), one.data_ptr(), 1, None, None, T, nominal.data_ptr(), 1, None, q_d.data_ptr(), noise.data_ptr(), out['q'].data_ptr(),
            out['f'].data_ptr(), out['dq'].data_ptr(), out['err'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), uvs.engine._stream()))
        return dict(out, pixels=pixels, status=status, k_done=k_done, stats=stats)

    fns = {'e': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True),
           'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'q': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, hold=HOLD),
           'v': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=one),
           'w': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=scenes, camera_index=index),
           'mv': lambda: uvs.engine._camera_closed_loop_fused(fp, cam, q_d, noise, x0, 'host', uvs.engine.CAMERA_LOGS, scenes=scene_one,
                                                              motion=no_motion),
           'mw': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, target_motion=motions),
           'mx': run_mx,
           'mz': lambda: loop(fp, plant, q_d, noise, x0=x0, target_motion=motions),
           'y': lambda: loop(fa, plant, q_d, noise, fused=True, believed=nominal, cameras=one),
           'my': run_my_null,
           'my16': lambda: loop(fa, plant, q_d, noise, fused=True, target_motion=motions)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b, rows=slice(None), rows_b=slice(None)):
        done = a['k_done'][rows]
        ok = all(torch.equal(a[key][rows], b[key][rows_b]) for key in ('status', 'k_done', 'pixels'))
        ok = ok and torch.equal(a['stats'][rows].view(torch.int64), b['stats'][rows_b].view(torch.int64))
        ok = ok and ('held' in a) == ('held' in b) and ('held' not in a or torch.equal(a['held'][rows], b['held'][rows_b]))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            if key in a:
                spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
                ok = ok and torch.equal(a[key][:, rows].view(torch.int64)[spec], b[key][:, rows_b].view(torch.int64)[spec])
        return ok

    assert same(first['mv'], first['v']), 'the moving kernel without a motion and the scenes kernel disagree'
    assert same(first['mw'], first['mz']), 'the one launch and the stepwise loop disagree'
    assert same(first['my'], first['y']), 'the moving baseline without a motion and the scenes baseline disagree'
    assert not same(first['mw'], first['v']), 'the motions show'
    for c, rows in parts:
        assert same(first['mw'], first['mx'][c], rows), f'motion {c}: the one launch and the launch per motion disagree'
    gated = ('e', 'n', 'q', 'v', 'w')
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in gated:
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'e': 'the uniform fused launch, camera_loop_kernel', 'n': 'the 12 px bar, camera_occluded_kernel', 'q': f'the wide bar, hold = {HOLD}, camera_held_kernel',
            'v': "(e)'s trials through camera_scene_kernel, n_cams = 1", 'w': f'{N} scenes x {per} trials, one launch'}
    passed = True
    for name in gated:
        say(f'  ({name}) {what[name]:52s} this library   {fmt_ms(ms[name])}   = {med[name] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[name + '_parent_a'], med[name + '_parent_b']
            say(f'  ({name}) {"":52s} the parent\'s, 1  {fmt_ms(ms[name + "_parent_a"])}')
            say(f'  ({name}) {"":52s} the parent\'s, 2  {fmt_ms(ms[name + "_parent_b"])}')
            ok = med[name] <= max(a, b) + abs(a - b)
            passed = passed and ok
            say(f'  ({name}) new / slower parent run = {med[name] / max(a, b):.4f}; the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %: '
                f'{"passes" if ok else "DOES NOT pass"}; outputs bit-identical')
    say(f'  (mv) (v)\'s trials through moving_target_kernel, motion = NULL              {fmt_ms(ms["mv"])}   = {med["mv"] / K * 1e3:.1f} us per step')
    say(f'  (mw) {N} motions x {per} trials, one launch                                  {fmt_ms(ms["mw"])}   = {med["mw"] / K * 1e3:.1f} us per step')
    say(f'  (mx) the same as {N} launches of {per} trials, one per motion                  {fmt_ms(ms["mx"])}')
    say(f'  (mz) (mw) stepwise: K x (moving features, estimator step)                  {fmt_ms(ms["mz"])}   = {med["mz"] / K * 1e3:.1f} us per step')
    say(f'  (y) the scenes baseline loop on the nominal camera, n_cams = 1             {fmt_ms(ms["y"])}')
    say(f'  (my) (y)\'s trials through moving_baseline_kernel, motion = NULL            {fmt_ms(ms["my"])}')
    say(f'  (my16) the baseline over the {N} motions, one launch                         {fmt_ms(ms["my16"])}')
    say(f'  (mv) / (v) = {med["mv"] / med["v"]:.4f}, (mw) / (mx) = {med["mw"] / med["mx"]:.4f}, (mw) / (mz) = {med["mw"] / med["mz"]:.4f}, (my) / (y) = '
        f'{med["my"] / med["y"]:.4f} (reported, not gated); (mv) has the bits of (v), (mw) those of (mx) and of (mz), (my) those of (y)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (e) {failed(first["e"])}, (mw) {failed(first["mw"])}, (y) {failed(first["y"])}, (my16) {failed(first["my16"])}')
    say()
    if PARENT_LIB is not None:
        say(f'gate: (e), (n), (q), (v), (w) against two runs of the parent\'s library: {"pass" if passed else "DO NOT pass"}')
        say()
    say('# examples/camera_loop.py --moving (its defaults)')
    for line in example.moving_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def delayed_section():
    """(e), (n), (q), (v), (w), (mv), (mw) against the parent's; (dv) .. (dy5): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, HOLD, N = 299, 1024, 30, 16
    LAT, PER = example.LATENCIES, 64
    TL = len(LAT) * PER
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --delayed on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess); the 12 px bar {example.BAR}, the wide '
        f'bar {example.WIDE_BAR} with hold = {HOLD}; {N} scenes and {N} motions of examples/camera_loop.py (seed 0) x {T // N} trials; the latencies '
        f'{LAT} x {PER} trials = {TL} trials')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    bar, wide = uvs.engine.occluders([example.BAR], T), uvs.engine.occluders([example.WIDE_BAR], T)
    one = uvs.engine.camera_scenes(plant)
    scenes = uvs.engine.camera_scenes(example.scene_plants(uvs, plant, N, 0))
    per = T // N
    index = torch.as_tensor(np.repeat(np.arange(N, dtype=np.int32), per), device='cuda')
    nominal = uvs.engine.believed_models(plant)
    motions = uvs.engine.target_motions(np.repeat(example.moving_velocities(N, 4, 0), per, axis=0), example.MOVING_WINDOW, 4, T)
    cam = plant.to_camera(uvs.plant.DISC_RADIUS)
    scene_one = (one.data_ptr(), 1, None), one, None, True           # the nominal camera as the one scene
    no_motion, no_latency = (None, None), (None, None)               # the entry points with motion = NULL, latency = NULL
    # the latency experiment: the same 64 starts and noise under each of the 5 latencies
    ql = q_d[:PER].repeat(len(LAT), 1).contiguous()
    nl = noise[:, :PER].repeat(1, len(LAT), 1).contiguous()
    xl = x0[:PER].repeat(len(LAT), 1).contiguous()
    latency = np.repeat(np.array(LAT, np.int64), PER)
    parts = [(c, slice(c * PER, (c + 1) * PER)) for c in range(len(LAT))]
    cut = (ql[:PER].contiguous(), nl[:, :PER].contiguous(), xl[:PER].contiguous())

    def baseline_null(entry, *front):                                # a baseline loop through the C ABI with NULL operands
        import ctypes as C
        out = {key: torch.empty((K, T, comp), dtype=torch.float64, device='cuda') for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.empty((T, 3), dtype=torch.float64, device='cuda'), torch.empty((T, 4), dtype=torch.int32, device='cuda')
        uvs._vision.check(getattr(uvs._vision.lib(), entry)(
            C.byref(fa), one.data_ptr(), 1, None, *front, T, nominal.data_ptr(), 1, None, q_d.data_ptr(), noise.data_ptr(), out['q'].data_ptr(),
            out['f'].data_ptr(), out['dq'].data_ptr(), out['err'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), uvs.engine._stream()))
        return dict(out, pixels=pixels, status=status, k_done=k_done, stats=stats)

    fns = {'e': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True),
           'n': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=bar),
           'q': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, occluders=wide, hold=HOLD),
           'v': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=one),
           'w': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, cameras=scenes, camera_index=index),
           'mv': lambda: uvs.engine._camera_closed_loop_fused(fp, cam, q_d, noise, x0, 'host', uvs.engine.CAMERA_LOGS, scenes=scene_one,
                                                              motion=no_motion),
           'mw': lambda: loop(fp, plant, q_d, noise, x0=x0, fused=True, target_motion=motions),
           'dv': lambda: uvs.engine._camera_closed_loop_fused(fp, cam, q_d, noise, x0, 'host', uvs.engine.CAMERA_LOGS, scenes=scene_one,
                                                              motion=None, latency=no_latency),
           'dw': lambda: loop(fp, plant, ql, nl, x0=xl, fused=True, latency=latency),
           'dx': lambda: [loop(fp, plant, *cut[:2], x0=cut[2], fused=True, latency=d) for d in LAT],
           'dz': lambda: loop(fp, plant, ql, nl, x0=xl, latency=latency),
           'my': lambda: baseline_null('uvs_camera_believed_loop_moving_f64', None),
           'dy': lambda: baseline_null('uvs_camera_believed_loop_delayed_f64', None, None),
           'dy5': lambda: loop(fa, plant, ql, nl, fused=True, latency=latency)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b, rows=slice(None), rows_b=slice(None)):
        done = a['k_done'][rows]
        ok = all(torch.equal(a[key][rows], b[key][rows_b]) for key in ('status', 'k_done', 'pixels'))
        ok = ok and torch.equal(a['stats'][rows].view(torch.int64), b['stats'][rows_b].view(torch.int64))
        ok = ok and ('held' in a) == ('held' in b) and ('held' not in a or torch.equal(a['held'][rows], b['held'][rows_b]))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            if key in a:
                spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
                ok = ok and torch.equal(a[key][:, rows].view(torch.int64)[spec], b[key][:, rows_b].view(torch.int64)[spec])
        return ok

    assert same(first['dv'], first['mv']), 'the delayed kernel without a latency and the moving kernel disagree'
    assert same(first['dw'], first['dz']), 'the one launch and the stepwise loop disagree'
    assert same(first['dy'], first['my']), 'the delayed baseline without a latency and the moving baseline disagree'
    for c, rows in parts:
        assert same(first['dw'], first['dx'][c], rows), f'latency {LAT[c]}: the one launch and the launch per latency disagree'
    assert not same(first['dw'], first['dx'][0], parts[1][1]), 'the latencies show'
    gated = ('e', 'n', 'q', 'v', 'w', 'mv', 'mw')
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in gated:
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'e': 'the uniform fused launch, camera_loop_kernel', 'n': 'the 12 px bar, camera_occluded_kernel', 'q': f'the wide bar, hold = {HOLD}, camera_held_kernel',
            'v': "(e)'s trials through camera_scene_kernel, n_cams = 1", 'w': f'{N} scenes x {per} trials, one launch',
            'mv': "(v)'s trials through moving_target_kernel, NULL", 'mw': f'{N} motions x {per} trials, one launch'}
    passed = True
    for name in gated:
        say(f'  ({name}) {what[name]:52s} this library   {fmt_ms(ms[name])}   = {med[name] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[name + '_parent_a'], med[name + '_parent_b']
            say(f'  ({name}) {"":52s} the parent\'s, 1  {fmt_ms(ms[name + "_parent_a"])}')
            say(f'  ({name}) {"":52s} the parent\'s, 2  {fmt_ms(ms[name + "_parent_b"])}')
            ok = med[name] <= max(a, b) + abs(a - b)
            passed = passed and ok
            say(f'  ({name}) new / slower parent run = {med[name] / max(a, b):.4f}; the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %: '
                f'{"passes" if ok else "DOES NOT pass"}; outputs bit-identical')
    say(f'  (dv) (mv)\'s trials through delayed_frames_kernel, latency = NULL           {fmt_ms(ms["dv"])}   = {med["dv"] / K * 1e3:.1f} us per step')
    say(f'  (dw) {len(LAT)} latencies x {PER} trials, one launch                                  {fmt_ms(ms["dw"])}   = {med["dw"] / K * 1e3:.1f} us per step')
    say(f'  (dx) the same as {len(LAT)} launches of {PER} trials, one per latency                  {fmt_ms(ms["dx"])}')
    say(f'  (dz) (dw) stepwise: K x (features, delay, estimator step)                  {fmt_ms(ms["dz"])}   = {med["dz"] / K * 1e3:.1f} us per step')
    say(f'  (my) the moving baseline loop on the nominal camera, motion = NULL         {fmt_ms(ms["my"])}')
    say(f'  (dy) (my)\'s trials through delayed_baseline_kernel, latency = NULL         {fmt_ms(ms["dy"])}')
    say(f'  (dy5) the baseline over the {len(LAT)} latencies x {PER} trials, one launch              {fmt_ms(ms["dy5"])}')
    say(f'  (dv) / (mv) = {med["dv"] / med["mv"]:.4f}, (dw) / (dx) = {med["dw"] / med["dx"]:.4f}, (dw) / (dz) = {med["dw"] / med["dz"]:.4f}, (dy) / (my) = '
        f'{med["dy"] / med["my"]:.4f} (reported, not gated); (dv) has the bits of (mv), (dw) those of (dx) and of (dz), (dy) those of (my)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (e) {failed(first["e"])}, (dw) {failed(first["dw"])}, (my) {failed(first["my"])}, (dy5) {failed(first["dy5"])}')
    say()
    if PARENT_LIB is not None:
        say(f'gate: (e), (n), (q), (v), (w), (mv), (mw) against two runs of the parent\'s library: {"pass" if passed else "DO NOT pass"}')
        say()
    say('# examples/camera_loop.py --latency (its defaults)')
    for line in example.latency_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def aligned_section():
    """(dv), (dy) against the parent's; (av) .. (ay25): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T = 299, 1024
    LAT, TOLD, PER = example.LATENCIES, example.ASSUMED, 64
    cells = [(d, a) for d in LAT for a in TOLD]
    TL = len(cells) * PER
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --aligned on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess); the latencies {LAT} x the assumed '
        f'latencies {TOLD} x {PER} trials = {TL} trials')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    one = uvs.engine.camera_scenes(plant)
    nominal = uvs.engine.believed_models(plant)
    cam = plant.to_camera(uvs.plant.DISC_RADIUS)
    scene_one = (one.data_ptr(), 1, None), one, None, True           # the nominal camera as the one scene
    null = (None, None)                                              # latency = NULL, assumed = NULL
    # the experiment: the same 64 starts and noise in each of the 25 cells
    ql = q_d[:PER].repeat(len(cells), 1).contiguous()
    nl = noise[:, :PER].repeat(1, len(cells), 1).contiguous()
    xl = x0[:PER].repeat(len(cells), 1).contiguous()
    latency = np.repeat(np.array([d for d, _ in cells], np.int64), PER)
    told = np.repeat(np.array([a for _, a in cells], np.int64), PER)
    parts = [(c, slice(c * PER, (c + 1) * PER)) for c in range(len(cells))]
    cut = (ql[:PER].contiguous(), nl[:, :PER].contiguous(), xl[:PER].contiguous())

    def baseline_null(entry, *front):                                # a baseline loop through the C ABI with NULL operands
        import ctypes as C
        out = {key: torch.empty((K, T, comp), dtype=torch.float64, device='cuda') for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.empty((T, 3), dtype=torch.float64, device='cuda'), torch.empty((T, 4), dtype=torch.int32, device='cuda')
        uvs._vision.check(getattr(uvs._vision.lib(), entry)(
            C.byref(fa), one.data_ptr(), 1, None, *front, T, nominal.data_ptr(), 1, None, q_d.data_ptr(), noise.data_ptr(), out['q'].data_ptr(),
            out['f'].data_ptr(), out['dq'].data_ptr(), out['err'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), uvs.engine._stream()))
        return dict(out, pixels=pixels, status=status, k_done=k_done, stats=stats)

    fused = uvs.engine._camera_closed_loop_fused
    fns = {'dv': lambda: fused(fp, cam, q_d, noise, x0, 'host', uvs.engine.CAMERA_LOGS, scenes=scene_one, motion=None, latency=null),
           'av': lambda: fused(fp, cam, q_d, noise, x0, 'host', uvs.engine.CAMERA_LOGS, scenes=scene_one, motion=None, latency=None, assumed=null),
           'dy': lambda: baseline_null('uvs_camera_believed_loop_delayed_f64', None, None),
           'ay': lambda: baseline_null('uvs_camera_believed_loop_aligned_f64', None, None, None),
           'aw': lambda: loop(fp, plant, ql, nl, x0=xl, fused=True, latency=latency, assumed_latency=told),
           'ax': lambda: [loop(fp, plant, *cut[:2], x0=cut[2], fused=True, latency=d, assumed_latency=a) for d, a in cells],
           'az': lambda: loop(fp, plant, ql, nl, x0=xl, latency=latency, assumed_latency=told),
           'ay25': lambda: loop(fa, plant, ql, nl, fused=True, latency=latency, assumed_latency=told)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b, rows=slice(None), rows_b=slice(None)):
        done = a['k_done'][rows]
        ok = all(torch.equal(a[key][rows], b[key][rows_b]) for key in ('status', 'k_done', 'pixels'))
        ok = ok and torch.equal(a['stats'][rows].view(torch.int64), b['stats'][rows_b].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            if key in a:
                spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
                ok = ok and torch.equal(a[key][:, rows].view(torch.int64)[spec], b[key][:, rows_b].view(torch.int64)[spec])
        return ok

    assert same(first['av'], first['dv']), 'the aligned kernel that is not told and the delayed kernel disagree'
    assert same(first['ay'], first['dy']), 'the aligned baseline that is not told and the delayed baseline disagree'
    assert same(first['aw'], first['az']), 'the one launch and the stepwise loop disagree'
    for c, rows in parts:
        assert same(first['aw'], first['ax'][c], rows), f'cell {cells[c]}: the one launch and the launch per cell disagree'
    assert not same(first['aw'], first['ax'][0], parts[1][1]), 'telling shows'
    gated = {'av': 'dv', 'ay': 'dy'}
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in gated.values():
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'dv': 'delayed_frames_kernel, latency = NULL', 'av': "(dv)'s trials through aligned_frames_kernel, NULL, NULL",
            'dy': 'delayed_baseline_kernel, latency = NULL', 'ay': "(dy)'s trials through aligned_baseline_kernel, NULL, NULL"}
    passed = True
    for new, old in gated.items():
        say(f'  ({old}) {what[old]:56s} this library   {fmt_ms(ms[old])}   = {med[old] / K * 1e3:.1f} us per step')
        say(f'  ({new}) {what[new]:56s} this library   {fmt_ms(ms[new])}   = {med[new] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[old + '_parent_a'], med[old + '_parent_b']
            say(f'  ({old}) {"":56s} the parent\'s, 1  {fmt_ms(ms[old + "_parent_a"])}')
            say(f'  ({old}) {"":56s} the parent\'s, 2  {fmt_ms(ms[old + "_parent_b"])}')
            ok = med[new] <= max(a, b) + abs(a - b)
            passed = passed and ok
            say(f'  ({new}) / slower parent run of ({old}) = {med[new] / max(a, b):.4f}; the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %: '
                f'{"passes" if ok else "DOES NOT pass"}; outputs bit-identical')
    say(f'  (aw) {len(LAT)} latencies x {len(TOLD)} assumed x {PER} trials, one launch                         {fmt_ms(ms["aw"])}   = {med["aw"] / K * 1e3:.1f} us per step')
    say(f'  (ax) the same as {len(cells)} launches of {PER} trials, one per cell                      {fmt_ms(ms["ax"])}')
    say(f'  (az) (aw) stepwise: K x (features, delay, gather, estimator step)           {fmt_ms(ms["az"])}   = {med["az"] / K * 1e3:.1f} us per step')
    say(f'  (ay25) the baseline over the {len(cells)} cells x {PER} trials, one launch                 {fmt_ms(ms["ay25"])}')
    say(f'  (av) / (dv) = {med["av"] / med["dv"]:.4f}, (ay) / (dy) = {med["ay"] / med["dy"]:.4f}, (aw) / (ax) = {med["aw"] / med["ax"]:.4f}, (aw) / (az) = '
        f'{med["aw"] / med["az"]:.4f}; (av) has the bits of (dv), (ay) those of (dy), (aw) those of (ax) and of (az)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (dv) {failed(first["dv"])}, (aw) {failed(first["aw"])}, (ay25) {failed(first["ay25"])}')
    say()
    if PARENT_LIB is not None:
        say(f'gate (DESIGN.md 4.20): (av) against two runs of the parent\'s (dv), (ay) against two of its (dy): {"pass" if passed else "DO NOT pass"}')
        say()
    say('# examples/camera_loop.py --latency --told (its defaults)')
    for line in example.told_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def predicted_section():
    """(av), (ay) against the parent's; (pv) .. (pz25): see the module docstring."""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import camera_loop as example
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T = 299, 1024
    LAT, AHEAD, PER = example.LATENCIES, example.HORIZONS, 64
    cells = [(d, p) for d in LAT for p in AHEAD]
    TL = len(cells) * PER
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED)
    assert fp.steps == K
    loop = uvs.engine.camera_closed_loop
    say(f'# tools/time_camera.py --predicted on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess); the latencies {LAT} x the horizons '
        f'{AHEAD} x {PER} trials = {TL} trials, every controller told its latency')
    say('# host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
    x0 = uvs.engine.camera_guess(plant, q_d, uvs.engine.camera_features(plant, q_d))
    one = uvs.engine.camera_scenes(plant)
    nominal = uvs.engine.believed_models(plant)
    cam = plant.to_camera(uvs.plant.DISC_RADIUS)
    scene_one = (one.data_ptr(), 1, None), one, None, True           # the nominal camera as the one scene
    null = (None, None)                                              # an operand that is NULL
    four = uvs.engine._latency_operand(np.full(T, 4, np.int32), q_d.device)
    # the experiment: the same 64 starts and noise in each of the 25 cells
    ql = q_d[:PER].repeat(len(cells), 1).contiguous()
    nl = noise[:, :PER].repeat(1, len(cells), 1).contiguous()
    xl = x0[:PER].repeat(len(cells), 1).contiguous()
    latency = np.repeat(np.array([d for d, _ in cells], np.int64), PER)
    ahead = np.repeat(np.array([p for _, p in cells], np.int64), PER)
    parts = [(c, slice(c * PER, (c + 1) * PER)) for c in range(len(cells))]
    cut = (ql[:PER].contiguous(), nl[:, :PER].contiguous(), xl[:PER].contiguous())

    def baseline(entry, *front):                                     # a baseline loop through the C ABI; front: latency, assumed[, predict]
        import ctypes as C
        out = {key: torch.empty((K, T, comp), dtype=torch.float64, device='cuda') for key, comp in (('q', 6), ('f', 8), ('dq', 6), ('err', 8))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.empty((T, 3), dtype=torch.float64, device='cuda'), torch.empty((T, 4), dtype=torch.int32, device='cuda')
        uvs._vision.check(getattr(uvs._vision.lib(), entry)(
            C.byref(fa), one.data_ptr(), 1, None, None, *front, T, nominal.data_ptr(), 1, None, q_d.data_ptr(), noise.data_ptr(), out['q'].data_ptr(),
            out['f'].data_ptr(), out['dq'].data_ptr(), out['err'].data_ptr(), status.data_ptr(), k_done.data_ptr(), stats.data_ptr(),
            pixels.data_ptr(), uvs.engine._stream()))
        return dict(out, pixels=pixels, status=status, k_done=k_done, stats=stats)

    fused = uvs.engine._camera_closed_loop_fused
    logs = uvs.engine.CAMERA_LOGS
    fns = {'av': lambda: fused(fp, cam, q_d, noise, x0, 'host', logs, scenes=scene_one, motion=None, latency=None, assumed=null),
           'pv': lambda: fused(fp, cam, q_d, noise, x0, 'host', logs, scenes=scene_one, motion=None, latency=None, assumed=None, predict=null),
           'ay': lambda: baseline('uvs_camera_believed_loop_aligned_f64', None, None),
           'py': lambda: baseline('uvs_camera_believed_loop_predicted_f64', None, None, None),
           'a4': lambda: fused(fp, cam, q_d, noise, x0, 'host', logs, scenes=scene_one, motion=None, latency=four, assumed=four),
           'p4': lambda: fused(fp, cam, q_d, noise, x0, 'host', logs, scenes=scene_one, motion=None, latency=four, assumed=four, predict=four),
           'ay4': lambda: baseline('uvs_camera_believed_loop_aligned_f64', four[0], four[0]),
           'py4': lambda: baseline('uvs_camera_believed_loop_predicted_f64', four[0], four[0], four[0]),
           'pw': lambda: loop(fp, plant, ql, nl, x0=xl, fused=True, latency=latency, assumed_latency=latency, predict=ahead),
           'px': lambda: [loop(fp, plant, *cut[:2], x0=cut[2], fused=True, latency=d, assumed_latency=d, predict=p) for d, p in cells],
           'py25': lambda: loop(fa, plant, ql, nl, fused=True, latency=latency, assumed_latency=latency, predict=ahead),
           'pz25': lambda: loop(fa, plant, ql, nl, fused=False, latency=latency, assumed_latency=latency, predict=ahead)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b, rows=slice(None), rows_b=slice(None)):
        done = a['k_done'][rows]
        ok = all(torch.equal(a[key][rows], b[key][rows_b]) for key in ('status', 'k_done', 'pixels'))
        ok = ok and torch.equal(a['stats'][rows].view(torch.int64), b['stats'][rows_b].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):                 # the specified rows: q, f up to and including k_done, the others before it
            if key in a:
                spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
                ok = ok and torch.equal(a[key][:, rows].view(torch.int64)[spec], b[key][:, rows_b].view(torch.int64)[spec])
        return ok

    assert same(first['pv'], first['av']), 'the predicted kernel without a horizon and the aligned kernel disagree'
    assert same(first['py'], first['ay']), 'the predicted baseline without a horizon and the aligned baseline disagree'
    assert same(first['py25'], first['pz25']), "the baseline's one launch and its stepwise loop disagree"
    for c, rows in parts:
        assert same(first['pw'], first['px'][c], rows), f'cell {cells[c]}: the one launch and the launch per cell disagree'
    assert not same(first['pw'], first['px'][0], parts[1][1]), 'predicting shows'
    assert not same(first['p4'], first['a4']) and not same(first['py4'], first['ay4']), 'predicting shows'
    compared = {'pv': 'av', 'py': 'ay'}
    if PARENT_LIB is not None:
        parent = ctypes.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')

        def with_parent(fn):
            def run():
                mine, uvs._vision._lib = uvs._vision._lib, parent
                try:
                    return fn()
                finally:
                    uvs._vision._lib = mine
            return run

        for name in ('av', 'ay', 'a4', 'ay4'):
            run = with_parent(fns[name])
            old = run()
            torch.cuda.synchronize()
            assert same(first[name], old), f'this library and the parent disagree on ({name})'
            fns[name + '_parent_a'], fns[name + '_parent_b'] = run, with_parent(fns[name])
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'av': 'aligned_frames_kernel, NULL, NULL', 'pv': "(av)'s trials through predicted_frames_kernel, NULL x 3",
            'ay': 'aligned_baseline_kernel, NULL, NULL', 'py': "(ay)'s trials through predicted_baseline_kernel, NULL x 3",
            'a4': 'aligned_frames_kernel, d = a = 4', 'p4': 'predicted_frames_kernel, d = a = p = 4',
            'ay4': 'aligned_baseline_kernel, d = a = 4', 'py4': 'predicted_baseline_kernel, d = a = p = 4'}
    for new, old in (('pv', 'av'), ('py', 'ay'), ('p4', 'a4'), ('py4', 'ay4')):
        say(f'  ({old}) {what[old]:58s} this library   {fmt_ms(ms[old])}   = {med[old] / K * 1e3:.1f} us per step')
        say(f'  ({new}) {what[new]:58s} this library   {fmt_ms(ms[new])}   = {med[new] / K * 1e3:.1f} us per step')
        if PARENT_LIB is not None:
            a, b = med[old + '_parent_a'], med[old + '_parent_b']
            say(f'  ({old}) {"":58s} the parent\'s, 1  {fmt_ms(ms[old + "_parent_a"])}')
            say(f'  ({old}) {"":58s} the parent\'s, 2  {fmt_ms(ms[old + "_parent_b"])}')
            say(f'  ({new}) / slower parent run of ({old}) = {med[new] / max(a, b):.4f}, / faster = {med[new] / min(a, b):.4f}; the two parent runs differ '
                f'by {abs(a - b) / max(a, b) * 100:.2f} %' + ('; outputs bit-identical' if new in compared else ''))
    say(f'  (pw) {len(LAT)} latencies x {len(AHEAD)} horizons x {PER} trials, one launch                        {fmt_ms(ms["pw"])}   = {med["pw"] / K * 1e3:.1f} us per step')
    say(f'  (px) the same as {len(cells)} launches of {PER} trials, one per cell                      {fmt_ms(ms["px"])}')
    say(f'  (py25) the baseline over the {len(cells)} cells x {PER} trials, one launch                 {fmt_ms(ms["py25"])}')
    say(f'  (pz25) (py25) stepwise: K x (features, delay, gather, two projections, law)  {fmt_ms(ms["pz25"])}')
    say(f'  (pv) / (av) = {med["pv"] / med["av"]:.4f}, (py) / (ay) = {med["py"] / med["ay"]:.4f}, (p4) / (a4) = {med["p4"] / med["a4"]:.4f}, (py4) / (ay4) = '
        f'{med["py4"] / med["ay4"]:.4f}, (pw) / (px) = {med["pw"] / med["px"]:.4f}, (py25) / (pz25) = {med["py25"] / med["pz25"]:.4f}; (pv) has the bits '
        f'of (av), (py) those of (ay), (pw) those of (px), (py25) those of (pz25)')
    failed = lambda out: int((out['k_done'] < K).sum())              # noqa: E731
    say(f'  trials that FAILed: (av) {failed(first["av"])}, (a4) {failed(first["a4"])}, (p4) {failed(first["p4"])}, (pw) {failed(first["pw"])}, '
        f'(py25) {failed(first["py25"])}')
    say()
    say('# examples/camera_loop.py --latency --predict (its defaults)')
    for line in example.predicted_table(uvs):
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


def score_section():
    """(pv) against the parent's; (lv), (lx), (cj), (cs): see the module docstring."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import camera_loop as example
    import kernel_resources
    plant = uvs.SyntheticPlant.ur10()
    rng = np.random.default_rng(2025)
    K, T, m, n = 299, 1024, 8, 6
    fp = uvs.engine.make_params(m, n, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
    assert fp.steps == K
    say(f'# tools/time_camera.py --score on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
        f'{uvs.lib().uvs_version().decode()}')
    say(f'# GMCKF, {T} trials x {K} steps, white noise 0.3 px, x0 handed in (the nominal model\'s guess), the nominal camera as the one scene, every '
        f'optional operand NULL, all five logs')
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
    q[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
    q_d = torch.as_tensor(q, device='cuda')
    noise = torch.as_tensor(rng.standard_normal((K, T, m)) * 0.3, device='cuda')
    f0 = uvs.engine.camera_features(plant, q_d)
    x0 = uvs.engine.camera_guess(plant, q_d, f0)
    one = uvs.engine.camera_scenes(plant)

    def loop(library, entry, x=None):                                # a one-launch estimator loop through the C ABI, its logs allocated here
        f64 = dict(dtype=torch.float64, device='cuda')
        out = {key: torch.empty((K, T, comp), **f64) for key, comp in (('q', n), ('f', m), ('dq', n), ('err', m), ('kappa', m))}
        status, k_done = (torch.empty(T, dtype=torch.int32, device='cuda') for _ in range(2))
        stats, pixels = torch.empty((T, 3), **f64), torch.empty((T, 4), dtype=torch.int32, device='cuda')
        logs = [out[key].data_ptr() for key in ('q', 'f', 'dq', 'err', 'kappa')]
        if x is not None:
            if x:
                out['x'] = torch.empty((K, T, m * n), **f64)
            logs.append(out['x'].data_ptr() if x else None)
        uvs._vision.check(getattr(library, entry)(C.byref(fp), one.data_ptr(), 1, None, None, None, None, None, T, None, None, None, 0, 0, q_d.data_ptr(),
                                                  noise.data_ptr(), x0.data_ptr(), f0.data_ptr(), *logs, status.data_ptr(), k_done.data_ptr(),
                                                  stats.data_ptr(), pixels.data_ptr(), None, uvs.engine._stream()))
        return dict(out, pixels=pixels, status=status, k_done=k_done, stats=stats)

    mine = uvs._vision.lib()
    fns = {'pv': lambda: loop(mine, 'uvs_camera_closed_loop_predicted_f64'),
           'lv': lambda: loop(mine, 'uvs_camera_closed_loop_logged_f64', False),
           'lx': lambda: loop(mine, 'uvs_camera_closed_loop_logged_f64', True)}
    first = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()

    def same(a, b):
        done = a['k_done']
        ok = all(torch.equal(a[key], b[key]) for key in ('status', 'k_done', 'pixels')) and torch.equal(a['stats'].view(torch.int64), b['stats'].view(torch.int64))
        for key in ('err', 'q', 'f', 'dq', 'kappa'):
            spec = torch.arange(K, device='cuda')[:, None] < (done[None, :] + (1 if key in ('q', 'f') else 0))
            ok = ok and torch.equal(a[key].view(torch.int64)[spec], b[key].view(torch.int64)[spec])
        return ok

    assert same(first['lv'], first['pv']) and same(first['lx'], first['pv']), 'the logged kernel and the predicted kernel disagree'
    if PARENT_LIB is not None:
        parent = C.CDLL(os.path.abspath(PARENT_LIB))
        for name, (res, args) in uvs._vision.SYMBOLS.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
        say(f'# parent library: {parent.uvs_vision_version().decode()}')
        assert same(loop(parent, 'uvs_camera_closed_loop_predicted_f64'), first['pv']), 'this library and the parent disagree on (pv)'
        fns['pv_parent_a'] = fns['pv_parent_b'] = lambda: loop(parent, 'uvs_camera_closed_loop_predicted_f64')
        fns['pv_parent_b'] = lambda: loop(parent, 'uvs_camera_closed_loop_predicted_f64')
    say('# (pv), (lv), (lx): host clock around synchronised calls, alternating blocks in one process, allocation of the logs included; medians of 20')
    ms = wall_alternate(fns, rounds=5, block=4)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say()
    what = {'pv': 'predicted_frames_kernel, NULL x 4', 'lv': "(pv)'s trials through logged_frames_kernel, x_log = NULL",
            'lx': f'the same with the log: {K * T * m * n * 8 / 1e6:.0f} MB of X'}
    for name in ('pv', 'lv', 'lx'):
        say(f'  ({name}) {what[name]:58s} this library   {fmt_ms(ms[name])}   = {med[name] / K * 1e3:.1f} us per step')
    if PARENT_LIB is not None:
        a, b = med['pv_parent_a'], med['pv_parent_b']
        say(f'  (pv) {"":58s} the parent\'s, 1  {fmt_ms(ms["pv_parent_a"])}')
        say(f'  (pv) {"":58s} the parent\'s, 2  {fmt_ms(ms["pv_parent_b"])}')
        say(f'  the two parent runs differ by {abs(a - b) / max(a, b) * 100:.2f} %; (pv) new / slower parent run = {med["pv"] / max(a, b):.4f}, / faster = '
            f'{med["pv"] / min(a, b):.4f}; outputs bit-identical')
        for name in ('lv', 'lx'):
            say(f'  ({name}) / slower parent run of (pv) = {med[name] / max(a, b):.4f}, / faster = {med[name] / min(a, b):.4f}')
    say(f'  (lv) / (pv) = {med["lv"] / med["pv"]:.4f}: the price of the text; (lx) / (lv) = {med["lx"] / med["lv"]:.4f}, (lx) / (pv) = '
        f'{med["lx"] / med["pv"]:.4f}: the price of the log; (lv) and (lx) have the bits of (pv) in every other output')
    say(f'  trials that FAILed: {int((first["pv"]["k_done"] < K).sum())}')
    say()
    out = first['lx']
    j_out = torch.empty((K, T, m, n), dtype=torch.float64, device='cuda')
    kw = {key: out[key] for key in ('x', 'q', 'dq', 'k_done')}
    us = alternate({'cj': lambda: uvs.engine.camera_jacobian(plant, out['q'], out=j_out),
                    'cs': lambda: uvs.engine.camera_jacobian_score(plant=plant, dt=fp.dt, **kw)}, rounds=5, block=20, warm=5)
    moved = {'cj': K * T * 8 * (n + m * n), 'cs': K * T * 8 * (m * n + 2 * n + 6)}
    say(f'# (cj), (cs): HIP events around the engine calls (four lanes per record, one per disc), alternating blocks, {K * T} records')
    for name, label in (('cj', 'engine.camera_jacobian over the q log'), ('cs', 'engine.camera_jacobian_score over the x, q and dq logs')):
        mid = float(np.median(us[name]))
        say(f'  ({name}) {label:58s} {fmt(us[name])}   {moved[name] / 1e6:.0f} MB, {moved[name] / mid / 1e3:.0f} GB/s')
    say()
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    say('# registers, LDS and scratch of the new kernels next to the predicted namesakes (tools/kernel_resources.py)')
    short = lambda name: name.split('(')[0].replace('uvs_vision::', '').replace('void ', '')   # noqa: E731
    for name, r in sorted(k.items()):
        if 'logged_frames_kernel' in name:
            twin = k[name.replace('logged_frames_kernel', 'predicted_frames_kernel').replace('LoggedLoopArgs', 'PredictedLoopArgs')]
            say(f'  {short(name):44s} vgpr {r["vgpr"]:3d}  agpr {r["agpr"]:3d}  sgpr {r["sgpr"]:3d}  scratch {r["scratch"]} B  LDS {r["lds"]:5d} B   '
                f'(predicted: vgpr {twin["vgpr"]:3d}  agpr {twin["agpr"]:3d}  sgpr {twin["sgpr"]:3d}  scratch {twin["scratch"]} B  LDS {twin["lds"]:5d} B)')
        elif 'image_jacobian_kernel' in name or 'jacobian_score_kernel' in name:
            say(f'  {short(name):44s} vgpr {r["vgpr"]:3d}  agpr {r["agpr"]:3d}  sgpr {r["sgpr"]:3d}  scratch {r["scratch"]} B  LDS {r["lds"]:5d} B')
    say()
    say('# examples/camera_loop.py --score (its defaults)')
    for line in example.score_table(uvs):
        say(line)
    for flags, kwargs in (('--latency', dict(latency=True)), ('--moving', dict(moving=True)), ('--scenes 8', dict(n_scenes=8))):
        say()
        say(f'# examples/camera_loop.py --score {flags}')
        for line in example.score_table(uvs, **kwargs):
            say(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write('\n'.join(lines) + '\n')


if SCORE:
    score_section()
    sys.exit(0)
if PREDICTED:
    predicted_section()
    sys.exit(0)
if ALIGNED:
    aligned_section()
    sys.exit(0)
if DELAYED:
    delayed_section()
    sys.exit(0)
if MOVING:
    moving_section()
    sys.exit(0)
if SCENES:
    scenes_section()
    sys.exit(0)
if PAINTED:
    painted_section()
    sys.exit(0)
if HELD:
    held_section()
    sys.exit(0)
if OCCLUDED:
    occluded_section()
    sys.exit(0)
if GRID:
    grid_section()
    sys.exit(0)
if BELIEVED:
    believed_section()
    sys.exit(0)
if ANALYTICAL:
    analytical_section()
    sys.exit(0)

plant = uvs.SyntheticPlant.ur10()
cam = plant.to_camera()                              # the uvs_camera struct, built once: the wrappers take it in place of the plant
rng = np.random.default_rng(2025)
say(f'# tools/time_camera.py on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
    f'{uvs.lib().uvs_version().decode()}')
say(f'# (a)-(c): HIP events, medians of {ROUNDS} x {BLOCK} iterations in alternating blocks after {WARM} warm-up calls; discs of radius '
    f'{uvs.plant.DISC_RADIUS} m seen from joints within 0.05 rad of the goal pose')
say()
ok = True
for T in (1, 64, 4096):
    q = torch.as_tensor(Q_GOAL + rng.uniform(-0.05, 0.05, (T, 6)), device='cuda')
    discs = uvs.engine.camera_project(cam, q)
    frames = torch.empty((T, 256, 256, 3), dtype=torch.uint8, device='cuda')
    f_a, f_b, f_c = (torch.empty((T, 8), dtype=torch.float64, device='cuda') for _ in range(3))

    def run_a():
        uvs.engine.render_discs(discs, out=frames)
        uvs.engine.detect_circles(frames, out=f_a)

    us = alternate({'a': run_a, 'b': lambda: uvs.engine.disc_features(discs, out=f_b), 'c': lambda: uvs.engine.camera_features(cam, q, out=f_c)})
    torch.cuda.synchronize()
    same = torch.equal(f_a.view(torch.int64), f_b.view(torch.int64)) and torch.equal(f_b.view(torch.int64), f_c.view(torch.int64))
    assert bool(torch.isfinite(f_a).all()) and same, 'the three routes disagree'
    a, b = stats(us['a'])[0], stats(us['b'])[0]
    ok = ok and b < a
    say(f'T = {T}')
    say(f'  (a) render_discs + detect_circles (frames in HBM)  {fmt(us["a"])}')
    say(f'  (b) disc_features (no frame)                       {fmt(us["b"])}')
    say(f'  (c) camera_features (from the joints, one launch)  {fmt(us["c"])}')
    say(f'  (b) / (a) = {b / a:.3f}: (b) is {"BELOW" if b < a else "NOT below"} (a); features of (a), (b), (c) bit-identical')
say()
say(f'acceptance: (b) below (a) at every T: {"yes" if ok else "NO"}')

# ---- (d) the loop through pixels, wall clock
T, K = 1024, 299
fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, True)
assert fp.steps == K
q0 = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (T, 1))
q0[:, :2] += rng.uniform(-0.1, 0.0, (T, 2))
q0_d = torch.as_tensor(q0, device='cuda')
noise = torch.as_tensor(rng.standard_normal((K, T, 8)) * 0.3, device='cuda')
noise_kct = noise.permute(0, 2, 1).contiguous()                      # closed_loop's default layout [step][component][trial]


out = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise)
torch.cuda.synchronize()
ms_pixels = wall(lambda: uvs.engine.camera_closed_loop(fp, plant, q0_d, noise))
# the same with the initial guess handed in: what is left is the loop itself (2 K launches, their ctypes calls, the logs' allocation)
f0 = uvs.engine.camera_features(plant, q0_d).cpu().numpy()
robot, x0 = uvs.SyntheticRobot(plant, 0.05), np.empty((T, 48))
for t in range(T):
    robot.start(q0[t])
    x0[t] = uvs.plant.analytic_guess(robot, f0[t], (256, 256), 8, 6)
x0_d = torch.as_tensor(x0, device='cuda')
given = uvs.engine.camera_closed_loop(fp, plant, q0_d, noise, x0=x0_d)
assert all(torch.equal(given[key].view(torch.int64), out[key].view(torch.int64)) for key in ('err', 'q', 'f', 'dq'))
ms_loop = wall(lambda: uvs.engine.camera_closed_loop(fp, plant, q0_d, noise, x0=x0_d))
ideal = uvs.engine.closed_loop(fp, plant.to_struct(), q0_d, noise_kct, want=('err', 'q'))
ms_ideal = wall(lambda: uvs.engine.closed_loop(fp, plant.to_struct(), q0_d, noise_kct, want=('err', 'q')))
say()
say(f'(d) T = {T}, K = {K}, GMCKF, white noise 0.3 px; wall clock of {len(ms_pixels)} runs after one warm-up run, host work (analytic guess per trial, '
    'allocation) included')
say(f'  camera_closed_loop (through pixels, 2 launches per step)   median {np.median(ms_pixels):9.1f} ms   (min {min(ms_pixels):.1f}, max {max(ms_pixels):.1f})'
    f'   = {np.median(ms_pixels) / K * 1e3:.1f} us per step')
say(f'  the same with x0 handed in (the loop alone)                median {np.median(ms_loop):9.1f} ms   (min {min(ms_loop):.1f}, max {max(ms_loop):.1f})'
    f'   = {np.median(ms_loop) / K * 1e3:.1f} us per step')
say(f'  closed_loop (ideal features, plant in the kernel; context) median {np.median(ms_ideal):9.1f} ms   (min {min(ms_ideal):.1f}, max {max(ms_ideal):.1f})')
done = out['k_done'].cpu().numpy()
say(f'  through pixels: {int((out["status"] == 0).sum())} of {T} trials SUCCESS, smallest mask {int(out["pixels"].min())} px; '
    f'median ISE / IAE / ITAE {np.median(out["stats"].cpu().numpy()[done == K], axis=0).round(3).tolist()}')
say(f'  ideal features: {int((ideal["status"] == 0).sum())} of {T} trials SUCCESS; '
    f'median ISE / IAE / ITAE {np.median(ideal["stats"].cpu().numpy(), axis=0).round(3).tolist()}')


# ---- (e)-(g) the same loop as one launch, against (d) in alternating blocks
loop = uvs.engine.camera_closed_loop
fused = loop(fp, plant, q0_d, noise, x0=x0_d, fused=True)
torch.cuda.synchronize()
same = all(torch.equal(fused[key].view(torch.int64), given[key].view(torch.int64)) for key in ('err', 'q', 'f', 'dq', 'kappa', 'stats'))
same = same and all(torch.equal(fused[key], given[key]) for key in ('status', 'k_done', 'pixels'))
assert same, 'the one-launch loop and the two-launch loop disagree'
ms = wall_alternate({'d_loop': lambda: loop(fp, plant, q0_d, noise, x0=x0_d),
                     'e': lambda: loop(fp, plant, q0_d, noise, x0=x0_d, fused=True),
                     'g': lambda: loop(fp, plant, q0_d, noise, x0=x0_d, fused=True, want=()),
                     'f': lambda: loop(fp, plant, q0_d, noise, fused=True, guess='device')})
ms_called = wall_alternate({'d_called': lambda: loop(fp, plant, q0_d, noise)}, rounds=2, block=3)
say()
say(f'(e)-(g) T = {T}, K = {K}, GMCKF, white noise 0.3 px; host clock around synchronised calls, alternating blocks, allocation included')
say(f'  (d) two launches per step, x0 handed in (the loop alone)     {fmt_ms(ms["d_loop"])}')
say(f'  (e) fused=True, x0 handed in (one launch)                    {fmt_ms(ms["e"])}   = {np.median(ms["e"]) / K * 1e3:.1f} us per step')
say(f'  (g) (e) with want=()                                         {fmt_ms(ms["g"])}')
say(f'  (d) two launches per step, as called (host guess per trial)  {fmt_ms(ms_called["d_called"])}')
say(f"  (f) fused=True, guess='device', as called (three launches)   {fmt_ms(ms['f'])}")
e_med, d_med, f_med, dc_med = (float(np.median(v)) for v in (ms['e'], ms['d_loop'], ms['f'], ms_called['d_called']))
say(f'  (e) / (d) the loop alone = {e_med / d_med:.3f}: (e) is {"BELOW" if e_med < d_med else "NOT below"} (d);  '
    f'(f) / (d) as called = {f_med / dc_med:.4f}: (f) is {"BELOW" if f_med < dc_med else "NOT below"} (d)')
say(f'  logs, stats, status, k_done and pixels of (e) and (d): bit-identical; median ISE / IAE / ITAE of (e) '
    f'{np.median(fused["stats"].cpu().numpy()[done == K], axis=0).round(3).tolist()}, of (d) '
    f'{np.median(given["stats"].cpu().numpy()[done == K], axis=0).round(3).tolist()}')
for T_other in (64, 4096):
    q_o = torch.as_tensor(q0[np.arange(T_other) % T] + rng.uniform(-0.01, 0.01, (T_other, 6)), device='cuda')
    noise_o = torch.as_tensor(rng.standard_normal((K, T_other, 8)) * 0.3, device='cuda')
    x0_o = uvs.engine.camera_guess(plant, q_o, uvs.engine.camera_features(plant, q_o))
    ms_o = wall_alternate({'d_loop': lambda: loop(fp, plant, q_o, noise_o, x0=x0_o), 'e': lambda: loop(fp, plant, q_o, noise_o, x0=x0_o, fused=True)},
                          rounds=3, block=3)
    say(f'  T = {T_other:5d}: (d) the loop alone {fmt_ms(ms_o["d_loop"])};  (e) {fmt_ms(ms_o["e"])}')

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, 'w').write('\n'.join(lines) + '\n')
