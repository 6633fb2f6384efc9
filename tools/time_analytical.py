#!/usr/bin/env python3
"""Time the calibrated IBVS baseline (uvs_analytical_closed_loop_f64) at BASELINE config 2 size -- 65 536 trials x 299 steps, alpha-stable
1.5 noise from the device generator -- alternating with the RMCKF launch (GMCKF, sigma 10, default kernel) on the same inputs, HIP events
around each launch.  Both launches log the err stream only (bench.py's headline also logs X and q, hence its longer time).
Writes profiles/r07/analytical_time.json (or the path given).  usage: tools/time_analytical.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uvs_amd as uvs  # noqa: E402
import torch  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r07', 'analytical_time.json')
T, WARM, REPS = 65536, 3, 20
cfg = json.load(open(os.path.join(ROOT, 'examples', 'config.json')))
plan = uvs.batch.plan_trials(cfg, cells=[1.5], epoch=T)
K = len(uvs.engine.loop_clock(0.05, 15))
noise = uvs.batch.device_noise(cfg, plan, 0, T, K)
q0 = torch.as_tensor(plan.q_start.copy(), device='cuda')
plant = uvs.SyntheticPlant.ur10().to_struct()
desired = cfg['experiments']['desired_f']
fa = uvs.engine.make_params(8, 6, 'ANALYTICAL', desired=desired)
fr = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, desired=desired)
ra = uvs.engine.analytical_closed_loop(fa, plant, q0, noise, want=('err',))
rr = uvs.engine.closed_loop(fr, plant, q0, noise, want=('err',))
ms = {'ANALYTICAL': [], 'GMCKF': []}
for i in range(WARM + REPS):
    a = uvs.engine.analytical_closed_loop(fa, plant, q0, noise, want=('err',), reuse=ra)
    r = uvs.engine.closed_loop(fr, plant, q0, noise, want=('err',), reuse=rr)
    torch.cuda.synchronize()
    if i >= WARM:
        ms['ANALYTICAL'].append(a['events'][0].elapsed_time(a['events'][1]))
        ms['GMCKF'].append(r['events'][0].elapsed_time(r['events'][1]))
st = a['status'].cpu().numpy()
# paper counts per trial-step: fp64 operations of plant + Jacobian + least squares; HBM bytes of noise in, err out
flop, byts = 1250, 8 * 8 + 8 * 8
med = {k: float(np.median(v)) for k, v in ms.items()}
steps = T * K
res = dict(trials=T, steps=K, reps=REPS, ms_per_launch=med['ANALYTICAL'], ms_all=ms['ANALYTICAL'], rmckf_ms_per_launch=med['GMCKF'],
           rmckf_ms_all=ms['GMCKF'], ratio_to_rmckf=med['ANALYTICAL'] / med['GMCKF'], trial_steps_per_s=steps / (med['ANALYTICAL'] * 1e-3),
           paper_flop_per_trial_step=flop, paper_bytes_per_trial_step=byts,
           fp64_peak_share=steps * flop / (med['ANALYTICAL'] * 1e-3) / 78.6e12, hbm_share=steps * byts / (med['ANALYTICAL'] * 1e-3) / 8e12,
           fail=int((st == 1).sum()), device=torch.cuda.get_device_name(0), library=uvs.lib().uvs_version().decode())
os.makedirs(os.path.dirname(OUT), exist_ok=True)
json.dump(res, open(OUT, 'w'), indent=1)
print(json.dumps({k: v for k, v in res.items() if not k.endswith('_all')}))
