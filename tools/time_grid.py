#!/usr/bin/env python3
"""What a hyperparameter grid costs in one launch (uvs_rmckf_closed_loop_grid_f64) against the launches it replaces.  For RMCKF and MCKF and grids of
H cells x 128 trials (H = 64, 128, 512: 8 192, 16 384 and 65 536 trials), reference config at alpha = 1.5, per-trial statistics only (no streams):
  (a) the grid launch: per-trial kernel_bw x gain, inputs of 128 trials read through `source`;
  (b) the same cells as H uniform launches through one set of buffers (lanes_per_filter 0: what a user would call today);
  (c) ONE uniform launch of the same T trials on the same lane mapping as (a) (two lanes per filter), inputs of T physical trials.
  (d) the per-trial kernel on the inputs and launch-wide values of (c) (every member of uvs_trial_params NULL): the same arithmetic as (c), so
      (d) / (c) is what the kernel itself costs; (a) / (c) also contains whatever the grid's parameters change in the work (MCKF iterates more in
      narrow-bandwidth cells) and the smaller input footprint of `source`.
(b) / (a) is the feature's gain, (a) / (c) the price of per-trial parameters.  HIP events, inputs resident, everything warmed up, the three versions
alternated `--reps` times in one process; medians, and the run-to-run spread (max - min) / median of (c).
usage: tools/time_grid.py [--reps 5] [--out profiles/r09/grid_time.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09', 'grid_time.json'))
    ap.add_argument('--sizes', type=int, nargs='*', default=[64, 128, 512])
    args = ap.parse_args()
    import torch
    import uvs_amd as uvs
    E = 128
    cfg = uvs.batch.load_config(os.path.join(ROOT, 'examples', 'config.json'))
    ex, p = cfg['experiments'], cfg['estimator']['estimator_params']
    plan = uvs.batch.plan_trials(cfg, [1.5], E)
    K = len(uvs.engine.loop_clock(ex['dt'], ex['t_max']))
    noise = uvs.batch.device_noise(cfg, plan, 0, E, K).contiguous()
    q0 = torch.as_tensor(plan.q_start.copy(), device='cuda')
    plant = uvs.SyntheticPlant.ur10(ex['desired_f']).to_struct()
    doc = {'workload': f'reference config, alpha = 1.5, {E} trials per grid cell, {K} steps, statistics only', 'device': torch.cuda.get_device_name(0),
           'library_version': uvs.lib().uvs_version().decode(), 'reps': args.reps, 'results': []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for method in ('GMCKF', 'MCKF'):
        mk = lambda lanes, bw=p['kernel_bw'], gain=ex['ibvs_gain']: uvs.engine.make_params(   # noqa: E731
            8, 6, method, bw, p['annealing'], ex['dt'], ex['t_max'], gain, ex['desired_f'], True, lanes, None, p['fpi_threshold'], p['fpi_epoch_max'])
        for H in args.sizes:
            T = H * E
            ng = 2 ** int(np.log2(np.sqrt(H / 2)))                   # kernel_bw x gain, 2 : 1 or 4 : 1 (H a power of two)
            cells = [(b, g) for b in np.linspace(2.0, 33.0, H // ng) for g in np.linspace(0.05, 0.425, ng)]
            assert len(cells) == H
            tp = dict(kernel_bw=torch.as_tensor(np.repeat([c[0] for c in cells], E), device='cuda'),
                      gain=torch.as_tensor(np.repeat([c[1] for c in cells], E), device='cuda'),
                      source=torch.as_tensor((np.arange(T) % E).astype(np.int32), device='cuda'))
            fp_grid, fp_one = mk(0), mk(2)
            fps = [mk(0, b, g) for b, g in cells]
            q_all, nz_all = q0.repeat(H, 1), noise.repeat(1, 1, H)
            buf = uvs.engine.closed_loop(fp_grid, plant, q0, noise, want=(), trial_params=tp)      # one set of buffers for all three (T trials)
            run_a = lambda: uvs.engine.closed_loop(fp_grid, plant, q0, noise, want=(), reuse=buf, trial_params=tp)          # noqa: E731
            run_c = lambda: uvs.engine.closed_loop(fp_one, plant, q_all, nz_all, want=(), reuse=buf)                        # noqa: E731

            run_d = lambda: uvs.engine.closed_loop(fp_one, plant, q_all, nz_all, want=(), reuse=buf, trial_params={})      # noqa: E731

            def run_b():
                for f in fps:
                    uvs.engine.closed_loop(f, plant, q0, noise, want=(), reuse=buf)
            for fn in (run_a, run_b, run_c, run_d):                   # warm-up
                fn()
            torch.cuda.synchronize()
            ms = {'a': [], 'b': [], 'c': [], 'd': []}
            for _ in range(args.reps):
                for key, fn in (('a', run_a), ('b', run_b), ('c', run_c), ('d', run_d)):
                    ms[key].append(timed(fn))
            med = {k_: float(np.median(v)) for k_, v in ms.items()}
            spread_c = (max(ms['c']) - min(ms['c'])) / med['c']
            row = {'method': method, 'grid_cells': H, 'trials': T, 'grid_launch_ms': med['a'], 'uniform_launches_ms': med['b'], 'one_uniform_launch_ms': med['c'],
                   'grid_kernel_uniform_values_ms': med['d'], 'gain_b_over_a': med['b'] / med['a'], 'price_a_over_c': med['a'] / med['c'], 'kernel_price_d_over_c': med['d'] / med['c'],
                   'spread_c': spread_c,
                   'segments_grid': int(uvs.lib().uvs_rmckf_closed_loop_segments(ctypes.byref(fp_grid), ctypes.byref(plant), T)), 'samples_ms': ms}
            doc['results'].append(row)
            print(json.dumps({k_: v for k_, v in row.items() if k_ != 'samples_ms'}), flush=True)
            del q_all, nz_all, buf
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        rows = doc.pop('results')                                     # one line per measurement
        fh.write(json.dumps(doc, indent=1)[:-2] + ',\n "results": [\n  ' + ',\n  '.join(json.dumps(r) for r in rows) + '\n ]\n}\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
