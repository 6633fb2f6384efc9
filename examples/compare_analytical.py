#!/usr/bin/env python3
"""What does not knowing the Jacobian cost?  One config.json swept twice over the same trial plan -- once with its estimator (GMCKF = the
paper's RMCKF by default), once with the calibrated baseline (Method.ANALYTICAL) -- then per sweep cell the paired differences of the three
error norms over the trials both runs finished, and the FAIL counts.  Same seeds, same q_start jitter, same noise streams in both runs.
    python examples/compare_analytical.py [config.json] [--epoch N]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uvs_amd as uvs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('config', nargs='?', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'config.json'))
ap.add_argument('--epoch', type=int, default=None)
args = ap.parse_args()
cfg = json.load(open(args.config))
est = cfg['estimator']['method'] if cfg['estimator']['method'] != 'ANALYTICAL' else 'GMCKF'
runs = {}
for method in (est, 'ANALYTICAL'):
    c = json.loads(json.dumps(cfg))
    c['estimator']['method'] = method
    runs[method] = uvs.batch.run_sweep(c, epoch=args.epoch)
e, a = runs[est], runs['ANALYTICAL']
print(f'{"cell":>6} {"value":>8} {"FAIL " + est:>12} {"FAIL ANALYT.":>12}   paired mean ({est} - ANALYTICAL) of ||ISE|| ||IAE|| ||ITAE||')
for c in np.unique(e.plan.cell):
    sel = e.plan.cell == c
    both = sel & (e.status == 0) & (a.status == 0)
    d = (e.stats[both] - a.stats[both]).mean(axis=0) if both.any() else np.full(3, np.nan)
    print(f'{c:6d} {e.plan.cells[c]:8.4g} {int((e.status[sel] == 1).sum()):12d} {int((a.status[sel] == 1).sum()):12d}   '
          f'{d[0]:12.5g} {d[1]:12.5g} {d[2]:12.5g}  ({int(both.sum())} pairs)')
