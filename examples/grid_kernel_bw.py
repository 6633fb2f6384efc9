#!/usr/bin/env python3
"""A kernel_bw x ibvs_gain study in one launch per noise cell (batch.run_grid): median ITAE and FAIL count of every grid cell for one estimator, over
the same trials (common random numbers: the seeds and start poses the reference's driver draws), next to the reference's defaults (kernel_bw 10,
gain 0.2, marked *).
usage: examples/grid_kernel_bw.py [--method GMCKF] [--alpha 1.5] [--epoch 100] [--config examples/config.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='GMCKF', choices=('KF', 'MCKF', 'IMCCKF', 'GMCKF'))
    ap.add_argument('--alpha', type=float, default=1.5, help='the swept noise parameter of the one noise cell (alpha, or rho for the other noise types)')
    ap.add_argument('--epoch', type=int, default=100)
    ap.add_argument('--config', default=os.path.join(ROOT, 'examples', 'config.json'))
    ap.add_argument('--kernel-bw', type=float, nargs='*', default=[2, 5, 10, 20, 40])
    ap.add_argument('--gain', type=float, nargs='*', default=[0.1, 0.2, 0.4])
    args = ap.parse_args()
    import uvs_amd as uvs
    cfg = json.load(open(args.config))
    cfg['estimator']['method'] = args.method
    res = uvs.batch.run_grid(cfg, {'kernel_bw': args.kernel_bw, 'ibvs_gain': args.gain}, cells=[args.alpha], epoch=args.epoch)
    summ = res.cell_summary()
    bw0, gain0 = cfg['estimator']['estimator_params']['kernel_bw'], cfg['experiments']['ibvs_gain']
    print(f'{args.method}, {args.epoch} trials per cell, noise parameter {args.alpha}: median ITAE (FAILed trials), one launch of {len(res.grid) * args.epoch} trials, '
          f'{res.seconds * 1e3:.1f} ms with noise generation')
    print('kernel_bw \\ gain' + ''.join(f'{g:>22g}' for g in args.gain))
    for i, bw in enumerate(args.kernel_bw):
        cells = []
        for j, g in enumerate(args.gain):
            s = summ[(0, i * len(args.gain) + j)]
            mark = '*' if (bw == bw0 and g == gain0) else ' '
            cells.append(f'{s["itae_median"]:>14.1f} ({s["trials"] - s["success"]:3d}){mark}')
        print(f'{bw:>16g}' + ''.join(f'{c:>22s}' for c in cells))


if __name__ == '__main__':
    main()
