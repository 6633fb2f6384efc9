#!/usr/bin/env python3
"""What does the camera's pixel grid do to the estimators?  The same small batch of closed-loop trials twice: through engine.closed_loop, which
feeds the estimator the ideal projections of the discs plus noise, and through engine.camera_closed_loop, which feeds it what the centre-of-mass
detector returns for the 256 x 256 frame of those discs (the reference's live route) plus the same noise.  Prints the median ISE / IAE / ITAE of
both, side by side, and the smallest colour mask the detector ever saw.
--fused runs the pixel loop as one launch with the initial guess computed on the device (engine.camera_closed_loop(fused=True, guess='device')).
--baseline answers the question the reference's experiment asks -- what does not knowing the Jacobian cost? -- through pixels: the chosen
estimator and the calibrated control law (Method.ANALYTICAL, fp.method == ANALYTICAL) on the same starts and the same noise, paired trial by
trial over the trials both ran to the end, with the FAIL count of each.
usage: examples/camera_loop.py [--method GMCKF] [--trials 64] [--sigma 0.3] [--radius 0.024] [--seed 0] [--fused] [--baseline]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='GMCKF', choices=('KF', 'MCKF', 'IMCCKF', 'GMCKF'))
    ap.add_argument('--trials', type=int, default=64)
    ap.add_argument('--sigma', type=float, default=0.3, help='standard deviation of the white measurement noise, pixels')
    ap.add_argument('--radius', type=float, default=None, help='physical disc radius in metres (default plant.DISC_RADIUS: about 8 px at the goal)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--fused', action='store_true', help='the pixel loop as one launch, initial guess on the device, no log returned')
    ap.add_argument('--baseline', action='store_true', help='pair the estimator with the calibrated law (ANALYTICAL) through the same pixels')
    args = ap.parse_args()
    import torch
    import uvs_amd as uvs
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
