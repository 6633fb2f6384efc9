#!/usr/bin/env python3
"""Time the circle detector of the live route on the host and on the device, in one run on one GPU box:
  (a) host utils.detect4Circles per 256x256 frame;
  (b) step_host fed by (a): the loop iteration of Experiment.run() with an external robot and perception='host';
  (c) FilterBank.step_image per iteration at T = 1 and T = 64, frames in pinned host memory (and, at T = 1, a numpy frame that the
      bank copies into its pinned buffer first: what Experiment hands over with perception='device');
  (d) engine.detect_circles with the frames resident in HBM at T = 1, 64 and 4 096: HIP-event time and the achieved GB/s against the
      196 608 B per frame the kernel has to read.
(a)-(c) are host clocks around calls that end in a stream synchronisation, taken in alternating blocks so that all see the same machine
state; every figure is the median of at least 200 iterations after a warm-up, with the 10th and 90th percentile.  Also counts how many
feature values of the fixture scenes and of the timing scenes are bit-equal to the host detector's.
Writes profiles/detect_device.txt (or the path given).  usage: tools/time_detect.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uvs_amd as uvs  # noqa: E402
import torch  # noqa: E402
from oracle.plant_ref import render_discs  # noqa: E402  (synthetic camera frames: test infrastructure)

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'detect_device.txt')
ROUNDS, BLOCK, WARM = 5, 50, 20                      # 250 timed iterations per figure, in 5 alternating blocks
FRAME_BYTES = 256 * 256 * 3
ORDER = ('red', 'green', 'blue', 'pink')
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


def scene(rng):
    slots = rng.permutation(9)[:4]
    centres = {c: (64.0 * (s % 3) + 64 + rng.uniform(-12, 12), 64.0 * (s // 3) + 64 + rng.uniform(-12, 12)) for c, s in zip(ORDER, slots)}
    return render_discs(centres, {c: rng.uniform(4.0, 9.0) for c in ORDER}, soften=True)


def bit_equal(name, frames):
    with np.errstate(all='ignore'):
        host = np.stack([uvs.utils.detect4Circles(f) for f in frames])
    dev = uvs.utils.detect4Circles_device(frames)
    same = int(np.sum((dev == host) | (np.isnan(dev) & np.isnan(host))))
    say(f'  {name:34s} {"all" if same == dev.size else same} of {dev.size} values bit-equal, max |diff| '
        f'{np.nanmax(np.abs(dev - host), initial=0.0):.3e} px')


rng = np.random.default_rng(2025)
pool = np.stack([scene(rng) for _ in range(64)])
desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, desired, False, 0, 0)
say(f'# tools/time_detect.py on {torch.cuda.get_device_name(0)}; {uvs._vision.lib().uvs_vision_version().decode()}; '
    f'{uvs.lib().uvs_version().decode()}')
say(f'# medians of {ROUNDS} x {BLOCK} iterations in alternating blocks after {WARM} warm-up calls; host clock around calls that end in a '
    'stream synchronisation')

say('bit-equality against the host detector (gate 1e-11 px)')
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'detect_circles.npz'))
fixture = np.stack([render_discs({c: (G['cu'][i, j], G['cv'][i, j]) for j, c in enumerate(ORDER)}, {c: G['radius'][i, j] for j, c in enumerate(ORDER)},
                                 soften=bool(G['soften'][i])) for i in range(len(G['f4']))])
bit_equal('14 fixture scenes', fixture)
bit_equal('64 timing scenes', pool)
half = np.full((256, 256, 3), 96, np.uint8)
half[:, :128], half[:128, 128:], half[128:, 128:192], half[128:, 192:] = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 0, 255)
noisy = (rng.integers(0, 2, (256, 256, 3)) * 255).astype(np.uint8)
bit_equal('half-frame blobs + random 0/255', np.stack([half, noisy]))

# ---- (a), (b), (c): per loop iteration, T = 1
banks = {k: uvs.engine.FilterBank(fp, 1, rng.standard_normal((1, 48)) * 40.0) for k in ('b', 'c_pinned', 'c_numpy')}
pinned = torch.from_numpy(pool).pin_memory()
state = dict(f=np.zeros(8), k=0)


def iter_a(i):
    return uvs.utils.detect4Circles(pool[i % len(pool)])


def iter_b(i):
    f_old = state['f']
    state['f'] = f = uvs.utils.detect4Circles(pool[i % len(pool)])
    return banks['b'].step_host(f, f_old, i % 299)


def iter_c_pinned(i):
    return banks['c_pinned'].step_image(pinned[i % len(pool)], i % 299)


def iter_c_numpy(i):
    return banks['c_numpy'].step_image(pool[i % len(pool)], i % 299)


def alternate(fns, rounds=ROUNDS, block=BLOCK, warm=WARM):
    us = {name: [] for name in fns}
    for name, fn in fns.items():
        for i in range(warm):
            fn(i)
    n = 0
    for _ in range(rounds):
        for name, fn in fns.items():
            for i in range(block):
                t0 = time.perf_counter()
                fn(n + i)
                us[name].append((time.perf_counter() - t0) * 1e6)
        n += block
    return us


us = alternate({'a': iter_a, 'b': iter_b, 'c_pinned': iter_c_pinned, 'c_numpy': iter_c_numpy})
say()
say('per loop iteration, T = 1')
say(f'  (a) host detect4Circles                         {fmt(us["a"])}')
say(f'  (b) host detect4Circles + step_host             {fmt(us["b"])}')
say(f'  (c) step_image, frame in pinned memory          {fmt(us["c_pinned"])}')
say(f'  (c) step_image, numpy frame (copied to pinned)  {fmt(us["c_numpy"])}')
b, c, cn = stats(us['b'])[0], stats(us['c_pinned'])[0], stats(us['c_numpy'])[0]
say(f'  (c) pinned / (b) = {c / b:.4f}, (c) numpy / (b) = {cn / b:.4f}: step_image is {"BELOW" if max(c, cn) < b else "NOT below"} the host route')

# ---- (c) at T = 64 against 64 host detections + one step_host
T = 64
bank_h, bank_d = (uvs.engine.FilterBank(fp, T, rng.standard_normal((T, 48)) * 40.0) for _ in range(2))
state64 = dict(f=np.zeros((T, 8)))


def iter_b64(i):
    f_old = state64['f']
    state64['f'] = f = np.stack([uvs.utils.detect4Circles(img) for img in pool])
    return bank_h.step_host(f, f_old, i % 299)


def iter_c64(i):
    return bank_d.step_image(pinned, i % 299)


us64 = alternate({'c64': iter_c64})
us64.update(alternate({'b64': iter_b64}, rounds=2, block=10, warm=2))   # 64 x (a) per iteration: 20 iterations say enough
say()
say('per loop iteration, T = 64')
say(f'  (b) 64 x host detect4Circles + step_host        {fmt(us64["b64"])}')
say(f'  (c) step_image, frames in pinned memory         {fmt(us64["c64"])}')
say(f'      = {stats(us64["c64"])[0] / T:.1f} us per frame; {T * FRAME_BYTES / stats(us64["c64"])[0] / 1e3:.1f} GB/s over the host link, step included')

# ---- (d) detector alone, frames in HBM, HIP events
say()
say('(d) engine.detect_circles, frames resident in HBM, HIP events (250 launches each after 20 warm-up launches)')
for T in (1, 64, 4096):
    frames = torch.from_numpy(pool).cuda().repeat((T + len(pool) - 1) // len(pool), 1, 1, 1)[:T].contiguous()
    out = torch.empty((T, 8), dtype=torch.float64, device='cuda')
    for _ in range(20):
        uvs.engine.detect_circles(frames, out=out)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(250)]
    for e0, e1 in ev:
        e0.record()
        uvs.engine.detect_circles(frames, out=out)
        e1.record()
    torch.cuda.synchronize()
    t_us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    med = stats(t_us)[0]
    say(f'  T = {T:5d}  {fmt(t_us)}   {med / T:8.3f} us per frame   {T * FRAME_BYTES / med / 1e3:8.1f} GB/s read')
    assert torch.isfinite(out).all()

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
open(OUT, 'w').write('\n'.join(lines) + '\n')
