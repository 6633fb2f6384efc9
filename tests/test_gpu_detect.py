"""The device circle detector (uvs_detect_circles_u8 of include/uvs_vision.h: engine.detect_circles, FilterBank.step_image, the
``*_device`` functions of utils, Experiment's perception='device') against the host detectors of utils.py, which tests/test_detect.py holds
bit for bit to outputs of the reference itself.

Gate.  The kernel forms S = sum_i count[i] * p[i] over 256 non-negative terms (each product rounded once, then 255 additions: at most 257 u
relative, u = 2^-53); numpy sums the 65 536 products pairwise (about 33 u).  The two differ by under 3.3e-14 relatively, on a pixel
coordinate <= 255 that is under 8.4e-12: the gate is 1e-11 pixel, absolute.  Mask sizes are integers and must be equal.  Every test prints
how many of its values are bit-equal to the host's."""
import os

import numpy as np
import pytest

from conftest import load_golden, rel_err as rel
from oracle import plant_ref
from oracle.plant_ref import render_discs

pytestmark = pytest.mark.gpu

GATE_PX = 1e-11
ORDER = ('red', 'green', 'blue', 'pink')
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'detect_circles.npz'))
SIDE, DENSE = 256, 256 * 256 * 3


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    uvs_amd.lib()
    uvs_amd._vision.lib()
    return uvs_amd


@pytest.fixture(scope='module')
def scenes():
    """The 14 fixture scenes, rendered as tests/test_detect.py renders them: (14, 256, 256, 3) uint8, unflipped."""
    out = []
    for i in range(len(G['f4'])):
        centres = {c: (G['cu'][i, j], G['cv'][i, j]) for j, c in enumerate(ORDER)}
        radii = {c: G['radius'][i, j] for j, c in enumerate(ORDER)}
        out.append(render_discs(centres, radii, soften=bool(G['soften'][i])))
    return np.stack(out)


def host_counts(img):
    """Mask sizes of red, green, blue, pink: the reference's integer thresholds (utils.py:15-24, :130-144), written out independently."""
    r, g, b = (img[:, :, ch].astype(int) for ch in range(3))
    lo, hi = (lambda x: x < 250), (lambda x: x > 250)
    return np.array([(hi(r) & lo(g) & lo(b)).sum(), (lo(r) & hi(g) & lo(b)).sum(), (lo(r) & lo(g) & hi(b)).sum(), (hi(r) & lo(g) & hi(b)).sum()])


def host_f(uvs, frames, n_colours=4):
    fn = {4: uvs.utils.detect4Circles, 3: uvs.utils.detectRGBCircles, 1: uvs.utils.detectGreenCircle}[n_colours]
    with np.errstate(all='ignore'):
        return np.stack([fn(img) for img in frames])


def device_f(uvs, frames, n_colours=4, pinned=False, **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(frames))
    t = t.pin_memory() if pinned else t.cuda()
    out = uvs.engine.detect_circles(t, n_colours, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def report(name, dev, host):
    same = int(np.sum((dev == host) | (np.isnan(dev) & np.isnan(host))))
    print(f'{name}: {"all" if same == dev.size else same} of {dev.size} values bit-equal to the host detector; '
          f'max |diff| {np.nanmax(np.abs(dev - host), initial=0.0):.3e} px')


def random_scene(rng, colours=ORDER):
    """Discs well inside the frame and apart from each other: every colour present keeps a finite centre of mass."""
    slots = rng.permutation(9)[:len(colours)]                                          # 3 x 3 grid of 64-pixel cells around the centre
    centres = {c: (64.0 * (s % 3) + 64 + rng.uniform(-12, 12), 64.0 * (s // 3) + 64 + rng.uniform(-12, 12)) for c, s in zip(colours, slots)}
    return render_discs(centres, {c: rng.uniform(4.0, 9.0) for c in colours}, soften=bool(rng.integers(2)))


# ------------------------------------------------------------------------------------------------------------- fixture scenes
@pytest.mark.parametrize('n_colours,key', [(4, 'f4'), (3, 'f3'), (1, 'f1')])
def test_fixture_scenes_in_one_batch(uvs, scenes, n_colours, key):
    import torch
    assert np.all(np.isfinite(G[key]))
    pixels = torch.zeros((len(scenes), n_colours), dtype=torch.int32, device='cuda')
    f = device_f(uvs, scenes, n_colours, pixels=pixels)
    report(f'fixture scenes, n_colours={n_colours}', f, G[key])
    assert f.shape == G[key].shape and np.abs(f - G[key]).max() < GATE_PX
    want = np.stack([host_counts(img) for img in scenes])
    want = {4: want, 3: want[:, :3], 1: want[:, 1:2]}[n_colours]
    assert want.min() > 0 and np.array_equal(pixels.cpu().numpy(), want)


def test_wrappers_return_what_the_reference_functions_return(uvs, scenes):
    f4 = uvs.utils.detect4Circles_device(scenes)
    assert isinstance(f4, np.ndarray) and np.abs(f4 - G['f4']).max() < GATE_PX
    one = uvs.utils.detect4Circles_device(scenes[3])
    assert one.shape == (8,) and np.array_equal(one, f4[3])
    assert np.array_equal(uvs.utils.detectRGBCircles_device(scenes[3]), f4[3][:6])
    assert np.array_equal(uvs.utils.detectGreenCircle_device(scenes[3]), f4[3][2:4])


# ------------------------------------------------------------------------------------------------------------- product table
def test_inexact_grid_products_bit_for_bit(uvs):
    """One mask pixel, so one term and no summation order: the result must be the host's bits.  The 24 grid indices whose product
    fl(g[i] * 255) is not the integer i; a kernel that weighs by i, or forgets the vertical flip, fails here."""
    p = np.linspace(0, 1, 256) * np.uint8(255)
    inexact = [i for i in range(256) if p[i] != i]
    assert len(inexact) == 24 and {33, 37, 41} <= set(inexact)
    frames = np.full((2 * len(inexact), SIDE, SIDE, 3), 96, np.uint8)
    for j, i in enumerate(inexact):
        colour = plant_ref.DISC_COLOURS[ORDER[j % 4]]
        frames[2 * j, SIDE - 1 - 7, i] = colour                                       # column i, flipped row 7
        frames[2 * j + 1, SIDE - 1 - i, 11] = colour                                  # flipped row i, column 11
    host, dev = host_f(uvs, frames), device_f(uvs, frames)
    report('single-pixel frames', dev, host)
    for j, i in enumerate(inexact):
        c = j % 4
        assert host[2 * j, 2 * c] != i and host[2 * j + 1, 2 * c + 1] != i and host[2 * j, 2 * c + 1] == 7.0     # weighing by i would show
    assert np.isfinite(host).sum() == 2 * len(frames)
    assert np.array_equal(dev, host, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- threshold edges
def test_threshold_edges(uvs):
    """Channels from {248, ..., 252}, every combination present many times: 250 itself is on neither side, 251 is above, 249 below."""
    import torch
    rng = np.random.default_rng(250)
    combos = np.array([(r, g, b) for r in range(248, 253) for g in range(248, 253) for b in range(248, 253)], np.uint8)
    frame = combos[rng.permutation(SIDE * SIDE) % len(combos)].reshape(SIDE, SIDE, 3)
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) == 125
    want = host_counts(frame)
    assert want.min() > 0
    pixels = torch.zeros((1, 4), dtype=torch.int32, device='cuda')
    f = device_f(uvs, frame[None], pixels=pixels)
    assert np.array_equal(pixels.cpu().numpy()[0], want), (pixels.cpu().numpy()[0], want)
    host = host_f(uvs, frame[None])
    report('threshold-edge frame', f, host)
    assert np.all(np.isfinite(host)) and np.abs(f - host).max() < GATE_PX


# ------------------------------------------------------------------------------------------------------------- missing colour
def test_missing_colour_gives_nan_like_the_reference(uvs):
    frame = render_discs({'red': (50, 50), 'green': (100, 100), 'blue': (150, 150)}, 8.0)
    host, f = host_f(uvs, frame[None])[0], device_f(uvs, frame[None])[0]
    report('three discs, no pink', f, host)
    assert np.all(np.isnan(f[6:])) and np.all(np.isnan(host[6:]))
    assert np.all(np.isfinite(host[:6])) and np.all(np.isfinite(f[:6])) and np.abs(f[:6] - host[:6]).max() < GATE_PX


# ------------------------------------------------------------------------------------------------------------- batch shapes
@pytest.mark.parametrize('T', [1, 3, 5])
def test_batch_shapes_strides_memory_kinds_and_noise(uvs, T):
    import torch
    rng = np.random.default_rng(T)
    frames = np.stack([random_scene(rng) for _ in range(T)])
    host = host_f(uvs, frames)
    assert np.all(np.isfinite(host))
    hbm = device_f(uvs, frames)
    report(f'T={T} random scenes', hbm, host)
    assert np.abs(hbm - host).max() < GATE_PX
    assert np.array_equal(device_f(uvs, frames, pinned=True), hbm), 'pinned host frames and HBM frames give different bits'
    # a padded batch: frame stride 196 608 + 64 B, the gap filled with bytes that would count as red
    for make in (lambda n: torch.empty(n, dtype=torch.uint8, device='cuda'), lambda n: torch.empty(n, dtype=torch.uint8).pin_memory()):
        buf = make(T * (DENSE + 64)).view(T, DENSE + 64)
        buf[:] = torch.tensor([255, 0, 0, 255], dtype=torch.uint8).repeat((DENSE + 64) // 4).to(buf.device)
        view = buf[:, :DENSE].view(T, SIDE, SIDE, 3)
        view.copy_(torch.from_numpy(frames))
        assert T == 1 or view.stride(0) == DENSE + 64
        out = uvs.engine.detect_circles(view)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), hbm)
    # one frame without a batch axis
    assert np.array_equal(uvs.engine.detect_circles(torch.from_numpy(frames[0]).cuda()).cpu().numpy(), hbm[:1])
    # the noise epilogue is f + noise, one rounding
    noise = rng.standard_normal((T, 8))
    noisy = device_f(uvs, frames, noise=torch.from_numpy(noise).cuda())
    assert np.array_equal(noisy, hbm + noise)
    # refusals reach Python as errors
    with pytest.raises(ValueError):
        uvs.engine.detect_circles(torch.from_numpy(frames))                             # pageable host memory: no hidden copy
    with pytest.raises(uvs.UvsError) as exc:
        uvs.engine.detect_circles(torch.zeros((1, 128, 128, 3), dtype=torch.uint8, device='cuda'))
    assert exc.value.code == -2
    with pytest.raises(uvs.UvsError) as exc:
        uvs.engine.detect_circles(torch.from_numpy(frames).cuda(), n_colours=2)
    assert exc.value.code == -1


def test_frames_past_two_gib(uvs):
    """Frame offsets are 64-bit: the last frame of a batch that spans more than 2^31 bytes gives the bits it gives alone."""
    import torch
    T = (1 << 31) // DENSE + 8
    frame = random_scene(np.random.default_rng(31))
    frames = torch.zeros((T, SIDE, SIDE, 3), dtype=torch.uint8, device='cuda')
    frames[-1] = torch.from_numpy(frame).cuda()
    assert (T - 1) * DENSE > 1 << 31
    f = uvs.engine.detect_circles(frames).cpu().numpy()
    alone = device_f(uvs, frame[None])
    assert np.all(np.isfinite(alone)) and np.array_equal(f[-1], alone[0]) and np.all(np.isnan(f[:-1]))


# ------------------------------------------------------------------------------------------------------------- fused step
@pytest.mark.parametrize('T', [1, 3])
def test_fused_step_is_detector_then_step(uvs, T):
    """Five step_image calls against step_host fed the device detection of the same frames with an explicit f_old (same kernels, same
    inputs: same bits) and against step_host fed the host detection (1e-8 relative)."""
    rng = np.random.default_rng(100 + T)
    desired = np.array([149., 145., 125., 121., 101., 145., 125., 169.])
    fp = uvs.engine.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, desired, False, 0, 0)
    x0 = rng.standard_normal((T, 48)) * 40.0
    f0 = host_f(uvs, np.stack([random_scene(rng) for _ in range(T)]))
    fused, explicit, hosted = (uvs.engine.FilterBank(fp, T, x0) for _ in range(3))
    fused.set_features(f0)
    f_dev_old, f_host_old, same, total = f0, f0, 0, 0
    for k in range(5):
        frames = np.stack([random_scene(rng) for _ in range(T)])
        noise = rng.standard_normal((T, 8)) * 0.3 if k % 2 else None
        f_host = host_f(uvs, frames)
        assert np.all(np.isfinite(f_host))
        f_dev = uvs.utils.detect4Circles_device(frames)
        if noise is not None:
            f_host, f_dev = f_host + noise, f_dev + noise
        dq, err, kappa, status, f = fused.step_image(frames if T > 1 else frames[0], k, noise)
        parity = (fused._host['calls'] - 1) & 1
        assert np.array_equal(fused._host['np']['f_old'][parity], f_dev_old), 'f_old of call k is not the f of call k - 1'
        assert np.array_equal(f, f_dev)
        same, total = same + int(np.sum(f == f_host)), total + f.size
        want = explicit.step_host(f_dev, f_dev_old, k)
        for name, a, b in zip(('dq', 'err', 'kappa', 'status'), (dq, err, kappa, status), want):
            assert np.array_equal(a, b), (k, name)
        ref = hosted.step_host(f_host, f_host_old, k)
        assert np.all(np.isfinite(ref[0])) and not np.any(ref[3])
        assert rel(dq, ref[0]) < 1e-8 and rel(err, ref[1]) < 1e-8 and rel(kappa, ref[2]) < 1e-8 and np.array_equal(status, ref[3])
        f_dev_old, f_host_old = f_dev.copy(), f_host.copy()
    print(f'fused step T={T}: {"all" if same == total else same} of {total} feature values bit-equal to the host detector')
    # a pinned tensor is read in place and gives the same bits as the numpy array copied into the bank's buffer
    import torch
    a, b = (uvs.engine.FilterBank(fp, T, x0) for _ in range(2))
    out_np = a.step_image(frames, 0)
    out_pin = b.step_image(torch.from_numpy(frames).pin_memory(), 0)
    for x, y in zip(out_np, out_pin):
        assert np.array_equal(x, y)
    assert np.array_equal(a._host['np']['f_old'][0], np.zeros((T, 8)))                    # no set_features: the reference's f = zeros


# ------------------------------------------------------------------------------------------------------------- drop-in
class CameraUR10(plant_ref.PinholeUR10):
    """The oracle's duck-typed robot with a camera: frames of four discs of fixed radius at its current features."""
    RADIUS = 6.0

    def getCameraImage(self):
        f = self.features()
        centres = {c: (f[2 * j], f[2 * j + 1]) for j, c in enumerate(ORDER)}
        return render_discs(centres, self.RADIUS), (plant_ref.RESOLUTION, plant_ref.RESOLUTION)


def test_experiment_with_device_perception(uvs, monkeypatch):
    g = load_golden('closed_gmckf_a1p5')
    meta = g['meta']
    calls = []
    step_image = uvs.engine.FilterBank.step_image
    monkeypatch.setattr(uvs.engine.FilterBank, 'step_image', lambda self, *a, **kw: (calls.append(1), step_image(self, *a, **kw))[1])

    def run(**kw):
        del calls[:]
        ex = uvs.Experiment(g['q_start'], g['desired'], None, meta['dt'], meta['dt'] * 20.5, meta['gain'], CameraUR10(meta['dt']),
                            uvs.Method.GMCKF, **meta['params'], **kw)
        return ex.run(), len(calls)

    host, n_host = run()
    dev, n_dev = run(perception='device')
    assert len(host[1]) == 20 and n_host == 0 and n_dev == 20, 'the device route did not go through step_image'
    assert np.all(np.isfinite(host[4])), 'a disc left the frame: the comparison would be vacuous'
    assert dev[0] == host[0] == uvs.ExperimentStatus.SUCCESS and len(dev[1]) == len(host[1])
    assert np.array_equal(dev[1], host[1])
    report('drop-in f_log', dev[4], host[4])
    for i, name in ((2, 'err'), (3, 'q'), (4, 'f')):
        assert rel(dev[i], host[i]) < 1e-8, name
