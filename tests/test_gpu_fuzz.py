"""Randomised cross-check of the closed-loop kernels against the C oracle (oracle/c): estimator, lane variant, horizon, gain, step,
bandwidth, annealing and noise scale drawn at random (fixed seed); short horizons keep the closed loop's sensitivity out of the
comparison, so the gates are tight."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def uvs():
    import torch
    assert torch.cuda.is_available()
    import uvs_amd
    uvs_amd.lib()
    return uvs_amd


def test_random_configurations_match_c_oracle(uvs):
    import torch
    from oracle import c_oracle
    import bench
    cfg = bench.config2()
    desired = cfg['experiments']['desired_f']
    plant = uvs.SyntheticPlant.ur10(desired).to_struct()
    rng = np.random.default_rng(2026)
    orng = np.random.default_rng(4)                                           # launch options from their own stream: the cases stay those of round 3
    worst = {}
    for case in range(48):
        method = ['GMCKF', 'KF', 'IMCCKF', 'MCKF'][case % 4]                   # the four estimators (oracle/c restates all of them)
        lanes = {'GMCKF': [0, 2, 4, 1, -2], 'KF': [0, 2, 4, -4], 'IMCCKF': [0, 2, 4, -2], 'MCKF': [0, 2, 4, -2, 1, -4]}[method]
        lane = lanes[(case // 4) % len(lanes)]
        T = int(rng.integers(1, 140))
        K = int(rng.integers(1, 60))
        dt = float(rng.choice([0.02, 0.05, 0.1]))
        t_max = dt * (K + 1) + (dt / 2 if rng.random() < 0.5 else 5.0)          # k_max >= K; sometimes a much longer annealing horizon
        gain = float(rng.uniform(0.05, 0.6))
        bw = float(rng.choice([2.0, 10.0, 50.0]))
        anneal = bool(rng.random() < 0.4)
        scale = float(rng.choice([0.0, 0.5, 3.0]))
        noise = scale * rng.standard_t(2.5, size=(T, K, 8))
        thr, cap = float(rng.choice([0.1, 1e-2, 1e-4])), int(rng.choice([1, 2, 5, 1000]))      # MCKF only
        q0 = np.tile(cfg['experiments']['q_start'], (T, 1)).astype(float)
        q0[:, :3] += rng.uniform(-0.15, 0.15, (T, 3))
        ref = c_oracle.closed_loop_batch(q0, noise, desired, method=method, kernel_bw=bw, annealing=anneal, dt=dt, t_max=t_max, gain=gain, steps=K, want_x=True,
                                         fpi_threshold=thr, fpi_epoch_max=cap)
        fp = uvs.engine.make_params(8, 6, method, bw, anneal, dt, t_max, gain, desired, True, lane, K, thr, cap)
        # round 4's launch options, drawn with the case: MCKF trials cut into 1-6 segments (needs >= 8 steps per segment to take effect),
        # the latency mapping for the estimators that have a four-lane kernel; the strict-pinv option on every sixth case
        opts = 0
        if method == 'MCKF' and lane in (0, 2):
            opts |= int(orng.integers(1, 7)) << 8
        elif lane == 0 and orng.random() < 0.5:
            opts |= 2
        if case % 6 == 5:
            opts |= 1
        fp.reserved = opts
        out = uvs.engine.closed_loop(fp, plant, torch.as_tensor(q0, device='cuda'), torch.as_tensor(np.ascontiguousarray(noise.transpose(1, 2, 0)), device='cuda'),
                                     want=('x', 'err', 'q'))
        tag = (case, method, lane, T, K, dt, gain, bw, anneal, scale, thr, cap, opts)
        assert np.array_equal(out['status'].cpu().numpy(), ref['status']) and np.array_equal(out['k_done'].cpu().numpy(), ref['k_done']), tag
        ok = ref['status'] == 0
        if not ok.any():
            continue
        for key, rk, tol in (('err', 'err', 1e-8), ('q', 'q', 1e-8), ('x', 'X', 1e-8)):
            a = out[key].cpu().numpy().transpose(2, 0, 1)[ok]
            d = rel_err(a, ref[rk][ok])
            worst[key] = max(worst.get(key, 0.0), d)
            assert d <= tol, (key, d) + tag
        assert rel_err(out['stats'].cpu().numpy()[ok], ref['stats'][ok]) <= 1e-8, tag
    print('fuzz: worst relative deviations', {k: f'{v:.1e}' for k, v in worst.items()})
