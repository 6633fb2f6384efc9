"""bench.py keeps the driver's contract: one JSON line with the agreed keys (GPU), and a CPU baseline that sizes itself honestly (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_available_cores_respects_affinity_and_quota():
    import bench
    n = bench.available_cores()
    assert 1 <= n <= len(os.sched_getaffinity(0))


def test_cpu_baseline_runs_the_oracle_on_a_small_sample():
    import bench
    q = np.tile(np.array([0.0, 0.0, 1.96349541, 0.0, -1.57079633, 0.0]), (2, 1))
    out = bench.cpu_baseline(q, budget_trials_per_core=1)
    assert out['kind'] == 'port' and out['unit'] == 'updates/s' and out['cores'] == bench.available_cores()
    assert out['value'] > 0 and 'oracle/rmckf_dense.py' in out['sample']


def test_rocm_smi_text_is_parsed():
    import bench
    text = """
============================ ROCm System Management Interface ============================
GPU[0]		: fclk clock level: 0: (1250Mhz)
GPU[0]		: mclk clock level: 0: (2000Mhz)
GPU[0]		: sclk clock level: 1: (2131Mhz)
======================================= Power Cap ========================================
GPU[0]		: Max Graphics Package Power (W): 1400.0
=================================== Power Consumption ====================================
GPU[0]		: Current Socket Graphics Package Power (W): 1357.0
"""
    assert bench.parse_rocm_smi(text) == (1357.0, 2131, 1400.0)
    assert bench.parse_rocm_smi('GPU[0] : sclk clock level: S: (95Mhz)\nGPU[0] : Average Graphics Package Power (W): 246.0') == (246.0, 95, None)
    assert bench.parse_rocm_smi('no such tool') == (None, None, None)


def test_profiler_environment_is_detected_and_scrubbed():
    """helper children (rocm-smi) must not inherit an injected profiler library; power / e2e are skipped under a profiler."""
    import bench
    plain = {'PATH': '/usr/bin', 'HOME': '/root'}
    assert not bench.under_profiler(plain) and bench.scrubbed_env(plain) == plain
    prof = dict(plain, LD_PRELOAD='/opt/rocm/lib/librocprofiler-sdk-tool.so', ROCPROFILER_LIBRARY_CTOR='1', ROCPROF_OUTPUT_PATH='/tmp/x',
                HSA_TOOLS_LIB='/opt/rocm/lib/librocprofiler64.so', ROCP_TOOL_LIB='x')
    assert bench.under_profiler(prof) and bench.under_profiler({'ROCPROF_COUNTERS': 'pmc: SQ_WAVES'})
    assert bench.under_profiler({'LD_PRELOAD': '/x/librocprofiler-sdk-tool.so.1'}) and not bench.under_profiler({'LD_PRELOAD': '/x/libjemalloc.so'})
    assert bench.scrubbed_env(prof) == plain
    mixed = dict(plain, LD_PRELOAD='/usr/lib/libguard.so:/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so', ROCP_TOOL_LIBRARIES='x')
    assert bench.scrubbed_env(mixed) == dict(plain, LD_PRELOAD='/usr/lib/libguard.so')       # only the profiler's entry goes


def test_plain_gpus_n_starts_its_own_ranks_and_a_failing_rank_is_loud(tmp_path):
    """`python bench.py --gpus 2` without WORLD_SIZE must not assert: the parent starts two fresh ranks under torch.distributed.run.
    On a box without a GPU every rank fails (no CPU fallback) -- the parent relays the failure as a non-zero exit code and prints no JSON.
    A WORLD_SIZE that contradicts --gpus is refused with the two valid invocations spelled out."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env['CUDA_VISIBLE_DEVICES'] = env['HIP_VISIBLE_DEVICES'] = ''         # also on a GPU box: this test is about the failing path
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--trials', '64', '--no-cpu-baseline',
                          '--no-side'], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert res.returncode != 0
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert 'AssertionError' not in res.stderr.split('Traceback')[0]          # the parent itself did not trip over WORLD_SIZE
    assert 'torch.distributed' in res.stderr or 'ChildFailedError' in res.stderr or 'no GPU' in res.stderr or 'HIP' in res.stderr
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], capture_output=True, text=True, timeout=120, cwd=ROOT,
                         env=dict(env, WORLD_SIZE='3', RANK='0', LOCAL_RANK='0'))
    assert res.returncode != 0 and 'WORLD_SIZE=3' in res.stderr and 'torch.distributed.run' in res.stderr


@pytest.mark.parametrize('layout,M,N,T,row_cap', [('kct', 8, 6, 300, 65536), ('ktc', 32, 7, 100, 65536), ('tkc', 8, 6, 90, 64)])
def test_dump_outputs_writes_bounded_seeded_samples(tmp_path, monkeypatch, layout, M, N, T, row_cap):
    """--dump-outputs: float64 .npy files of what the launch returned, [trial][step][comp] streams of a seeded trial sample, under 64 MB in
    all, the same trials on every call.  (32,7): the byte cap bounds the stream sample; row_cap < T: the per-trial rows are sampled too."""
    import torch
    import bench
    from uvs_amd import engine
    monkeypatch.setattr(bench, 'DUMP_ROW_TRIALS', row_cap)
    K = 299
    g = torch.Generator().manual_seed(1)
    shape = lambda c: {'kct': (K, c, T), 'ktc': (K, T, c), 'tkc': (T, K, c)}[layout]     # noqa: E731 -- engine.alloc_stream's, on the host
    bufs = {k: torch.rand(shape(c), generator=g, dtype=torch.float64) for k, c in (('x', M * N), ('err', M), ('q', N))}
    stats = torch.rand((T, 3), generator=g, dtype=torch.float64)
    status = torch.randint(0, 2, (T,), generator=g, dtype=torch.int32)
    k_done = torch.randint(1, K + 1, (T,), generator=g, dtype=torch.int32)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), torch, engine, bufs, layout, stats, status, k_done)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b')) == ['err.npy', 'k_done.npy', 'q.npy', 'stats.npy', 'status.npy', 'x.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) < 64 << 20
    out = {n[:-4]: np.load(tmp_path / 'a' / n) for n in names}
    for n in names:
        assert np.array_equal(out[n[:-4]], np.load(tmp_path / 'b' / n)) and out[n[:-4]].dtype == np.float64
    rows = min(T, bench.DUMP_ROW_TRIALS)
    assert out['stats'].shape == (rows, 3) and out['status'].shape == out['k_done'].shape == (rows,)
    S = out['x'].shape[0]
    assert 1 <= S <= min(T, bench.DUMP_STREAM_TRIALS) and out['x'].shape == (S, K, M * N) and out['err'].shape == (S, K, M) and out['q'].shape == (S, K, N)
    tkc = engine.as_tkc(bufs['err'], layout).numpy()
    hit = [t for t in range(T) if np.array_equal(tkc[t], out['err'][0])]     # the dumped rows are trials of the launch, whole
    assert len(hit) == 1 and np.array_equal(engine.as_tkc(bufs['x'], layout).numpy()[hit[0]], out['x'][0])
    if T <= bench.DUMP_ROW_TRIALS:
        assert np.array_equal(out['stats'], stats.numpy()) and np.array_equal(out['k_done'], k_done.numpy())


@pytest.mark.gpu
def test_plain_bench_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times the steps and prints the line without any side measurement; --dump-outputs writes the last step's outputs."""
    import bench
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--trials', '4096', '--dump-outputs', str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and abs(d['value'] - 4096 * 299 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    assert d['cpu_baseline'] is None and d['replay'] is None and d['roofline']['power'] is None and d['other_estimators'] is None
    out = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in os.listdir(tmp_path)}
    assert sorted(out) == ['err', 'k_done', 'q', 'stats', 'status', 'x']
    assert out['stats'].shape == (4096, 3) and np.all(out['status'] == 0) and np.all(out['k_done'] == 299)
    assert out['x'].shape == (bench.DUMP_STREAM_TRIALS, 299, 48) and np.all(np.isfinite(out['x'])) and np.all(np.isfinite(out['err']))


@pytest.mark.gpu
def test_bench_line_contract():
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--trials', '4096', '--no-cpu-baseline', '--full']
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1                                                   # exactly one JSON line on stdout
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
                'data', 'config', 'roofline', 'cpu_baseline'):
        assert key in d, key
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1 and d['higher_is_better'] is True and d['scaling'] == 'weak'
    assert d['config']['trials_total'] == 4096 and d['config']['ranks_seen'] == 1 and d['multi_gpu']['gather_inside_timed_region'] is False
    assert d['vs_baseline'] is None and d['dtype'] == 'f64' and d['data'] == 'synthetic' and d['unit'] == 'updates/s'
    assert 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-12
    assert d['value'] > 0 and abs(d['value'] - 4096 * 299 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    assert 'power' in r and (r['power'] is None or (len(r['power']['sclk_mhz']) >= 1 and min(r['power']['package_watts']) > 0))
    assert d['replay']['estimator_only']['achieved'] > 0


@pytest.mark.gpu
def test_drop_in_step_route_latency():
    """the drop-in step route -- what Experiment.run() pays per loop iteration with an external robot -- measured as bench.py reports it
    (`drop_in`): a real config-2 servo trial driven from the host, zero-copy pinned records.  <= 80 us per step at T = 1 (measured: 23-25 us; the reference's
    numpy takes 260-430 us per update, the round-5 tensor route ~100 us on the same trial), and the trial converges."""
    import torch
    import uvs_amd
    from uvs_amd import engine
    import bench
    d = bench.drop_in_step_latency(torch, uvs_amd, engine, torch.device('cuda'))
    print('drop-in step latency:', {k: round(v, 1) for k, v in d['step_latency_us'].items()}, 'us; tensor route', {k: round(v, 1) for k, v in d['tensor_route_us'].items()})
    assert d['step_latency_us']['T1'] <= 80.0 and d['step_latency_us']['T64'] <= 80.0
    assert d['step_latency_us']['T1'] < d['tensor_route_us']['T1']
    assert all(v['final_feature_error_px'] < 10.0 for v in d['detail'].values())
