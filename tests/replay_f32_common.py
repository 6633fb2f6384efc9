"""The inputs, the fp64 truth and the float32 restatement that the single-precision replay (uvs_rmckf_replay_f32) is held to:
one recipe for tests/test_replay_f32_oracle.py (CPU: the restatement against the truth, and the teeth of the gate) and
tests/test_gpu_replay_f32.py (the kernel against both).

Inputs: the recorded f / dq_prev streams and the first X of a closed_* fixture, made into T distinct trials -- f + N(0,1), dq scaled per
trial, x0 scaled per trial -- and ROW 0 OF dq SET TO 0.1 N(0,1): the estimator ignores it (H = 0 on the first step), every recorded
stream has zeros there, and a kernel that read it would otherwise pass everything.  All of it is rounded to float32 FIRST; the truth is
oracle/rmckf_block.run_replay on those float32 values, so input rounding is no part of any figure.

Figure: E(X, case) = max over trials of rel_err(X_trial, X64_trial), the maximum over all steps and entries relative to that trial's
max |X64|.  E_f32(case) is the figure of oracle/rmckf_block_f32 (a plain float32 evaluation, BlockFilter.step's formulas, no FMA); the
kernel's gate is 2 E_f32(case): its FMAs, rcp + Newton and exp2 are each at least as accurate as the restatement's operations, so it owes
no more error than a second float32 evaluation in another operation order, and two such evaluations differ from each other by up to the
sum of their errors.  Everything here is computed once per process and handed out read-only."""
import functools

import numpy as np

from conftest import load_golden, rel_err

T_RAGGED = 35                                                # 32 + 3: a full wavefront's worth of trials and a ragged second one
K_SHORT, K_FULL = 40, 299
SHORT_CASES = ['closed_gmckf_a1p5', 'closed_gmckf_a1p5_anneal', 'closed_kf_a1p5', 'closed_imcckf_a1p5', 'closed_imcckf_sigma30_anneal']
LONG_CASES = ['closed_gmckf_a1p5', 'closed_kf_a1p5', 'closed_imcckf_a1p5']                 # one K = 299 run per estimator
CASES = [(n, T_RAGGED, K_SHORT) for n in SHORT_CASES] + [(n, T_RAGGED, K_FULL) for n in LONG_CASES]
GPU_CASES = CASES + [('closed_gmckf_a1p5', 100, K_SHORT)]    # 3 x 32 + 4
E_F32_MAX = 2e-6                                             # a condition on the INPUTS (another seed if a case breaks it), not on the kernel
MARGIN = 2.0                                                 # E_kernel <= MARGIN * E_f32, see above
CONTRACT = 1e-5


def case_id(case):
    return '{}-T{}-K{}'.format(*case)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(name, T, K, seed=0):
    """dict(f (T, K + 1, 8), dq (T, K, 6), x0 (T, 48), desired (8,): float32, read-only; method, kernel_bw, annealing, k_max, dt, t_max, gain)."""
    g = load_golden(name)
    meta, p = g['meta'], g['meta']['params']
    rng = np.random.default_rng([seed, T, K])
    f_seq = np.vstack([g['f_init'][None], g['f']])[:K + 1]
    f = f_seq[None] + rng.normal(size=(T, K + 1, 8))
    dq = g['dq_prev'][None, :K] * (1 + 0.1 * rng.normal(size=(T, 1, 1)))
    x0 = g['X'][0][None] * (1 + 0.01 * rng.normal(size=(T, 1)))
    assert not g['dq_prev'][0].any()
    dq[:, 0] = 0.1 * rng.normal(size=(T, 6))                 # ignored by a correct estimator
    r32 = lambda a: _frozen(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    return dict(f=r32(f), dq=r32(dq), x0=r32(x0), desired=r32(g['desired']), desired64=g['desired'], method=meta['method'], kernel_bw=p['kernel_bw'],
                annealing=p['annealing'], k_max=int(meta['t_max'] / meta['dt']), dt=meta['dt'], t_max=meta['t_max'], gain=meta['gain'])


@functools.lru_cache(maxsize=None)
def truth(name, T, K):
    """rmckf_block.run_replay (fp64) on the float32 inputs, trial by trial: dict(X (T, K, 48), err (T, K, 8)) float64, read-only."""
    from oracle import rmckf_block
    inp = inputs(name, T, K)
    f, dq, x0 = (inp[k].astype(np.float64) for k in ('f', 'dq', 'x0'))
    runs = [rmckf_block.run_replay(f[t], dq[t], x0[t], inp['desired'].astype(np.float64), inp['gain'], inp['method'], inp['kernel_bw'], inp['annealing'],
                                   inp['k_max']) for t in range(T)]
    return dict(X=_frozen(np.stack([r['X'] for r in runs])), err=_frozen(np.stack([r['err'] for r in runs])))


def restate(name, T, K, filter_cls=None):
    """oracle/rmckf_block_f32.run_replay on the same inputs (filter_cls: a deliberately wrong subclass, tests/test_replay_f32_oracle.py)."""
    from oracle import rmckf_block_f32
    inp = inputs(name, T, K)
    return rmckf_block_f32.run_replay(inp['f'], inp['dq'], inp['x0'], inp['desired'], inp['method'], inp['kernel_bw'], inp['annealing'], inp['k_max'],
                                      filter_cls=filter_cls or rmckf_block_f32.BlockFilterF32)


def figure(X, name, T, K):
    """E of an X stream (T, K, 48), any float type, against the truth of the case."""
    X64 = truth(name, T, K)['X']
    assert X.shape == X64.shape
    return max(rel_err(X[t], X64[t]) for t in range(T))


@functools.lru_cache(maxsize=None)
def restatement(name, T, K):
    """The float32 oracle's run of the case, read-only, and its figure: (dict(X, err, kappa, P_final), E_f32)."""
    out = {k: _frozen(v) for k, v in restate(name, T, K).items()}
    assert out['X'].dtype == np.float32 and out['err'].dtype == np.float32
    return out, figure(out['X'], name, T, K)
