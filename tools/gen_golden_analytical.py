#!/usr/bin/env python3
"""Generate tests/golden/analytical_*.npz: the reference's own Experiment.run() on Method.ANALYTICAL (experiment.py:145-162, :300-320).
BUILD-CONTAINER ONLY (imports the reference through oracle/gen_golden.py, which it does not modify; only the .npz vectors travel).

The reference crashes on ANALYTICAL before its loop: experiment.py:121 (`Br = np.linalg.cholesky(R)`) reads R, which only the estimator
branch binds.  A sys.settrace line hook supplies it -- R = I_m on the `line` event of :121 -- and lines 121-122 then compute Br / Br_inv,
which no ANALYTICAL line reads (CPython 3.10 writes a trace function's f_locals edits back to the frame).  J_feature is captured on the
`line` event of :302 (`error = f - self.desired_f`), the hook point of oracle/gen_golden.py.  Both lines are found by their text and
asserted, so that a moved line fails here instead of capturing the wrong one.
    python tools/gen_golden_analytical.py            # rewrites tests/golden/analytical_*.npz
"""
import json
import linecache
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as G                                                # noqa: E402  (stubs cv2 / ZMQ, binds detect4Circles)

E, NoiseProfiler, NoiseType = G.E, G.NoiseProfiler, G.NoiseType
OUT = G.OUT


def _line_of(text):
    path = E.Experiment.run.__code__.co_filename
    first = E.Experiment.run.__code__.co_firstlineno
    hits = [i for i in range(first, first + 400) if linecache.getline(path, i).strip() == text]
    assert len(hits) == 1, (text, hits)
    return hits[0]


LINE_R = _line_of('Br = np.linalg.cholesky(R)')                      # experiment.py:121
LINE_ERR = _line_of('error = f - self.desired_f')                    # experiment.py:302


class InfAt:
    """Duck-typed noise profile: zero noise, except +inf in feature `feature` at call `call` (0-based)."""

    def __init__(self, call=40, feature=3, m=8):
        self.calls, self.call, self.feature, self.m = 0, call, feature, m

    def getNoise(self):
        out = np.zeros(self.m)
        if self.calls == self.call:
            out[self.feature] = np.inf
        self.calls += 1
        return out


def run_analytical(noise_prof, q_start):
    rec, code = [], E.Experiment.run.__code__

    def local(frame, event, arg):
        if event == 'line' and frame.f_lineno == LINE_R and 'R' not in frame.f_locals:
            frame.f_locals['R'] = np.eye(len(frame.f_locals['self'].desired_f))
        if event == 'line' and frame.f_lineno == LINE_ERR:
            rec.append(np.array(frame.f_locals['J_feature'], copy=True))
        return local
    ex = E.Experiment(q_start=np.array(q_start, float), desired_f=G.DESIRED, noise_prof=noise_prof, t_s=G.DT, t_max=G.T_MAX,
                      ibvs_gain=G.GAIN, robot=G.RefPlant(), method=E.Method.ANALYTICAL, method_params={})
    sys.settrace(lambda fr, ev, arg: local if fr.f_code is code else None)
    try:
        out = ex.run()
    finally:
        sys.settrace(None)
    return out, rec


def save(name, noise_type=None, noise_params=None, seed=None, q_start=G.Q_START, hold=False, hold_cnt=10, profile=None, dt=0.05, t_max=15,
         gain=0.2):
    G.DT, G.T_MAX, G.GAIN = dt, t_max, gain
    try:
        if profile is None and noise_type is not None:
            profile = NoiseProfiler(num_features=8, noise_type=noise_type, seed=seed, noise_hold=hold, noise_hold_cnt=hold_cnt,
                                    noise_params=dict(noise_params))
        out, rec = run_analytical(profile, q_start)
    finally:
        G.DT, G.T_MAX, G.GAIN = 0.05, 15, 0.2
    status, t, err, q, f, fd, cam, noise, bw = out
    k = len(t)
    J = np.stack([r.ravel() for r in rec])[:k] if k else np.zeros((0, 48))
    assert np.all(bw == -1)
    meta = dict(method='ANALYTICAL', noise_type=None if noise_type is None else noise_type.name, noise_params=noise_params, seed=seed,
                hold=bool(hold), hold_cnt=int(hold_cnt), dt=dt, t_max=t_max, gain=gain, profile=None if profile is None else type(profile).__name__,
                generator='tools/gen_golden_analytical.py', reference='experiment.py Experiment.run(), Method.ANALYTICAL')
    np.savez_compressed(os.path.join(OUT, f'analytical_{name}.npz'), meta=json.dumps(meta), status=status.value, k_done=k,
                        q_start=np.array(q_start, float), desired=G.DESIRED, t=t, err=err, q=q, f=f, noise=noise, cam=cam, J=J)
    print(f'analytical_{name}: status={status.name} k={k} |err[0]|={np.linalg.norm(err[0]):.6g} |err[-1]|={np.linalg.norm(err[-1]):.6g}')


def main():
    AS = lambda a: dict(alpha=a, beta=0, gamma=1, delta=0)           # noqa: E731
    MIX = dict(std=1.0, mean=50.0, rho=0.1)
    NT = NoiseType
    save('none')
    save('white', NT.WHITE_NOISE, dict(std=1.0), 123456)
    save('a1p5', NT.ALPHA_STABLE, AS(1.5), 123456)
    save('a1p0', NT.ALPHA_STABLE, AS(1.0), 123457)
    save('bimodal', NT.GAUSSIAN_BIMODAL, MIX, 123461)
    save('mix_hold', NT.GAUSSIAN_MIXTURE, MIX, 123459, hold=True)
    jit = NoiseProfiler(num_features=2, noise_type=NT.UNIFORM, seed=12345).getNoise().copy()   # main.py:132-134
    qj = G.Q_START.copy()
    qj[0] += 2 * (jit[0] - 1) * (np.pi / 18)
    qj[1] += 2 * (jit[1] - 1) * (np.pi / 9)
    save('jitter', NT.ALPHA_STABLE, AS(1.5), 123456, q_start=qj)
    save('dt0p02_t6_gain0p5', NT.ALPHA_STABLE, AS(1.5), 323456, dt=0.02, t_max=6, gain=0.5)
    save('inf_at_40', profile=InfAt(40, 3))


if __name__ == '__main__':
    main()
