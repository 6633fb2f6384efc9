"""CPU-only tests of the X log, the true image Jacobian and the score (include/uvs_vision.h, "THE ESTIMATE AS A LOG" and "THE TRUE IMAGE
JACOBIAN"; plant.projection_jacobian, plant.jacobian_score, plant.score_ratios; engine.camera_closed_loop(want=(..., 'x')),
engine.camera_jacobian, engine.camera_jacobian_score): the numpy rule against central differences of plant.features with every named
misreading measured, the sums on a table, header and ctypes table agree, every C refusal of the three entry points comes before any HIP
call in the stated order (host arrays with sentinels no kernel could use), every Python refusal before any device work, the built
library holds the 22 + 2 new kernels without scratch and under no pinned name, and the CPU restatement of the X log is
camera_predicted_common.estimator_trial's loop bit for bit in every other key, on trials that meet pixel_loop_common's preconditions.

Measured here (20 poses around the goal x three plants, h = 1e-5; 1, 3 and 4 points): the rule against central differences 1.7e-10,
1.8e-10 and 1.9e-10 relative Frobenius; the misreadings, over all records together (and at the closest single pose): uncentred pixels
0.75, 0.70, 0.72 (0.62); distance for depth 2.0e-2, 1.7e-2, 2.2e-2 (7.1e-4 with one point, 3.4e-3 otherwise); the w x term dropped 0.95,
0.92, 0.92 (0.79); the sign of v 1.15, 1.09, 1.15 (0.95); analytic_guess itself 0.75, 0.70, 0.72 (0.62)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import camera_common as cc
import camera_predicted_common as pc
import camera_score_common as sco
import pixel_loop_common as pl
from conftest import ROOT
from test_camera_grid_host import Buffers, DESIRED
from test_camera_latency_host import PINNED
from test_camera_moving_host import inside, triple_refusals
from test_camera_predicted_host import Predicted, same_bits, with_and_without

ARG, SHAPE, METHOD = -1, -2, -4


@pytest.fixture(scope='module')
def uvs():
    import uvs_amd
    if not os.path.exists(uvs_amd._vision.LIB_PATH):
        uvs_amd._vision.build()
    return uvs_amd


# ------------------------------------------------------------------------------------------------------------- the numpy rules
@pytest.mark.parametrize('n_points', [1, 3, 4])
def test_the_rule_is_the_derivative_of_the_projection(uvs, n_points):
    """plant.projection_jacobian against central differences of plant.features at h = 1e-5, over seeded poses: the plant as it is, with
    its points moved (plant.target_at, and the points= argument) and a plant.miscalibrated scene; bound 1e-7 relative Frobenius.  Every named
    misreading lies at least 1e-3 from the rule, as the relative Frobenius distance over the records of all poses and plants together --
    what a comparison of a batch of records sees.  (Pose by pose "distance for depth" can coincide with the rule: a disc on the optical
    axis is as far away as it is deep, and the one disc of the one-point plant passes within 7e-4 of that; the smallest single-pose
    distance is printed next to the asserted one.)"""
    P = uvs.plant
    nominal = pl.plant_of(n_points)
    velocity = np.random.default_rng(2).uniform(-2e-3, 2e-3, (n_points, 3))
    moved = P.target_at(nominal, velocity, 9, (3, 40))
    wrong = P.miscalibrated(nominal, focal_scale=1.07, point_offset=(0.01, -0.02, 0.015), joint_offset=0.02, link_scale=0.97)
    worst, far, rule, wrongs = 0.0, {name: np.inf for name in sco.MISREADINGS}, [], {name: [] for name in sco.MISREADINGS}
    for q in sco.poses(20, seed=n_points):
        for plant in (nominal, moved, wrong):
            J = P.projection_jacobian(plant, q)
            assert J.shape == (2 * n_points, 6)
            worst = max(worst, sco.rel(J, sco.central_differences(plant, q)))
            rule.append(J)
            for name in sco.MISREADINGS:
                wrongs[name].append(sco.misread_jacobian(uvs, plant, q, name))
                far[name] = min(far[name], sco.rel(wrongs[name][-1], J))
        assert np.array_equal(P.projection_jacobian(nominal, q, moved.points), P.projection_jacobian(moved, q)), 'points= is the moved plant'
    together = {name: sco.rel(np.stack(wrongs[name]), np.stack(rule)) for name in sco.MISREADINGS}
    print(f'{n_points} points: central differences {worst:.2e}; '
          + ', '.join(f'{name} {together[name]:.2e} (a single pose: {far[name]:.2e})' for name in sco.MISREADINGS))
    assert worst <= sco.FD_BOUND
    for name, d in together.items():
        assert d >= sco.MISREAD_MIN, (name, d)


def test_the_sums_on_a_table(uvs):
    P = uvs.plant
    J = P.projection_jacobian(pl.plant_of(4), cc.Q_GOAL) * 0.05
    for s in (1.0, 2.5, 0.125, -3.0):                                # X = s J: cosine +-1, scale s, rel_err |s - 1|, no shape error
        r = P.score_ratios(P.jacobian_score(s * J, J))
        assert abs(r['cosine'] - np.sign(s)) < 1e-12 and abs(r['scale'] - s) < 1e-12 * abs(s) and abs(r['rel_err'] - abs(s - 1)) < 1e-12
        assert r['shape_err'] < 1e-6
    rng = np.random.default_rng(0)
    X = rng.standard_normal(J.shape)
    X -= J * (X * J).sum() / (J * J).sum()                           # orthogonal to J in the Frobenius product
    sums = P.jacobian_score(X, J)
    r = P.score_ratios(sums)
    assert abs(r['cosine']) < 1e-12 and abs(r['scale']) < 1e-12 and abs(r['shape_err'] - 1) < 1e-12
    assert abs(sums[3] - (sums[0] + sums[1])) < 1e-9 * sums[3], 'Pythagoras'
    assert np.array_equal(P.jacobian_score(X.reshape(-1), J), sums), 'the flat layout of the logs'
    assert np.array_equal(sums[4:], [0.0, 0.0]), 'no dq: zeros'
    # step_ratio: a dq in X's null space promises nothing (0 / 0); out of it, X = s J promises s times what the plant delivers
    null = np.linalg.svd(J[:2])[2][-1]                               # (2, 6) has a null space
    sums = P.jacobian_score(J[:2], J[:2], null)
    assert sums[4] < 1e-20 * (J * J).sum()
    dq = rng.standard_normal(6)
    for s in (1.0, 8.0, 0.5):
        r = P.score_ratios(P.jacobian_score(s * J, J, dq))
        assert abs(r['step_ratio'] - 1 / s) < 1e-12
    batch = P.jacobian_score(np.stack([J, 2 * J]).reshape(2, -1), np.stack([J, J]), np.stack([dq, dq]))
    assert batch.shape == (2, 6) and np.array_equal(batch[0], P.jacobian_score(J, J, dq)) and np.array_equal(batch[1], P.jacobian_score(2 * J, J, dq))
    assert P.SCORE_SUMS == ('nx2', 'nj2', 'dot', 'diff2', 'xd_xd', 'xd_jd')


# ------------------------------------------------------------------------------------------------------------- header and table
def test_header_and_symbols_agree(uvs):
    header = open(os.path.join(ROOT, 'include', 'uvs_vision.h')).read()
    assert set(re.findall(r'\b(uvs_[a-z0-9_]+)\s*\(', header)) == set(uvs._vision.SYMBOLS), 'ctypes table and header disagree'
    declared = lambda fn: [' '.join(a.split()) for a in re.search(r'int ' + fn + r'\s*\(([^;]*)\);', header).group(1).split(',')]   # noqa: E731
    types = lambda fn: list(uvs._vision.SYMBOLS[fn][1])              # noqa: E731
    a, b = declared('uvs_camera_closed_loop_logged_f64'), declared('uvs_camera_closed_loop_predicted_f64')
    ta, tb = types('uvs_camera_closed_loop_logged_f64'), types('uvs_camera_closed_loop_predicted_f64')
    at = b.index('double *kappa_log') + 1
    b.insert(at, 'double *x_log')
    tb.insert(at, ctypes.c_void_p)
    assert a == b and ta == tb, "the predicted namesake's operands with x_log after kappa_log"
    ctype = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    for fn in ('uvs_camera_jacobian_f64', 'uvs_camera_jacobian_score_f64'):
        want = [ctypes.c_void_p if '*' in arg else ctype[arg.split()[0]] for arg in declared(fn)]
        assert types(fn) == want, fn
    names = [arg.split()[-1].lstrip('*') for arg in declared('uvs_camera_jacobian_f64')]
    assert names == ['cams', 'n_cams', 'cam_index', 'motion', 'n_points', 'T', 'rows', 'k0', 'q', 'j_out', 'stream']
    names = [arg.split()[-1].lstrip('*') for arg in declared('uvs_camera_jacobian_score_f64')]
    assert names == ['cams', 'n_cams', 'cam_index', 'motion', 'n_points', 'T', 'K', 'dt', 'x_log', 'q_log', 'dq_log', 'k_done', 'score', 'stream']
    for fn in ('uvs_camera_closed_loop_logged_f64', 'uvs_camera_jacobian_f64', 'uvs_camera_jacobian_score_f64'):
        assert getattr(uvs._vision.lib(), fn) is not None
    assert 'THE ESTIMATE AS A LOG' in header and 'THE TRUE IMAGE JACOBIAN' in header


# ------------------------------------------------------------------------------------------------------------- C refusals
class Logged(Predicted):
    """Predicted with an X log: a host array of sentinels."""
    def __init__(self, uvs, **kw):
        Predicted.__init__(self, uvs, **kw)
        self.x = np.full(3 * self.T * 48 + 8, 7.0)

    def untouched(self):
        return Predicted.untouched(self) and np.all(self.x == 7)


def logged_call(uvs, b, T=None, cams='own', n_cams=1, index=None, motion='own', latency='own', assumed='own', predict='own', x_log='own', tp='block',
                occ='rows', n_occ=1, hold=2, **over):
    a = {name: b.ptr(name) for name in ('q_start', 'noise', 'x0', 'f0', 'q', 'f', 'dq', 'err', 'kappa', 'status', 'k_done', 'stats', 'pixels')}
    a.update(fp=b.fp)
    a.update(over)
    if isinstance(tp, str):
        tp = b.trial_params(uvs)
    ref = lambda s: None if s is None else ctypes.byref(s)           # noqa: E731
    own = lambda given, mine: mine.ctypes.data if isinstance(given, str) else given   # noqa: E731
    return uvs._vision.lib().uvs_camera_closed_loop_logged_f64(
        ref(a['fp']), own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), own(latency, b.latency), own(assumed, b.assumed),
        own(predict, b.predict), b.T if T is None else T, ref(tp), own(occ, b.occ), b.paint.ctypes.data, n_occ, hold, a['q_start'], a['noise'],
        a['x0'], a['f0'], a['q'], a['f'], a['dq'], a['err'], a['kappa'], own(x_log, b.x), a['status'], a['k_done'], a['stats'], a['pixels'],
        b.held.ctypes.data, None)


def test_the_logged_loop_refuses_what_the_predicted_call_refuses_in_its_order(uvs):
    """test_camera_predicted_host's list, in its order, with and without the log and each of the four optional operands before it."""
    lib, b = uvs._vision.lib(), Logged(uvs)

    def call(**kw):
        codes = {with_and_without(lambda **inner: logged_call(uvs, b, x_log=x_log, **inner))(**kw) for x_log in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    for name in ('fp', 'q_start', 'x0', 'f0', 'status', 'k_done', 'stats'):
        assert call(**{name: None}) == ARG and b'NULL' in lib.uvs_vision_last_error(), name
    assert call(T=-1) == ARG
    bad = Buffers(uvs)
    bad.fp.steps = 0
    assert call(fp=bad.fp) == ARG
    bad = Buffers(uvs)
    bad.fp.lanes_per_filter = 2
    assert call(fp=bad.fp) == SHAPE and b'lanes_per_filter' in lib.uvs_vision_last_error()
    bad = Buffers(uvs)
    bad.fp.m = 4                                                     # two points: no such camera
    assert call(fp=bad.fp) == ARG and b'n_points' in lib.uvs_vision_last_error()
    bad = Buffers(uvs)
    bad.fp.n = 5
    assert call(fp=bad.fp) == SHAPE
    bad = Buffers(uvs)
    bad.fp.method = 1                                                # UVS_METHOD_ANALYTICAL
    assert call(fp=bad.fp) == METHOD
    mckf = Logged(uvs, n_points=3, method='MCKF')
    mckf.fp.m = 6
    assert logged_call(uvs, mckf) == METHOD and b'MCKF' in lib.uvs_vision_last_error(), 'MCKF at (6, 6) is not built here either'
    for n_in in (0, -3):
        assert call(tp=b.trial_params(uvs, n_in=n_in)) == ARG and b'n_in' in lib.uvs_vision_last_error(), n_in
    for n_occ in (-1, 5):
        assert call(n_occ=n_occ) == ARG and b'n_occ' in lib.uvs_vision_last_error(), n_occ
    assert call(occ=None, n_occ=2) == ARG and b'NULL occ' in lib.uvs_vision_last_error()
    assert call(hold=-1) == ARG and b'hold' in lib.uvs_vision_last_error()
    assert call(hold=-1, cams=None) == ARG and b'hold' in lib.uvs_vision_last_error()
    assert call(n_occ=9, n_cams=0) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert call(n_occ=9, hold=-1) == ARG and b'n_occ' in lib.uvs_vision_last_error()
    assert call(fp=bad.fp, cams=None) == METHOD
    for x_log in ('own', None):
        for predict in ('own', None):
            triple_refusals(lambda **kw: logged_call(uvs, b, predict=predict, x_log=x_log, **kw), lib, b.T)
    assert call(T=0, tp=None, occ=None, n_occ=0, hold=0) == 0
    assert b.untouched() and mckf.untouched(), 'a refused call wrote'


class Records:
    """Host arrays with sentinels for the two stand-alone calls."""
    def __init__(self, T=2, K=3):
        self.T, self.K = T, K
        self.cams = np.full(T * 472 // 8 + 8, 7.0)
        self.index = np.full(T, 7, np.int32)
        self.motion = np.full(T * 13, 7.0)
        self.k_done = np.full(T, 7, np.int32)
        for name in ('q', 'j', 'x', 'dq', 'score'):
            setattr(self, name, np.full(K * T * 48, 7.0))

    def untouched(self):
        return all(np.all(getattr(self, name) == 7) for name in ('cams', 'index', 'motion', 'k_done', 'q', 'j', 'x', 'dq', 'score'))


def own(given, mine):
    return mine.ctypes.data if isinstance(given, str) else given


def jacobian_call(uvs, b, cams='own', n_cams=1, index=None, motion='own', n_points=4, T=None, rows=None, k0=0, q='own', j='own'):
    return uvs._vision.lib().uvs_camera_jacobian_f64(own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), n_points,
                                                     b.T if T is None else T, b.K if rows is None else rows, k0, own(q, b.q), own(j, b.j), None)


def score_call(uvs, b, cams='own', n_cams=1, index=None, motion='own', n_points=4, T=None, K=None, dt=0.05, x='own', q='own', dq='own', k_done='own',
               score='own'):
    return uvs._vision.lib().uvs_camera_jacobian_score_f64(own(cams, b.cams), n_cams, own(index, b.index), own(motion, b.motion), n_points,
                                                           b.T if T is None else T, b.K if K is None else K, dt, own(x, b.x), own(q, b.q),
                                                           own(dq, b.dq), own(k_done, b.k_done), own(score, b.score), None)


def test_the_jacobian_call_refuses_before_any_hip_call_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Records()

    def call(**kw):
        codes = {jacobian_call(uvs, b, motion=motion, **kw) for motion in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    for name in ('q', 'j'):
        assert call(**{name: None}) == ARG and b'NULL q or j_out' in lib.uvs_vision_last_error(), name
    for T in (-1, 2 ** 31):
        assert call(T=T) == ARG and b'T out of range' in lib.uvs_vision_last_error()
    for rows in (-1, 2 ** 31):
        assert call(rows=rows) == ARG and b'rows out of range' in lib.uvs_vision_last_error()
    for n_points in (0, 2, 5, -1):
        assert call(n_points=n_points) == ARG and b'n_points' in lib.uvs_vision_last_error()
    assert call(cams=None) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
    assert call(n_cams=0) == ARG and call(n_cams=b.T + 1) == ARG and b'cam_index' in lib.uvs_vision_last_error()
    assert call(k0=-1) == ARG and b'k0' in lib.uvs_vision_last_error()
    assert call(k0=2 ** 31 - 2, rows=2) == ARG and b'k0' in lib.uvs_vision_last_error()
    # the order
    assert call(q=None, T=-1) == ARG and b'NULL' in lib.uvs_vision_last_error()
    assert call(T=-1, rows=-1) == ARG and b'T out' in lib.uvs_vision_last_error()
    assert call(rows=-1, n_points=2) == ARG and b'rows' in lib.uvs_vision_last_error()
    assert call(n_points=2, cams=None) == ARG and b'n_points' in lib.uvs_vision_last_error()
    assert call(cams=None, k0=-1) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
    assert call(k0=-1, T=0) == ARG and call(cams=None, rows=0) == ARG, 'before the empty call'
    assert call(T=0) == 0 and call(rows=0) == 0 and lib.uvs_vision_last_error() == b''
    assert call(T=0, n_cams=5, index='own') == 0
    assert b.untouched(), 'a refused call wrote'


def test_the_score_call_refuses_before_any_hip_call_in_its_order(uvs):
    lib, b = uvs._vision.lib(), Records()

    def call(**kw):
        codes = {score_call(uvs, b, motion=motion, dq=dq, k_done=k_done, **kw)
                 for motion in ('own', None) for dq in ('own', None) for k_done in ('own', None)}
        assert len(codes) == 1, (kw, codes)
        return codes.pop()
    for name in ('x', 'q', 'score'):
        assert call(**{name: None}) == ARG and b'NULL x_log, q_log or score' in lib.uvs_vision_last_error(), name
    for T in (-1, 2 ** 31):
        assert call(T=T) == ARG and b'T out of range' in lib.uvs_vision_last_error()
    for K in (-1, 2 ** 31):
        assert call(K=K) == ARG and b'K out of range' in lib.uvs_vision_last_error()
    for n_points in (0, 2, 5):
        assert call(n_points=n_points) == ARG and b'n_points' in lib.uvs_vision_last_error()
    assert call(cams=None) == ARG and b'NULL cams' in lib.uvs_vision_last_error()
    assert call(n_cams=0) == ARG and call(n_cams=b.T + 1) == ARG and b'cam_index' in lib.uvs_vision_last_error()
    assert call(x=None, T=-1) == ARG and b'NULL' in lib.uvs_vision_last_error()
    assert call(T=-1, K=-1) == ARG and b'T out' in lib.uvs_vision_last_error()
    assert call(K=-1, n_points=2) == ARG and b'K out' in lib.uvs_vision_last_error()
    assert call(n_points=2, cams=None) == ARG and b'n_points' in lib.uvs_vision_last_error()
    assert call(cams=None, T=0) == ARG and call(n_cams=0, K=0) == ARG, 'before the empty call'
    assert call(T=0) == 0 and call(K=0) == 0 and lib.uvs_vision_last_error() == b''
    for dt in (0.0, -1.0, float('nan')):                              # dt is a factor: any double
        assert call(T=0, dt=dt) == 0
    assert b.untouched(), 'a refused call wrote'


# ------------------------------------------------------------------------------------------------------------- Python
def test_python_refuses_before_any_device_work(uvs):
    """On a machine without a GPU: each of these is a ValueError of its own, raised before torch.cuda is asked for anything."""
    import torch
    eng = uvs.engine
    plant = uvs.SyntheticPlant.ur10()
    q = torch.zeros((3, 6), dtype=torch.float64)
    fp = eng.make_params(8, 6, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    analytical = eng.make_params(8, 6, 'ANALYTICAL', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    x0 = np.zeros((3, 48))
    assert eng.CAMERA_LOGS == ('err', 'q', 'f', 'dq', 'kappa') and eng.ESTIMATOR_CAMERA_LOGS == eng.CAMERA_LOGS + ('x',)
    for fused in (True, False):                                      # the baseline has no estimate to log
        with pytest.raises(ValueError, match=r"has no \['x'\]"):
            eng.camera_closed_loop(analytical, plant, q, fused=fused, want=('err', 'x'))
    with pytest.raises(ValueError, match='on the device'):           # an estimator accepts it as far as the host goes
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=True, want=eng.ESTIMATOR_CAMERA_LOGS)
    five = eng.make_params(8, 5, 'GMCKF', 10.0, False, 0.05, 15.0, 0.2, DESIRED, steps=3)
    with pytest.raises(ValueError, match="log 'x' are built for the six-joint arms"):
        eng.camera_closed_loop(five, plant, torch.zeros((3, 5), dtype=torch.float64), x0=np.zeros((3, 40)), fused=True, want=('x',))
    with pytest.raises(ValueError, match='on the device'):           # without 'x' that refusal is not there
        eng.camera_closed_loop(five, plant, torch.zeros((3, 5), dtype=torch.float64), x0=np.zeros((3, 40)), fused=True)
    with pytest.raises(ValueError, match='predict needs fused=True'):   # the older refusals are what they were
        eng.camera_closed_loop(fp, plant, q, x0=x0, fused=False, predict=2, want=('x',))
    # camera_jacobian
    for bad in (-1, 1.0, True, 2 ** 31):
        with pytest.raises(ValueError, match='camera_jacobian: k is a step count'):
            eng.camera_jacobian(plant, q, k=bad)
    for bad in (torch.zeros(6), torch.zeros((3, 5)), torch.zeros((2, 3, 4, 6)), None):
        with pytest.raises(ValueError, match=r'camera_jacobian: q is \(T, 6\) or \(K, T, 6\)'):
            eng.camera_jacobian(plant, bad)
    with pytest.raises(ValueError, match='camera_jacobian: camera_index without cameras'):
        eng.camera_jacobian(plant, q, camera_index=[0, 0, 0])
    with pytest.raises(ValueError, match=r'camera_jacobian: camera_index must lie in \[0, 2\)'):
        eng.camera_jacobian(plant, q, cameras=[plant, plant], camera_index=[0, 2, 1])
    with pytest.raises(ValueError, match='camera_jacobian: 2 cameras for 3 trials'):
        eng.camera_jacobian(plant, q, cameras=[plant, plant])
    with pytest.raises(ValueError, match='camera_jacobian: motion_window without target_motion'):
        eng.camera_jacobian(plant, q, motion_window=(0, 5))
    with pytest.raises(ValueError, match='camera_jacobian: target_motion'):
        eng.camera_jacobian(plant, q, target_motion=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='camera_jacobian: a camera of 3 points'):
        eng.camera_jacobian(plant, q, cameras=[pl.plant_of(3)])
    with pytest.raises(ValueError, match='camera_jacobian: q is a tensor on the device'):
        eng.camera_jacobian(plant, q)
    with pytest.raises(ValueError, match='camera_jacobian: q is a tensor on the device'):
        eng.camera_jacobian(plant, torch.zeros((4, 3, 6), dtype=torch.float64), k=7, target_motion=np.zeros((4, 3)), motion_window=(2, 9))
    # camera_jacobian_score
    x, q3 = torch.zeros((4, 3, 48), dtype=torch.float64), torch.zeros((4, 3, 6), dtype=torch.float64)
    for bad in (q, torch.zeros((4, 3, 5)), None):
        with pytest.raises(ValueError, match=r'camera_jacobian_score: q is the \(K, T, 6\) log'):
            eng.camera_jacobian_score(x, bad, plant, 0.05)
    for bad in ('0.05', None, True):
        with pytest.raises(ValueError, match='camera_jacobian_score: dt is the control period'):
            eng.camera_jacobian_score(x, q3, plant, bad)
    with pytest.raises(ValueError, match='camera_jacobian_score: camera_index without cameras'):
        eng.camera_jacobian_score(x, q3, plant, 0.05, camera_index=[0, 0, 0])
    with pytest.raises(ValueError, match='camera_jacobian_score: motion_window without target_motion'):
        eng.camera_jacobian_score(x, q3, plant, 0.05, motion_window=(0, 5))
    with pytest.raises(ValueError, match='camera_jacobian_score: q is a tensor on the device'):
        eng.camera_jacobian_score(x, q3, plant, 0.05, dq=q3, k_done=torch.zeros(3, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------- the built library
def test_the_new_kernels_are_built_without_scratch(uvs):
    """logged_frames_kernel: what predicted_frames_kernel is built for, 22; image_jacobian_kernel and jacobian_score_kernel, one each.
    None uses scratch, no name contains a pinned one, and the pinned ones count what they did."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    k = kernel_resources.kernels(uvs._vision.LIB_PATH)
    loops = {name: r for name, r in k.items() if 'logged_frames_kernel' in name}
    expected = {f'<{shape}, {method}, {per_workgroup}>'
                for shape, methods in (('8, 6, 4', (2, 3, 4, 5)), ('6, 6, 2', (2, 4, 5)), ('2, 6, 1', (2, 3, 4, 5)))
                for method in methods for per_workgroup in (1, 4)}
    found = {re.search(r'logged_frames_kernel(<[^>]*>)', name).group(1) for name in loops}
    assert found == expected and len(loops) == 22, (sorted(found ^ expected), len(loops))
    assert all('LoggedLoopArgs' in name for name in loops)
    for name, r in loops.items():
        assert r['wg'] == 256 and r['vgpr'] <= 512 and r['lds'] <= 65536 and r['scratch'] == 0, (name, r)
        twin = k[name.replace('logged_frames_kernel', 'predicted_frames_kernel').replace('LoggedLoopArgs', 'PredictedLoopArgs')]
        assert r['lds'] == twin['lds'], (name, 'no LDS is added')
    alone = {name: r for name, r in k.items() if 'image_jacobian_kernel' in name or 'jacobian_score_kernel' in name}
    assert len(alone) == 2 and all(r['scratch'] == 0 and r['lds'] == 0 and r['wg'] == 256 for r in alone.values()), alone
    for name in list(loops) + list(alone):
        for pinned in PINNED + ('moving_project_kernel', 'moving_detect_kernel', 'delayed_frames_kernel', 'delayed_baseline_kernel', 'delay_line_kernel',
                                'aligned_frames_kernel', 'aligned_baseline_kernel', 'predicted_frames_kernel', 'predicted_baseline_kernel'):
            assert pinned not in name and not re.search(r'paint_\w*_kernel', name), (pinned, name)
    for pinned in ('camera_loop_kernel', 'camera_grid_kernel', 'camera_occluded_kernel', 'camera_held_kernel', 'camera_painted_kernel',
                   'camera_scene_kernel', 'moving_target_kernel', 'delayed_frames_kernel', 'aligned_frames_kernel', 'predicted_frames_kernel'):
        assert sum(pinned in name for name in k) == 22, pinned
    for kernel in ('render_discs_kernel', 'disc_features_kernel', 'camera_features_kernel'):
        assert sum(kernel in name for name in k) == 2, kernel
    assert sum('camera_analytical_' in name for name in k) == 9 and sum('camera_believed_' in name for name in k) == 10
    for six in ('scene_baseline_loop_kernel', 'moving_baseline_kernel', 'delayed_baseline_kernel', 'aligned_baseline_kernel', 'predicted_baseline_kernel'):
        assert sum(six in name for name in k) == 6, six
    assert sum('hold_pairs_kernel' in name for name in k) == 1 and sum('delay_line_kernel' in name for name in k) == 1


# ------------------------------------------------------------------------------------------------------------- the restatement
TRIALS = ((0, 0, 0), (2, 0, 2), (3, 3, 3))                           # (d, a, p): no latency, and two of the predicted suite's trials


@pytest.mark.parametrize('method,n_points', sco.ORACLE)
def test_the_logged_restatement_is_the_oracle_loop_and_nothing_else(uvs, method, n_points):
    """Every key but 'x' has camera_predicted_common.estimator_trial's bits; the trials meet pixel_loop_common's preconditions (FAIL-free,
    every disc inside the frame with a mask of at least MASK_MIN pixels, no pixel within RIM_MIN of a rim, calm under the nudge); row k of
    'x' is X_k: row 0 is x0, because step 0's regressor is the zero vector, and the rows move from the first regressor on."""
    for d, a, p in TRIALS:
        t, ref = sco.logged_trial(method, n_points, d, a, p), pc.estimator_trial(method, n_points, d, a, p)
        same_bits(t, ref, ('q', 'f', 'dq', 'err', 'kappa', 'stats', 'x0', 'f0', 'counts', 'pixels', 'fpi_iterations', 'discs'), (method, n_points, d, a, p))
        assert (t['status'], t['k_done']) == (0, sco.K) and t['x'].shape == (sco.K, 2 * n_points * 6)
        nudged = pc.estimator_trial(method, n_points, d, a, p, True)
        drift = max(float(np.abs(ref[key] - nudged[key]).max() / np.abs(ref[key]).max()) for key in ('q', 'f', 'dq', 'err', 'kappa'))
        assert drift <= pl.CALM_TOL and cc.closest_to_rim(t['discs']) > pl.RIM_MIN and inside(t['discs']) and int(t['counts'].min()) >= pl.MASK_MIN
        assert np.array_equal(t['x'][0], t['x0']), 'step 0: the regressor is zero, X_0 = x0'
        assert [np.array_equal(t['x'][k], t['x'][k - 1]) for k in range(1, sco.K)] == [k <= a for k in range(1, sco.K)], \
            'X stays where it is while the regressor is the zero vector (steps 0 .. a), and every later update moves it'
        err = (t['f'] + np.einsum('kij,kj->ki', t['x'].reshape(sco.K, -1, 6),
                                  np.array([sum((t['dq'][i] for i in pc.summed_steps(k, p)), np.zeros(6)) for k in range(sco.K)]))) \
            - np.asarray(pl.DESIRED[:2 * n_points], float)
        assert np.allclose(err, t['err'], rtol=0, atol=1e-9), 'the logged X_k is the matrix the law of step k read'
