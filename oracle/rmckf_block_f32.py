"""Oracle (test infrastructure): ``rmckf_block.BlockFilter.step`` restated in float32 for KF, IMCC-KF and GMCKF.

The reference against which the single-precision replay kernel (uvs_rmckf_replay_f32) is held: not "how far is fp32 from fp64" (that is
what this module MEASURES, against rmckf_block on the same float32 inputs) but "does the kernel owe more error than a plain float32
evaluation of the same formulas does".  So it states the formulas exactly as BlockFilter.step states them -- predict, innovation, the
weights, gain rows, the Joseph update (I - k h^T) P (I - k h^T)^T + k k^T -- and NOT in the kernel's form (P -= beta g g^T, gamma = d / (a d
+ 1), exp2 with a folded constant, reciprocals): an algebraic slip in the kernel's rearrangement is then a disagreement, not a shared habit.

Every operand and every intermediate is float32 (asserted); sums run left to right over explicit multiplies and adds -- no BLAS, no
einsum, so no fused multiply-add and no reordering behind numpy's back.  The one exception is the kernel's own: sigma_k is evaluated in
double and rounded once.  A leading batch axis runs T independent trials at once: X (T, m, n), P (T, m, n, n), Z (T, m), dq (T, n).
MCKF has no single-precision kernel and no restatement here.
"""
import numpy as np

from .rmckf_block import GMCKF, IMCCKF, KF, REG

F32 = np.float32


def _f32(a):
    assert isinstance(a, (np.ndarray, np.floating)) and a.dtype == F32, getattr(a, 'dtype', type(a))
    return a


def _dot(a, b):
    """sum_j a[..., j] b[..., j], left to right, every product and partial sum rounded to float32."""
    acc = _f32(a[..., 0] * b[..., 0])
    for j in range(1, a.shape[-1]):
        acc = _f32(acc + _f32(a[..., j] * b[..., j]))
    return acc


def _matmul(a, b):
    """a @ b over the last two axes, every entry the same plain left-to-right sum."""
    acc = _f32(a[..., :, 0, None] * b[..., 0, None, :])
    for c in range(1, a.shape[-1]):
        acc = _f32(acc + _f32(a[..., :, c, None] * b[..., c, None, :]))
    return acc


class BlockFilterF32:
    def __init__(self, x0, method=GMCKF, kernel_bw=10.0, annealing=False, k_max=300, reg=REG, anneal_span=100.0, m=8, n=6):
        if method not in (KF, IMCCKF, GMCKF):
            raise ValueError(method)
        x0 = _f32(np.asarray(x0))
        self.m, self.n, self.method = m, n, method
        self.kernel_bw, self.annealing, self.k_max, self.anneal_span = kernel_bw, annealing, k_max, anneal_span
        self.reg = F32(reg)
        self.X = x0.reshape(x0.shape[:-1] + (m, n)).copy()
        self.P = np.broadcast_to(np.eye(n, dtype=F32), self.X.shape[:-2] + (m, n, n)).copy()
        self.first = True
        self.sigma = F32(-1.0)

    # the pieces tests/test_replay_f32_oracle.py replaces, one at a time, to show that the gate on the kernel would notice
    def _regressor(self, dq_prev):
        return np.zeros_like(dq_prev) if self.first else dq_prev    # first_run: H = 0 (experiment.py:183-185)

    def _sigma(self, k):
        """sigma_k in double, rounded once (the kernel: (float)bandwidth(fp, k))."""
        return F32(self.kernel_bw + self.anneal_span * (1 - k / self.k_max) if self.annealing else self.kernel_bw)

    def _innovation_norm(self, nu):
        return _f32(np.sqrt(_dot(nu, nu)))

    def _covariance(self, P, kk, g, h):
        """Joseph form, R = 1."""
        A = _f32(np.eye(self.n, dtype=F32) - _f32(kk[..., :, None] * h[..., None, None, :]))      # I - k h^T
        APA = _matmul(_matmul(A, P), np.swapaxes(A, -1, -2))
        return _f32(APA + _f32(kk[..., :, None] * kk[..., None, :]))

    def step(self, Z, dq_prev, k):
        m = self.m
        Z, dq_prev = _f32(np.asarray(Z)), _f32(np.asarray(dq_prev))
        h = _f32(self._regressor(dq_prev))
        self.first = False
        hr = h[..., None, :]                                        # the one regressor, against every row
        P = _f32(self.P + np.eye(self.n, dtype=F32))                # predict
        nu = _f32(Z - _dot(self.X, hr))                             # innovation, row by row
        g = _dot(P, hr[..., None, :])                               # P_i h: (..., m, n)
        a = _dot(g, hr)                                             # h^T P_i h
        one = np.ones(nu.shape, F32)
        kappa = one
        if self.method == KF:
            gain_scale, r = one, one
        elif self.method == IMCCKF:                                 # one scalar weight couples the rows
            self.sigma = self._sigma(k)
            c = _f32(np.exp(_f32(_f32(F32(-0.5) * _f32(self._innovation_norm(nu) ** 2)) / _f32(self.sigma ** 2))))
            gain_scale, r = _f32(one * c[..., None]), one
        else:
            self.sigma = self._sigma(k)
            kappa = _f32(np.exp(_f32(_f32(F32(-0.5) * _f32(nu ** 2)) / _f32(self.sigma ** 2))))
            gain_scale, r = one, _f32(F32(1.0) / _f32(kappa + self.reg))
        s = _f32(_f32(gain_scale * a) + r)
        kk = _f32(_f32(gain_scale / s)[..., None] * g)              # (..., m, n) gain rows
        self.X = _f32(self.X + _f32(kk * nu[..., None]))
        self.P = _f32(self._covariance(P, kk, g, h))
        assert kappa.shape[-1] == m
        return kappa


def run_replay(f_seq, dq_seq, x0, desired_f, method=GMCKF, kernel_bw=10.0, annealing=False, k_max=300, reg=REG, anneal_span=100.0,
               filter_cls=BlockFilterF32):
    """rmckf_block.run_replay without the control law (the kernel solves none), on float32 streams: f_seq (..., K + 1, m), dq_seq (..., K, n),
    x0 (..., m n), desired_f (m,), all float32.  X (..., K, m n), err (..., K, m), kappa (..., K, m) and P_final, float32."""
    f_seq, dq_seq, x0, desired_f = (_f32(np.asarray(v)) for v in (f_seq, dq_seq, x0, desired_f))
    K, m, n = dq_seq.shape[-2], f_seq.shape[-1], dq_seq.shape[-1]
    filt = filter_cls(x0, method, kernel_bw, annealing, k_max, reg, anneal_span, m, n)
    Xs, errs, kaps = [], [], []
    with np.errstate(all='ignore'):                                 # a non-finite trial stays non-finite, quietly
        for k in range(K):
            kappa = filt.step(_f32(f_seq[..., k + 1, :] - f_seq[..., k, :]), dq_seq[..., k, :], k)
            Xs.append(filt.X.reshape(filt.X.shape[:-2] + (m * n,)).copy())
            errs.append(_f32(f_seq[..., k + 1, :] - desired_f))
            kaps.append(kappa.copy())
    return dict(X=_f32(np.stack(Xs, axis=-2)), err=_f32(np.stack(errs, axis=-2)), kappa=_f32(np.stack(kaps, axis=-2)), P_final=_f32(filt.P.copy()))
