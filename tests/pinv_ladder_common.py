"""The control law's promise -- dq = -gain pinv(J) y with numpy's pinv semantics (an SVD, singular values <= 1e-15 sigma_max dropped) -- over the
whole range of condition numbers: a seeded case list per shape, an exact reference in multiprecision, and a gate that is a perturbation bound
instead of a fixed tolerance.  CPU only; test_pinv_ladder_host.py holds the list and the two oracles to it, test_gpu_pinv_ladder.py the kernels.

Case classes (each case: dict(cls, name, J (m, n), y (m,))):
  ladder    J = U diag(s) V^T, U and V random orthogonal, sigma_max = 50; s geometric down to 50 10^-e ('geo') or all 50 but one ('one')
  deficient exact rank deficiency from exact parts: a zero column, a zero row, a column that is twice another, products A B of small-integer
            matrices times a power of two (rank 1, 2, 4 and min(m, n)), J = 0.  Whether a case is deficient depends on the shape (a zero column leaves a
            2 x 6 matrix at rank 2): the side is read off the exact spectrum, never assumed
  scaling   G diag(d) and diag(d) G, G = 50 randn, d graded over 10^-k .. 10^k: badly scaled, not deficient
  kahan     50 Q (I - c N), N the strict upper triangle of ones (m >= n): every entry of the factor ordinary, the inverse explodes like c^(n-1);
            with a generic y and with a y orthogonalised against u_min in multiprecision
  hidden    [[1, t], [0, 1]] (condition ~ t^2 behind a diagonal of ones) embedded by EXACT orthogonal factors -- columns of an integer Hadamard
            matrix -- so that the triangular factor of the QR is the pair itself; transposed for the (2, 6) shape
  scale     three ladder cases times 2^300 and 2^-300

The cutoff band.  Which side of numpy's cutoff an fp64 SVD puts a singular value on is decided by rounding when the exact sigma_i / sigma_max lies
in (2.5e-16, 1e-14); a case is only meaningful outside it, and the committed parameters are chosen so that NO case is inside (the host test
asserts it).  A rounded U diag(s) V^T cannot carry a singular value below ~1e-16 sigma_max, which is why the dropped side uses the exact constructions.

The gate.  For the exact truncated solution x, its condition kappa = sigma_max / (smallest kept sigma), and the residual r = y - J x,
    bound = 2^-53 (kappa |x|_2 + kappa |y|_2 / sigma_max + kappa^2 |r|_2 / sigma_max)
is the first-order perturbation bound of the least-squares problem for a relative backward error of one rounding.  A solver passes at
|x_got - x|_2 <= G bound with G = 16 C, C the worst ratio numpy's own pinv shows over this list (C_NUMPY below, measured on the CPU; the factor 16
covers the kernels' different but equally backward-stable algorithm and their fast reciprocal and rsqrt)."""
import functools

import mpmath as mp
import numpy as np

DPS = 80                                                     # decimal digits of the reference
SHAPES = ((8, 6), (6, 6), (2, 6), (32, 7))
SIGMA_MAX = 50.0
RCOND = 1e-15                                                # numpy.linalg.pinv's default
BAND = (2.5e-16, 1e-14)                                      # exact sigma_i / sigma_max in here: the side is decided by rounding
LADDER_E = (0, 1, 2, 4, 4.5, 5.5, 6, 6.5, 8, 9, 10, 10.5, 11, 12, 13)     # 4.5 / 5.5 / 6.5: around the normal equations' 2^20 gate
SCALING_K = (3, 6)
KAHAN_C = {'kept': (3, 10, 30, 100), 'dropped': (1000, 3000)}
KAHAN_SHIFT = {(7, 100): 60}                                 # (n, c) -> c: at n = 7, c = 100 puts sigma_min at 2.3e-15 sigma_max, inside the band
HIDDEN_T = (1e4, 1e9, 1e12)
SCALE_OF = (('geo', 2), ('one', 8), ('geo', 12))             # the ladder cases that are also run at 2^+-300
CLASSES = ('ladder', 'deficient', 'scaling', 'kahan', 'hidden', 'scale')
HAS_DROPPED = {'deficient', 'kahan', 'hidden'}               # classes that reach below the cutoff (kahan: m >= n only)
NORMAL_EQ_KAPPA, NORMAL_EQ_TOL = 1e6, 1e-8                   # normal-equation routes up to this kappa: max(G bound, 1e-8 |x|_inf), their documented contract
# The worst |np.linalg.pinv(J) y - x|_2 / bound over the case list of all four shapes, measured on the CPU (x86-64, OpenBLAS LAPACK) and rounded
# up; test_pinv_ladder_host.py measures it again and holds it below this figure and below 8.
C_NUMPY = 2.3
G = 16 * C_NUMPY


def _orthogonal(rng, k):
    q, r = np.linalg.qr(rng.standard_normal((k, k)))
    return q * np.sign(np.diag(r))


def _hadamard(k):
    """Integer matrix with k rows and mutually orthogonal columns of equal norm: Sylvester's for a power of two, else 2 x 2 blocks."""
    if k & (k - 1) == 0:
        h = np.ones((1, 1))
        while len(h) < k:
            h = np.block([[h, h], [h, -h]])
        return h
    assert k % 2 == 0
    return np.kron(np.eye(k // 2), np.array([[1.0, 1.0], [1.0, -1.0]]))


def _case(cls, name, J, y):
    J, y = np.ascontiguousarray(J, float), np.ascontiguousarray(y, float)
    J.setflags(write=False)
    y.setflags(write=False)
    return dict(cls=cls, name=name, J=J, y=y)


def _ladder_matrix(rng, m, n, kind, e):
    r = min(m, n)
    s = SIGMA_MAX * 10.0 ** (-e * np.arange(r) / max(r - 1, 1)) if kind == 'geo' else np.r_[np.full(r - 1, SIGMA_MAX), SIGMA_MAX * 10.0 ** -e]
    U, V = _orthogonal(rng, m), _orthogonal(rng, n)
    return (U[:, :r] * s) @ V[:, :r].T


@functools.lru_cache(maxsize=None)
def cases(m, n):
    """The committed case list of the shape, in a fixed order."""
    out = []
    gen = lambda *key: np.random.default_rng([20240607, m, n, *key])                                   # noqa: E731
    yv = lambda rng: 30.0 * rng.standard_normal(m)                                                     # noqa: E731
    # ---- spectral ladder
    for ie, e in enumerate(LADDER_E):
        for ik, kind in enumerate(('geo', 'one')):
            if kind == 'one' and (e == 0 or min(m, n) == 2):                                           # the same matrix as 'geo'
                continue
            rng = gen(0, ie, ik)
            out.append(_case('ladder', f'{kind}_e{e}', _ladder_matrix(rng, m, n, kind, e), yv(rng)))
    # ---- exactly deficient
    rng = gen(1)
    G0 = 50.0 * rng.standard_normal((m, n))
    Z = G0.copy(); Z[:, n // 2] = 0.0
    out.append(_case('deficient', 'zero_col', Z, yv(rng)))
    Z = G0.copy(); Z[m // 2, :] = 0.0
    out.append(_case('deficient', 'zero_row', Z, yv(rng)))
    Z = G0.copy(); Z[:, n - 1] = 2.0 * Z[:, 1]
    out.append(_case('deficient', 'doubled_col', Z, yv(rng)))
    for rank, p in ((1, 3), (2, -2), (4, 5), (min(m, n), 1)):                                          # the last one has full rank: the class's kept side
        A, B = rng.integers(-3, 4, (m, rank)).astype(float), rng.integers(-3, 4, (rank, n)).astype(float)
        out.append(_case('deficient', f'rank{rank}_product_2^{p}', (A @ B) * 2.0 ** p, yv(rng)))
    out.append(_case('deficient', 'zero', np.zeros((m, n)), yv(rng)))
    # ---- bad scaling without deficiency
    rng = gen(2)
    for k in SCALING_K:
        Gs = 50.0 * rng.standard_normal((m, n))
        out.append(_case('scaling', f'cols_k{k}', Gs * 10.0 ** np.linspace(-k, k, n), yv(rng)))
        Gs = 50.0 * rng.standard_normal((m, n))
        out.append(_case('scaling', f'rows_k{k}', Gs * 10.0 ** np.linspace(-k, k, m)[:, None], yv(rng)))
    # ---- Kahan-like
    if m >= n:
        rng = gen(3)
        for c in KAHAN_C['kept'] + KAHAN_C['dropped']:
            c = KAHAN_SHIFT.get((n, c), c)
            Q = _orthogonal(rng, m)[:, :n]
            J = SIGMA_MAX * Q @ (np.eye(n) - c * np.triu(np.ones((n, n)), 1))
            y = yv(rng)
            out.append(_case('kahan', f'c{c}', J, y))
            out.append(_case('kahan', f'c{c}_perp', J, _orthogonalised(J, y)))
    # ---- hidden pair
    rng = gen(4)
    for t in HIDDEN_T:
        if m >= n:
            T = np.eye(n); T[1, 4] = t                                                                 # rows 1, 4 / columns 1, 4 hold [[1, t], [0, 1]]
            J = _hadamard(m)[:, :n] @ T
        else:
            T = np.eye(m); T[1, 0] = t                                                                 # triangular factor of the QR of J^T: [[1, t], [0, 1]]
            J = T @ _hadamard(8)[:n, :m].T
        out.append(_case('hidden', f't{t:g}', J, yv(rng)))
    # ---- global scale
    for i, (kind, e) in enumerate(SCALE_OF):
        if min(m, n) == 2:
            kind = 'geo'
        for sgn in (+1, -1):
            rng = gen(5, i)
            out.append(_case('scale', f'{kind}_e{e}_2^{300 * sgn:+d}', _ladder_matrix(rng, m, n, kind, e) * 2.0 ** (300 * sgn), yv(rng)))
    assert len({c['name'] + c['cls'] for c in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------------------------------------- the exact reference
def _mpv(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, float).ravel()]


def _svd(J):
    """Exact-input SVD at DPS digits: (sigma descending, U columns, V rows) as lists of mpf."""
    with mp.workdps(DPS):
        m, n = J.shape
        if not J.any():
            return [mp.mpf(0)] * min(m, n), None, None
        U, S, V = mp.svd_r(mp.matrix(J.tolist()), compute_uv=True)
        sig = [S[i] for i in range(len(S))]
        us = [[U[r, i] for r in range(m)] for i in range(len(S))]
        vs = [[V[i, c] for c in range(n)] for i in range(len(S))]
        order = sorted(range(len(sig)), key=lambda i: -sig[i])
        return [sig[i] for i in order], [us[i] for i in order], [vs[i] for i in order]


def _orthogonalised(J, y):
    """y minus its component along the left singular vector of the smallest singular value, in multiprecision, rounded once."""
    with mp.workdps(DPS):
        _, us, _ = _svd(J)
        u, yy = us[-1], _mpv(y)
        dot = mp.fsum(a * b for a, b in zip(u, yy))
        return np.array([float(a - dot * b) for a, b in zip(yy, u)])


class Spectrum:
    """The exact SVD of one J with numpy's cutoff applied: what does not depend on y, computed once per case (spectrum(m, n, i))."""

    def __init__(self, J):
        self.J = J
        self.sig, self.us, self.vs = _svd(J)
        smax = self.sig[0]
        self.kept = [i for i, s in enumerate(self.sig) if smax > 0 and s > mp.mpf(RCOND) * smax]
        self.sigma = np.array([float(s) for s in self.sig])
        self.ratios = np.array([float(s / smax) if smax > 0 else 0.0 for s in self.sig])
        self.sigma_max = float(smax)
        self.kappa = float(smax / self.sig[self.kept[-1]]) if self.kept else 1.0
        self.side = 'dropped' if len(self.kept) < len(self.sig) else 'kept'
        self.in_band = bool(np.any((self.ratios > BAND[0]) & (self.ratios < BAND[1])))

    def solve(self, y):
        """For this right-hand side: dict(x (fp64-rounded), x_mp, bound, x_inf, kappa): the truncated pinv solution and its gate's yardstick."""
        with mp.workdps(DPS):
            m, n = self.J.shape
            yy = _mpv(y)
            x = [mp.mpf(0)] * n
            for i in self.kept:
                w = mp.fsum(a * b for a, b in zip(self.us[i], yy)) / self.sig[i]
                x = [xj + w * vj for xj, vj in zip(x, self.vs[i])]
            Jm = [_mpv(row) for row in self.J]
            r = [yy[i] - mp.fsum(a * b for a, b in zip(Jm[i], x)) for i in range(m)]
            nrm = lambda v: mp.sqrt(mp.fsum(a * a for a in v))                                          # noqa: E731
            if self.kept:
                k = mp.mpf(self.sig[0]) / self.sig[self.kept[-1]]
                bound = mp.mpf(2) ** -53 * (k * nrm(x) + k * nrm(yy) / self.sig[0] + k * k * nrm(r) / self.sig[0])
            else:
                bound = mp.mpf(0)                                                                       # J = 0: the command is exactly zero
            xf = np.array([float(v) for v in x])
            return dict(x=xf, x_mp=x, bound=float(bound), x_inf=float(np.abs(xf).max()), kappa=self.kappa)


@functools.lru_cache(maxsize=None)
def spectrum(m, n, i):
    return Spectrum(cases(m, n)[i]['J'])


def deviation(ref, got):
    """|got - x|_2 against the exact x, the difference formed in multiprecision; inf for a non-finite entry."""
    got = np.asarray(got, float).ravel()
    if not np.all(np.isfinite(got)):
        return float('inf')
    with mp.workdps(DPS):
        return float(mp.sqrt(mp.fsum((mp.mpf(float(g)) - x) ** 2 for g, x in zip(got, ref['x_mp']))))


def ratio(ref, got):
    """deviation / bound; 0 where both vanish (J = 0 and an exactly zero command), inf where only the bound does."""
    d = deviation(ref, got)
    return d / ref['bound'] if ref['bound'] > 0 else (0.0 if d == 0 else float('inf'))


def passes(ref, got, normal_equations=False):
    """The gate: G bound; for a normal-equation route up to NORMAL_EQ_KAPPA, max(G bound, 1e-8 |x|_inf)."""
    gate = G * ref['bound']
    if normal_equations and ref['kappa'] <= NORMAL_EQ_KAPPA:
        gate = max(gate, NORMAL_EQ_TOL * ref['x_inf'])
    return deviation(ref, got) <= gate
