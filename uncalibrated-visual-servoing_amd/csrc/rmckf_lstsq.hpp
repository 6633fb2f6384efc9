// Householder least squares of the tuned kernels' control law: lstsq_tall_tuned, and lstsq_tall_emu2 (a quad of lanes with the two-lane solver's bits).
#pragma once
#include "rmckf_math.hpp"
#include "rmckf_rows.hpp"

namespace uvs {

// Householder QR least squares, rows interleaved over the L lanes of a filter: local row r of lane s is global row r*L + s.
// In column c the local row m = c / L is the pivot row on lane c % L, an ordinary "below" row on lanes > c % L and already
// finished on lanes < c % L; rows r > m are below the pivot on every lane -- so all lanes run the same unrolled code and only
// the treatment of row m is selected per lane.
// Returns true when the |R_cc| spread marks the Jacobian as numerically rank-deficient (rmckf_device.hpp, "numpy.linalg.pinv
// semantics"): the caller flags the trial and the careful second pass redoes it; the solution computed here is then discarded.
// nonfinite: some entry of the panel's Jacobian part is NaN or infinite (decided on NaN norms; see the end of the function for +inf).  A non-finite entry of column j reaches, through the reflector
// of an earlier column at the latest, every remaining row of column j, so the squared column norm n2 that column j's own step forms is
// non-finite: the exponent watch sees it for free, and the closed-loop kernel needs no separate finiteness probe of X (24 instructions per step).
template <int M, int N, int L>
UVS_DEV bool lstsq_tall_tuned(double (&a)[M / L][N + 1], int sub, double (&sol)[N], bool &nonfinite, bool certify = false) {
    constexpr int R = M / L;
    double rdiag[N];
    double rmax = 0.0;
    Spread spread;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int m = c / L, owner = c % L;
        const bool is_piv = (L == 1) || (sub == owner);
        const bool is_below = (L > 1) && (sub > owner);
        double sig = is_below ? a[m][c] * a[m][c] : 0.0;
#pragma unroll
        for (int r = m + 1; r < R; ++r) sig = fma(a[r][c], a[r][c], sig);
        sig = pair_sum<L>(sig);
        const double piv = pair_from_dyn<L>(a[m][c], owner);
        const double n2 = fma(piv, piv, sig);
        spread.add(n2);
        double nrm, rn;
        fast_sqrt_rsqrt_1(n2, nrm, rn);                                 // |R_cc| and its reciprocal
        // R_cc = -sign(piv) |column|; v_pivot = piv - R_cc = sign(piv) (|piv| + nrm): sign transfers (v_bfi), no compares or selects.
        // A column that vanished (n2 == 0) sends NaNs through the rest of the solve: nothing guards against it here, because such a trial is
        // marked (spread.lo == 0) and redone by the careful second pass whatever this solve returns.
        const double vp = piv + copysign(nrm, piv);
        // tau = 2 / (v.v) = 1 / (nrm (nrm + |piv|)) = rn / |vp|
        const double tau = rn * fast_rcp_1(fabs(vp));
        const double vm = is_piv ? vp : (is_below ? a[m][c] : 0.0);     // this lane's entry of the Householder vector in row m
#pragma unroll
        for (int j = c + 1; j <= N; ++j) {
            double d = vm * a[m][j];
#pragma unroll
            for (int r = m + 1; r < R; ++r) d = fma(a[r][c], a[r][j], d);
            d = pair_sum<L>(d) * tau;
            a[m][j] = fma(-d, vm, a[m][j]);
            // row c of R is final on its owner lane (the partner holds a row that is finished already, or one whose entries its column's
            // norm bounds): the running largest |R_cj|, one v_max_f64 with |.| modifiers per entry (see Spread::add_largest)
            if (j < N) rmax = fmax(rmax, fabs(a[m][j]));
#pragma unroll
            for (int r = m + 1; r < R; ++r) a[r][j] = fma(-d, a[r][c], a[r][j]);
        }
        rdiag[c] = -copysign(rn, piv);                                  // 1 / R_cc straight from the rsqrt
    }
    if constexpr (L > 1) rmax = fmax(rmax, dpp_quad<kSwapPair>(rmax));
    if constexpr (L == 4) rmax = fmax(rmax, dpp_quad<kSwapHalf>(rmax));
    spread.add_largest(rmax);
#pragma unroll
    for (int c = N - 1; c >= 0; --c) {
        const int m = c / L, owner = c % L;
        double rhs = a[m][N];
#pragma unroll
        for (int j = c + 1; j < N; ++j) rhs = fma(-a[m][j], sol[j], rhs);
        rhs = pair_from_dyn<L>(rhs, owner);
        sol[c] = rhs * rdiag[c];
    }
    // solution growth (Spread::grows, round 5): the largest solution entry against the largest of the top N entries of Q^T y
    double smax = fabs(sol[0]), cmax = 0.0;
#pragma unroll
    for (int c = 1; c < N; ++c) smax = fmax(smax, fabs(sol[c]));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r * L < N) cmax = fmax(cmax, ((r + 1) * L <= N || r * L + sub < N) ? fabs(a[r][N]) : 0.0);
    }
    // (no exchange: a lane's verdict rests on ITS rows of Q^T y -- on lane 0 of the filter, whose mark is the one that is written, global rows
    // 0, L, 2 L, ...; a smaller denominator only marks sooner, and the healthy fixtures stay five orders of magnitude below the gate)
    const bool grows = spread.grows(smax, cmax);
    // (a column that vanished exactly -- lo == 0 -- sends NaNs through the remaining columns by itself: that trial is marked for the careful
    // second pass, which probes X entry by entry, and is not FAILed here)
    // NaN (high dword above +inf's 0x7ff00000) proves a non-finite entry.  A norm of exactly +inf does not: a FINITE entry beyond ~1e154
    // overflows the square, and numpy's SVD does not raise on that -- such a trial is marked for the careful pass (which probes X entry by
    // entry) instead of FAILed here.  An infinite entry in any but the last column turns a later column's norm into NaN (0 * inf in the
    // reflector); in the last column it goes the careful way too and FAILs there, at the same step.
    nonfinite = spread.hi > 0x7ff00000u && spread.lo != 0u;
    bool uncertified = false;
#ifdef UVS_NO_CERTIFICATE               // diagnostic build: A/B of what the cold strict-mode branch costs the plain step (register allocation)
    certify = false;
#endif
    if (__builtin_expect(certify, 0)) {
        // UVS_OPT_STRICT_PINV (round 6): a CERTIFICATE instead of a heuristic.  numpy's pinv (experiment.py:312) drops singular values below
        // 1e-15 sigma_max; when none is that small, pinv(J) y IS the least-squares solution just computed.  cond_2(R) <= |R|_F |R^-1|_F, so the
        // inverse of the triangle, column by column over the rows where they live (the back substitution above, six times, unit right-hand sides),
        // bounds the condition number from ABOVE: below ~2^42 the solve is certified -- a margin of 2^7 to numpy's cutoff for what rounding does to
        // the computed inverse at that conditioning -- and anything else marks the trial for the SVD pass, which then decides by the singular
        // values themselves.  |R|_F^2 <= 21 max^2 comes from the spread's running maximum.  ~170 instructions per step, in strict mode only.
        double inv2 = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double z[N];
            z[k] = rdiag[k];
            inv2 = fma(z[k], z[k], inv2);
#pragma unroll
            for (int c = k - 1; c >= 0; --c) {
                const int m = c / L, owner = c % L;
                double acc = 0.0;
#pragma unroll
                for (int j = c + 1; j <= k; ++j) acc = fma(a[m][j], z[j], acc);
                z[c] = -pair_from_dyn<L>(acc, owner) * rdiag[c];
                inv2 = fma(z[c], z[c], inv2);
            }
        }
        // high dwords add like exponents: certified when max^2 |R^-1|_F^2 < 2^78 up to the fields' slack (a factor 4), i.e. -- with 21 entries in
        // |R|_F^2 -- when cond^2 < 21 * 2^80 < 2^85
        const unsigned long long lhs = (unsigned long long)(unsigned)__double2hiint(inv2) + spread.hi;
        uncertified = !(lhs < 2ull * 0x3ff00000u + (78ull << 20));          // (NaN / inf in either factor compare as "not below")
    }
    return spread.suspect() || spread.hi == 0x7ff00000u || grows || uncertified;
}

template <int M, int N, int L>
UVS_DEV bool lstsq_tall_tuned(double (&a)[M / L][N + 1], int sub, double (&sol)[N]) {
    bool unused;
    return lstsq_tall_tuned<M, N, L>(a, sub, sol, unused);
}

// ------------------------------------------------------------------------------------------------ four lanes, the two-lane kernel's bits
// EMU2: a filter on the four lanes of a quad that reproduces the TWO-lane kernel's arithmetic bit for bit, so that the launcher may pick it for
// batches that do not fill the chip without changing a single result (an N-GPU sweep returns the bits of the 1-GPU sweep).  Quad lane
// `sub` = p + 2 h: p is the parity the two-lane kernel's lane has (u rows / v rows, kinematic half chain), h says which half of that lane's
// four local rows this lane holds (two-lane local row R2 = 2 h + r, global row 2 R2 + p).  Everything lane-local is the two-lane code on half
// the rows; every sum the two-lane kernel forms as a sequential chain over its four local rows is formed here in the same order -- h = 0 starts
// it, hands it to h = 1 (quad_perm [0,1,0,1]), which finishes it; the pair sum across p and a broadcast back (quad_perm [2,3,2,3]) follow.
constexpr int kQuadFromLow = 0x44;       // quad_perm [0,1,0,1]: value of the h = 0 lane of the same parity
constexpr int kQuadFromHigh = 0xEE;      // quad_perm [2,3,2,3]: value of the h = 1 lane of the same parity
// total = (chain finished on the h = 1 lanes) summed over the two parities, delivered to all four lanes
UVS_DEV double emu2_finish(double chain_on_high) {
    // both parities' finished chains fetched independently (quad_perm [2,2,2,2] and [3,3,3,3]) and added: the two-lane kernel's own + partner's,
    // commutative, so every lane holds its bits -- one cross-lane hop on the critical path instead of two (add on the h = 1 lanes, then broadcast)
    return dpp_quad<0xAA>(chain_on_high) + dpp_quad<0xFF>(chain_on_high);
}
// Householder least squares of the 8 x (6 + 1) panel: a[r][.] is the lane's local row r (two-lane local row 2 h + r).  Same operations on the
// same values in the same order as lstsq_tall_tuned<8, 6, 2>; see there for the algorithm and for what `nonfinite` and the return value mean.
template <int M, int N>
UVS_DEV bool lstsq_tall_emu2(double (&a)[2][N + 1], int sub, double (&sol)[N], bool &nonfinite) {
    static_assert(M == 8, "EMU2 splits the four local rows of a two-lane filter over two lanes");
    const int p = sub & 1;
    const bool high = sub & 2;
    double rdiag[N];
    double rmax_lo = 0.0, rmax_hi = 0.0;                            // largest |R_cj| of the rows finished on the h = 0 / h = 1 lanes
    Spread spread;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int m = c / 2, owner = c % 2;                         // two-lane local row of the pivot, parity that owns it
        const int hm = m / 2, rm = m % 2;                           // ... which lives on the h = hm lanes at local row rm
        const bool is_piv = (p == owner), is_below = (p > owner);
        // squared norm of the column below the pivot: two-lane order = (row m if below the pivot), rows m + 1 .. 3 of the lane, then the other parity
        double sig;
        {
            const double seed = is_below ? a[rm][c] * a[rm][c] : 0.0;
            if (hm == 0) {
                double s0 = seed;
                if (rm == 0) s0 = fma(a[1][c], a[1][c], s0);
                double s1 = dpp_quad<kQuadFromLow>(s0);
                s1 = fma(a[0][c], a[0][c], s1);
                s1 = fma(a[1][c], a[1][c], s1);
                sig = emu2_finish(s1);
            } else {
                double s1 = seed;
                if (rm == 0) s1 = fma(a[1][c], a[1][c], s1);
                sig = emu2_finish(s1);
            }
        }
        const double piv = pair_from_dyn<4>(a[rm][c], owner + 2 * hm);
        const double n2 = fma(piv, piv, sig);
        spread.add(n2);
        double nrm, rn;
        fast_sqrt_rsqrt_1(n2, nrm, rn);
        const double vp = piv + copysign(nrm, piv);
        const double tau = rn * fast_rcp_1(fabs(vp));
        const double vm = is_piv ? vp : (is_below ? a[rm][c] : 0.0);     // entry of the Householder vector in two-lane local row m
        // this lane's entries of the vector in its local rows 0, 1: the h = hm lanes hold row m (and, below it, ordinary rows); the h = 1 lanes hold only
        // ordinary rows while hm = 0; the h = 0 lanes are finished once hm = 1 (zero: they neither contribute nor change)
        double v[2];
        if (hm == 0) {
            v[0] = high ? a[0][c] : (rm == 0 ? vm : 0.0);
            v[1] = high ? a[1][c] : (rm == 1 ? vm : a[1][c]);
        } else {
            v[0] = high ? (rm == 0 ? vm : 0.0) : 0.0;
            v[1] = high ? (rm == 1 ? vm : a[1][c]) : 0.0;
        }
#pragma unroll
        for (int j = c + 1; j <= N; ++j) {
            double d1;
            if (hm == 0) {
                double d0 = v[rm] * a[rm][j];
                if (rm == 0) d0 = fma(v[1], a[1][j], d0);
                d1 = dpp_quad<kQuadFromLow>(d0);
                d1 = fma(v[0], a[0][j], d1);
                d1 = fma(v[1], a[1][j], d1);
            } else {
                d1 = v[rm] * a[rm][j];
                if (rm == 0) d1 = fma(v[1], a[1][j], d1);
            }
            const double d = emu2_finish(d1) * tau;
            // rows that are finished stay untouched, as in the two-lane code (a product with a zero entry could still flip the sign of a zero)
            const double u0 = fma(-d, v[0], a[0][j]), u1 = fma(-d, v[1], a[1][j]);
            if (hm == 0) {
                a[0][j] = (rm == 1) ? (high ? u0 : a[0][j]) : u0;
                a[1][j] = u1;
            } else {
                a[0][j] = (rm == 0) ? (high ? u0 : a[0][j]) : a[0][j];
                a[1][j] = high ? u1 : a[1][j];
            }
            if (j < N) { if (hm == 0) rmax_lo = fmax(rmax_lo, fabs(a[rm][j])); else rmax_hi = fmax(rmax_hi, fabs(a[rm][j])); }
        }
        rdiag[c] = -copysign(rn, piv);
    }
    {   // the two-lane kernel's watch: rows 2 m + {0, 1} for every column -- here the h = hm lanes of both parities
        double rmax = fmax(dpp_quad<kQuadFromLow>(rmax_lo), dpp_quad<kQuadFromHigh>(rmax_hi));
        rmax = fmax(rmax, dpp_quad<kSwapPair>(rmax));
        spread.add_largest(rmax);
    }
#pragma unroll
    for (int c = N - 1; c >= 0; --c) {
        const int m = c / 2, owner = c % 2, hm = m / 2, rm = m % 2;
        double rhs = a[rm][N];
#pragma unroll
        for (int j = c + 1; j < N; ++j) rhs = fma(-a[rm][j], sol[j], rhs);
        rhs = pair_from_dyn<4>(rhs, owner + 2 * hm);
        sol[c] = rhs * rdiag[c];
    }
    // solution growth: the two-lane kernel's verdict -- the same maxima on the lane whose mark is written (global rows < N of its parity: both rows of the h = 0 lane, row 0 of the h = 1 lane)
    double smax = fabs(sol[0]), cmax = fabs(a[0][N]);
#pragma unroll
    for (int c = 1; c < N; ++c) smax = fmax(smax, fabs(sol[c]));
    cmax = fmax(cmax, high ? 0.0 : fabs(a[1][N]));
    cmax = fmax(cmax, dpp_quad<kSwapHalf>(cmax));                   // lane 0 of the quad: global rows 0, 2 (its own) and 4 -- the rows of the two-lane kernel's lane 0
    nonfinite = spread.hi > 0x7ff00000u && spread.lo != 0u;
    return spread.suspect() || spread.hi == 0x7ff00000u || spread.grows(smax, cmax);
}

}  // namespace uvs
