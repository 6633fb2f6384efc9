// Lane exchanges (DPP) and the per-row estimator updates on a lane's registers (rmckf_row, the MCKF fixed-point pieces): shared by the tuned closed-loop
// kernel (rmckf_tuned.hpp), the wide kernel (rmckf_wide.hpp), the tuned replay kernels (rmckf_replay_tuned.hpp) and the solvers of rmckf_lstsq.hpp.
#pragma once
#include <type_traits>
#include "rmckf_device.hpp"
#include "rmckf_math.hpp"

namespace uvs {

// DPP quad_perm move of a double (two 32-bit moves).  CTRL = a | b<<2 | c<<4 | d<<6 selects the source lane of each lane of a quad.
template <int CTRL>
UVS_DEV double dpp_quad(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
constexpr int kSwapPair = 0xB1;      // quad_perm [1,0,3,2]: partner lane
constexpr int kFromEven = 0xA0;      // quad_perm [0,0,2,2]: value of the pair's even lane
constexpr int kFromOdd = 0xF5;       // quad_perm [1,1,3,3]: value of the pair's odd lane

constexpr int kSwapHalf = 0x4E;      // quad_perm [2,3,0,1]: the other pair of the quad
// Explicit parking of a double in two AGPRs (the "a" constraint keeps the halves in accumulator registers between put and get).  For state that
// is live THROUGH a register-hungry rare branch: left to itself the allocator keeps such state in VGPRs and runs the branch's own arrays out of
// AGPRs, one v_accvgpr move per use (measured on the MCKF fixed-point branch: 700 moves per firing against 168 with the covariance blocks parked).
struct ParkedDouble { int lo, hi; };
UVS_DEV ParkedDouble agpr_park(double v) {
    ParkedDouble a;
    asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a.lo) : "v"(__double2loint(v)));
    asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a.hi) : "v"(__double2hiint(v)));
    return a;
}
UVS_DEV double agpr_unpark(const ParkedDouble &a) {
    int lo, hi;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(lo) : "a"(a.lo));
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(hi) : "a"(a.hi));
    return __hiloint2double(hi, lo);
}
// DPP row_shr:SH of a double: lane i of a 16-lane row receives lane i - SH (0.0 where that falls out of the row)
template <int SH>
UVS_DEV double dpp_row_shr(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x110 + SH, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x110 + SH, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// Sum over the L (1, 2 or 4) lanes of a filter; every lane gets the bit-identical total.
template <int L>
UVS_DEV double pair_sum(double v) {
    if constexpr (L == 1) return v;
    v += dpp_quad<kSwapPair>(v);
    if constexpr (L == 4) v += dpp_quad<kSwapHalf>(v);
    return v;
}
// Value held by lane OWNER of the group, delivered to all its lanes.
template <int L, int OWNER>
UVS_DEV double pair_from(double v) {
    if constexpr (L == 1) return v;
    if constexpr (L == 2) return OWNER ? dpp_quad<kFromOdd>(v) : dpp_quad<kFromEven>(v);
    return dpp_quad<OWNER * 0x55>(v);                   // quad_perm [o,o,o,o]
}
template <int L>
UVS_DEV double pair_from_dyn(double v, int owner) {      // owner is a compile-time constant after unrolling
    if constexpr (L == 1) return v;
    switch (owner) {
        case 0: return pair_from<L, 0>(v);
        case 1: return pair_from<L, 1>(v);
        case 2: return pair_from<L, (L > 2 ? 2 : 0)>(v);
        default: return pair_from<L, (L > 2 ? 3 : 0)>(v);
    }
}
// Pin a value in a VGPR.  Without it LLVM folds "cond ? a[1] : a[0]" on a register-resident array into a variably indexed
// access, which on AMDGPU means: spill the array to scratch and load it back through memory -- per lane, per step.
UVS_DEV double in_reg(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
// Per-lane choice c ? a : b between two register-resident values, as a select.  Both are pinned BEFORE the choice: with the pin inside the arms
// ("c ? in_reg(a) : in_reg(b)") the volatile asm cannot be speculated and the choice becomes two exec-mask regions -- two saveexec pairs and a
// taken branch per choice, which a lone wavefront pays in full (tools/ubench/control.hip) -- instead of two v_cndmask_b32.  The same bits either way.
// SELECT = false keeps the regions: the kernels that run two wavefronts per SIMD hide them, and IMCC-KF has no register left for the second candidate.
template <bool SELECT>
UVS_DEV double pick2(bool c, double a, double b) {
    if constexpr (!SELECT) return c ? in_reg(a) : in_reg(b);
    a = in_reg(a);
    b = in_reg(b);
    return c ? a : b;
}
// Per-lane choice among the L values v[0..L) by the lane's position in its group.
template <int L>
UVS_DEV double pick_sub(const double *v, int sub) {
    if constexpr (L == 1) return v[0];
    if constexpr (L == 2) return sub ? in_reg(v[1]) : in_reg(v[0]);
    const double lo = (sub & 1) ? in_reg(v[1]) : in_reg(v[0]), hi = (sub & 1) ? in_reg(v[3]) : in_reg(v[2]);
    return (sub & 2) ? hi : lo;
}

// One row of the block-form estimator on a lane's registers: predict P_i + Q, innovation, correntropy weight, gain,
// state update, rank-1 Joseph downdate.  x: row i of X; pb: its packed covariance block; dq: the regressor (the previous command);
// zi: the row's measurement f_i - f_old_i.  chk accumulates 0 * x so that it turns NaN as soon as an entry of X is non-finite.
// Shared by the tuned closed-loop kernel and both tuned replay kernels.
// What the first pass of the fixed-point MCKF (experiment.py:194-250) leaves for the convergence test ||Xc - X|| / ||X|| <= fpi_threshold
// (:244, norms over ALL rows of the filter): the lane's share of both squared norms, and whether a correntropy weight underflowed to 0
// (inv(Cy) raises in the reference and the correction is skipped, :231-236).
struct FpiProbe {
    double num = 0.0, den = 0.0;                                 // num = +inf: not decidable here, leave the trial to the careful pass
    bool skip = false;                                           // a weight Cy underflowed to 0: the whole correction of this step is skipped
    bool poison = false;                                         // a weight of one of the lane's rows is subnormal: NaN gain, the trial FAILs
    bool unsure = false;                                         // ... or sits so close to the underflow that only the careful pass may decide
    double row_gamma = 0.0, row_a = 0.0, row_nu = 0.0;           // first-pass gain, h.P h and innovation of the row just processed
    double row_s2 = 0.0, row_gg = 0.0;                           // (gamma nu)^2 and |g|^2 of that row: the terms of num, for kernels that sum them in another lane order (EMU2)
    bool known = false;                                          // the caller already holds this row's innovation and weight argument (its pre-pass formed them:
    double known_nu = 0.0, known_arg = 0.0;                      // the same operations on the same values) -- the row does not form them again
};
// exp(x) == 0.0 in fp64 exactly when x < ln(2^-1075) = -745.1332191019412076...  The argument itself carries a few ulp of rounding
// (1.6e-13 absolute) that differ between this arithmetic and numpy's, so within 1e-11 of the boundary the tuned kernels do not decide
// themselves but mark the trial for the second pass.  (Round 2 used a band of +-0.005: at alpha = 1 that marked ~8 of 65 536 trials per
// sweep, and the eight lone wavefronts of the second pass took three times as long as the whole first pass.)
constexpr double kExpZeroBelow = -745.1332191019512, kExpNonzeroAbove = -745.1332191019312;
// A weight that is subnormal but not 0 -- at most 2^-1024, so that its reciprocal overflows -- does not make inv(Cy) raise: it returns inf,
// the reference's dense product Br @ inv(Cy) @ Br.T (experiment.py:232) turns 0 * inf into NaN, and the gain, the state and the trial are
// lost (pinv raises in the control law, :312-316: ExperimentStatus.FAIL at this step).  With Cauchy-like noise and the reference's shipped
// parameters that is how ~7 % of its alpha = 1 trials end (innovations between 37.7 and 38.6 sigma; fixtures tests/golden/fpi_*_fail,
// fpi_default_*).  The kernels reproduce it by poisoning the gain of the row.
constexpr double kRcpOverflowsAtOrBelow = 0x1p-1024;
constexpr double kRcpOverflowArg = -709.78271289338397;          // ln(2^-1024): the same boundary on the argument of the exponential
constexpr double kExpArgBand = 1e-11;                            // |argument - boundary| within which the tuned kernels hand the verdict to the careful pass
UVS_DEV double mckf_poison(double gain, double cy) { return (cy <= kRcpOverflowsAtOrBelow) ? __builtin_nan("") : gain; }

// Pre-pass of an MCKF step over the lane's rows: innovation of every row against the prior state, to find out whether some Cy is
// exactly 0 -- inv(Cy) then raises in the reference and the step keeps only the prediction (experiment.py:225-236; with Cauchy-like noise
// that is 1-2 % of the steps, it is not an exotic path).  `probe(r)` returns nu_r^2 * (-1 / (2 sigma^2)), the argument of the weight.
template <int R, typename ArgOfRow>
UVS_DEV void mckf_underflow_prepass(FpiProbe &fpi, ArgOfRow arg_of_row) {
    bool zero = false, unsure = false, poison = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double a = arg_of_row(r);
        zero |= a < kExpZeroBelow;
        unsure |= (a >= kExpZeroBelow) && (a <= kExpNonzeroAbove);    // (a NaN argument is not "unsure": that trial FAILs by itself, no second pass)
        poison |= a < kRcpOverflowArg;                                // decided on the argument: no weight has to stay live for it
        unsure |= fabs(a - kRcpOverflowArg) <= kExpArgBand;           // ... and within rounding of that boundary only the careful pass (which decides on the weight) may say
    }
    fpi.skip = zero;
    fpi.unsure = unsure;
    fpi.poison = poison;                                              // (a zero weight anywhere in the filter wins: inv(Cy) raises first)
}
// The reference's NaN state after a subnormal weight (see kRcpOverflowsAtOrBelow), applied to the finiteness probe of the step: the trial
// FAILs at this step exactly as if its X had turned NaN; what the rows computed instead (a gain of ~0) lands in rows at and after k_done,
// which are unspecified.  skip and poison must already be filter-wide (summed over the lanes of the filter).
UVS_DEV double mckf_poisoned(const FpiProbe &f, double chk) { return (f.poison && !f.skip) ? __builtin_nan("") : chk; }

// Verdict after the rows of a step (num / den summed over the lanes of the filter): true when the first pass is not the whole story --
// a second fixed-point pass would run, the correction would be skipped, or the test is too close to call in different rounding.  The
// tuned kernels then mark the trial and the careful second pass (generic template, full fixed-point iteration) redoes it.  On the
// reference's own configuration (threshold 0.1) every step of every fixture converges in the first pass.
UVS_DEV bool fpi_needs_more(const FpiProbe &f, const uvs_filter_params &fp) {
    const double thr2 = fp.fpi_threshold * fp.fpi_threshold;
    return f.unsure || fp.fpi_epoch_max <= 1 || !(f.num <= thr2 * f.den * (1.0 - 1e-9));
}

// ---- second and later fixed-point passes of the MCKF (experiment.py:215-245), one row (block) at a time on a lane's registers.
// Undo of the optimistic first-pass commit of rmckf_row: from (x_new, P_new) and the row's gamma, a, nu back to the prior x and the
// predicted block P + Q, and the first-pass gain row k1 = gamma (P + Q) h.  P_new h = g (1 - beta a) gives g without a second copy of P.
template <int N>
UVS_DEV void mckf_undo_row(double (&x)[N], double (&pb)[Sym<N>::NP], const double (&h)[N], double gamma, double a, double nu, double (&k1)[N]) {
    const double beta = gamma * (2.0 - gamma * (a + 1.0));
    const double inv = fast_rcp(1.0 - beta * a);                // (1 - gamma a)^2 + gamma^2 a > 0
    double g[N];
#pragma unroll
    for (int l = 0; l < N; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) acc = fma(pb[Sym<N>::at(l, j)], h[j], acc);
        g[l] = acc * inv;
    }
#pragma unroll
    for (int l = 0; l < N; ++l) {
        const double w = beta * g[l];
#pragma unroll
        for (int j = l; j < N; ++j) pb[Sym<N>::at(l, j)] = fma(w, g[j], pb[Sym<N>::at(l, j)]);
        k1[l] = g[l] * gamma;
        x[l] = fma(-k1[l], nu, x[l]);
    }
}
// Lower Cholesky factor of a row's predicted block, packed; the diagonal keeps 1 / L_jj and ljj[] the L_jj themselves.  The predicted block
// does not change between the passes of a step, so a kernel that keeps a row on one lane factors it once per step (round 4 refactored it every pass).
template <int N>
UVS_DEV void mckf_factor_row(const double (&pp)[Sym<N>::NP], double (&Lc)[Sym<N>::NP], double (&ljj)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double dsum = pp[Sym<N>::at(j, j)];
#pragma unroll
        for (int k2 = 0; k2 < j; ++k2) dsum = fma(-Lc[Sym<N>::at(k2, j)], Lc[Sym<N>::at(k2, j)], dsum);
        double lj, rl;
        fast_sqrt_rsqrt(dsum, lj, rl);
        Lc[Sym<N>::at(j, j)] = rl;                               // the diagonal keeps 1 / L_jj: only reciprocals of it are ever needed
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = pp[Sym<N>::at(j, i)];
#pragma unroll
            for (int k2 = 0; k2 < j; ++k2) v = fma(-Lc[Sym<N>::at(k2, i)], Lc[Sym<N>::at(k2, j)], v);
            Lc[Sym<N>::at(j, i)] = v * rl;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) ljj[j] = fast_rcp(Lc[Sym<N>::at(j, j)]);       // L_jj back from its reciprocal
}
// One further pass for one row: current iterate xc = x + k nu0 -> new gain row kn (same arithmetic as Rows::update_mckf in
// rmckf_device.hpp, which the careful / generic kernels run).  dd[l] = xn[l] - xc[l] and xcv[l] = xc[l] are this row's terms of
// ||xn - xc||^2 and ||xc||^2 (the caller sums them in the filter's row order); bad: a weight Cy is 0.
template <int N>
UVS_DEV void mckf_iterate_row(const double (&x)[N], const double (&Lc)[Sym<N>::NP], const double (&ljj)[N], const double (&h)[N], double zi,
                              double neg_half_inv_s2, const double (&k)[N], double (&kn)[N], double (&dd)[N], double (&xcv)[N], bool &bad) {
    double nu0 = zi, xc[N], ex[N], t[N], g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) nu0 = fma(-x[j], h[j], nu0);    // prior innovation (the gain is applied to it, experiment.py:242)
#pragma unroll
    for (int j = 0; j < N; ++j) xc[j] = fma(k[j], nu0, x[j]);
#pragma unroll
    for (int i = 0; i < N; ++i) {                                // L ex = x - xc
        double v = x[i] - xc[i];
#pragma unroll
        for (int k2 = 0; k2 < i; ++k2) v = fma(-Lc[Sym<N>::at(k2, i)], ex[k2], v);
        ex[i] = v * Lc[Sym<N>::at(i, i)];
    }
    double ez = zi;
#pragma unroll
    for (int j = 0; j < N; ++j) ez = fma(-xc[j], h[j], ez);
    const double cy = exp_nonpos((ez * ez) * neg_half_inv_s2);
    bad |= (cy == 0.0);
#pragma unroll
    for (int j = 0; j < N; ++j) {                                // t = Cx^-1 L^T h
        double v = ljj[j] * h[j];
#pragma unroll
        for (int i = j + 1; i < N; ++i) v = fma(Lc[Sym<N>::at(j, i)], h[i], v);
        t[j] = v * fast_rcp(exp_nonpos((ex[j] * ex[j]) * neg_half_inv_s2));    // a Cx of 0 gives inf -> NaN state -> the trial FAILs
    }
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {                                // g = L t = P_hat h
        double v = ljj[i] * t[i];
#pragma unroll
        for (int j = 0; j < i; ++j) v = fma(Lc[Sym<N>::at(j, i)], t[j], v);
        g[i] = v;
        a = fma(h[i], v, a);
    }
    const double gain = mckf_poison(cy * fast_rcp(fma(a, cy, 1.0)), cy);     // cy == 0 is `bad` (the caller skips the correction), not poison
#pragma unroll
    for (int l = 0; l < N; ++l) {
        kn[l] = g[l] * gain;
        dd[l] = fma(kn[l], nu0, x[l]) - xc[l];
        xcv[l] = xc[l];
    }
}
// Final state of a row after the iteration: x + k nu0 and the Joseph form with a gain row that is no longer gamma (P + Q) h
// (experiment.py:297): P - k g^T - g k^T + (h.g + 1) k k^T, g = (P + Q) h.
template <int N>
UVS_DEV void mckf_commit_row(double (&x)[N], double (&pp)[Sym<N>::NP], const double (&h)[N], double zi, const double (&k)[N], double &chk) {
    double nu0 = zi, g[N], a = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) nu0 = fma(-x[j], h[j], nu0);
#pragma unroll
    for (int l = 0; l < N; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) acc = fma(pp[Sym<N>::at(l, j)], h[j], acc);
        g[l] = acc;
        a = fma(h[l], acc, a);
    }
    const double c2 = a + 1.0;
#pragma unroll
    for (int l = 0; l < N; ++l) {
#pragma unroll
        for (int j = l; j < N; ++j) {
            double v = pp[Sym<N>::at(l, j)];
            v = fma(-k[l], g[j], v);
            v = fma(-g[l], k[j], v);
            v = fma(c2 * k[l], k[j], v);
            pp[Sym<N>::at(l, j)] = v;
        }
        x[l] = fma(k[l], nu0, x[l]);
        chk = fma(x[l], 0.0, chk);
    }
}

// Hook: a kernel may hand the row update work that is independent of it -- the streaming stores of values finished earlier -- to be
// issued at N + 1 fixed points spread over the row's arithmetic (hook(integral_constant<int, i>), i = 0..N), each pinned between
// scheduling fences.  A wavefront that issues its stores in one burst stalls at the full store queue while the SIMD has nothing else to run;
// one store every ~20 arithmetic instructions keeps both busy.  NoHook (every other kernel): nothing is emitted, the schedule is hipcc's.
struct NoHook {};
template <int I, typename Hook>
UVS_DEV void row_hook(Hook &hook) {
    if constexpr (!std::is_same<Hook, NoHook>::value) {
        __builtin_amdgcn_sched_barrier(0);
        hook(std::integral_constant<int, I>{});
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Share: KF and IMCC-KF weigh every row of a filter alike (gain factor 1 / (a + 1) resp. c / (c a + 1) with ONE c), so their covariance
// blocks stay identical for all rows: P_i <- P_i + I - beta g g^T with g = (P_i + I) h, and beta a function of h^T g alone.  A kernel may
// keep one block per lane: the leading row runs the full update and leaves g and the gain factor in a RowShare, the other rows of the lane
// only move their x (rmckf_row_follow: 20 instructions instead of 127).  Same operations on the same values: bit-identical results.
struct NoShare {};
template <int N>
struct RowShare { double g[N]; double gamma; };

template <int N, int METHOD, typename Hook, typename Share>
UVS_DEV void rmckf_row(double (&x)[N], double (&pb)[Sym<N>::NP], const double (&dq)[N], double zi, double neg_half_inv_s2, double c_shared,
                       double reg, double &kap, double &chk, FpiProbe &fpi, Hook &hook, Share &share) {
    static_assert(std::is_same<Hook, NoHook>::value || N == 6, "hook points are placed for n = 6");
    double g[N];
    double pred = 0.0;
    row_hook<0>(hook);
    double nu;
    if (METHOD == UVS_METHOD_MCKF && fpi.known) {
        nu = fpi.known_nu;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) pred = fma(x[j], dq[j], pred);
        nu = zi - pred;                                          // innovation (experiment.py:274)
    }
#pragma unroll
    for (int l = 0; l < N; ++l) pb[Sym<N>::at(l, l)] += 1.0;     // P + Q (experiment.py:167)
#pragma unroll
    for (int l = 0; l < N; ++l) {
        double acc = pb[Sym<N>::at(l, 0)] * dq[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = fma(pb[Sym<N>::at(l, j)], dq[j], acc);
        g[l] = acc;
        if (l == 1) row_hook<1>(hook);
        if (l == 3) row_hook<2>(hook);
    }
    row_hook<3>(hook);
    double a = 0.0;
#pragma unroll
    for (int l = 0; l < N; ++l) a = fma(dq[l], g[l], a);
    double gamma;
    if constexpr (METHOD == UVS_METHOD_GMCKF) {
        kap = exp_nonpos((nu * nu) * neg_half_inv_s2);           // utils.py:171-172
        const double d = kap + reg;                              // gamma = 1 / (a + 1/d) = d / (a d + 1) (experiment.py:280-286)
        gamma = d * fast_rcp(fma(a, d, 1.0));
    } else if constexpr (METHOD == UVS_METHOD_MCKF) {
        // first fixed-point pass: Xc = X, so Cx = I and P_hat = P; gain = 1 / (a + 1 / Cy) (experiment.py:225-242).  The state update
        // and the Joseph form below are then exactly those of the other estimators; kappa of the control law is 1 (:303-308)
        const double cy = exp_nonpos(fpi.known ? fpi.known_arg : (nu * nu) * neg_half_inv_s2);
        // skipped correction: X stays, P keeps the prediction (gamma = 0 below).  (A subnormal weight -- fpi.poison -- is not injected here:
        // a select on the gain costs this register-bound kernel 108 B of scratch; the caller FAILs the trial through mckf_poisoned.)
        gamma = fpi.skip ? 0.0 : cy * fast_rcp(fma(a, cy, 1.0));
        kap = 1.0;
        double gg = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) { gg = fma(g[j], g[j], gg); fpi.den = fma(x[j], x[j], fpi.den); }
        const double s = gamma * nu;
        fpi.num = fma(s * s, gg, fpi.num);                       // ||K (Z - H X)||^2 of this row (0 when skipped: no second pass then)
        fpi.row_s2 = s * s;
        fpi.row_gg = gg;
        fpi.row_gamma = gamma;
        fpi.row_a = a;
        fpi.row_nu = nu;
    } else if constexpr (METHOD == UVS_METHOD_IMCCKF) {          // K = c P H^T (c H P H^T + R)^-1 (experiment.py:262-264)
        kap = 1.0;
        gamma = c_shared * fast_rcp(fma(c_shared, a, 1.0));
    } else {                                                     // KF (experiment.py:192)
        kap = 1.0;
        gamma = fast_rcp(a + 1.0);
    }
    row_hook<4>(hook);
    if constexpr (!std::is_same<Share, NoShare>::value) {
        static_assert(METHOD == UVS_METHOD_KF || METHOD == UVS_METHOD_IMCCKF, "only estimators with one gain factor per filter share a block");
#pragma unroll
        for (int j = 0; j < N; ++j) share.g[j] = g[j];
        share.gamma = gamma;
    }
    // MCKF: an INFINITE innovation (a non-finite feature reached the filter) gives Cy = 0, inv(Cy) raises in the reference and the step keeps only
    // the prediction (gamma = 0 above) -- the state survives.  0 * inf must not turn it into NaN here: the innovation is clamped to the largest
    // finite value for the product (two instructions; a NaN innovation still arrives as a NaN gain and FAILs the trial as in the reference).
    const double step = (METHOD == UVS_METHOD_MCKF) ? gamma * fmax(fmin(nu, 1.7976931348623157e308), -1.7976931348623157e308) : gamma * nu;
    const double beta = gamma * (2.0 - gamma * (a + 1.0));
#pragma unroll
    for (int j = 0; j < N; ++j) {
        x[j] = fma(g[j], step, x[j]);                            // X + K (Z - H X) (experiment.py:291)
        chk = fma(x[j], 0.0, chk);
    }
    row_hook<5>(hook);
#pragma unroll
    for (int l = 0; l < N; ++l) {                                // Joseph update with R = 1: P -= beta g g^T
        const double w = beta * g[l];
#pragma unroll
        for (int j = l; j < N; ++j) pb[Sym<N>::at(l, j)] = fma(-w, g[j], pb[Sym<N>::at(l, j)]);
        if (l == 1) row_hook<6>(hook);
    }
}

template <int N, int METHOD, typename Hook>
UVS_DEV void rmckf_row(double (&x)[N], double (&pb)[Sym<N>::NP], const double (&dq)[N], double zi, double neg_half_inv_s2, double c_shared,
                       double reg, double &kap, double &chk, FpiProbe &fpi, Hook &hook) {
    NoShare none;
    rmckf_row<N, METHOD>(x, pb, dq, zi, neg_half_inv_s2, c_shared, reg, kap, chk, fpi, hook, none);
}

template <int N, int METHOD>
UVS_DEV void rmckf_row(double (&x)[N], double (&pb)[Sym<N>::NP], const double (&dq)[N], double zi, double neg_half_inv_s2, double c_shared,
                       double reg, double &kap, double &chk, FpiProbe &fpi) {
    NoHook none;
    rmckf_row<N, METHOD>(x, pb, dq, zi, neg_half_inv_s2, c_shared, reg, kap, chk, fpi, none);
}

// A row whose covariance block is the leading row's (see RowShare): innovation and state update only (experiment.py:274, 291).
template <int N>
UVS_DEV void rmckf_row_follow(double (&x)[N], const RowShare<N> &share, const double (&dq)[N], double zi, double &chk) {
    double pred = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) pred = fma(x[j], dq[j], pred);
    const double step = share.gamma * (zi - pred);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        x[j] = fma(share.g[j], step, x[j]);
        chk = fma(x[j], 0.0, chk);
    }
}

template <int N, int METHOD>
UVS_DEV void rmckf_row(double (&x)[N], double (&pb)[Sym<N>::NP], const double (&dq)[N], double zi, double neg_half_inv_s2, double c_shared,
                       double reg, double &kap, double &chk) {
    static_assert(METHOD != UVS_METHOD_MCKF, "MCKF rows need the fixed-point probe");
    FpiProbe unused;
    rmckf_row<N, METHOD>(x, pb, dq, zi, neg_half_inv_s2, c_shared, reg, kap, chk, unused);
}

}  // namespace uvs
