// Calibrated IBVS baseline (Method.ANALYTICAL, experiment.py:145-162 and :300-320): the closed loop with the interaction matrix
// evaluated from the model at every step instead of estimated.  Per step k of a trial:
//   f = project(q) + noise                                  noisy raw-pixel features (experiment.py:130-135)
//   J = J_img(f, |cam - disc|) kron(I2, R^T) J_robot(q)     the initial guess's row formulas with the NOISY u, v (:146-162)
//   dq = -gain pinv(J) (f - f*)                             kappa = 1 (:302-312); pinv raises on a non-finite J -> FAIL, k_done = k
//   q <- q + dq dt                                          (:320)
// No covariance, no filter state: a trial is q, the command and 3 M statistics accumulators.  One lane per trial (the plant, the 6 x N
// camera Jacobian and the 8 x 7 Householder panel all fit one lane's registers, and nothing has to cross lanes), 64 trials per wavefront.
//
// Two passes, as for the estimators (uvs_rmckf.h, above uvs_rmckf_closed_loop_f64): the first solves by Householder least squares with the
// default watches (UVS_OPT_STRICT_PINV: with the certificate) and stops a trial at its first suspect solve, marking it UVS_STATUS_SUSPECT;
// the CAREFUL instantiation re-runs exactly those trials from step 0, probes J entry by entry for the FAIL test and solves every step with
// numpy's pinv semantics (QR finished by a Jacobi SVD of the factor, numpy's cutoff).
#pragma once
#include <hip/hip_runtime.h>
#include "rmckf_device.hpp"
#include "rmckf_lstsq.hpp"

namespace uvs {

struct AnalyticalArgs {
    uvs_filter_params fp;
    uvs_plant plant;
    long long T;
    View q_start, noise, j_out, err_out, q_out, f_out, dq_out;
    double *stats;
    int *status, *k_done;
};

template <int M, int N, bool CAREFUL>
__global__ __launch_bounds__(64) void analytical_kernel(const AnalyticalArgs A) {
    static_assert(M >= N, "the calibrated control law is instantiated for tall Jacobians");
    const long long trial = (long long)blockIdx.x * 64 + threadIdx.x;
    // careful pass: the plant is read from an LDS copy, not kept in scalar registers -- next to the SVD's vector registers the kernel
    // arguments held in SGPRs would spill to scratch
    __shared__ uvs_plant lds_plant;
    if constexpr (CAREFUL) {
        static_assert(sizeof(uvs_plant) % 8 == 0, "copied as doubles");
        for (int i = threadIdx.x; i < (int)(sizeof(uvs_plant) / 8); i += 64)
            reinterpret_cast<double *>(&lds_plant)[i] = reinterpret_cast<const double *>(&A.plant)[i];
        __syncthreads();
    }
    if (trial >= A.T) return;                                               // (one lane per trial: no group shuffles to keep uniform)
    if constexpr (CAREFUL) {
        if (A.status[trial] != UVS_STATUS_SUSPECT) return;
    }
    const uvs_filter_params &fp = A.fp;
    const uvs_plant &pl = CAREFUL ? lds_plant : A.plant;
    const int K = fp.steps;
    const bool certify = (fp.reserved & UVS_OPT_STRICT_PINV) != 0;

    double q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j] = *A.q_start.at(trial, 0, j);
    // statistics accumulators: registers in the first pass; in the careful pass, whose SVD would push them to scratch, LDS (12 KB per workgroup)
    double ise[CAREFUL ? 1 : M], iae[CAREFUL ? 1 : M], itae[CAREFUL ? 1 : M];
    __shared__ double lds_acc[CAREFUL ? 3 * M : 1][64];
    const int lane = threadIdx.x;
#pragma unroll
    for (int r = 0; r < M; ++r) {
        if constexpr (CAREFUL) lds_acc[r][lane] = lds_acc[M + r][lane] = lds_acc[2 * M + r][lane] = 0.0;
        else ise[r] = iae[r] = itae[r] = 0.0;
    }
    double t = fp.dt;                                                       // start() steps the clock once (ur10_simulation.py:57)
    int status = UVS_STATUS_SUCCESS, k_done = K;
    bool flagged = false;

    double nz[M];
#pragma unroll
    for (int r = 0; r < M; ++r) nz[r] = (A.noise.on() && K > 0) ? *A.noise.at(trial, 0, r) : 0.0;

    for (int k = 0; k < K; ++k) {
        double nz_next[M];                                                  // prefetch the next step's noise under this step's arithmetic
#pragma unroll
        for (int r = 0; r < M; ++r) nz_next[r] = (!CAREFUL && A.noise.on() && k + 1 < K) ? *A.noise.at(trial, k + 1, r) : 0.0;
        if constexpr (CAREFUL) {                                            // (careful pass: no prefetch, fewer values live across the SVD)
#pragma unroll
            for (int r = 0; r < M; ++r) nz[r] = A.noise.on() ? *A.noise.at(trial, k, r) : 0.0;
        }

        double rot[9], pos[3], Jc[6][N];
        camera_jacobian<N>(pl, q, rot, pos, Jc);
        double f[M], err[M], J[M][N];
#pragma unroll
        for (int p = 0; p < M / 2; ++p) {
            const double *w = pl.points[p];
            const double u = project_axis(rot, pos, w, 0, pl.focal, pl.center) + nz[2 * p];       // experiment.py:130-135
            const double v = project_axis(rot, pos, w, 1, pl.focal, pl.center) + nz[2 * p + 1];
            const double depth = point_depth(pos, w);                                             // computeZ(4, recalculate_fkine=True)
            feature_jacobian_row<N>(pl.focal, u, v, depth, 0, Jc, J[2 * p]);
            feature_jacobian_row<N>(pl.focal, u, v, depth, 1, Jc, J[2 * p + 1]);
            f[2 * p] = u;
            f[2 * p + 1] = v;
        }
        double a[M][N + 1];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            err[r] = f[r] - fp.desired[r];                                  // experiment.py:302
#pragma unroll
            for (int j = 0; j < N; ++j) a[r][j] = J[r][j];
            a[r][N] = err[r];                                               // kappa = 1 (:306)
        }
        // the step's rows are stored before the solve (J is dead during it; a FAILed step's rows lie at k_done, past what counts)
        if (A.j_out.on()) {
#pragma unroll
            for (int r = 0; r < M; ++r)
#pragma unroll
                for (int j = 0; j < N; ++j) *A.j_out.at(trial, k, r * N + j) = J[r][j];
        }
#pragma unroll
        for (int r = 0; r < M; ++r) {
            if (A.err_out.on()) *A.err_out.at(trial, k, r) = err[r];
            if (A.f_out.on()) *A.f_out.at(trial, k, r) = f[r];
        }
        auto accumulate = [&]() {                                           // ISE / IAE / ITAE terms of a logged step
#pragma unroll
            for (int r = 0; r < M; ++r) {
                const double ae = fabs(err[r]);
                if constexpr (CAREFUL) {
                    lds_acc[r][lane] = fma(err[r], err[r], lds_acc[r][lane]);
                    lds_acc[M + r][lane] += ae;
                    lds_acc[2 * M + r][lane] = fma(t, ae, lds_acc[2 * M + r][lane]);
                } else {
                    ise[r] = fma(err[r], err[r], ise[r]);
                    iae[r] += ae;
                    itae[r] = fma(t, ae, itae[r]);
                }
            }
        };
        double sol[N];
        if constexpr (CAREFUL) {
            bool bad = false;                                               // pinv raises exactly on a non-finite J (:313-316)
#pragma unroll
            for (int r = 0; r < M; ++r)
#pragma unroll
                for (int j = 0; j < N; ++j) bad |= !finite64(J[r][j]);
            if (bad) {
                status = UVS_STATUS_FAIL;
                k_done = k;
                break;
            }
            accumulate();                                                   // (before the SVD: fewer values live across it)
            lstsq_tall<M, N, 1, true>(a, 0, sol);
        } else {
            // nonfinite: a NaN column norm, which only a non-finite entry of J produces -> FAIL at this step; an infinite norm (an inf in the
            // last column, or a finite entry whose square overflows) is "suspect" and the careful pass decides entry by entry
            bool nonfinite = false;
            const bool suspect = lstsq_tall_tuned<M, N, 1>(a, 0, sol, nonfinite, certify);
            if (nonfinite) {
                status = UVS_STATUS_FAIL;
                k_done = k;
                break;
            }
            if (suspect) {                                                  // the careful pass redoes the whole trial: stop here
                flagged = true;
                break;
            }
            accumulate();
        }
        double dq[N];
#pragma unroll
        for (int j = 0; j < N; ++j) dq[j] = -fp.gain * sol[j];             // experiment.py:312
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (A.q_out.on()) *A.q_out.at(trial, k, j) = q[j];
            if (A.dq_out.on()) *A.dq_out.at(trial, k, j) = dq[j];
        }
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = fma(dq[j], fp.dt, q[j]);        // new_q = q + dq * t_s (experiment.py:320)
        t += fp.dt;
#pragma unroll
        for (int r = 0; r < M; ++r) nz[r] = nz_next[r];
    }

    if (!CAREFUL && flagged) {
        A.status[trial] = UVS_STATUS_SUSPECT;
        return;
    }
    double s2[3] = {0.0, 0.0, 0.0};                                         // the same reduction order as the estimators' kernels
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const double e1 = CAREFUL ? lds_acc[r][lane] : ise[r % (CAREFUL ? 1 : M)];
        const double e2 = CAREFUL ? lds_acc[M + r][lane] : iae[r % (CAREFUL ? 1 : M)];
        const double e3 = CAREFUL ? lds_acc[2 * M + r][lane] : itae[r % (CAREFUL ? 1 : M)];
        s2[0] = fma(e1, e1, s2[0]);
        s2[1] = fma(e2, e2, s2[1]);
        s2[2] = fma(e3, e3, s2[2]);
    }
    if (A.stats) {
#pragma unroll
        for (int i = 0; i < 3; ++i) A.stats[3 * trial + i] = sqrt(group_sum<1>(s2[i]));
    }
    A.status[trial] = status;
    if (A.k_done) A.k_done[trial] = k_done;
}

}  // namespace uvs
