// libuvs_vision.so, second unit: the pixel closed loop (engine.camera_closed_loop) as ONE launch per batch, and its analytic initial guess.
// The estimator is the one of libuvs_rmckf.so, read from its device header (Rows::update, control_law, bandwidth, camera_jacobian,
// feature_jacobian_row); the sensor side is vision_device.hpp.  Both libraries compile with -ffp-contract=off, so every value this unit
// forms has the bits the two-launch loop (uvs_camera_features_f64, then uvs_rmckf_step_f64, K times) forms.
//
// Mapping of camera_loop_kernel.  A workgroup of 256 threads = four wavefronts is alone on its compute unit (one wavefront per SIMD, so the
// kernel may take the whole register file: the estimator state alone is 108 dwords per lane at (8,6,4)).  It carries G trials:
//   G = 4, batches of more than 256 trials: wavefront w owns trial w of the workgroup on the sensor side;
//   G = 1, batches of up to 256 trials (one per compute unit of an MI355X): the four wavefronts share one trial, each repeats the short
//     projection for itself and detects every fourth feature pair (one colour each), so a step's detection takes a quarter of the time.
//   sensor side, every step: lane i < n advances joint i and takes its sine and cosine, lane p < n_points multiplies the links and projects
//     its disc into LDS, then the 64 lanes walk the (colour, 64-index block) pairs of centre_of_mass in its order -- only the blocks the disc's
//     clipped bounding box touches; every other one has the exact partial +0.0 -- and lane 0 finishes the colour: the features go to LDS and
//     to the log.
//   estimator side, every step: wavefront 0 alone.  Lanes L slot + sub, sub < L, are the L lanes of the workgroup's trial `slot`; the lanes
//     from G L on shadow those (same slot modulo G) so that every cross-lane move has a full wavefront, and store nothing.  State (X, P),
//     previous features, previous command and the error sums stay in registers over all K steps.
// Barriers hand the sines, the discs, the features and the command over.  Every barrier is reached by all 256 threads the same number of
// times: no thread leaves the step loop on its own -- a FAILed trial or a padding trial (which shadows trial T - 1) goes on computing and
// stores nothing -- and the one early exit, "every trial of this workgroup has failed", is read by every thread from the same G LDS words
// after the last barrier of the step, before anything rewrites them.
#include "../csrc/rmckf_device.hpp"

#include <climits>

#include "uvs_vision.h"
#include "vision_device.hpp"

namespace uvs_vision {

constexpr int kLoopTrials = 4;                                   // trials per workgroup of a large batch = wavefronts per workgroup
constexpr int kLoopThreads = 64 * kLoopTrials;
constexpr long long kSmallBatch = 256;                           // up to one trial per compute unit of an MI355X: one trial per workgroup
constexpr int kJoints = 6;                                       // the DH arms of this project (camera_jacobian<6>)

struct LoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;
    long long T;
    const double *q_start, *noise, *x0, *f0;
    double *q_log, *f_log, *dq_log, *err_log, *kappa_log;        // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

template <int M, int N, int L, int METHOD_T, int G>
__global__ __launch_bounds__(kLoopThreads) void camera_loop_kernel(const LoopArgs A) {
    constexpr int R = M / L, W = kLoopThreads / 64;
    static_assert((G == 1 || G == W) && W == kColours && G * L <= 64 && N <= UVS_CAMERA_MAX_JOINTS && M <= 2 * kColours, "one or four trials per workgroup");
    __shared__ double s_sin[W][UVS_CAMERA_MAX_JOINTS], s_cos[W][UVS_CAMERA_MAX_JOINTS];   // per wavefront (G = 1: four copies of one trial's)
    __shared__ double s_disc[W][kColours * 3];
    __shared__ double s_f[G][M];                                 // this step's features, sensor side -> estimator side
    __shared__ double s_dq[G][N];                                // this step's command, estimator side -> sensor side
    __shared__ int s_alive[G];                                   // trial has not FAILed, as of the end of this step
    __shared__ int s_pix[G][kColours];                           // smallest mask so far
    __shared__ double s_sum[G][3][M];                            // per-feature ISE, IAE, ITAE after the loop
    // Three rows per lane, (6,6,2): X, P and the careful solve's two n x n matrices do not fit 512 registers together.  The control law reads X
    // alone, so wavefront 0 parks P in LDS around it (plane [entry][lane]: consecutive lanes, consecutive banks).
    constexpr bool PARK = R * uvs::Sym<N>::NP > 42;
    __shared__ double s_park[PARK ? R * uvs::Sym<N>::NP : 1][PARK ? 64 : 1];

    const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const uvs_filter_params &fp = A.fp;
    const uvs_camera &cam = A.cam;
    const long long T = A.T;
    const int K = fp.steps, npts = cam.n_points;

    // sensor side: this wavefront's trial, and the feature pairs it detects: all of its own trial's, or every fourth of the workgroup's one trial
    const int ws = G == 1 ? 0 : w;
    const bool writer = G == W || w == 0;                        // G = 1: the four wavefronts hold the same joints; the first one logs them
    const int j_first = G == 1 ? w : 0, j_step = G == 1 ? W : 1;
    long long trial = static_cast<long long>(blockIdx.x) * G + ws;
    const bool valid = trial < T;
    if (!valid) trial = T - 1;                                   // a padding wavefront shadows the last trial and stores nothing
    double q = lane < N ? A.q_start[trial * N + lane] : 0.0;
    // Row k of a [K][T][comp] log is step_rows * comp doubles past row k - 1.  The cursors below are this lane's own addresses in row 0 (NULL for
    // a log that is not wanted, or where this lane has nothing to store), kept in vector registers: fifteen pointers as scalars did not fit.
    const long long step_rows = T;
    double *q_at = (valid && writer && lane < N && A.q_log != nullptr) ? A.q_log + trial * N + lane : nullptr;
    double *f_at = (valid && lane == 0 && A.f_log != nullptr) ? A.f_log + trial * M : nullptr;
    const double *noise_at = A.noise != nullptr ? A.noise + trial * M : nullptr;
    bool seen = true;                                            // this trial has not FAILed before this step: its rows q[k], f[k] are due
    if (lane < kColours) s_pix[ws][lane] = INT_MAX;

    // estimator side (wavefront 0): this lane's trial and rows
    const int slot = (lane / L) & (G - 1), sub = lane % L;
    long long etrial = static_cast<long long>(blockIdx.x) * G + slot;
    const bool owner = lane < G * L;                             // the lanes beyond shadow these
    const bool evalid = owner && etrial < T;
    if (etrial >= T) etrial = T - 1;
    double *err_at = (evalid && A.err_log != nullptr) ? A.err_log + etrial * M + sub * R : nullptr;
    double *kappa_at = (evalid && A.kappa_log != nullptr) ? A.kappa_log + etrial * M + sub * R : nullptr;
    double *dq_at = (evalid && sub == 0 && A.dq_log != nullptr) ? A.dq_log + etrial * N : nullptr;
    uvs::Rows<M, N, L> st;
    st.init_cov();
    double f_prev[R], des[R], dq[N], ise[R], iae[R], itae[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = sub * R + r;
        des[r] = fp.desired[row];
        f_prev[r] = A.f0[etrial * M + row];
        ise[r] = iae[r] = itae[r] = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) st.x[r][j] = A.x0[(etrial * M + row) * N + j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) dq[j] = 0.0;                     // first step: H = 0 (experiment.py:183)
    double t = 0.0 + fp.dt;                                      // engine._loop_times: t_s accumulated in floating point
    int status = UVS_STATUS_SUCCESS, k_done = K;
    bool alive = true;
    const bool strict = (fp.reserved & UVS_OPT_STRICT_PINV) != 0;

    for (int k = 0; k < K; ++k) {
        // ---- joints: q_k = q_{k-1} + dq_{k-1} * dt, one rounded multiply and one rounded add (joint_sincos)
        if (lane < N) {
            if (k > 0) {
                const double step = s_dq[ws][lane] * fp.dt;
                q = q + step;
            }
            if (seen && q_at != nullptr) *q_at = q;
            double s, c;
            sincos(q + cam.theta_offset[lane], &s, &c);
            s_sin[w][lane] = s;
            s_cos[w][lane] = c;
        }
        __syncthreads();
        // ---- projection (camera_features_kernel's)
        if (lane < npts) {
            double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
#pragma unroll 1                                                 // a rolled loop reads the DH table where it is used: unrolled, the whole table sits in SGPRs
            for (int i = 0; i < cam.n_joints; ++i) chain_link(cam, i, s_sin[w][i], s_cos[w][i], pose);
            project_disc(cam, lane, pose, &s_disc[w][3 * lane]);
        }
        __syncthreads();
        // ---- frame-free detection: feature pair j is the centre of mass of disc j's colour
#pragma unroll 1
        for (int j = j_first; j < npts; j += j_step) {
            const Disc me = load_disc(&s_disc[w][3 * j], true);  // disc j shows colour j (npts == 1: green)
            int x0, x1, y0, y1;
            disc_box(me, x0, x1, y0, y1);
            ColourSum sum;
#pragma unroll 1
            for (int b = 0; b < 4; ++b) {                        // the colour's four wavefronts of centre_of_mass, in index order
                const int lo = 64 * b, hi = lo + 63;
                // outside the clipped box disc_counts_at returns (0, 0) for all 64 indices, whose partial is (+0.0, +0.0, 0)
                const bool touched = me.r2 >= 0.0 && ((x0 <= hi && x1 >= lo) || (y0 <= hi && y1 >= lo));
                double su = 0.0, sv = 0.0;
                int n = 0;
                if (__builtin_amdgcn_readfirstlane(static_cast<int>(touched))) {   // the same discs in every lane: wavefront-uniform
                    int cc, rc;
                    disc_counts_in_box(s_disc[w], npts, j, me, x0, x1, y0, y1, lo + lane, cc, rc);
                    wave_partial(cc, rc, lo + lane, su, sv, n);
                }
                sum.add(su, sv, n);
            }
            if (lane == 0) {                                     // the lane the shuffle tree ends in
                double u, v;
                sum.centre(u, v);
                if (noise_at != nullptr) {                       // f += noise (experiment.py:135)
                    u += noise_at[2 * j];
                    v += noise_at[2 * j + 1];
                }
                s_f[ws][2 * j] = u;
                s_f[ws][2 * j + 1] = v;
                if (seen) {
                    s_pix[ws][j] = sum.count < s_pix[ws][j] ? sum.count : s_pix[ws][j];
                    if (f_at != nullptr) {
                        f_at[2 * j] = u;
                        f_at[2 * j + 1] = v;
                    }
                }
            }
        }
        __syncthreads();
        // ---- estimator and control law of the workgroup's four trials (step_kernel's sequence)
        if (w == 0) {
            double z[R], err[R], kap[R], cmd[N];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double fv = s_f[slot][sub * R + r];
                z[r] = fv - f_prev[r];
                f_prev[r] = fv;
                err[r] = fv - des[r];
            }
            st.template update<METHOD_T>(fp, z, dq, uvs::bandwidth(fp, k), kap);   // h = the previous command; zero on k = 0
            const int bad = st.any_nonfinite();
            if (alive && bad) {                                  // FAIL at this step; the trial stops
                alive = false;
                status = UVS_STATUS_FAIL;
                k_done = k;
            }
            if constexpr (PARK) {
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int e = 0; e < uvs::Sym<N>::NP; ++e) s_park[r * uvs::Sym<N>::NP + e][lane] = st.p[r][e];
                asm volatile("" ::: "memory");                   // the loads below are loads: nothing of P is carried in registers
            }
            const bool suspect = strict || uvs::control_law<M, N, L, false>(st, kap, err, fp.gain, sub, cmd);
            if (__any(suspect)) {                                // the careful solve for a filter whose watch fires, or for every one when strict
                double careful[N];
                uvs::control_law<M, N, L, true>(st, kap, err, fp.gain, sub, careful);
#pragma unroll
                for (int j = 0; j < N; ++j) cmd[j] = suspect ? careful[j] : cmd[j];
            }
            if constexpr (PARK) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int e = 0; e < uvs::Sym<N>::NP; ++e) st.p[r][e] = s_park[r * uvs::Sym<N>::NP + e][lane];
            }
            if (alive && evalid) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (err_at != nullptr) err_at[r] = err[r];
                    if (kappa_at != nullptr) kappa_at[r] = kap[r];
                    const double ae = fabs(err[r]);              // stats_kernel's sums, in its order over k
                    ise[r] = fma(err[r], err[r], ise[r]);
                    iae[r] += ae;
                    itae[r] = fma(t, ae, itae[r]);
                }
                if (dq_at != nullptr) {
#pragma unroll
                    for (int j = 0; j < N; ++j) dq_at[j] = cmd[j];
                }
            }
#pragma unroll
            for (int j = 0; j < N; ++j) dq[j] = cmd[j];
            if (owner && sub == 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) s_dq[slot][j] = cmd[j];
                s_alive[slot] = alive ? 1 : 0;
            }
        }
        __syncthreads();
        t += fp.dt;
        if (q_at != nullptr) q_at += step_rows * N;
        if (f_at != nullptr) f_at += step_rows * M;
        if (noise_at != nullptr) noise_at += step_rows * M;
        if (err_at != nullptr) err_at += step_rows * M;
        if (kappa_at != nullptr) kappa_at += step_rows * M;
        if (dq_at != nullptr) dq_at += step_rows * N;
        seen = s_alive[ws] != 0;
        int any_alive = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) any_alive |= s_alive[g];
        if (any_alive == 0) break;                               // the same G words in all 256 threads: a uniform exit
    }

    if (w == 0 && owner) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            s_sum[slot][0][sub * R + r] = ise[r];
            s_sum[slot][1][sub * R + r] = iae[r];
            s_sum[slot][2][sub * R + r] = itae[r];
        }
        if (evalid && sub == 0) {
            A.status[etrial] = status;
            A.k_done[etrial] = k_done;
        }
    }
    __syncthreads();
    if (lane < 3 && valid && writer) {                           // lane i: the norm over the features in order, as stats_kernel forms it
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc = fma(s_sum[ws][lane][i], s_sum[ws][lane][i], acc);
        A.stats[3 * trial + lane] = sqrt(acc);
    }
    if (lane < npts && valid && writer && A.pixels != nullptr) A.pixels[trial * npts + lane] = s_pix[ws][lane];
}

// The analytic initial guess of plant.analytic_guess, one lane per trial: the geometric Jacobian in the camera frame at q_start, the depths
// |camera - point|, and the image Jacobian rows at the DETECTED features.
__global__ __launch_bounds__(64) void camera_guess_kernel(const uvs_camera cam, long long T, const double *__restrict__ q_start,
                                                          const double *__restrict__ f0, double *__restrict__ x0_out) {
    constexpr int N = kJoints;
    const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    if (t >= T) return;
    uvs_plant pl;                                                // camera_jacobian reads the DH table alone
    double q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pl.theta_offset[i] = cam.theta_offset[i];
        pl.d[i] = cam.d[i];
        pl.a[i] = cam.a[i];
        pl.cos_alpha[i] = cam.cos_alpha[i];
        pl.sin_alpha[i] = cam.sin_alpha[i];
        q[i] = q_start[t * N + i];
    }
    double rot[9], pos[3], Jc[6][N];
    uvs::camera_jacobian<N>(pl, q, rot, pos, Jc);
    const int m = 2 * cam.n_points;
    for (int p = 0; p < cam.n_points; ++p) {
        const double depth = uvs::point_depth(pos, cam.points[p]);
        const double u = f0[t * m + 2 * p], v = f0[t * m + 2 * p + 1];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double x[N];
            uvs::feature_jacobian_row<N>(cam.focal, u, v, depth, half, Jc, x);
#pragma unroll
            for (int j = 0; j < N; ++j) x0_out[(t * m + 2 * p + half) * N + j] = x[j];
        }
    }
}

// MCKF: the fixed-point iteration's working set next to three rows per lane spills at (6,6,2) (684 B of scratch per lane), so that one
// instantiation is not built and the entry point refuses it; at (8,6,4) and (2,6,1) it has none and is built.
template <int M, int N, int L, bool WITH_MCKF>
bool launch_loop(int method, hipStream_t s, const LoopArgs &A) {
    const bool small = A.T <= kSmallBatch;
    const unsigned blocks = static_cast<unsigned>(small ? A.T : (A.T + kLoopTrials - 1) / kLoopTrials);
#define UVS_LOOP_METHOD(METHOD)                                                                                                          \
    if (method == METHOD) {                                                                                                              \
        if (small) hipLaunchKernelGGL((camera_loop_kernel<M, N, L, METHOD, 1>), dim3(blocks), dim3(kLoopThreads), 0, s, A);               \
        else hipLaunchKernelGGL((camera_loop_kernel<M, N, L, METHOD, kLoopTrials>), dim3(blocks), dim3(kLoopThreads), 0, s, A);           \
        return true;                                                                                                                     \
    }
    UVS_LOOP_METHOD(UVS_METHOD_GMCKF)
    UVS_LOOP_METHOD(UVS_METHOD_KF)
    UVS_LOOP_METHOD(UVS_METHOD_IMCCKF)
    if constexpr (WITH_MCKF) {
        UVS_LOOP_METHOD(UVS_METHOD_MCKF)
    }
#undef UVS_LOOP_METHOD
    return false;
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start, const double *noise,
                               const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                               double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    g_err[0] = '\0';
    if (fp == nullptr || cam == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp or cam");
    if (q_start == nullptr || x0 == nullptr || f0 == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start, x0 or f0");
    if (status == nullptr || k_done == nullptr || stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (fp->steps < 1 || fp->k_max <= 0) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1 and k_max > 0");
    if (cam->n_joints < 1 || cam->n_joints > UVS_CAMERA_MAX_JOINTS) return fail(UVS_ERR_ARG, "%s", "n_joints must be 1 .. 8");
    if (!colours_ok(cam->n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (fp->method != UVS_METHOD_KF && fp->method != UVS_METHOD_MCKF && fp->method != UVS_METHOD_IMCCKF && fp->method != UVS_METHOD_GMCKF)
        return fail(UVS_ERR_METHOD, "%s", "method must be KF, MCKF, IMCCKF or GMCKF (the calibrated baseline's pixel loop is uvs_camera_analytical_loop_f64)");
    if (fp->method == UVS_METHOD_MCKF && fp->fpi_epoch_max < 1) return fail(UVS_ERR_ARG, "%s", "MCKF needs fpi_epoch_max >= 1");
    if (fp->lanes_per_filter != 0) return fail(UVS_ERR_SHAPE, "%s", "lanes_per_filter must be 0: the loop kernel has one mapping per shape");
    if (fp->m != 2 * cam->n_points) return fail(UVS_ERR_SHAPE, "%s", "fp->m must be 2 * cam->n_points");
    if (fp->n != cam->n_joints) return fail(UVS_ERR_SHAPE, "%s", "fp->n must be cam->n_joints");
    if (fp->n != kJoints || (fp->m != 8 && fp->m != 6 && fp->m != 2)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    if (fp->method == UVS_METHOD_MCKF && fp->m == 6) return fail(UVS_ERR_METHOD, "%s", "MCKF is not built at (6, 6): use the two-launch loop");
    if (T == 0) return UVS_OK;
    const LoopArgs A{*fp, *cam, T, q_start, noise, x0, f0, q_log, f_log, dq_log, err_log, kappa_log, status, k_done, stats, pixels};
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool ok = false;
    if (fp->m == 8) ok = launch_loop<8, 6, 4, true>(fp->method, s, A);       // the lane counts uvs_rmckf_step_f64 resolves for lanes_per_filter == 0
    else if (fp->m == 6) ok = launch_loop<6, 6, 2, false>(fp->method, s, A);
    else if (fp->m == 2) ok = launch_loop<2, 6, 1, true>(fp->method, s, A);
    if (!ok) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched("camera_loop_kernel launch: %s");
}

int uvs_camera_guess_f64(const uvs_camera *cam, int64_t T, const double *q_start, const double *f0, double *x0_out, void *stream) {
    g_err[0] = '\0';
    if (cam == nullptr || q_start == nullptr || f0 == nullptr || x0_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL cam, q_start, f0 or x0_out");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(cam->n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (cam->n_joints != kJoints) return fail(UVS_ERR_SHAPE, "%s", "the analytic guess is instantiated for 6 joints");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(camera_guess_kernel, dim3(static_cast<unsigned>((T + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), *cam,
                       static_cast<long long>(T), q_start, f0, x0_out);
    return launched("camera_guess_kernel launch: %s");
}

}  // extern "C"
