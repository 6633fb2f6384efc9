// libuvs_vision.so, third unit: the calibrated IBVS baseline (Method.ANALYTICAL, experiment.py:145-162 and :300-320) THROUGH PIXELS -- one
// step for T trials (uvs_camera_analytical_step_f64) and the pixel closed loop as ONE launch per batch (uvs_camera_analytical_loop_f64).
// The interaction matrix is evaluated from the model at the noisy DETECTED features instead of estimated: camera_jacobian, point_depth,
// feature_jacobian_row and control_law are those of libuvs_rmckf.so, read from its device header; the sensor side is vision_device.hpp.
//
// The step is defined once, in analytical_step (camera_analytical_device.hpp, shared with the believed-model unit), and both kernels call
// it on the same operands; the library compiles with
// -ffp-contract=off, so the loop kernel forms the bits of the stepwise loop (uvs_camera_features_f64, then the step kernel, K times).
//
// Mapping.  A filter of M rows is spread over L lanes as in the estimator kernels (4, 2, 1 lanes at 8, 6, 2 rows): lane `sub` of a trial
// evaluates the camera Jacobian for itself (the same bits in the L lanes: the same operands), then its own R = M / L rows of J into
// Rows::x, and the L lanes solve together in control_law.  There is no covariance: Rows::p is never touched and takes no register.
//   camera_analytical_step_kernel: 64 / L trials per wavefront; padding lanes shadow the last trial, so every cross-lane move of the
//     solver sees a full wavefront, and store nothing.
//   camera_analytical_loop_kernel: the mapping of camera_loop_kernel (uvs_camera_loop.hip), decided and measured there -- 256 threads = one
//     wavefront per SIMD, G = 1 trial per workgroup up to 256 trials and G = 4 beyond, the sensor side as it is there -- with the estimator
//     side of wavefront 0 replaced by the step, for which the sensor side hands the joints over in LDS next to the features.  Every barrier
//     is at the top level of the step loop and reached by all 256 threads; padding and FAILed trials keep computing and store nothing; the
//     one early exit ("every trial of this workgroup has failed") is read by every thread from the same G LDS words.
#include "camera_analytical_device.hpp"

namespace uvs_vision {

constexpr int kALoopTrials = 4;                                  // trials per workgroup of a large batch = wavefronts per workgroup
constexpr int kALoopThreads = 64 * kALoopTrials;
constexpr long long kASmallBatch = 256;                          // up to one trial per compute unit of an MI355X: one trial per workgroup

struct AStepArgs {
    uvs_filter_params fp;
    uvs_camera cam;
    long long T;
    const double *q, *f;
    double *dq_out, *err_out, *j_out;
    int32_t *status;
};

template <int M, int N, int L>
__global__ __launch_bounds__(64) void camera_analytical_step_kernel(const AStepArgs A) {
    constexpr int R = M / L;
    const long long gl = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    long long trial = gl / L;
    const int sub = static_cast<int>(gl % L);
    const bool valid = trial < A.T;
    if (!valid) trial = A.T - 1;                                 // a padding lane shadows the last trial and stores nothing
    double q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j] = A.q[trial * N + j];
    const double *f = A.f + trial * M;
    uvs::Rows<M, N, L> st;
    double err[R], cmd[N];
    const int bad = analytical_step<M, N, L>(A.cam, A.fp, q, [f](int i) { return f[i]; }, sub, st, err, cmd);
    if (!valid) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = sub * R + r;
        A.err_out[trial * M + row] = err[r];
        if (A.j_out != nullptr) {
#pragma unroll
            for (int j = 0; j < N; ++j) A.j_out[(trial * M + row) * N + j] = st.x[r][j];
        }
    }
    if (sub == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) A.dq_out[trial * N + j] = cmd[j];
        A.status[trial] = bad ? UVS_STATUS_FAIL : UVS_STATUS_SUCCESS;
    }
}

struct ALoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;
    long long T;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;                    // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

template <int M, int N, int L, int G>
__global__ __launch_bounds__(kALoopThreads) void camera_analytical_loop_kernel(const ALoopArgs A) {
    constexpr int R = M / L, W = kALoopThreads / 64;
    static_assert((G == 1 || G == W) && W == kColours && G * L <= 64 && N <= UVS_CAMERA_MAX_JOINTS && M <= 2 * kColours, "one or four trials per workgroup");
    __shared__ double s_sin[W][UVS_CAMERA_MAX_JOINTS], s_cos[W][UVS_CAMERA_MAX_JOINTS];   // per wavefront (G = 1: four copies of one trial's)
    __shared__ double s_disc[W][kColours * 3];
    __shared__ double s_q[G][N];                                 // this step's joints, sensor side -> control side
    __shared__ double s_f[G][M];                                 // this step's features, sensor side -> control side
    __shared__ double s_dq[G][N];                                // this step's command, control side -> sensor side
    __shared__ int s_alive[G];                                   // trial has not FAILed, as of the end of this step
    __shared__ int s_pix[G][kColours];                           // smallest mask so far
    __shared__ double s_sum[G][3][M];                            // per-feature ISE, IAE, ITAE after the loop
    // The control side reads the camera from an LDS copy: its 6 x 6 camera Jacobian uses the whole DH table in every step, and held in scalar
    // registers next to the sensor side's the table spilled (36 B of scratch per lane in the four-trial form).  Written once here; the
    // step loop's barriers stand between this and the first read.
    __shared__ uvs_camera s_cam;
    static_assert(sizeof(uvs_camera) % 8 == 0, "copied as doubles");
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(uvs_camera) / 8); i += kALoopThreads)
        reinterpret_cast<double *>(&s_cam)[i] = reinterpret_cast<const double *>(&A.cam)[i];

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
    // this lane's own addresses in row 0 of the [K][T][comp] logs (NULL: not wanted, or nothing of this lane's), advanced by a row per step
    const long long step_rows = T;
    double *q_at = (valid && writer && lane < N && A.q_log != nullptr) ? A.q_log + trial * N + lane : nullptr;
    double *f_at = (valid && lane == 0 && A.f_log != nullptr) ? A.f_log + trial * M : nullptr;
    const double *noise_at = A.noise != nullptr ? A.noise + trial * M : nullptr;
    bool seen = true;                                            // this trial has not FAILed before this step: its rows q[k], f[k] are due
    if (lane < kColours) s_pix[ws][lane] = INT_MAX;

    // control side (wavefront 0): this lane's trial and rows; the lanes from G L on shadow the first ones and store nothing
    const int slot = (lane / L) & (G - 1), sub = lane % L;
    long long etrial = static_cast<long long>(blockIdx.x) * G + slot;
    const bool owner = lane < G * L;
    const bool evalid = owner && etrial < T;
    if (etrial >= T) etrial = T - 1;
    double *err_at = (evalid && A.err_log != nullptr) ? A.err_log + etrial * M + sub * R : nullptr;
    double *dq_at = (evalid && sub == 0 && A.dq_log != nullptr) ? A.dq_log + etrial * N : nullptr;
    double ise[R], iae[R], itae[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ise[r] = iae[r] = itae[r] = 0.0;
    double t = 0.0 + fp.dt;                                      // engine._loop_times: t_s accumulated in floating point
    int status = UVS_STATUS_SUCCESS, k_done = K;
    bool alive = true;

    for (int k = 0; k < K; ++k) {
        // ---- joints: q_k = q_{k-1} + dq_{k-1} * dt, one rounded multiply and one rounded add (joint_sincos)
        if (lane < N) {
            if (k > 0) {
                const double step = s_dq[ws][lane] * fp.dt;
                q = q + step;
            }
            if (seen && q_at != nullptr) *q_at = q;
            if (writer) s_q[ws][lane] = q;
            double s, c;
            sincos(q + cam.theta_offset[lane], &s, &c);
            s_sin[w][lane] = s;
            s_cos[w][lane] = c;
        }
        __syncthreads();
        // ---- projection (camera_features_kernel's)
        if (lane < npts) {
            double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
#pragma unroll 1                                                 // a rolled loop reads the DH table where it is used
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
        // ---- the calibrated law of the workgroup's trials (camera_analytical_step_kernel's sequence)
        if (w == 0) {
            double qk[N], err[R], cmd[N];
#pragma unroll
            for (int j = 0; j < N; ++j) qk[j] = s_q[slot][j];
            uvs::Rows<M, N, L> st;
            const int bad = analytical_step<M, N, L>(s_cam, fp, qk, [slot](int i) { return s_f[slot][i]; }, sub, st, err, cmd);
            if (alive && bad) {                                  // FAIL at this step; the trial stops
                alive = false;
                status = UVS_STATUS_FAIL;
                k_done = k;
            }
            if (alive && evalid) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (err_at != nullptr) err_at[r] = err[r];
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

template <int M, int N, int L>
static void launch_step(hipStream_t s, const AStepArgs &A) {
    const unsigned blocks = static_cast<unsigned>((A.T * L + 63) / 64);
    hipLaunchKernelGGL((camera_analytical_step_kernel<M, N, L>), dim3(blocks), dim3(64), 0, s, A);
}

template <int M, int N, int L>
static void launch_aloop(hipStream_t s, const ALoopArgs &A) {
    if (A.T <= kASmallBatch)
        hipLaunchKernelGGL((camera_analytical_loop_kernel<M, N, L, 1>), dim3(static_cast<unsigned>(A.T)), dim3(kALoopThreads), 0, s, A);
    else
        hipLaunchKernelGGL((camera_analytical_loop_kernel<M, N, L, kALoopTrials>), dim3(static_cast<unsigned>((A.T + kALoopTrials - 1) / kALoopTrials)),
                           dim3(kALoopThreads), 0, s, A);
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_analytical_step_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q, const double *f,
                                   double *dq_out, double *err_out, double *j_out, int32_t *status, void *stream) {
    g_err[0] = '\0';
    if (q == nullptr || f == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q or f");
    if (dq_out == nullptr || err_out == nullptr || status == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL dq_out, err_out or status");
    if (const int rc = check_analytical(fp, cam, T)) return rc;
    if (T == 0) return UVS_OK;
    const AStepArgs A{*fp, *cam, T, q, f, dq_out, err_out, j_out, status};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fp->m == 8) launch_step<8, 6, 4>(s, A);                  // the lane counts of the estimators' step and loop kernels
    else if (fp->m == 6) launch_step<6, 6, 2>(s, A);
    else launch_step<2, 6, 1>(s, A);
    return launched("camera_analytical_step_kernel launch: %s");
}

int uvs_camera_analytical_loop_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start, const double *noise,
                                   double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done,
                                   double *stats, int32_t *pixels, void *stream) {
    g_err[0] = '\0';
    if (q_start == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start");
    if (status == nullptr || k_done == nullptr || stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    if (const int rc = check_analytical(fp, cam, T)) return rc;
    if (fp->steps < 1) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1");
    if (T == 0) return UVS_OK;
    const ALoopArgs A{*fp, *cam, T, q_start, noise, q_log, f_log, dq_log, err_log, status, k_done, stats, pixels};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fp->m == 8) launch_aloop<8, 6, 4>(s, A);
    else if (fp->m == 6) launch_aloop<6, 6, 2>(s, A);
    else launch_aloop<2, 6, 1>(s, A);
    return launched("camera_analytical_loop_kernel launch: %s");
}

}  // extern "C"
