// libuvs_vision.so, fourth unit: the calibrated IBVS baseline on a WRONG model, per trial.  The sensor side of the pixel loop projects and
// detects with the camera that renders the frames; the control side evaluates its interaction matrix from a model.  In
// uvs_camera_analytical.hip the two are one struct; here the second is `believed[...]`, a device array of uvs_camera structs out of which
// every trial picks its own (through an index, or by its trial number, or the one struct there is), so that a robustness curve --
// miscalibration level x trials -- is one launch.  A wrong model is a uvs_camera with other numbers in it: no kernel knows a miscalibration knob.
//
// The step is analytical_step of camera_analytical_device.hpp, the one definition; with believed == the true camera every kernel here
// gives the bits of its calibrated counterpart.
//
// Where the model lives.  In the calibrated kernels it is a kernel argument: uniform, in scalar registers.  Per trial it would be per lane,
// about 90 dwords on top of the 240 / 254 VGPRs of the (8,6,4) / (6,6,2) step forms.  So every kernel that runs the step stages its trials'
// models through LDS (472 B each) once, before the first step, and analytical_step reads s_cam[slot] where it uses a value:
//   camera_believed_step_kernel: the mapping of camera_analytical_step_kernel (64 / L trials per wavefront, padding lanes shadow the last
//     trial and store nothing) with the 64 / L models of the wavefront in LDS: 7 552 B, 15 104 B, 30 208 B at L = 4, 2, 1.
//   camera_believed_loop_kernel: the mapping of camera_analytical_loop_kernel (256 threads, G = 1 trial per workgroup up to 256 trials and
//     G = 4 beyond, four barriers per step at the top level, one uniform early exit) with s_cam[G] in place of its one s_cam.  The sensor
//     side keeps reading the true camera from the kernel arguments.
//   camera_believed_guess_kernel: camera_guess_kernel's arithmetic, one lane per trial, the model read from memory where it is used.
//
// An index outside [0, n_believed) never becomes an address: model_of returns -1 for it, the staging loop writes zeros in its place (the
// lanes of that trial keep computing on them: every cross-lane move of the solver sees a full wavefront), and the trial is FAILed by the
// flag, not by what the zeros give: status FAIL (the loop: k_done = 0) and not one other store.
#include "camera_analytical_device.hpp"

namespace uvs_vision {

constexpr int kBLoopTrials = 4;                                  // as uvs_camera_analytical.hip
constexpr int kBLoopThreads = 64 * kBLoopTrials;
constexpr long long kBSmallBatch = 256;
constexpr int kCamWords = static_cast<int>(sizeof(uvs_camera) / 8);
static_assert(sizeof(uvs_camera) % 8 == 0, "copied as doubles");

struct Believed {
    const uvs_camera *models;                                    // [n]
    long long n;
    const int32_t *index;                                        // [T] or NULL: n == 1 (all trials the one model) or n == T (trial t model t)
};

// The model of `trial`, or -1 when its index names none.
__device__ __forceinline__ long long model_of(const Believed &B, long long trial) {
    const long long i = B.index != nullptr ? static_cast<long long>(B.index[trial]) : (B.n == 1 ? 0 : trial);
    return (i >= 0 && i < B.n) ? i : -1;
}

// The models of the trials first .. first + COUNT - 1 (clamped to the last trial: padding shadows it) into s_cam[COUNT], by all THREADS threads;
// zeros for a trial without a model.  The caller's next barrier stands between this and the first read.
template <int COUNT, int THREADS>
__device__ __forceinline__ void stage_models(const Believed &B, long long first, long long T, uvs_camera *s_cam) {
    for (int i = threadIdx.x; i < COUNT * kCamWords; i += THREADS) {
        const int slot = i / kCamWords, word = i - slot * kCamWords;
        long long trial = first + slot;
        if (trial >= T) trial = T - 1;
        const long long model = model_of(B, trial);
        reinterpret_cast<double *>(s_cam)[i] = model >= 0 ? reinterpret_cast<const double *>(B.models + model)[word] : 0.0;
    }
}

struct BStepArgs {
    uvs_filter_params fp;
    Believed B;
    long long T;
    const double *q, *f;
    double *dq_out, *err_out, *j_out;
    int32_t *status;
};

template <int M, int N, int L>
__global__ __launch_bounds__(64) void camera_believed_step_kernel(const BStepArgs A) {
    constexpr int R = M / L, TRIALS = 64 / L;
    __shared__ uvs_camera s_cam[TRIALS];
    stage_models<TRIALS, 64>(A.B, static_cast<long long>(blockIdx.x) * TRIALS, A.T, s_cam);
    __syncthreads();
    const int slot = threadIdx.x / L, sub = threadIdx.x % L;
    long long trial = static_cast<long long>(blockIdx.x) * TRIALS + slot;
    const bool valid = trial < A.T;
    if (!valid) trial = A.T - 1;                                 // a padding lane shadows the last trial and stores nothing
    const bool known = model_of(A.B, trial) >= 0;
    double q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j] = A.q[trial * N + j];
    const double *f = A.f + trial * M;
    uvs::Rows<M, N, L> st;
    double err[R], cmd[N];
    const int bad = analytical_step<M, N, L>(s_cam[slot], A.fp, q, [f](int i) { return f[i]; }, sub, st, err, cmd);
    if (!valid) return;
    if (!known) {                                                // no model: FAIL and nothing else
        if (sub == 0) A.status[trial] = UVS_STATUS_FAIL;
        return;
    }
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

struct BLoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;                                              // the sensor side's: the camera that renders the frames
    Believed B;                                                  // the control side's
    long long T;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;                    // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

// camera_analytical_loop_kernel with the control side's model per trial.  What differs from it: s_cam[G] staged from memory, and a trial
// without a model starts FAILed (not alive, not seen), so that it logs no row and writes status and k_done alone.
template <int M, int N, int L, int G>
__global__ __launch_bounds__(kBLoopThreads) void camera_believed_loop_kernel(const BLoopArgs A) {
    constexpr int R = M / L, W = kBLoopThreads / 64;
    static_assert((G == 1 || G == W) && W == kColours && G * L <= 64 && N <= UVS_CAMERA_MAX_JOINTS && M <= 2 * kColours, "one or four trials per workgroup");
    __shared__ double s_sin[W][UVS_CAMERA_MAX_JOINTS], s_cos[W][UVS_CAMERA_MAX_JOINTS];   // per wavefront (G = 1: four copies of one trial's)
    __shared__ double s_disc[W][kColours * 3];
    __shared__ double s_q[G][N];                                 // this step's joints, sensor side -> control side
    __shared__ double s_f[G][M];                                 // this step's features, sensor side -> control side
    __shared__ double s_dq[G][N];                                // this step's command, control side -> sensor side
    __shared__ int s_alive[G];                                   // trial has not FAILed, as of the end of this step
    __shared__ int s_pix[G][kColours];                           // smallest mask so far
    __shared__ double s_sum[G][3][M];                            // per-feature ISE, IAE, ITAE after the loop
    __shared__ uvs_camera s_cam[G];                              // the believed models of the workgroup's trials; the step loop's barriers stand
    stage_models<G, kBLoopThreads>(A.B, static_cast<long long>(blockIdx.x) * G, A.T, s_cam);   // between this and the first read

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
    const bool known = model_of(A.B, trial) >= 0;                // the same word in all 64 lanes
    double q = lane < N ? A.q_start[trial * N + lane] : 0.0;
    // this lane's own addresses in row 0 of the [K][T][comp] logs (NULL: not wanted, or nothing of this lane's), advanced by a row per step
    const long long step_rows = T;
    double *q_at = (valid && writer && lane < N && A.q_log != nullptr) ? A.q_log + trial * N + lane : nullptr;
    double *f_at = (valid && lane == 0 && A.f_log != nullptr) ? A.f_log + trial * M : nullptr;
    const double *noise_at = A.noise != nullptr ? A.noise + trial * M : nullptr;
    bool seen = known;                                           // this trial has not FAILed before this step: its rows q[k], f[k] are due
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
    bool alive = model_of(A.B, etrial) >= 0;                     // no model: FAILed before step 0
    int status = alive ? UVS_STATUS_SUCCESS : UVS_STATUS_FAIL, k_done = alive ? K : 0;

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
        // ---- the law of the workgroup's trials, each on its own model (camera_believed_step_kernel's sequence)
        if (w == 0) {
            double qk[N], err[R], cmd[N];
#pragma unroll
            for (int j = 0; j < N; ++j) qk[j] = s_q[slot][j];
            uvs::Rows<M, N, L> st;
            const int bad = analytical_step<M, N, L>(s_cam[slot], fp, qk, [slot](int i) { return s_f[slot][i]; }, sub, st, err, cmd);
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
    if (lane < 3 && valid && writer && known) {                  // lane i: the norm over the features in order, as stats_kernel forms it
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc = fma(s_sum[ws][lane][i], s_sum[ws][lane][i], acc);
        A.stats[3 * trial + lane] = sqrt(acc);
    }
    if (lane < npts && valid && writer && known && A.pixels != nullptr) A.pixels[trial * npts + lane] = s_pix[ws][lane];
}

// camera_guess_kernel (uvs_camera_loop.hip) on the trial's own model: one lane per trial.  A trial without a model writes nothing.
__global__ __launch_bounds__(64) void camera_believed_guess_kernel(const Believed B, long long T, int n_points, const double *__restrict__ q_start,
                                                                   const double *__restrict__ f0, double *__restrict__ x0_out) {
    constexpr int N = kAJoints;
    const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    if (t >= T) return;
    const long long model = model_of(B, t);
    if (model < 0) return;
    const uvs_camera &cam = B.models[model];
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
    const int m = 2 * n_points;
    const double focal = cam.focal;
    for (int p = 0; p < n_points; ++p) {
        const double depth = uvs::point_depth(pos, cam.points[p]);
        const double u = f0[t * m + 2 * p], v = f0[t * m + 2 * p + 1];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double x[N];
            uvs::feature_jacobian_row<N>(focal, u, v, depth, half, Jc, x);
#pragma unroll
            for (int j = 0; j < N; ++j) x0_out[(t * m + 2 * p + half) * N + j] = x[j];
        }
    }
}

// What the entry points ask of the believed operand; before the first HIP call.
static int check_believed(const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, int64_t T) {
    if (believed == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL believed");
    if (n_believed < 1 || n_believed > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "n_believed must be 1 .. 2^31 - 1");
    if (believed_index == nullptr && n_believed != 1 && n_believed != T)
        return fail(UVS_ERR_ARG, "%s", "without believed_index, n_believed must be 1 or T");
    return UVS_OK;
}

template <int M, int N, int L>
static void launch_bstep(hipStream_t s, const BStepArgs &A) {
    const unsigned blocks = static_cast<unsigned>((A.T * L + 63) / 64);
    hipLaunchKernelGGL((camera_believed_step_kernel<M, N, L>), dim3(blocks), dim3(64), 0, s, A);
}

template <int M, int N, int L>
static void launch_bloop(hipStream_t s, const BLoopArgs &A) {
    if (A.T <= kBSmallBatch)
        hipLaunchKernelGGL((camera_believed_loop_kernel<M, N, L, 1>), dim3(static_cast<unsigned>(A.T)), dim3(kBLoopThreads), 0, s, A);
    else
        hipLaunchKernelGGL((camera_believed_loop_kernel<M, N, L, kBLoopTrials>), dim3(static_cast<unsigned>((A.T + kBLoopTrials - 1) / kBLoopTrials)),
                           dim3(kBLoopThreads), 0, s, A);
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_step_f64(const uvs_filter_params *fp, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                 const int32_t *believed_index, const double *q, const double *f, double *dq_out, double *err_out,
                                 double *j_out, int32_t *status, void *stream) {
    g_err[0] = '\0';
    if (fp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp");
    if (q == nullptr || f == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q or f");
    if (dq_out == nullptr || err_out == nullptr || status == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL dq_out, err_out or status");
    uvs_camera shape{};                                          // there is no true camera here: the shape is fp's own
    shape.n_joints = fp->n;
    shape.n_points = fp->m / 2;
    if (const int rc = check_analytical(fp, &shape, T)) return rc;
    if (const int rc = check_believed(believed, n_believed, believed_index, T)) return rc;
    if (T == 0) return UVS_OK;
    const BStepArgs A{*fp, {believed, n_believed, believed_index}, T, q, f, dq_out, err_out, j_out, status};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fp->m == 8) launch_bstep<8, 6, 4>(s, A);
    else if (fp->m == 6) launch_bstep<6, 6, 2>(s, A);
    else launch_bstep<2, 6, 1>(s, A);
    return launched("camera_believed_step_kernel launch: %s");
}

int uvs_camera_believed_loop_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                 const int32_t *believed_index, const double *q_start, const double *noise, double *q_log, double *f_log,
                                 double *dq_log, double *err_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                                 void *stream) {
    g_err[0] = '\0';
    if (q_start == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start");
    if (status == nullptr || k_done == nullptr || stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    if (const int rc = check_analytical(fp, cam, T)) return rc;
    if (fp->steps < 1) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1");
    if (const int rc = check_believed(believed, n_believed, believed_index, T)) return rc;
    if (T == 0) return UVS_OK;
    const BLoopArgs A{*fp, *cam, {believed, n_believed, believed_index}, T, q_start, noise, q_log, f_log, dq_log, err_log, status, k_done, stats, pixels};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fp->m == 8) launch_bloop<8, 6, 4>(s, A);
    else if (fp->m == 6) launch_bloop<6, 6, 2>(s, A);
    else launch_bloop<2, 6, 1>(s, A);
    return launched("camera_believed_loop_kernel launch: %s");
}

int uvs_camera_believed_guess_f64(int64_t T, int32_t n_points, const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index,
                                  const double *q_start, const double *f0, double *x0_out, void *stream) {
    g_err[0] = '\0';
    if (q_start == nullptr || f0 == nullptr || x0_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start, f0 or x0_out");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (const int rc = check_believed(believed, n_believed, believed_index, T)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(camera_believed_guess_kernel, dim3(static_cast<unsigned>((T + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       Believed{believed, n_believed, believed_index}, static_cast<long long>(T), static_cast<int>(n_points), q_start, f0, x0_out);
    return launched("camera_believed_guess_kernel launch: %s");
}

}  // extern "C"
