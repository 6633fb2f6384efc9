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
//   camera_believed_loop_kernel: the believed flavour of the baseline loop's one text (camera_analytical_device.hpp; this unit states
//     level 1): camera_analytical_loop_kernel with s_cam[G] staged from memory in place of its one s_cam, and a trial without
//     a model FAILed before step 0.  The sensor side keeps reading the true camera from the kernel arguments.
//   camera_believed_guess_kernel: camera_guess_kernel's arithmetic (guess_trial, camera_sensor_device.hpp), one lane per trial, the model
//     read from memory where it is used.
//
// An index outside [0, n_believed) never becomes an address: model_of returns -1 for it, the staging loop writes zeros in its place (the
// lanes of that trial keep computing on them: every cross-lane move of the solver sees a full wavefront), and the trial is FAILed by the
// flag, not by what the zeros give: status FAIL (the loop: k_done = 0) and not one other store.
#define UVS_BASELINE_FLAVOUR 1                                   // kBaselineWithModel
#include "camera_analytical_device.hpp"

namespace uvs_vision {

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

// camera_guess_kernel (uvs_camera_loop.hip) on the trial's own model: one lane per trial.  A trial without a model writes nothing.
__global__ __launch_bounds__(64) void camera_believed_guess_kernel(const Believed B, long long T, int n_points, const double *__restrict__ q_start,
                                                                   const double *__restrict__ f0, double *__restrict__ x0_out) {
    const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    if (t >= T) return;
    const long long model = model_of(B, t);
    if (model < 0) return;
    guess_trial(B.models[model], t, n_points, q_start, f0, x0_out);
}

template <int M, int N, int L>
static void launch_bstep(hipStream_t s, const BStepArgs &A) {
    const unsigned blocks = static_cast<unsigned>((A.T * L + 63) / 64);
    hipLaunchKernelGGL((camera_believed_step_kernel<M, N, L>), dim3(blocks), dim3(64), 0, s, A);
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
    BaselineRequest r{};
    r.fp = fp; r.cam = cam; r.T = T; r.believed = believed; r.n_believed = n_believed; r.believed_index = believed_index;
    r.q_start = q_start; r.noise = noise; r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_baseline_loop(r);
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
