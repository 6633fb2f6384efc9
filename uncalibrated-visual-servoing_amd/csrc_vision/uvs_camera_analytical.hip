// libuvs_vision.so, third unit: the calibrated IBVS baseline (Method.ANALYTICAL, experiment.py:145-162 and :300-320) THROUGH PIXELS -- one
// step for T trials (uvs_camera_analytical_step_f64) and the pixel closed loop as ONE launch per batch (uvs_camera_analytical_loop_f64).
// The interaction matrix is evaluated from the model at the noisy DETECTED features instead of estimated: camera_jacobian, point_depth,
// feature_jacobian_row and control_law are those of libuvs_rmckf.so, read from its device header; the sensor side is camera_sensor_device.hpp.
//
// The step is defined once, in analytical_step (camera_analytical_device.hpp, shared with the believed-model unit), and both kernels call
// it on the same operands; the library compiles with -ffp-contract=off, so the loop kernel forms the bits of the stepwise loop
// (uvs_camera_features_f64, then the step kernel, K times).
//
// Mapping.  A filter of M rows is spread over L lanes as in the estimator kernels (4, 2, 1 lanes at 8, 6, 2 rows): lane `sub` of a trial
// evaluates the camera Jacobian for itself (the same bits in the L lanes: the same operands), then its own R = M / L rows of J into
// Rows::x, and the L lanes solve together in control_law.  There is no covariance: Rows::p is never touched and takes no register.
//   camera_analytical_step_kernel: 64 / L trials per wavefront; padding lanes shadow the last trial, so every cross-lane move of the
//     solver sees a full wavefront, and store nothing.
//   camera_analytical_loop_kernel: the calibrated flavour of the baseline loop's one text, which camera_analytical_device.hpp holds and
//     describes; this unit compiles it at level 0 (uvs_camera_believed.hip states level 1 and gets the believed flavour).
#define UVS_BASELINE_FLAVOUR 0                                   // kBaselineCalibrated
#include "camera_analytical_device.hpp"

namespace uvs_vision {

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

template <int M, int N, int L>
static void launch_step(hipStream_t s, const AStepArgs &A) {
    const unsigned blocks = static_cast<unsigned>((A.T * L + 63) / 64);
    hipLaunchKernelGGL((camera_analytical_step_kernel<M, N, L>), dim3(blocks), dim3(64), 0, s, A);
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
    BaselineRequest r{};
    r.fp = fp; r.cam = cam; r.T = T;
    r.q_start = q_start; r.noise = noise; r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_baseline_loop(r);
}

}  // extern "C"
