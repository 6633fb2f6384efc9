// libuvs_vision.so, second unit: the pixel closed loop (engine.camera_closed_loop) as ONE launch per batch, and its analytic initial guess.
// The loop kernel's text, its mapping and its launcher are camera_loop_device.hpp, which this unit compiles in its uniform flavour
// (camera_loop_kernel: one uvs_filter_params for the batch); uvs_camera_grid.hip compiles the per-trial flavour of the same text.
#define UVS_CAMERA_FLAVOUR 0                                     // kFlavourUniform
#include "camera_loop_device.hpp"

namespace uvs_vision {

// The analytic initial guess (guess_trial, camera_sensor_device.hpp) on the camera that renders the frames, one lane per trial.
__global__ __launch_bounds__(64) void camera_guess_kernel(const uvs_camera cam, long long T, const double *__restrict__ q_start,
                                                          const double *__restrict__ f0, double *__restrict__ x0_out) {
    const long long t = static_cast<long long>(blockIdx.x) * 64 + threadIdx.x;
    if (t >= T) return;
    guess_trial(cam, t, cam.n_points, q_start, f0, x0_out);
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start, const double *noise,
                               const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                               double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cam = cam; r.T = T;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_camera_loop(r);
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
