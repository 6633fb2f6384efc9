// libuvs_vision.so, thirteenth unit: the pixel closed loop behind a CAMERA LATENCY (the rule: plant.delayed_step).  Two
// things live here.  (1) uvs_camera_closed_loop_delayed_f64 and its kernel, the eighth flavour of camera_loop_device.hpp's one text,
// delayed_frames_kernel: the moving flavour with the switch DELAYED on -- lane 0 of the sensor-side wavefront passes every detection through
// an LDS ring of the last nine and hands on the one of step max(k - d, 0), d the output trial's latency.  A unit of its own, like
// uvs_camera_moving.hip, so that its 22 instantiations compile next to the others and those keep their resource figures.
// (2) uvs_delay_features_f64 and delay_line_kernel: the same rule for the stepwise loops, one thread per (trial, disc), as a gather from
// the logs of noise-free sensed rows and mask sizes that the features calls have written.
#define UVS_CAMERA_FLAVOUR 7                                     // kFlavourDelayed
#include "camera_loop_device.hpp"

namespace uvs_vision {

constexpr int kDelayThreads = 256;

// Thread i = t * n_points + j: disc j of trial t.  sensed and counts are the [K][T][2 n_points] and [K][T][n_points] logs, of which the rows
// 0 .. k are read; noise, f and pixels are rows of step k.  Every thread writes its own words only.
__global__ __launch_bounds__(kDelayThreads) void delay_line_kernel(int64_t pairs, int n_points, int k, const int32_t *__restrict__ latency,
                                                                   const double *__restrict__ sensed, const int32_t *__restrict__ counts,
                                                                   const double *__restrict__ noise, double *__restrict__ f,
                                                                   int32_t *__restrict__ pixels) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kDelayThreads + threadIdx.x;
    if (i >= pairs) return;
    const int64_t t = i / n_points;
    const int64_t at = static_cast<int64_t>(delayed_step(k, latency_of(latency, t))) * pairs + i;   // the pair's place in row kk
    double u = sensed[2 * at], v = sensed[2 * at + 1];
    if (noise != nullptr) {                                      // step k's noise, as noisy_centre adds it
        u += noise[2 * i];
        v += noise[2 * i + 1];
    }
    f[2 * i] = u;
    f[2 * i + 1] = v;
    pixels[i] = counts[at];
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_delayed_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                       const uvs_target_motion *motion, const int32_t *latency, int64_t T,
                                       const uvs_camera_trial_params *tp, const uvs_occluder *occ, const int32_t *paint, int32_t n_occ,
                                       int32_t hold, const double *q_start, const double *noise, const double *x0, const double *f0,
                                       double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status,
                                       int32_t *k_done, double *stats, int32_t *pixels, int32_t *held, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cams = cams; r.n_cams = n_cams; r.cam_index = cam_index; r.motion = motion; r.latency = latency;
    r.T = T; r.tp = tp; r.occ = occ; r.paint = paint; r.n_occ = n_occ; r.hold = hold;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.held = held; r.stream = stream;
    return run_camera_loop(r);
}

int uvs_delay_features_f64(int64_t T, int32_t n_points, int32_t k, const int32_t *latency, const double *sensed_log, const int32_t *count_log,
                           const double *noise_row, double *f_row, int32_t *pixels_row, void *stream) {
    g_err[0] = '\0';
    if (sensed_log == nullptr || count_log == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL sensed_log or count_log");
    if (f_row == nullptr || pixels_row == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_row or pixels_row");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    const int64_t pairs = T * n_points;
    hipLaunchKernelGGL(delay_line_kernel, dim3(static_cast<unsigned>((pairs + kDelayThreads - 1) / kDelayThreads)), dim3(kDelayThreads), 0,
                       static_cast<hipStream_t>(stream), pairs, static_cast<int>(n_points), static_cast<int>(k), latency, sensed_log, count_log,
                       noise_row, f_row, pixels_row);
    return launched("delay_line_kernel launch: %s");
}

}  // extern "C"
