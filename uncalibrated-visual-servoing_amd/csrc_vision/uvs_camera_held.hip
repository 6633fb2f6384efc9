// libuvs_vision.so, seventh unit: the pixel closed loop that HOLDS a lost disc's last detection (the rule:
// plant.hold_features).  Two things live here.  (1) uvs_camera_closed_loop_held_f64 and its kernel, the fourth flavour of
// camera_loop_device.hpp's one text, camera_held_kernel: the occluded flavour with the switch HOLD on -- lane 0 of the sensor-side
// wavefront leaves step k - 1's pair in LDS where a mask is empty and the hold is not used up, and counts misses and held steps in LDS
// next to the smallest masks.  A unit of its own, like uvs_camera_occluded.hip, so that its 22 instantiations compile next to the others
// and those keep their resource figures.  (2) uvs_hold_features_f64 and hold_pairs_kernel: the same rule for the stepwise loops, one
// thread per (trial, disc), on the row that uvs_camera_features[_occluded]_f64 has just written.
#define UVS_CAMERA_FLAVOUR 3                                     // kFlavourHeld
#include "camera_loop_device.hpp"

namespace uvs_vision {

constexpr int kHoldThreads = 256;

// Thread i = t * n_points + j: disc j of trial t.  pixels, f and held are rows of (T, n_points), (T, 2 n_points) and (T, n_points); miss is
// the loop's own [T][4].  Every thread reads and writes its own words only.
__global__ __launch_bounds__(kHoldThreads) void hold_pairs_kernel(int64_t pairs, int n_points, int hold, int k, const double *__restrict__ f_prev,
                                                                  double *__restrict__ f, const int32_t *__restrict__ pixels,
                                                                  int32_t *__restrict__ miss, int32_t *__restrict__ held) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kHoldThreads + threadIdx.x;
    if (i >= pairs) return;
    const int64_t t = i / n_points;
    const int64_t at = t * kColours + (i - t * n_points);
    int was_held = 0;
    if (pixels[i] != 0) {                                        // the integer count decides, never the pair
        miss[at] = 0;
    } else {
        const int m = miss[at];
        if (k >= 1 && m < hold) {                                // lost, and the hold is not used up: step k - 1's reported pair, no noise of step k
            f[2 * i] = f_prev[2 * i];
            f[2 * i + 1] = f_prev[2 * i + 1];
            miss[at] = m + 1;
            was_held = 1;
        }                                                        // lost otherwise: the NaN pair stays
    }
    if (held != nullptr) held[i] = was_held;
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_held_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                    const uvs_occluder *occ, int32_t n_occ, int32_t hold, const double *q_start, const double *noise,
                                    const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                                    double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, int32_t *held,
                                    void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cam = cam; r.T = T; r.tp = tp; r.occ = occ; r.n_occ = n_occ; r.hold = hold;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.held = held; r.stream = stream;
    return run_camera_loop(r);
}

int uvs_hold_features_f64(int64_t T, int32_t n_points, int32_t hold, int32_t k, const double *f_prev_row, double *f_row,
                          const int32_t *pixels_row, int32_t *miss, int32_t *held_row, void *stream) {
    g_err[0] = '\0';
    if (f_row == nullptr || pixels_row == nullptr || miss == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_row, pixels_row or miss");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (hold < 0) return fail(UVS_ERR_ARG, "%s", "hold must be >= 0");
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (k >= 1 && f_prev_row == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_prev_row with k >= 1");
    if (T == 0) return UVS_OK;
    const int64_t pairs = T * n_points;
    hipLaunchKernelGGL(hold_pairs_kernel, dim3(static_cast<unsigned>((pairs + kHoldThreads - 1) / kHoldThreads)), dim3(kHoldThreads), 0,
                       static_cast<hipStream_t>(stream), pairs, static_cast<int>(n_points), static_cast<int>(hold), static_cast<int>(k), f_prev_row,
                       f_row, pixels_row, miss, held_row);
    return launched("hold_pairs_kernel launch: %s");
}

}  // extern "C"
