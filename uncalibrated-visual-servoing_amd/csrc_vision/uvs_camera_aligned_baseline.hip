// libuvs_vision.so, sixteenth unit: the calibrated IBVS baseline's one-launch pixel loop whose law is TOLD a camera latency.
// uvs_camera_believed_loop_aligned_f64 and its kernel, the sixth flavour of camera_analytical_device.hpp's one loop text,
// aligned_baseline_kernel: delayed_baseline_kernel whose law reads the joints of step max(k - a, 0), a the trial's ASSUMED latency, from a
// ring of the last nine steps' joints -- the camera Jacobian, the depths and the interaction matrix are those of the pose the assumed
// frame shows.  The features stay the reported row of step k, the q log and the joint integration stay current.  A unit of its own, so
// that the five other flavours keep their resource figures.
#define UVS_BASELINE_FLAVOUR 5                                   // kBaselineWithAssumed
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_aligned_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed, int64_t T,
                                         const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, const double *q_start,
                                         const double *noise, double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status,
                                         int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    BaselineRequest r{};
    r.fp = fp; r.cams = cams; r.n_cams = n_cams; r.cam_index = cam_index; r.motion = motion; r.latency = latency; r.assumed = assumed;
    r.T = T; r.believed = believed; r.n_believed = n_believed; r.believed_index = believed_index;
    r.q_start = q_start; r.noise = noise; r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_baseline_loop(r);
}

}  // extern "C"
