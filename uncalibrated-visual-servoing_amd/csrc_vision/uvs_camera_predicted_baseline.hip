// libuvs_vision.so, eighteenth unit: the calibrated IBVS baseline's one-launch pixel loop whose law PREDICTS the features over the camera
// latency.  uvs_camera_believed_loop_predicted_f64 and its kernel, the seventh flavour of camera_analytical_device.hpp's one
// loop text, predicted_baseline_kernel: aligned_baseline_kernel whose law is handed f^ = f_reported + (h(q_k) - h(q_{max(k - p, 0)})), p the
// trial's prediction HORIZON and h the (u, v) of the law's own model, projected once per step by the projection kernel's text, in lanes next
// to the ones that project the scene, into a ring of the last nine steps' rows.  The f log stays the reported row; err and the sums are f^ - f*.  A unit of its own, so that the six other
// flavours keep their resource figures.
#define UVS_BASELINE_FLAVOUR 6                                   // kBaselineWithHorizon
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_predicted_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                           const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed,
                                           const int32_t *predict, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                           const int32_t *believed_index, const double *q_start, const double *noise, double *q_log,
                                           double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done, double *stats,
                                           int32_t *pixels, void *stream) {
    BaselineRequest r{};
    r.fp = fp; r.cams = cams; r.n_cams = n_cams; r.cam_index = cam_index; r.motion = motion; r.latency = latency; r.assumed = assumed;
    r.predict = predict;
    r.T = T; r.believed = believed; r.n_believed = n_believed; r.believed_index = believed_index;
    r.q_start = q_start; r.noise = noise; r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_baseline_loop(r);
}

}  // extern "C"
