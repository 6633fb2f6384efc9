// libuvs_vision.so, nineteenth unit: the pixel closed loop that LOGS its estimate.  uvs_camera_closed_loop_logged_f64 and its
// kernel, the eleventh flavour of camera_loop_device.hpp's one text, logged_frames_kernel: the predicted flavour with the switch LOGGED on --
// every owner lane of wavefront 0 stores the R rows of X_k it holds, the matrix step k's update left, into row k of x_log next to the
// step's dq row, under the condition of the err, kappa and dq rows.  Everything else stays what it was; x_log == NULL gives the predicted kernel's bits.  A unit of its
// own, like uvs_camera_predicted.hip, so that its 22 instantiations compile next to the others and those keep their resource figures.
#define UVS_CAMERA_FLAVOUR 10                                    // kFlavourLogged
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_logged_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                      const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed,
                                      const int32_t *predict, int64_t T, const uvs_camera_trial_params *tp, const uvs_occluder *occ,
                                      const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start, const double *noise,
                                      const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                                      double *kappa_log, double *x_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                                      int32_t *held, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cams = cams; r.n_cams = n_cams; r.cam_index = cam_index; r.motion = motion; r.latency = latency; r.assumed = assumed;
    r.predict = predict;
    r.T = T; r.tp = tp; r.occ = occ; r.paint = paint; r.n_occ = n_occ; r.hold = hold;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log; r.x_log = x_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.held = held; r.stream = stream;
    return run_camera_loop(r);
}

}  // extern "C"
