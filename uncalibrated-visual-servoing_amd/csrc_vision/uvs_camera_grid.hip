// libuvs_vision.so, fifth unit: the pixel closed loop with PER-TRIAL estimator parameters -- a hyperparameter grid over the same starts and
// noise in one launch (uvs_camera_closed_loop_grid_f64, engine.camera_closed_loop(trial_params=...)).  The kernel is the per-trial flavour
// of camera_loop_device.hpp's one text, camera_grid_kernel: see the PTP paragraph at its head.  A unit of its own so that its 22
// instantiations compile next to the uniform ones, not after them, and so that those keep their resource figures.
#define UVS_CAMERA_FLAVOUR 1                                     // kFlavourPerTrial
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_grid_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                    const double *q_start, const double *noise, const double *x0, const double *f0, double *q_log,
                                    double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status, int32_t *k_done,
                                    double *stats, int32_t *pixels, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cam = cam; r.T = T; r.tp = tp;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_camera_loop(r);
}

}  // extern "C"
