// libuvs_vision.so, fifth unit: the pixel closed loop with PER-TRIAL estimator parameters -- a hyperparameter grid over the same starts and
// noise in one launch (uvs_camera_closed_loop_grid_f64, engine.camera_closed_loop(trial_params=...)).  The kernel is the per-trial flavour
// of camera_loop_device.hpp's one text, camera_grid_kernel: see the PTP paragraph at its head.  A unit of its own so that its 22
// instantiations compile next to the uniform ones, not after them, and so that those keep their resource figures.
#define UVS_CAMERA_PER_TRIAL
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_grid_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                    const double *q_start, const double *noise, const double *x0, const double *f0, double *q_log,
                                    double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status, int32_t *k_done,
                                    double *stats, int32_t *pixels, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_loop_args(fp, cam, T, q_start, x0, f0, status, k_done, stats)) return rc;
    if (tp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL tp (a block whose members are all NULL is the uniform call)");
    if (tp->source != nullptr && tp->n_in < 1) return fail(UVS_ERR_ARG, "%s", "source needs n_in >= 1: the trials q_start, noise, x0 and f0 hold");
    if (T == 0) return UVS_OK;
    const GridLoopArgs A{{*fp, *cam, T, q_start, noise, x0, f0, q_log, f_log, dq_log, err_log, kappa_log, status, k_done, stats, pixels}, *tp};
    if (!launch_loop_shape(*fp, static_cast<hipStream_t>(stream), A)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched("camera_grid_kernel launch: %s");
}

}  // extern "C"
