// libuvs_vision.so, twelfth unit: the calibrated IBVS baseline's one-launch pixel loop on MOVING TARGETS.
// uvs_camera_believed_loop_moving_f64 and its kernel, the fourth flavour of camera_analytical_device.hpp's one loop text,
// moving_baseline_kernel: scene_baseline_loop_kernel whose sensor side projects every disc where its trial's motion has taken it.  The law's
// model -- believed, or with believed == cams the trial's own scene -- does not move: the controller does not know the target's motion, so
// its depths go stale.  That is the experiment.  A unit of its own, so that the three other flavours keep their resource figures.
#define UVS_CAMERA_SCENES
#define UVS_CAMERA_MOVING
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_moving_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                        const uvs_target_motion *motion, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                        const int32_t *believed_index, const double *q_start, const double *noise, double *q_log,
                                        double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done, double *stats,
                                        int32_t *pixels, void *stream) {
    g_err[0] = '\0';
    if (q_start == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start");
    if (status == nullptr || k_done == nullptr || stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    if (fp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp");
    const uvs_camera shape = scene_shape(fp->n, fp->m / 2);         // the shape is fp's: no struct's own n_joints / n_points is read
    if (const int rc = check_analytical(fp, &shape, T)) return rc;
    if (fp->steps < 1) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1");
    if (believed == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL believed");
    if (n_believed < 1 || n_believed > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "n_believed must be 1 .. 2^31 - 1");
    if (believed_index == nullptr && n_believed != 1 && n_believed != T)
        return fail(UVS_ERR_ARG, "%s", "without believed_index, n_believed must be 1 or T");
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0) return UVS_OK;
    const MovingBaselineArgs A{{*fp, shape, {believed, n_believed, believed_index}, {cams, n_cams, cam_index}, T, q_start, noise, q_log, f_log,
                                dq_log, err_log, status, k_done, stats, pixels},
                               motion};                              // NULL is legal: nothing moves
    launch_baseline_loop(*fp, static_cast<hipStream_t>(stream), A);
    return launched("moving_baseline_kernel launch: %s");
}

}  // extern "C"
