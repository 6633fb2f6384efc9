// libuvs_vision.so, fourteenth unit: the calibrated IBVS baseline's one-launch pixel loop behind a CAMERA LATENCY.
// uvs_camera_believed_loop_delayed_f64 and its kernel, the fifth flavour of camera_analytical_device.hpp's one loop text,
// delayed_baseline_kernel: moving_baseline_kernel whose detector is handed the frame of step max(k - d, 0), d the trial's latency, through
// an LDS ring of detections per disc.  The law's joints are the current ones -- encoders are not delayed -- so an interaction matrix at
// q_k is fed features of the pose d steps ago.  That is the experiment.  A unit of its own, so that the four other flavours keep their
// resource figures.
#define UVS_CAMERA_SCENES
#define UVS_CAMERA_MOVING
#define UVS_CAMERA_DELAYED
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_delayed_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, int64_t T, const uvs_camera *believed,
                                         int64_t n_believed, const int32_t *believed_index, const double *q_start, const double *noise,
                                         double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done,
                                         double *stats, int32_t *pixels, void *stream) {
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
    const DelayedBaselineArgs A{{{*fp, shape, {believed, n_believed, believed_index}, {cams, n_cams, cam_index}, T, q_start, noise, q_log, f_log,
                                  dq_log, err_log, status, k_done, stats, pixels},
                                 motion},                            // NULL is legal: nothing moves
                                latency};                            // NULL is legal: no latency
    launch_baseline_loop(*fp, static_cast<hipStream_t>(stream), A);
    return launched("delayed_baseline_kernel launch: %s");
}

}  // extern "C"
