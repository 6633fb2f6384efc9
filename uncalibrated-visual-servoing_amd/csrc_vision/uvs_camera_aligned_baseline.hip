// libuvs_vision.so, sixteenth unit: the calibrated IBVS baseline's one-launch pixel loop whose law is TOLD a camera latency.
// uvs_camera_believed_loop_aligned_f64 and its kernel, the sixth flavour of camera_analytical_device.hpp's one loop text,
// aligned_baseline_kernel: delayed_baseline_kernel whose law reads the joints of step max(k - a, 0), a the trial's ASSUMED latency, from a
// ring of the last nine steps' joints -- the camera Jacobian, the depths and the interaction matrix are those of the pose the assumed
// frame shows.  The features stay the reported row of step k, the q log and the joint integration stay current.  A unit of its own, so
// that the five other flavours keep their resource figures.
#define UVS_CAMERA_SCENES
#define UVS_CAMERA_MOVING
#define UVS_CAMERA_DELAYED
#define UVS_CAMERA_ALIGNED
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_aligned_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed, int64_t T,
                                         const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, const double *q_start,
                                         const double *noise, double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status,
                                         int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
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
    const AlignedBaselineArgs A{{{{*fp, shape, {believed, n_believed, believed_index}, {cams, n_cams, cam_index}, T, q_start, noise, q_log, f_log,
                                   dq_log, err_log, status, k_done, stats, pixels},
                                  motion},                           // NULL is legal: nothing moves
                                 latency},                           // NULL is legal: no latency
                                assumed};                            // NULL is legal: the law is not told
    launch_baseline_loop(*fp, static_cast<hipStream_t>(stream), A);
    return launched("aligned_baseline_kernel launch: %s");
}

}  // extern "C"
