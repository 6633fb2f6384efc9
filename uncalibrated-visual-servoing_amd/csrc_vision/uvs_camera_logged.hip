// libuvs_vision.so, nineteenth unit: the pixel closed loop that LOGS its estimate.  uvs_camera_closed_loop_logged_f64 and its
// kernel, the eleventh flavour of camera_loop_device.hpp's one text, logged_frames_kernel: the predicted flavour with the switch LOGGED on --
// every owner lane of wavefront 0 stores the R rows of X_k it holds, the matrix step k's update left, into row k of x_log next to the
// step's dq row, under the condition of the err, kappa and dq rows.  Everything else stays what it was; x_log == NULL gives the predicted kernel's bits.  A unit of its
// own, like uvs_camera_predicted.hip, so that its 22 instantiations compile next to the others and those keep their resource figures.
#define UVS_CAMERA_PER_TRIAL
#define UVS_CAMERA_OCCLUDED
#define UVS_CAMERA_HELD
#define UVS_CAMERA_PAINTED
#define UVS_CAMERA_SCENES
#define UVS_CAMERA_MOVING
#define UVS_CAMERA_DELAYED
#define UVS_CAMERA_ALIGNED
#define UVS_CAMERA_PREDICTED
#define UVS_CAMERA_LOGGED
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
    g_err[0] = '\0';
    if (fp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp");
    const uvs_camera shape = scene_shape(fp->n, fp->m / 2);         // the shape is fp's: no struct's own n_joints / n_points is read
    if (const int rc = check_loop_args(fp, &shape, T, q_start, x0, f0, status, k_done, stats)) return rc;
    if (tp != nullptr && tp->source != nullptr && tp->n_in < 1)
        return fail(UVS_ERR_ARG, "%s", "source needs n_in >= 1: the trials q_start, noise, x0 and f0 hold");
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (hold < 0) return fail(UVS_ERR_ARG, "%s", "hold must be >= 0");
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0) return UVS_OK;
    const uvs_camera_trial_params none{};                            // NULL tp: every member NULL
    const LoggedLoopArgs A{{{{{{{{{{{*fp, shape, T, q_start, noise, x0, f0, q_log, f_log, dq_log, err_log, kappa_log, status, k_done, stats, pixels},
                                 tp != nullptr ? *tp : none},
                                occ, n_occ},
                               hold, held},
                              paint},
                             {cams, n_cams, cam_index}},
                            motion},                                 // NULL is legal: nothing moves
                           latency},                                 // NULL is legal: no latency
                          assumed},                                  // NULL is legal: the controller is not told
                         predict},                                   // NULL is legal: no prediction
                        x_log};                                      // NULL is legal: no log of X, the predicted namesake bit for bit
    if (!launch_loop_shape(*fp, static_cast<hipStream_t>(stream), A)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched("logged_frames_kernel launch: %s");
}

}  // extern "C"
