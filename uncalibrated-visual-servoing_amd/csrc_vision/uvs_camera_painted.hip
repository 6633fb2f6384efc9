// libuvs_vision.so, eighth unit: the pixel closed loop behind occluders that may be PAINTED a disc's colour (the rule:
// plant.render_discs(occluder_colours=...)).  uvs_camera_closed_loop_painted_f64 and its kernel, the fifth flavour of
// camera_loop_device.hpp's one text, camera_painted_kernel: the held flavour with the switch PAINT on -- the lanes that evaluate the trial's
// rectangles also leave their paints in one LDS dword, and the detection adds the pixels of the rectangles painted a colour to that
// colour's counts.  A unit of its own, like uvs_camera_held.hip, so that its instantiations compile next to the others and those keep their
// resource figures.
#define UVS_CAMERA_PER_TRIAL
#define UVS_CAMERA_OCCLUDED
#define UVS_CAMERA_HELD
#define UVS_CAMERA_PAINTED
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_painted_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                       const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start,
                                       const double *noise, const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log,
                                       double *err_log, double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                                       int32_t *held, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_loop_args(fp, cam, T, q_start, x0, f0, status, k_done, stats)) return rc;
    if (tp != nullptr && tp->source != nullptr && tp->n_in < 1)
        return fail(UVS_ERR_ARG, "%s", "source needs n_in >= 1: the trials q_start, noise, x0 and f0 hold");
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (hold < 0) return fail(UVS_ERR_ARG, "%s", "hold must be >= 0");
    if (T == 0) return UVS_OK;
    const uvs_camera_trial_params none{};                            // NULL tp: every member NULL
    const PaintedLoopArgs A{{{{{*fp, *cam, T, q_start, noise, x0, f0, q_log, f_log, dq_log, err_log, kappa_log, status, k_done, stats, pixels},
                               tp != nullptr ? *tp : none},
                              occ, n_occ},
                             hold, held},
                            paint};                                  // NULL: every rectangle opaque
    if (!launch_loop_shape(*fp, static_cast<hipStream_t>(stream), A)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched("camera_painted_kernel launch: %s");
}

}  // extern "C"
