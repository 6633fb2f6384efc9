// libuvs_vision.so, sixth unit: the pixel closed loop with OCCLUDERS in front of the camera, per output trial, next to the per-trial estimator
// parameters (uvs_camera_closed_loop_occluded_f64, engine.camera_closed_loop(occluders=...)).  The kernel is the third flavour of
// camera_loop_device.hpp's one text, camera_occluded_kernel: the per-trial flavour with the switch OCC on -- lanes o < n_occ of each
// sensor-side wavefront evaluate their trial's rectangles for the step into LDS next to the projection, and the detection walk reads them
// from there (vision_device.hpp: occluder_rect, box_counts<OVER, true>).  A unit of its own, like uvs_camera_grid.hip, so that its 22
// instantiations compile next to the others and those keep their resource figures.
#define UVS_CAMERA_PER_TRIAL
#define UVS_CAMERA_OCCLUDED
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_occluded_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                        const uvs_occluder *occ, int32_t n_occ, const double *q_start, const double *noise, const double *x0,
                                        const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log,
                                        int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_loop_args(fp, cam, T, q_start, x0, f0, status, k_done, stats)) return rc;
    if (tp != nullptr && tp->source != nullptr && tp->n_in < 1)
        return fail(UVS_ERR_ARG, "%s", "source needs n_in >= 1: the trials q_start, noise, x0 and f0 hold");
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (T == 0) return UVS_OK;
    const uvs_camera_trial_params none{};                            // NULL tp: every member NULL
    const OccludedLoopArgs A{{{*fp, *cam, T, q_start, noise, x0, f0, q_log, f_log, dq_log, err_log, kappa_log, status, k_done, stats, pixels},
                              tp != nullptr ? *tp : none},
                             occ, n_occ};
    if (!launch_loop_shape(*fp, static_cast<hipStream_t>(stream), A)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched("camera_occluded_kernel launch: %s");
}

}  // extern "C"
