// libuvs_vision.so, sixth unit: the pixel closed loop with OCCLUDERS in front of the camera, per output trial, next to the per-trial estimator
// parameters (uvs_camera_closed_loop_occluded_f64, engine.camera_closed_loop(occluders=...)).  The kernel is the third flavour of
// camera_loop_device.hpp's one text, camera_occluded_kernel: the per-trial flavour with the switch OCC on -- lanes o < n_occ of each
// sensor-side wavefront evaluate their trial's rectangles for the step into LDS next to the projection, and the detection walk reads them
// from there (vision_device.hpp: occluder_rect, box_counts<OVER, true>).  A unit of its own, like uvs_camera_grid.hip, so that its 22
// instantiations compile next to the others and those keep their resource figures.
#define UVS_CAMERA_FLAVOUR 2                                     // kFlavourOccluded
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_occluded_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                        const uvs_occluder *occ, int32_t n_occ, const double *q_start, const double *noise, const double *x0,
                                        const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log,
                                        int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cam = cam; r.T = T; r.tp = tp; r.occ = occ; r.n_occ = n_occ;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_camera_loop(r);
}

}  // extern "C"
