// libuvs_vision.so, eighth unit: the pixel closed loop behind occluders that may be PAINTED a disc's colour (the rule:
// plant.render_discs(occluder_colours=...)).  uvs_camera_closed_loop_painted_f64 and its kernel, the fifth flavour of
// camera_loop_device.hpp's one text, camera_painted_kernel: the held flavour with the switch PAINT on -- the lanes that evaluate the trial's
// rectangles also leave their paints in one LDS dword, and the detection adds the pixels of the rectangles painted a colour to that
// colour's counts.  A unit of its own, like uvs_camera_held.hip, so that its instantiations compile next to the others and those keep their
// resource figures.
#define UVS_CAMERA_FLAVOUR 4                                     // kFlavourPainted
#include "camera_loop_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_closed_loop_painted_f64(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera_trial_params *tp,
                                       const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start,
                                       const double *noise, const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log,
                                       double *err_log, double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                                       int32_t *held, void *stream) {
    LoopRequest r{};
    r.fp = fp; r.cam = cam; r.T = T; r.tp = tp; r.occ = occ; r.paint = paint; r.n_occ = n_occ; r.hold = hold;
    r.q_start = q_start; r.noise = noise; r.x0 = x0; r.f0 = f0;
    r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log; r.kappa_log = kappa_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.held = held; r.stream = stream;
    return run_camera_loop(r);
}

}  // extern "C"
