// libuvs_vision.so, tenth unit: the calibrated IBVS baseline's one-launch pixel loop with a SCENE PER TRIAL.
// uvs_camera_believed_loop_scenes_f64 and its kernel, the third flavour of camera_analytical_device.hpp's one loop text,
// scene_baseline_loop_kernel: camera_believed_loop_kernel whose sensor side reads its trial's camera from a second staged array.  With
// believed == cams and believed_index == cam_index it is the calibrated law on every trial's own camera.  A unit of its own, so that the
// two other flavours keep their resource figures.
#define UVS_BASELINE_FLAVOUR 2                                   // kBaselineWithScenes
#include "camera_analytical_device.hpp"

using namespace uvs_vision;

extern "C" {

int uvs_camera_believed_loop_scenes_f64(const uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int64_t T,
                                        const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, const double *q_start,
                                        const double *noise, double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status,
                                        int32_t *k_done, double *stats, int32_t *pixels, void *stream) {
    BaselineRequest r{};
    r.fp = fp; r.cams = cams; r.n_cams = n_cams; r.cam_index = cam_index;
    r.T = T; r.believed = believed; r.n_believed = n_believed; r.believed_index = believed_index;
    r.q_start = q_start; r.noise = noise; r.q_log = q_log; r.f_log = f_log; r.dq_log = dq_log; r.err_log = err_log;
    r.status = status; r.k_done = k_done; r.stats = stats; r.pixels = pixels; r.stream = stream;
    return run_baseline_loop(r);
}

}  // extern "C"
