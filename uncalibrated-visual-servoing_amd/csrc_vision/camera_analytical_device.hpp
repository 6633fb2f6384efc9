// The step of the calibrated IBVS baseline, defined ONCE for the units that run it: uvs_camera_analytical.hip (the model is the camera that
// renders the frames, uniform over the launch) and uvs_camera_believed.hip (the model is a per-trial uvs_camera read from memory).  Both
// compile it with -ffp-contract=off on the same operands in the same order, so a believed model that equals the true one gives the bits of
// the calibrated kernels.  Next to it: what every entry point of the two units asks of (fp, cam, T) before its first HIP call.
#pragma once
#include "../csrc/rmckf_device.hpp"

#include <climits>

#include "uvs_vision.h"
#include "vision_device.hpp"

namespace uvs_vision {

constexpr int kAJoints = 6;                                      // the DH arms of this project (camera_jacobian<6>)

// One step of the calibrated law for this lane's R rows of its trial.  q: the trial's joints; feat(i): component i of the trial's detected
// features (raw pixels, noise added).  Writes this lane's rows of J into st.x and of f - desired into err, and the command (replicated in
// the L lanes) into cmd.  Returns non-zero when an entry of J -- any row of the trial -- is not finite: pinv raises there (experiment.py:313-316).
// All L lanes of a trial, and all 64 lanes of the wavefront, must call it.
template <int M, int N, int L, class Feat>
__device__ __forceinline__ int analytical_step(const uvs_camera &cam, const uvs_filter_params &fp, const double (&q)[N], Feat feat, int sub,
                                               uvs::Rows<M, N, L> &st, double (&err)[M / L], double (&cmd)[N]) {
    constexpr int R = M / L;
    uvs_plant pl;                                                // camera_jacobian reads the DH table alone
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pl.theta_offset[i] = cam.theta_offset[i];
        pl.d[i] = cam.d[i];
        pl.a[i] = cam.a[i];
        pl.cos_alpha[i] = cam.cos_alpha[i];
        pl.sin_alpha[i] = cam.sin_alpha[i];
    }
    double rot[9], pos[3], Jc[6][N];
    uvs::camera_jacobian<N>(pl, q, rot, pos, Jc);
    double kap[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = sub * R + r, p = row >> 1;
        const double depth = uvs::point_depth(pos, cam.points[p]);   // computeZ(recalculate_fkine=True): the true camera-disc distance
        const double u = feat(2 * p), v = feat(2 * p + 1);           // the NOISY DETECTED pixels (experiment.py:149-162)
        uvs::feature_jacobian_row<N>(cam.focal, u, v, depth, row & 1, Jc, st.x[r]);
        err[r] = feat(row) - fp.desired[row];
        kap[r] = 1.0;                                                // experiment.py:306
    }
    const int bad = st.any_nonfinite();
    // the pixel loop's own solver sequence (uvs_camera_loop.hip): the plain solve with its watches, the careful one for a solve whose watch fires
    const bool strict = (fp.reserved & UVS_OPT_STRICT_PINV) != 0;
    const bool suspect = strict || uvs::control_law<M, N, L, false>(st, kap, err, fp.gain, sub, cmd);
    if (__any(suspect)) {
        double careful[N];
        uvs::control_law<M, N, L, true>(st, kap, err, fp.gain, sub, careful);
#pragma unroll
        for (int j = 0; j < N; ++j) cmd[j] = suspect ? careful[j] : cmd[j];
    }
    return bad;
}

// What the entry points ask of (fp, cam, T); every refusal comes before the first HIP call.
inline int check_analytical(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T) {
    if (fp == nullptr || cam == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp or cam");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (cam->n_joints < 1 || cam->n_joints > UVS_CAMERA_MAX_JOINTS) return fail(UVS_ERR_ARG, "%s", "n_joints must be 1 .. 8");
    if (!colours_ok(cam->n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (fp->method != UVS_METHOD_ANALYTICAL)
        return fail(UVS_ERR_METHOD, "%s", "method must be ANALYTICAL (the estimators' pixel loop is uvs_camera_closed_loop_f64)");
    if (fp->reserved != 0 && fp->reserved != UVS_OPT_STRICT_PINV) return fail(UVS_ERR_ARG, "%s", "reserved must be 0 or UVS_OPT_STRICT_PINV");
    if (fp->lanes_per_filter != 0) return fail(UVS_ERR_SHAPE, "%s", "lanes_per_filter must be 0: the kernels have one mapping per shape");
    if (fp->m != 2 * cam->n_points) return fail(UVS_ERR_SHAPE, "%s", "fp->m must be 2 * cam->n_points");
    if (fp->n != cam->n_joints) return fail(UVS_ERR_SHAPE, "%s", "fp->n must be cam->n_joints");
    if (fp->n != kAJoints || (fp->m != 8 && fp->m != 6 && fp->m != 2)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return UVS_OK;
}

}  // namespace uvs_vision
