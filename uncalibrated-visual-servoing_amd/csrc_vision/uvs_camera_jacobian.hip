// libuvs_vision.so, twentieth unit: the TRUE image Jacobian of the synthetic camera, dh/dq of the projection the pixel loops render, and the
// score of a logged X stream against it (the rules: plant.projection_jacobian and plant.jacobian_score).
// uvs_camera_jacobian_f64 (image_jacobian_kernel) and uvs_camera_jacobian_score_f64 (jacobian_score_kernel).  ONE device function,
// disc_jacobian, forms the two rows of a disc in both kernels, on the same operands in the same order, so the score's J has the bits the
// Jacobian call stores.  The chain is vision_device.hpp's chain_link -- the projection kernels' -- with z_i and o_i kept after every link.
//
// Mapping (both kernels).  Four lanes per record, lane = 4 record + disc: a lane owns the disc's two rows, 12 doubles = 96 contiguous
// bytes of the 48 n_points-byte record, so the sixteen records of a wavefront are one contiguous run of memory and every 16-byte access of
// a lane sits next to its neighbour's (a lane per record would stride 384 B between lanes).  Each lane repeats the six-link chain for
// itself: about 300 fp64 operations against 96 + 96 + 24 bytes moved.  The score's six sums are partial sums per disc, combined by the
// record's first lane in disc order through three wavefront shuffles: fixed order, no atomics, nothing depends on the launch's shape.
// Lanes of a disc the shape does not have, and the padding lanes of the last wavefront, compute on record 0's operands and store nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "uvs_vision.h"
#include "vision_device.hpp"

namespace uvs_vision {

constexpr int kScoreThreads = 256;
constexpr int kRecordLanes = kColours;                           // one lane per disc slot
constexpr int kScoreSums = 6;
constexpr long long kMostRecords = 1ll << 36;                     // four lanes each in workgroups of 256: 2^30 workgroups, a grid the launch can express

// du/dq and dv/dq of disc p of `cam` at joints q and step k of the motion `mot` (NULL: nothing moves): J[0] the u row, J[1] the v row.
__device__ __forceinline__ void disc_jacobian(const uvs_camera &cam, const uvs_target_motion *mot, int p, int k, const double *__restrict__ q,
                                              double (&J)[2][kSceneJoints]) {
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    double z[kSceneJoints][3], o[kSceneJoints][3];               // axis and origin of joint j: those of frame j - 1 (frame 0: the base)
#pragma unroll
    for (int i = 0; i < kSceneJoints; ++i) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            z[i][r] = pose[r][2];
            o[i][r] = pose[r][3];
        }
        double s, c;
        sincos(q[i] + cam.theta_offset[i], &s, &c);
        chain_link(cam, i, s, c, pose);
    }
    const long long moved = mot != nullptr ? motion_steps(mot->k_on, mot->k_off, k) : 0;
    double w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = moved_coordinate(cam.points[p][c], mot != nullptr ? mot->v[p][c] : 0.0, moved);
    const double dx = w[0] - pose[0][3], dy = w[1] - pose[1][3], dz = w[2] - pose[2][3];
    const double xc = pose[0][0] * dx + pose[1][0] * dy + pose[2][0] * dz;   // p = R^T (w - c): project_disc_at's
    const double yc = pose[0][1] * dx + pose[1][1] * dy + pose[2][1] * dz;
    const double zc = pose[0][2] * dx + pose[1][2] * dy + pose[2][2] * dz;
    const double zc2 = zc * zc;
#pragma unroll
    for (int j = 0; j < kSceneJoints; ++j) {
        const double ax = w[0] - o[j][0], ay = w[1] - o[j][1], az = w[2] - o[j][2];
        const double cx = z[j][1] * az - z[j][2] * ay, cy = z[j][2] * ax - z[j][0] * az, cz = z[j][0] * ay - z[j][1] * ax;   // z x (w - o)
        const double px = -(pose[0][0] * cx + pose[1][0] * cy + pose[2][0] * cz);                                           // dp/dq_j
        const double py = -(pose[0][1] * cx + pose[1][1] * cy + pose[2][1] * cz);
        const double pz = -(pose[0][2] * cx + pose[1][2] * cy + pose[2][2] * cz);
        J[0][j] = cam.focal * (px / zc - xc * pz / zc2);
        J[1][j] = cam.focal * (py / zc - yc * pz / zc2);
    }
}

// What a lane of either kernel is: record = row * T + t, its disc, and whether it has anything to store
struct RecordLane {
    long long record, row, t;
    int disc;
    bool live;
};
__device__ __forceinline__ RecordLane record_lane(int n_points, long long T, long long rows) {
    const long long i = static_cast<long long>(blockIdx.x) * kScoreThreads + threadIdx.x;
    RecordLane L;
    L.disc = static_cast<int>(i & (kRecordLanes - 1));
    L.record = i / kRecordLanes;
    L.live = L.record < rows * T && L.disc < n_points;
    if (!L.live) {                                               // computes on record 0, disc 0 and stores nothing
        L.record = 0;
        L.disc = 0;
    }
    L.row = L.record / T;
    L.t = L.record - L.row * T;
    return L;
}

__global__ __launch_bounds__(kScoreThreads) void image_jacobian_kernel(const Scenes S, const uvs_target_motion *__restrict__ motion, int n_points,
                                                                       long long T, long long rows, int k0, const double *__restrict__ q,
                                                                       double *__restrict__ j_out) {
    const RecordLane L = record_lane(n_points, T, rows);
    if (!L.live) return;
    double *out = j_out + (L.record * n_points + L.disc) * (2 * kSceneJoints);
    const long long scene = model_of(S, L.t);
    if (scene < 0) {                                             // names no scene: never an address
#pragma unroll
        for (int e = 0; e < 2 * kSceneJoints; ++e) out[e] = NAN;
        return;
    }
    double J[2][kSceneJoints];
    disc_jacobian(S.models[scene], motion != nullptr ? motion + L.t : nullptr, L.disc, k0 + static_cast<int>(L.row), q + L.record * kSceneJoints, J);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < kSceneJoints; ++j) out[r * kSceneJoints + j] = J[r][j];
}

__global__ __launch_bounds__(kScoreThreads) void jacobian_score_kernel(const Scenes S, const uvs_target_motion *__restrict__ motion, int n_points,
                                                                       long long T, long long K, double dt, const double *__restrict__ x_log,
                                                                       const double *__restrict__ q_log, const double *__restrict__ dq_log,
                                                                       const int32_t *__restrict__ k_done, double *__restrict__ score) {
    const RecordLane L = record_lane(n_points, T, K);
    const long long scene = model_of(S, L.t);
    const bool masked = k_done != nullptr && L.row >= k_done[L.t];   // a row that was never written: not read
    double sum[kScoreSums];
#pragma unroll
    for (int e = 0; e < kScoreSums; ++e) sum[e] = (masked || scene < 0) ? NAN : 0.0;
    if (L.live && !masked && scene >= 0) {
        double J[2][kSceneJoints], X[2][kSceneJoints], dq[kSceneJoints];
        disc_jacobian(S.models[scene], motion != nullptr ? motion + L.t : nullptr, L.disc, static_cast<int>(L.row), q_log + L.record * kSceneJoints, J);
        const double *x = x_log + (L.record * n_points + L.disc) * (2 * kSceneJoints);
#pragma unroll
        for (int e = 0; e < 2 * kSceneJoints; ++e) X[e / kSceneJoints][e % kSceneJoints] = x[e];
#pragma unroll
        for (int j = 0; j < kSceneJoints; ++j) dq[j] = dq_log != nullptr ? dq_log[L.record * kSceneJoints + j] : 0.0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double xd = 0.0, jd = 0.0;
#pragma unroll
            for (int j = 0; j < kSceneJoints; ++j) {
                const double xv = X[r][j], js = dt * J[r][j], d = xv - js;
                sum[0] += xv * xv;
                sum[1] += js * js;
                sum[2] += xv * js;
                sum[3] += d * d;
                xd += xv * dq[j];
                jd += js * dq[j];
            }
            sum[4] += xd * xd;
            sum[5] += xd * jd;
        }
        if (dq_log == nullptr) sum[4] = sum[5] = 0.0;
    }
    // the discs' partial sums, added in disc order by the record's first lane; every lane of the wavefront takes part in the shuffles
    double total[kScoreSums];
#pragma unroll
    for (int e = 0; e < kScoreSums; ++e) {
        total[e] = sum[e];
#pragma unroll
        for (int d = 1; d < kRecordLanes; ++d) {
            const double other = __shfl_down(sum[e], d, 64);
            if (d < n_points) total[e] += other;
        }
    }
    const long long i = static_cast<long long>(blockIdx.x) * kScoreThreads + threadIdx.x;
    if ((i & (kRecordLanes - 1)) == 0 && i / kRecordLanes < K * T) {
        double *out = score + (i / kRecordLanes) * kScoreSums;
#pragma unroll
        for (int e = 0; e < kScoreSums; ++e) out[e] = total[e];
    }
}

static int check_records(int64_t T, int64_t rows, int32_t n_points, const char *rows_name) {
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (rows < 0 || rows > INT32_MAX) return fail(UVS_ERR_ARG, "%s out of range", rows_name);
    if (!colours_ok(n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    return UVS_OK;
}

static unsigned record_blocks(int64_t T, int64_t rows) {
    const long long lanes = static_cast<long long>(T) * rows * kRecordLanes;
    return static_cast<unsigned>((lanes + kScoreThreads - 1) / kScoreThreads);
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

int uvs_camera_jacobian_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                            int32_t n_points, int64_t T, int64_t rows, int32_t k0, const double *q, double *j_out, void *stream) {
    g_err[0] = '\0';
    if (q == nullptr || j_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q or j_out");
    if (const int rc = check_records(T, rows, n_points, "rows")) return rc;
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (k0 < 0 || static_cast<int64_t>(k0) + rows > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "k0 must be >= 0 and k0 + rows at most 2^31 - 1");
    if (T == 0 || rows == 0) return UVS_OK;
    if (static_cast<long long>(T) * rows > kMostRecords) return fail(UVS_ERR_ARG, "%s", "rows * T above 2^36 records");
    hipLaunchKernelGGL(image_jacobian_kernel, dim3(record_blocks(T, rows)), dim3(kScoreThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, motion, static_cast<int>(n_points), static_cast<long long>(T), static_cast<long long>(rows),
                       static_cast<int>(k0), q, j_out);
    return launched("image_jacobian_kernel launch: %s");
}

int uvs_camera_jacobian_score_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                  int32_t n_points, int64_t T, int64_t K, double dt, const double *x_log, const double *q_log,
                                  const double *dq_log, const int32_t *k_done, double *score, void *stream) {
    g_err[0] = '\0';
    if (x_log == nullptr || q_log == nullptr || score == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL x_log, q_log or score");
    if (const int rc = check_records(T, K, n_points, "K")) return rc;
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0 || K == 0) return UVS_OK;
    if (static_cast<long long>(T) * K > kMostRecords) return fail(UVS_ERR_ARG, "%s", "K * T above 2^36 records");
    hipLaunchKernelGGL(jacobian_score_kernel, dim3(record_blocks(T, K)), dim3(kScoreThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, motion, static_cast<int>(n_points), static_cast<long long>(T), static_cast<long long>(K), dt,
                       x_log, q_log, dq_log, k_done, score);
    return launched("jacobian_score_kernel launch: %s");
}

}  // extern "C"
