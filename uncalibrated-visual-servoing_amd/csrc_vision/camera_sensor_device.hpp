// What the one-launch pixel loops share, written ONCE: the sensor side of a step -- joints, projection, frame-free detection, lane 0's report,
// the epilogue's stores -- for the estimator loop (camera_loop_device.hpp, eleven flavours) and the baseline loop (camera_analytical_device.hpp,
// seven); the analytic initial guess of a trial for the two guess kernels; and the mapping's constants with the launch decision that goes with them.
// The pieces are __device__ __forceinline__ functions over LDS row pointers and plain values: they declare no LDS and nothing is shared at
// run time, so every kernel keeps the registers, LDS and scratch it had when the text was written out in it (a shared
// __device__ body behind __global__ wrappers did move the allocation).  Every value is formed by the operations, in the order, of
// uvs_camera_features_f64 -- the library compiles with -ffp-contract=off -- which is what holds the one-launch loops to the stepwise ones bit for bit.
#pragma once
#include "../csrc/rmckf_device.hpp"

#include <climits>
#include <tuple>

#include "uvs_vision.h"
#include "vision_device.hpp"

// A loop header's kernel name from its table and the unit's flavour level (an integer literal), and that name as text for launched()
#define UVS_PASTE_(a, b) a##b
#define UVS_PASTE(a, b) UVS_PASTE_(a, b)
#define UVS_STR_(x) #x
#define UVS_STR(x) UVS_STR_(x)

namespace uvs_vision {

constexpr int kLoopTrials = 4;                                   // trials per workgroup of a large batch = wavefronts per workgroup
constexpr int kLoopThreads = 64 * kLoopTrials;
constexpr long long kSmallBatch = 256;                           // up to one trial per compute unit of an MI355X: one trial per workgroup
constexpr int kJoints = 6;                                       // the DH arms of this project (camera_jacobian<6>)

// The launch of a loop kernel over T trials: G = 1 trial per workgroup up to kSmallBatch, G = kLoopTrials beyond
struct LoopLaunch {
    bool small;
    unsigned blocks;
};
inline LoopLaunch loop_launch(long long T) {
    const bool small = T <= kSmallBatch;
    return {small, static_cast<unsigned>(small ? T : (T + kLoopTrials - 1) / kLoopTrials)};
}

// ---- joints, in two halves: where a kernel stores q_k between or after them is its own choice, and is measured.  Lane i < n
// advances joint i, q_k = q_{k-1} + dq_{k-1} * dt -- one rounded multiply and one rounded add (joint_sincos) -- from step 1 on (dq_row is
// read from then on alone), and leaves the sine and cosine of its DH angle in the wavefront's rows.
__device__ __forceinline__ void advance_joint(int i, int k, const double *dq_row, double dt, double &q) {
    if (k > 0) {
        const double step = dq_row[i] * dt;
        q = q + step;
    }
}
__device__ __forceinline__ void joint_sincos_rows(const uvs_camera &cam, int i, double q, double *sin_row, double *cos_row) {
    double s, c;
    sincos(q + cam.theta_offset[i], &s, &c);
    sin_row[i] = s;
    cos_row[i] = c;
}

// ---- projection (camera_features_kernel's): lane p < n_points multiplies the links and leaves its disc at disc_row[3 p]
__device__ __forceinline__ void project_lane_disc(const uvs_camera &cam, int p, const double *sin_row, const double *cos_row, double *disc_row) {
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
#pragma unroll 1                                                 // a rolled loop reads the DH table where it is used: unrolled, the whole table sits in SGPRs
    for (int i = 0; i < cam.n_joints; ++i) chain_link(cam, i, sin_row[i], cos_row[i], pose);
    project_disc(cam, p, pose, disc_row + 3 * p);
}

// The same for a MOVING target: disc p stands at step k of the trial's motion `mot` (LDS).  The moved point lives in
// transient registers of this call alone -- nothing is written back to the staged camera, which four wavefronts may share.
__device__ __forceinline__ void project_lane_disc_at(const uvs_camera &cam, int p, const uvs_target_motion &mot, int k, const double *sin_row,
                                                     const double *cos_row, double *disc_row) {
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
#pragma unroll 1
    for (int i = 0; i < cam.n_joints; ++i) chain_link(cam, i, sin_row[i], cos_row[i], pose);
    project_moved_disc(cam, p, mot, k, pose, disc_row + 3 * p);
}

// ---- frame-free detection: feature pair j is the centre of mass of disc j's colour (npts == 1: green).  The 64 lanes walk the colour's four
// 64-index blocks of centre_of_mass in index order -- only the blocks the disc's clipped bounding box touches.  All 64 lanes must call it,
// on the same discs (and, OCC, the same rectangles); lane 0, where the shuffle tree ends, holds the sums.
// PAINT (with OCC): the rectangles carry paints (vision_device.hpp).  The mask of the colour is then the disc's and that of the rectangles
// painted it, so a block is touched when the disc's box OR such a rectangle reaches it -- also where the disc draws nothing at all.
template <bool OCC, bool PAINT = false>
__device__ __forceinline__ ColourSum detect_pair(const double *disc_row, int npts, int j, int lane, const Rects &rects = Rects{},
                                                 uint32_t paints = kNoPaints) {
    static_assert(OCC || !PAINT, "paints belong to rectangles");
    const Disc me = load_disc(disc_row + 3 * j, true);
    int x0, x1, y0, y1;
    disc_box(me, x0, x1, y0, y1);
    ColourSum sum;
    int any_painted = 0;                                         // PAINT: is an active rectangle painted this colour?  Once per colour, uniform
    if constexpr (PAINT) any_painted = painted_at_all(rects, paints, npts == 1 ? 1 : j);
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
        const int lo = 64 * b, hi = lo + 63;
        // outside the clipped box disc_counts_at returns (0, 0) for all 64 indices, whose partial is (+0.0, +0.0, 0): exact to add, so not formed
        bool touched = me.r2 >= 0.0 && ((x0 <= hi && x1 >= lo) || (y0 <= hi && y1 >= lo));
        if constexpr (PAINT) {
            if (any_painted) touched = touched || paint_reaches(rects, paints, npts == 1 ? 1 : j, lo, hi);
        }
        double su = 0.0, sv = 0.0;
        int n = 0;
        if (__builtin_amdgcn_readfirstlane(static_cast<int>(touched))) {   // the same discs in every lane: wavefront-uniform
            int cc, rc;
            if constexpr (PAINT)
                painted_counts_in_box(disc_row, npts, j, npts == 1 ? 1 : j, me, x0, x1, y0, y1, lo + lane, cc, rc, rects, paints, any_painted);
            else
                disc_counts_in_box<OCC>(disc_row, npts, j, me, x0, x1, y0, y1, lo + lane, cc, rc, rects);
            wave_partial(cc, rc, lo + lane, su, sv, n);
        }
        sum.add(su, sv, n);
    }
    return sum;
}

// ---- lane 0's report of pair j, in two halves so that a kernel that holds a lost disc's pair can step in between.  First the pair as
// detected: the centre (NaN for an empty mask) and f += noise (experiment.py:135); noise_row is the trial's row of this step, or NULL.
__device__ __forceinline__ void noisy_centre(const ColourSum &sum, const double *noise_row, int j, double &u, double &v) {
    sum.centre(u, v);
    if (noise_row != nullptr) {
        u += noise_row[2 * j];
        v += noise_row[2 * j + 1];
    }
}

// Then where it goes: to the estimator or control side through f_row (LDS), always, and -- for a trial whose rows are still due (`seen`) --
// into the smallest mask so far and the f log (f_log_row: the trial's row of this step, or NULL).
__device__ __forceinline__ void report_pair(int count, int j, double u, double v, bool seen, double *f_row, int *pix_row, double *f_log_row) {
    f_row[2 * j] = u;
    f_row[2 * j + 1] = v;
    if (seen) {
        pix_row[j] = count < pix_row[j] ? count : pix_row[j];
        if (f_log_row != nullptr) {
            f_log_row[2 * j] = u;
            f_log_row[2 * j + 1] = v;
        }
    }
}

// ---- epilogue of a trial whose outputs are `due`: lane i < 3 forms norm i over the features in order, as stats_kernel forms it, from the
// per-feature ISE, IAE and ITAE sums; lane p < npts stores disc p's smallest mask (pixels may be NULL).
template <int M>
__device__ __forceinline__ void store_norms_and_pixels(bool due, int lane, int npts, long long trial, const double (&sums)[3][M], const int *pix_row,
                                                       double *stats, int32_t *pixels) {
    if (lane < 3 && due) {
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc = fma(sums[lane][i], sums[lane][i], acc);
        stats[3 * trial + lane] = sqrt(acc);
    }
    if (lane < npts && due && pixels != nullptr) pixels[trial * npts + lane] = pix_row[lane];
}

// ---- the analytic initial guess of plant.analytic_guess for trial t, by one lane: the geometric Jacobian in the camera frame at q_start
// on the model `cam`, the depths |camera - point|, and the image Jacobian rows at the DETECTED features f0, into the trial's x0 rows.
__device__ __forceinline__ void guess_trial(const uvs_camera &cam, long long t, int n_points, const double *__restrict__ q_start,
                                            const double *__restrict__ f0, double *__restrict__ x0_out) {
    constexpr int N = kJoints;
    uvs_plant pl;                                                // camera_jacobian reads the DH table alone
    double q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pl.theta_offset[i] = cam.theta_offset[i];
        pl.d[i] = cam.d[i];
        pl.a[i] = cam.a[i];
        pl.cos_alpha[i] = cam.cos_alpha[i];
        pl.sin_alpha[i] = cam.sin_alpha[i];
        q[i] = q_start[t * N + i];
    }
    double rot[9], pos[3], Jc[6][N];
    uvs::camera_jacobian<N>(pl, q, rot, pos, Jc);
    const int m = 2 * n_points;
    const double focal = cam.focal;
    for (int p = 0; p < n_points; ++p) {
        const double depth = uvs::point_depth(pos, cam.points[p]);
        const double u = f0[t * m + 2 * p], v = f0[t * m + 2 * p + 1];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double x[N];
            uvs::feature_jacobian_row<N>(focal, u, v, depth, half, Jc, x);
#pragma unroll
            for (int j = 0; j < N; ++j) x0_out[(t * m + 2 * p + half) * N + j] = x[j];
        }
    }
}

}  // namespace uvs_vision
