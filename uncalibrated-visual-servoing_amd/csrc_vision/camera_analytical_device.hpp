// The calibrated IBVS baseline, defined ONCE for the units that run it: uvs_camera_analytical.hip (the model is the camera that renders the
// frames, uniform over the launch) and uvs_camera_believed.hip (the model is a per-trial uvs_camera read from memory).  Two things live here.
// (1) The step, analytical_step, which every kernel of the two units calls.  Both compile it with -ffp-contract=off on the same operands in
// the same order, so a believed model that equals the true one gives the bits of the calibrated kernels.
// (2) The pixel loop as ONE launch per batch: one kernel text in seven flavours, chosen per TRANSLATION UNIT as camera_loop_device.hpp chooses
// its eleven: a unit states ONE integer before it includes this header, #define UVS_BASELINE_FLAVOUR <0 .. 6>, a value of BaselineFlavour
// below.  The flavours are a strict chain, so every switch of the kernel text is a comparison of that level, and the level alone picks the
// argument block (BaselineLoopArgsList) and the kernel's name (UVS_BASELINE_KERNEL_<f>).  The host side is shared too: every loop entry
// point fills a BaselineRequest from its parameters and calls run_baseline_loop (at the end of this header).
// Level kBaselineCalibrated (uvs_camera_analytical.hip) is camera_analytical_loop_kernel(ALoopArgs): one model, taken from the kernel
// argument, every trial known.  Level kBaselineWithModel (uvs_camera_believed.hip) is camera_believed_loop_kernel(BLoopArgs): the control
// side's model of every trial is staged from memory into s_cam[G], and a trial whose index names no model starts FAILed (not alive, not seen),
// so that it logs no row and writes status and k_done alone.  Same names, argument blocks, registers and LDS as when each was written out in its unit.
// Level kBaselineWithScenes (uvs_camera_scenes_baseline.hip) is a third flavour, scene_baseline_loop_kernel(SLoopArgs): the
// believed one whose sensor side reads the trial's own camera as well, from a second staged array.
// Level kBaselineWithMotion (uvs_camera_moving_baseline.hip) is a fourth, moving_baseline_kernel(MovingBaselineArgs): the scenes
// one whose sensor side projects every disc where its trial's motion has taken it.  The law's model does not move.
// Level kBaselineWithLatency (uvs_camera_delayed_baseline.hip) is a fifth, delayed_baseline_kernel(DelayedBaselineArgs): the
// moving one whose detector is handed the frame of step max(k - d, 0), d the trial's latency, through an LDS ring of detections per disc
// (DESIGN.md 4.24).  The law's joints stay the current ones.
// Level kBaselineWithAssumed (uvs_camera_aligned_baseline.hip) is a sixth, aligned_baseline_kernel(AlignedBaselineArgs): the
// delayed one whose law is told a latency -- the joints handed to analytical_step at step k are q_{max(k - a, 0)}, a the trial's ASSUMED
// latency, through s_q as a ring of the last nine steps' joints.  The q log and the joint integration stay current.
// Level kBaselineWithHorizon (uvs_camera_predicted_baseline.hip) is a seventh, predicted_baseline_kernel(PredictedBaselineArgs):
// the aligned one whose law is handed f^ = f_reported + (h(q_k) - h(q_{max(k - p, 0)})), p the trial's prediction HORIZON and h the (u, v) the
// projection kernel gives for the law's own model.  The sensor-side wavefront of a trial projects the law's model at q_k
// next to the scene, once per step, into slot k mod 9 of the ring s_h -- lanes N .. 2 N - 1 take the model's sines in the sincos call that
// lanes 0 .. N - 1 take the scene's in, lanes n_points .. 2 n_points - 1 multiply the model's links in the call the first n_points multiply
// the scene's in (measured: 0.5 % over the aligned twin, against 6.3 % with the two done one after the other) -- and the barriers that were
// there stand between that store and the law's reads.
// Next to them: what every entry point of the two units asks of (fp, cam, T) before its first HIP call.
//
// The loop's mapping is the one of camera_loop_kernel (camera_loop_device.hpp), decided and measured there -- 256 threads = one wavefront per
// SIMD, G = 1 trial per workgroup up to 256 trials and G = 4 beyond, the sensor side of camera_sensor_device.hpp on the camera that renders
// the frames -- with the estimator side of wavefront 0 replaced by the step, for which the sensor side hands the joints over in LDS next to
// the features.  Every barrier is at the top level of the step loop and reached by all 256 threads; padding and FAILed trials keep computing
// and store nothing; the one early exit ("every trial of this workgroup has failed") is read by every thread from the same G LDS words.
#pragma once
#include "camera_sensor_device.hpp"

namespace uvs_vision {

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

// ---------------------------------------------------------------------------------------------------------------- the loop, one launch
// (Believed, model_of and stage_models, which the believed flavour reads its models with, are vision_device.hpp's: the scenes share them.)
struct ALoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;
    long long T;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;                    // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

struct BLoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;                                              // the sensor side's: the camera that renders the frames
    Believed B;                                                  // the control side's
    long long T;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;                    // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

// The third flavour (level kBaselineWithScenes, uvs_camera_scenes_baseline.hip): scene_baseline_loop_kernel, the
// believed flavour whose SENSOR side reads the trial's own camera too, from a second staged array, s_scene[G].  `cam` is the shape alone.
struct SLoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;                                              // n_joints and n_points of the launch (fp's); word 0 of every staged scene
    Believed B;                                                  // the control side's
    Scenes S;                                                    // the sensor side's: the cameras that render the trials' frames
    long long T;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;                    // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};

// The fourth flavour (level kBaselineWithMotion, uvs_camera_moving_baseline.hip): moving_baseline_kernel, the scenes
// flavour with a motion per OUTPUT trial, staged into s_mot[G] next to the scenes.  The SENSOR side's points move; the law's model stays.
struct MovingBaselineArgs : SLoopArgs {
    const uvs_target_motion *motion;                             // [T] by output trial, or NULL: nothing moves
};

// The fifth flavour (level kBaselineWithLatency, uvs_camera_delayed_baseline.hip): delayed_baseline_kernel, the
// moving flavour with a latency per OUTPUT trial.  The detections go through s_ring; the law reads the current joints.
struct DelayedBaselineArgs : MovingBaselineArgs {
    const int32_t *latency;                                      // [T] by output trial, or NULL: none
};

// The sixth flavour (level kBaselineWithAssumed, uvs_camera_aligned_baseline.hip): aligned_baseline_kernel, the
// delayed flavour with an ASSUMED latency per OUTPUT trial.  s_q is a ring; the law reads the joints of step max(k - a, 0).
struct AlignedBaselineArgs : DelayedBaselineArgs {
    const int32_t *assumed;                                      // [T] by output trial, or NULL: none
};

// The seventh flavour (level kBaselineWithHorizon, uvs_camera_predicted_baseline.hip): predicted_baseline_kernel,
// the aligned flavour with a prediction HORIZON per OUTPUT trial.  s_h is a ring of the law's model's (u, v) at the last nine steps' joints.
struct PredictedBaselineArgs : AlignedBaselineArgs {
    const int32_t *predict;                                      // [T] by output trial, or NULL: none
};

// The unit's flavour: the value it gave UVS_BASELINE_FLAVOUR.  Row f of the three tables below -- level, argument block, kernel name -- is one flavour.
enum BaselineFlavour {
    kBaselineCalibrated, kBaselineWithModel, kBaselineWithScenes, kBaselineWithMotion, kBaselineWithLatency, kBaselineWithAssumed,
    kBaselineWithHorizon
};
using BaselineLoopArgsList = std::tuple<ALoopArgs, BLoopArgs, SLoopArgs, MovingBaselineArgs, DelayedBaselineArgs, AlignedBaselineArgs,
                                        PredictedBaselineArgs>;
#define UVS_BASELINE_KERNEL_0 camera_analytical_loop_kernel
#define UVS_BASELINE_KERNEL_1 camera_believed_loop_kernel
#define UVS_BASELINE_KERNEL_2 scene_baseline_loop_kernel
#define UVS_BASELINE_KERNEL_3 moving_baseline_kernel
#define UVS_BASELINE_KERNEL_4 delayed_baseline_kernel
#define UVS_BASELINE_KERNEL_5 aligned_baseline_kernel
#define UVS_BASELINE_KERNEL_6 predicted_baseline_kernel

#ifndef UVS_BASELINE_FLAVOUR
#error "state the unit's flavour before including this header: #define UVS_BASELINE_FLAVOUR <0 .. 6>, a value of BaselineFlavour"
#endif
constexpr int kBaselineFlavour = UVS_BASELINE_FLAVOUR;
static_assert(kBaselineFlavour >= kBaselineCalibrated && kBaselineFlavour <= kBaselineWithHorizon, "UVS_BASELINE_FLAVOUR is a value of BaselineFlavour");
constexpr bool kCameraBelieved = kBaselineFlavour >= kBaselineWithModel, kBaselineScenes = kBaselineFlavour >= kBaselineWithScenes;
constexpr bool kBaselineMoving = kBaselineFlavour >= kBaselineWithMotion, kBaselineDelayed = kBaselineFlavour >= kBaselineWithLatency;
constexpr bool kBaselineAligned = kBaselineFlavour >= kBaselineWithAssumed, kBaselinePredicted = kBaselineFlavour >= kBaselineWithHorizon;
using BaselineLoopArgs = std::tuple_element_t<kBaselineFlavour, BaselineLoopArgsList>;
#define UVS_BASELINE_LOOP_KERNEL UVS_PASTE(UVS_BASELINE_KERNEL_, UVS_BASELINE_FLAVOUR)

// Has `trial` a model?  Calibrated: always, folded away.  Believed: the same word in all 64 lanes of a sensor-side wavefront.
__device__ __forceinline__ bool has_model(const ALoopArgs &, long long) { return true; }
__device__ __forceinline__ bool has_model(const BLoopArgs &a, long long trial) { return model_of(a.B, trial) >= 0; }
// Scenes: a model to believe in AND a scene to be rendered by; a trial without either starts FAILed
__device__ __forceinline__ bool has_model(const SLoopArgs &a, long long trial) { return model_of(a.B, trial) >= 0 && model_of(a.S, trial) >= 0; }
// The control side's models of the workgroup's trials into LDS, by all kLoopThreads threads.  Calibrated: the one model of the launch -- the
// 6 x 6 camera Jacobian uses the whole DH table in every step, and held in scalar registers next to the sensor side's the table spilled (36 B
// of scratch per lane in the four-trial form).
template <int G>
__device__ __forceinline__ void stage_loop_models(const ALoopArgs &a, uvs_camera *s_cam) {
    for (int i = threadIdx.x; i < kCamWords; i += kLoopThreads) reinterpret_cast<double *>(s_cam)[i] = reinterpret_cast<const double *>(&a.cam)[i];
}
template <int G>
__device__ __forceinline__ void stage_loop_models(const BLoopArgs &a, uvs_camera *s_cam) {
    stage_models<G, kLoopThreads>(a.B, static_cast<long long>(blockIdx.x) * G, a.T, s_cam);
}
template <int G>
__device__ __forceinline__ void stage_loop_models(const SLoopArgs &a, uvs_camera *s_cam) {
    stage_models<G, kLoopThreads>(a.B, static_cast<long long>(blockIdx.x) * G, a.T, s_cam);
}
// The sensor side's cameras of the workgroup's trials into LDS.  The other two flavours have the one camera of the launch: nothing to stage.
template <int G>
__device__ __forceinline__ void stage_loop_scenes(const ALoopArgs &, uvs_camera *) {}
template <int G>
__device__ __forceinline__ void stage_loop_scenes(const BLoopArgs &, uvs_camera *) {}
template <int G>
__device__ __forceinline__ void stage_loop_scenes(const SLoopArgs &a, uvs_camera *s_scene) {
    stage_scenes<G, kLoopThreads>(a.S, a.cam, static_cast<long long>(blockIdx.x) * G, a.T, s_scene);
}
// The motions of the workgroup's trials into LDS.  The other three flavours have none: nothing to stage.
template <int G>
__device__ __forceinline__ void stage_loop_motions(const ALoopArgs &, uvs_target_motion *) {}
template <int G>
__device__ __forceinline__ void stage_loop_motions(const BLoopArgs &, uvs_target_motion *) {}
template <int G>
__device__ __forceinline__ void stage_loop_motions(const SLoopArgs &, uvs_target_motion *) {}
template <int G>
__device__ __forceinline__ void stage_loop_motions(const MovingBaselineArgs &a, uvs_target_motion *s_mot) {
    stage_motions<G, kLoopThreads>(a.motion, static_cast<long long>(blockIdx.x) * G, a.T, s_mot);
}
// The latency of `trial`.  The first four flavours have none.
__device__ __forceinline__ int loop_latency(const ALoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_latency(const BLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_latency(const SLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_latency(const DelayedBaselineArgs &a, long long trial) { return latency_of(a.latency, trial); }
// The assumed latency of `trial`.  The first five flavours have none.
__device__ __forceinline__ int loop_assumed(const ALoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_assumed(const BLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_assumed(const SLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_assumed(const AlignedBaselineArgs &a, long long trial) { return latency_of(a.assumed, trial); }
// project_lane_disc_at's text (camera_sensor_device.hpp) over a chain of the launch's n joints -- a model's own n_joints word is never a
// bound -- for the seventh flavour alone, where the lanes that project the scene and the lanes that project the law's model run it side by
// side: a motion whose window is empty moves nothing (moved_coordinate returns the coordinate itself), so it is project_disc's bits.
__device__ __forceinline__ void project_lane_disc_of(const uvs_camera &cam, int n, int p, const uvs_target_motion &mot, int k, const double *sin_row,
                                                     const double *cos_row, double *out) {
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
#pragma unroll 1
    for (int i = 0; i < n; ++i) chain_link(cam, i, sin_row[i], cos_row[i], pose);
    project_moved_disc(cam, p, mot, k, pose, out);
}
// The prediction horizon of `trial`.  The first six flavours have none.
__device__ __forceinline__ int loop_horizon(const ALoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_horizon(const BLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_horizon(const SLoopArgs &, long long) { return 0; }
__device__ __forceinline__ int loop_horizon(const PredictedBaselineArgs &a, long long trial) { return latency_of(a.predict, trial); }

template <int M, int N, int L, int G>
__global__ __launch_bounds__(kLoopThreads) void UVS_BASELINE_LOOP_KERNEL(const BaselineLoopArgs A) {
    constexpr bool BELIEVED = kCameraBelieved;
    constexpr int R = M / L, W = kLoopThreads / 64;
    static_assert((G == 1 || G == W) && W == kColours && G * L <= 64 && N <= UVS_CAMERA_MAX_JOINTS && M <= 2 * kColours, "one or four trials per workgroup");
    __shared__ double s_sin[W][UVS_CAMERA_MAX_JOINTS], s_cos[W][UVS_CAMERA_MAX_JOINTS];   // per wavefront (G = 1: four copies of one trial's)
    __shared__ double s_disc[W][kColours * 3];
    constexpr bool ALIGNED = kBaselineAligned;
    __shared__ double s_q[G][ALIGNED ? kDelaySlots : 1][N];      // this step's joints, sensor side -> control side (ALIGNED: the last nine steps', slot k mod 9)
    __shared__ double s_f[G][M];                                 // this step's features, sensor side -> control side
    __shared__ double s_dq[G][N];                                // this step's command, control side -> sensor side
    __shared__ int s_alive[G];                                   // trial has not FAILed, as of the end of this step
    __shared__ int s_pix[G][kColours];                           // smallest mask so far
    __shared__ double s_sum[G][3][M];                            // per-feature ISE, IAE, ITAE after the loop
    __shared__ uvs_camera s_cam[BELIEVED ? G : 1];               // the control side's models; written once here, and the step loop's barriers
    stage_loop_models<G>(A, s_cam);                              // stand between this and the first read
    constexpr bool SCENES = kBaselineScenes;
    __shared__ uvs_camera s_scene[SCENES ? G : 1];               // SCENES: the sensor side's cameras; the barrier before the step loop stands
    stage_loop_scenes<G>(A, s_scene);                            // between this and step 0's sines
    constexpr bool MOVING = kBaselineMoving;
    __shared__ uvs_target_motion s_mot[MOVING ? G : 1];          // MOVING: the motions of those trials; the same barrier covers them
    stage_loop_motions<G>(A, s_mot);
    constexpr bool DELAYED = kBaselineDelayed;
    __shared__ DelayCell s_ring[DELAYED ? G : 1][DELAYED ? kColours : 1][DELAYED ? kDelaySlots : 1];   // DELAYED: the last nine detections of every disc
    constexpr bool PREDICTED = kBaselinePredicted;
    __shared__ double s_msin[PREDICTED ? W : 1][UVS_CAMERA_MAX_JOINTS], s_mcos[PREDICTED ? W : 1][UVS_CAMERA_MAX_JOINTS];   // PREDICTED: the sines of the LAW's model
    __shared__ double s_h[PREDICTED ? G : 1][PREDICTED ? kDelaySlots : 1][PREDICTED ? 3 * kColours : 1];   // PREDICTED: its (u, v, r) at the last nine steps' joints, slot k mod 9
    __shared__ double s_hdump[PREDICTED && G == 1 ? W : 1][PREDICTED ? 3 * kColours : 1];   // PREDICTED, one trial: where the three wavefronts that do not write s_h leave theirs
    __shared__ uvs_target_motion s_still;                        // PREDICTED: the motion that moves nothing, for the model's lanes
    if constexpr (PREDICTED) {
        for (int i = threadIdx.x; i < kMotionWords; i += kLoopThreads) reinterpret_cast<uint64_t *>(&s_still)[i] = 0ull;   // covered like s_mot
    }

    const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const uvs_filter_params &fp = A.fp;
    const uvs_camera &cam = A.cam;                               // the sensor side keeps reading the true camera from the kernel arguments
    const long long T = A.T;
    const int K = fp.steps, npts = cam.n_points;

    // sensor side: this wavefront's trial, and the feature pairs it detects: all of its own trial's, or every fourth of the workgroup's one trial
    const int ws = G == 1 ? 0 : w;
    const uvs_camera &scene = SCENES ? s_scene[ws] : cam;        // the camera that renders this trial's frames
    const bool writer = G == W || w == 0;                        // G = 1: the four wavefronts hold the same joints; the first one logs them
    const int j_first = G == 1 ? w : 0, j_step = G == 1 ? W : 1;
    long long trial = static_cast<long long>(blockIdx.x) * G + ws;
    const bool valid = trial < T;
    if (!valid) trial = T - 1;                                   // a padding wavefront shadows the last trial and stores nothing
    const bool known = has_model(A, trial);
    int delay = 0;                                               // DELAYED: the latency of the trial (a padding wavefront: of the one it shadows)
    if constexpr (DELAYED) delay = loop_latency(A, trial);
    // PREDICTED: lanes N .. 2 N - 1 carry the same joints through the same two operations, for the sines of the LAW's model next to the scene's
    const int joint = (PREDICTED && lane >= N) ? lane - N : lane;
    const int joint_lanes = PREDICTED ? 2 * N : N;
    double q = lane < joint_lanes ? A.q_start[trial * N + joint] : 0.0;
    // this lane's own addresses in row 0 of the [K][T][comp] logs (NULL: not wanted, or nothing of this lane's), advanced by a row per step
    const long long step_rows = T;
    double *q_at = (valid && writer && lane < N && A.q_log != nullptr) ? A.q_log + trial * N + lane : nullptr;
    double *f_at = (valid && lane == 0 && A.f_log != nullptr) ? A.f_log + trial * M : nullptr;
    const double *noise_at = A.noise != nullptr ? A.noise + trial * M : nullptr;
    bool seen = known;                                           // this trial has not FAILed before this step: its rows q[k], f[k] are due
    if (lane < kColours) s_pix[ws][lane] = INT_MAX;

    // control side (wavefront 0): this lane's trial and rows; the lanes from G L on shadow the first ones and store nothing
    const int slot = (lane / L) & (G - 1), sub = lane % L;
    long long etrial = static_cast<long long>(blockIdx.x) * G + slot;
    const bool owner = lane < G * L;
    const bool evalid = owner && etrial < T;
    if (etrial >= T) etrial = T - 1;
    double *err_at = (evalid && A.err_log != nullptr) ? A.err_log + etrial * M + sub * R : nullptr;
    double *dq_at = (evalid && sub == 0 && A.dq_log != nullptr) ? A.dq_log + etrial * N : nullptr;
    int assumed = 0;                                             // ALIGNED: the assumed latency of this lane's trial (a shadow lane: of the one it shadows)
    if constexpr (ALIGNED) {
        if (w == 0) assumed = loop_assumed(A, etrial);
    }
    int horizon = 0;                                             // PREDICTED: the prediction horizon of this lane's trial (a shadow lane: of the one it shadows)
    if constexpr (PREDICTED) {
        if (w == 0) horizon = loop_horizon(A, etrial);
    }
    double ise[R], iae[R], itae[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ise[r] = iae[r] = itae[r] = 0.0;
    double t = 0.0 + fp.dt;                                      // engine._loop_times: t_s accumulated in floating point
    bool alive = has_model(A, etrial);                           // no model: FAILed before step 0
    int status = alive ? UVS_STATUS_SUCCESS : UVS_STATUS_FAIL, k_done = alive ? K : 0;
    if constexpr (SCENES) __syncthreads();                       // the staged scenes: step 0's sines read them before the step's first barrier

    for (int k = 0; k < K; ++k) {
        // ---- the sensor side of the step (camera_sensor_device.hpp): joints, projection, detection
        if constexpr (PREDICTED) {
            if (lane < 2 * N) {                                  // one sincos for both: lanes < N the scene's, the others the law's model's (staged
                advance_joint(joint, k, s_dq[ws], fp.dt, q);     // before the barrier that precedes step 0)
                if (seen && q_at != nullptr) *q_at = q;          // q_at is NULL beyond lane N - 1
                if (writer && lane < N) s_q[ws][k % kDelaySlots][lane] = q;
                const bool mine = lane < N;
                joint_sincos_rows(mine ? scene : s_cam[ws], joint, q, mine ? s_sin[w] : s_msin[w], mine ? s_cos[w] : s_mcos[w]);
            }
        } else if (lane < N) {
            advance_joint(lane, k, s_dq[ws], fp.dt, q);
            if (seen && q_at != nullptr) *q_at = q;              // before the sines: where this text measured fastest
            if (writer) s_q[ws][ALIGNED ? k % kDelaySlots : 0][lane] = q;
            joint_sincos_rows(scene, lane, q, s_sin[w], s_cos[w]);
        }
        __syncthreads();
        if constexpr (PREDICTED) {                               // lanes < npts: the scene's disc where the motion has taken it; the next npts lanes: h(q_k),
            if (lane < 2 * npts) {                               // the projection kernel's text on the law's model, whose points do not move
                const bool mine = lane < npts;
                const int p = mine ? lane : lane - npts;
                double *row = mine ? s_disc[w] : (writer ? s_h[ws][k % kDelaySlots] : s_hdump[G == 1 ? w : 0]);
                project_lane_disc_of(mine ? scene : s_cam[ws], N, p, mine ? s_mot[ws] : s_still, k, mine ? s_sin[w] : s_msin[w],
                                     mine ? s_cos[w] : s_mcos[w], row + 3 * p);
            }
        } else if constexpr (MOVING) {                           // the disc where step k of the trial's motion has taken it
            if (lane < npts) project_lane_disc_at(scene, lane, s_mot[ws], k, s_sin[w], s_cos[w], s_disc[w]);
        } else {
            if (lane < npts) project_lane_disc(scene, lane, s_sin[w], s_cos[w], s_disc[w]);
        }
        __syncthreads();
#pragma unroll 1
        for (int j = j_first; j < npts; j += j_step) {
            ColourSum sum = detect_pair<false>(s_disc[w], npts, j, lane);
            if (lane == 0) {                                     // the lane the shuffle tree ends in
                if constexpr (DELAYED) delay_line(s_ring[ws][j], sum, k, delay);   // in place: the detection of step max(k - delay, 0)
                double u, v;
                noisy_centre(sum, noise_at, j, u, v);
                report_pair(sum.count, j, u, v, seen, s_f[ws], s_pix[ws], f_at);
            }
        }
        __syncthreads();
        // ---- the law of the workgroup's trials, each on its model (the step kernel's sequence)
        if (w == 0) {
            double qk[N], err[R], cmd[N];
#pragma unroll
            for (int j = 0; j < N; ++j) qk[j] = s_q[slot][ALIGNED ? delayed_step(k, assumed) % kDelaySlots : 0][j];   // ALIGNED: the joints the assumed frame shows
            uvs::Rows<M, N, L> st;
            int bad;
            if constexpr (PREDICTED) {                           // the law on f^: the difference first, then one add -- two rounded operations
                const double *now = s_h[slot][k % kDelaySlots], *then = s_h[slot][delayed_step(k, horizon) % kDelaySlots];
                bad = analytical_step<M, N, L>(s_cam[BELIEVED ? slot : 0], fp, qk,
                                               [slot, now, then](int i) { const int at = 3 * (i >> 1) + (i & 1); const double moved = now[at] - then[at]; return s_f[slot][i] + moved; }, sub, st, err, cmd);
            } else {
                bad = analytical_step<M, N, L>(s_cam[BELIEVED ? slot : 0], fp, qk, [slot](int i) { return s_f[slot][i]; }, sub, st, err, cmd);
            }
            if (alive && bad) {                                  // FAIL at this step; the trial stops
                alive = false;
                status = UVS_STATUS_FAIL;
                k_done = k;
            }
            if (alive && evalid) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (err_at != nullptr) err_at[r] = err[r];
                    const double ae = fabs(err[r]);              // stats_kernel's sums, in its order over k
                    ise[r] = fma(err[r], err[r], ise[r]);
                    iae[r] += ae;
                    itae[r] = fma(t, ae, itae[r]);
                }
                if (dq_at != nullptr) {
#pragma unroll
                    for (int j = 0; j < N; ++j) dq_at[j] = cmd[j];
                }
            }
            if (owner && sub == 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) s_dq[slot][j] = cmd[j];
                s_alive[slot] = alive ? 1 : 0;
            }
        }
        __syncthreads();
        t += fp.dt;
        if (q_at != nullptr) q_at += step_rows * N;
        if (f_at != nullptr) f_at += step_rows * M;
        if (noise_at != nullptr) noise_at += step_rows * M;
        if (err_at != nullptr) err_at += step_rows * M;
        if (dq_at != nullptr) dq_at += step_rows * N;
        seen = s_alive[ws] != 0;
        int any_alive = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) any_alive |= s_alive[g];
        if (any_alive == 0) break;                               // the same G words in all 256 threads: a uniform exit
    }

    if (w == 0 && owner) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            s_sum[slot][0][sub * R + r] = ise[r];
            s_sum[slot][1][sub * R + r] = iae[r];
            s_sum[slot][2][sub * R + r] = itae[r];
        }
        if (evalid && sub == 0) {
            A.status[etrial] = status;
            A.k_done[etrial] = k_done;
        }
    }
    __syncthreads();
    store_norms_and_pixels<M>(valid && writer && known, lane, npts, trial, s_sum[ws], s_pix[ws], A.stats, A.pixels);
}

inline void launch_baseline_loop(const uvs_filter_params &fp, hipStream_t s, const BaselineLoopArgs &A) {
    const LoopLaunch at = loop_launch(A.T);
#define UVS_BASELINE_SHAPE(M, N, L)                                                                                                      \
    if (at.small) hipLaunchKernelGGL((UVS_BASELINE_LOOP_KERNEL<M, N, L, 1>), dim3(at.blocks), dim3(kLoopThreads), 0, s, A);               \
    else hipLaunchKernelGGL((UVS_BASELINE_LOOP_KERNEL<M, N, L, kLoopTrials>), dim3(at.blocks), dim3(kLoopThreads), 0, s, A);
    if (fp.m == 8) { UVS_BASELINE_SHAPE(8, 6, 4) }               // the lane counts of the estimators' step and loop kernels
    else if (fp.m == 6) { UVS_BASELINE_SHAPE(6, 6, 2) }
    else { UVS_BASELINE_SHAPE(2, 6, 1) }
#undef UVS_BASELINE_SHAPE
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
    if (fp->n != kJoints || (fp->m != 8 && fp->m != 6 && fp->m != 2)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return UVS_OK;
}

// What the entry points ask of the believed operand; before the first HIP call.
inline int check_believed(const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, int64_t T) {
    if (believed == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL believed");
    if (n_believed < 1 || n_believed > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "n_believed must be 1 .. 2^31 - 1");
    if (believed_index == nullptr && n_believed != 1 && n_believed != T)
        return fail(UVS_ERR_ARG, "%s", "without believed_index, n_believed must be 1 or T");
    return UVS_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the one host path
// Every operand a baseline loop can take.  An entry point fills the ones it has from its parameters; the others stay NULL / 0 and are not
// read at its unit's flavour.  `cam` belongs to the flavours below kBaselineWithScenes, (cams, n_cams, cam_index) to those from it on.
struct BaselineRequest {
    const uvs_filter_params *fp;
    const uvs_camera *cam;
    const uvs_camera *cams;
    int64_t n_cams;
    const int32_t *cam_index;
    const uvs_target_motion *motion;
    const int32_t *latency, *assumed, *predict;
    int64_t T;
    const uvs_camera *believed;
    int64_t n_believed;
    const int32_t *believed_index;
    const double *q_start, *noise;
    double *q_log, *f_log, *dq_log, *err_log;
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
    void *stream;
};

// The unit's argument block from the request, member by name; a template so that a branch for a member the block does not have is discarded.
// `cam`: the camera of the launch, or from kBaselineWithScenes on its shape alone.  static, like run_baseline_loop below: the body reads the
// unit's own constants.
template <class Args>
static void fill_baseline_args(Args &A, const BaselineRequest &r, const uvs_camera &cam) {
    A.fp = *r.fp; A.cam = cam; A.T = r.T;
    A.q_start = r.q_start; A.noise = r.noise;
    A.q_log = r.q_log; A.f_log = r.f_log; A.dq_log = r.dq_log; A.err_log = r.err_log;
    A.status = r.status; A.k_done = r.k_done; A.stats = r.stats; A.pixels = r.pixels;
    if constexpr (kCameraBelieved) { A.B.models = r.believed; A.B.n = r.n_believed; A.B.index = r.believed_index; }
    if constexpr (kBaselineScenes) { A.S.models = r.cams; A.S.n = r.n_cams; A.S.index = r.cam_index; }
    if constexpr (kBaselineMoving) A.motion = r.motion;          // NULL is legal: nothing moves
    if constexpr (kBaselineDelayed) A.latency = r.latency;       // NULL is legal: no latency
    if constexpr (kBaselineAligned) A.assumed = r.assumed;       // NULL is legal: the law is not told
    if constexpr (kBaselinePredicted) A.predict = r.predict;     // NULL is legal: no prediction
}

// What every baseline loop entry point does, at the unit's flavour: the refusals that apply there, in the order the entry points always made
// them -- q_start, then the outputs, then fp -- and before the first HIP call; T == 0 is a call that does nothing; the argument block; the
// launch.  The flavours that take scenes derive the shape from fp, as the estimator loops' do.
// static: the body differs from unit to unit under one signature, so it must not be merged across the library's units at link time.
static int run_baseline_loop(const BaselineRequest &r) {
    g_err[0] = '\0';
    if (r.q_start == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start");
    if (r.status == nullptr || r.k_done == nullptr || r.stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    uvs_camera shape;
    const uvs_camera *cam = r.cam;
    if constexpr (kBaselineScenes) {
        if (r.fp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp");
        shape = scene_shape(r.fp->n, r.fp->m / 2);               // the shape is fp's: no struct's own n_joints / n_points is read
        cam = &shape;
    }
    if (const int rc = check_analytical(r.fp, cam, r.T)) return rc;
    if (r.fp->steps < 1) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1");
    if constexpr (kCameraBelieved) {
        if (const int rc = check_believed(r.believed, r.n_believed, r.believed_index, r.T)) return rc;
    }
    if constexpr (kBaselineScenes) {
        if (const int rc = check_scenes(r.cams, r.n_cams, r.cam_index, r.T)) return rc;
    }
    if (r.T == 0) return UVS_OK;
    BaselineLoopArgs A{};
    fill_baseline_args(A, r, *cam);
    launch_baseline_loop(*r.fp, static_cast<hipStream_t>(r.stream), A);
    return launched(UVS_STR(UVS_BASELINE_LOOP_KERNEL) " launch: %s");
}

}  // namespace uvs_vision
