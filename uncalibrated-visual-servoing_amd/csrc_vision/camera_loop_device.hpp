// The pixel closed loop as ONE launch per batch: the one kernel text of the eleven estimator loop units, uvs_camera_loop.hip (camera_loop_kernel,
// one uvs_filter_params for the batch) to uvs_camera_logged.hip.  One text, eleven flavours, chosen per TRANSLATION UNIT as ../csrc does for
// closed_loop_grid_kernel: a unit states ONE integer before it includes this header, #define UVS_CAMERA_FLAVOUR <0 .. 10>, a value of
// CameraFlavour below.  The flavours are a strict chain -- level f is level f - 1 plus one capability -- so every switch of the kernel text is
// a comparison of that level, and the level alone picks the argument block (CameraLoopArgsList) and the kernel's name (UVS_CAMERA_KERNEL_<f>).
// Every unit keeps its kernel's name, argument block, registers, LDS and time per instantiation.  (A shared __device__ body
// behind several __global__ wrappers moved the register allocation there; nothing here is shared at run time.)
// The host side is shared too: every entry point fills a LoopRequest from its parameters and calls run_camera_loop (at the end of this
// header), which refuses, fills the unit's argument block member by name and launches.
// The estimator is the one of libuvs_rmckf.so, read from its device header (Rows::update, control_law, bandwidth, bandwidth_of); the sensor
// side is camera_sensor_device.hpp: inlined functions over this kernel's LDS rows, which the baseline loop (camera_analytical_device.hpp)
// calls too, together with the mapping's constants and the launch decision.  Both libraries compile with -ffp-contract=off, so every
// value a kernel here forms has the bits the two-launch loop (uvs_camera_features_f64, then uvs_rmckf_step_f64, K times) forms.
//
// Mapping.  A workgroup of 256 threads = four wavefronts is alone on its compute unit (one wavefront per SIMD, so the kernel may take the
// whole register file: the estimator state alone is 108 dwords per lane at (8,6,4)).  It carries G trials:
//   G = 4, batches of more than 256 trials: wavefront w owns trial w of the workgroup on the sensor side;
//   G = 1, batches of up to 256 trials (one per compute unit of an MI355X): the four wavefronts share one trial, each repeats the short
//     projection for itself and detects every fourth feature pair (one colour each), so a step's detection takes a quarter of the time.
//   sensor side, every step: lane i < n advances joint i and takes its sine and cosine, lane p < n_points multiplies the links and projects
//     its disc into LDS, then the 64 lanes walk the (colour, 64-index block) pairs of centre_of_mass in its order -- only the blocks the disc's
//     clipped bounding box touches; every other one has the exact partial +0.0 -- and lane 0 finishes the colour: the features go to LDS and
//     to the log.
//   estimator side, every step: wavefront 0 alone.  Lanes L slot + sub, sub < L, are the L lanes of the workgroup's trial `slot`; the lanes
//     from G L on shadow those (same slot modulo G) so that every cross-lane move has a full wavefront, and store nothing.  State (X, P),
//     previous features, previous command and the error sums stay in registers over all K steps.
// Barriers hand the sines, the discs, the features and the command over.  Every barrier is reached by all 256 threads the same number of
// times: no thread leaves the step loop on its own -- a FAILed trial or a padding trial (which shadows trial T - 1) goes on computing and
// stores nothing -- and the one early exit, "every trial of this workgroup has failed", is read by every thread from the same G LDS words
// after the last barrier of the step, before anything rewrites them.
//
// PTP.  Trial t reads q_start, the noise rows, x0 and f0 of input trial source[t] (n_in of them; the noise row stride is n_in * M) and writes
// every output at t.  On the estimator side lane L slot + sub holds ITS trial's sigma_0, gain, regulariser and fixed-point threshold -- the
// four trials of wavefront 0 belong to different grid cells, so these are per-lane values, never wavefront-uniform -- parked in LDS (G x 4
// doubles a lane reads once per step: MCKF at (8,6,4) has no four register pairs to spare over the step) and its own desired features in
// the register array that held fp's.  A source index outside [0, n_in) never becomes an address: the trial is `void`, computes on input
// trial 0 so that every barrier is still reached, counts as failed for the early exit, and stores status FAIL, k_done = 0 and nothing else.
//
// OCC.  A third flavour: a unit at level kFlavourOccluded (uvs_camera_occluded.hip) sees
// camera_occluded_kernel(OccludedLoopArgs) with PTP and OCC on.  Lane o < 4 of each sensor-side wavefront evaluates rectangle o of its OUTPUT
// trial for step k (occluder_rect; lanes from n_occ on write "covers nothing") into s_occ[w] next to the projection, before the second barrier;
// the detection loop reads the four dwords from there and hands them to disc_counts_in_box<true>, which takes the unoccluded walk for every
// disc no rectangle meets.  A padding or void trial evaluates the rectangles of the trial it shadows.  Barriers and exits are where they were.
//
// HOLD.  A fourth flavour: a unit at level kFlavourHeld (uvs_camera_held.hip) sees
// camera_held_kernel(HeldLoopArgs) with HOLD on too.  A disc whose mask is empty at step k >= 1 keeps the pair reported at step k - 1 for up
// to `hold` steps in a row (plant.hold_features states the rule).  That pair is still in s_f[ws][2 j] when lane 0 of the sensor-side wavefront
// is about to write disc j -- the estimator read it before the last barrier and nothing wrote it since -- so holding is "leave it there and
// log it".  The counters of consecutive misses and of held steps sit in LDS next to s_pix, written by that lane alone (G = 1: wavefront j owns
// colour j).  Barriers and exits are where they were; padding and void trials store nothing, `held` included.
//
// PAINT.  A fifth flavour: a unit at level kFlavourPainted (uvs_camera_painted.hip)
// sees camera_painted_kernel(PaintedLoopArgs) with PAINT on too.  An occluder may be painted a disc's colour: a distractor, whose pixels enter
// that colour's mask.  Lane o < 4, where it evaluates rectangle o into s_occ[w], also leaves the rectangle's paint as byte o of s_paint[w]
// (paint_slot; opaque from n_occ on and for a NULL operand) -- one dword per trial, indexed by OUTPUT trial like the occluders -- and the
// detection loop hands both to detect_pair<true, true>.  Barriers and exits are where they were.
//
// SCENES.  A sixth flavour: a unit at level kFlavourScenes (uvs_camera_scenes.hip) sees
// camera_scene_kernel(ScenesLoopArgs) with SCENES on too.  The camera that renders a trial's frames is the trial's own: a uvs_camera struct in
// memory, picked by OUTPUT trial through (cams, n_cams, cam_index) as the believed loop picks its models.  The workgroup's G scenes are staged
// once, before the step loop, into s_cam[G] (472 B each, by all 256 threads; one barrier of its own, before the first step, because the first
// reader -- the sines -- comes before the step's first barrier), and joint_sincos_rows and project_lane_disc read s_cam[ws] where the other
// flavours read the kernel argument.  A.cam holds the launch's shape alone (n_joints, n_points, from fp) and is word 0 of every staged
// struct.  A padding trial stages the scene of the trial it shadows; a trial whose index names no scene stages zeros and is `void` exactly as
// one whose source index names no input trial is: FAILed by its flag, not by what the zeros give.  The step's barriers and exits are where they were.
//
// MOVING.  A seventh flavour: a unit at level kFlavourMoving (uvs_camera_moving.hip) sees
// moving_target_kernel(MovingLoopArgs) with MOVING on too.  The discs of a trial move: a uvs_target_motion per OUTPUT trial (velocities and one
// window), staged once into s_mot[G] (104 B each) next to the scenes -- the barrier that covers those covers these -- and read by lanes
// < n_points alone, where project_lane_disc_at forms the moved point in transient registers; nothing is written back to s_cam, which the four
// wavefronts of the one-trial form share.  A padding trial stages the motion of the trial it shadows; a NULL operand stages zeros: nothing
// moves.  The step's barriers and exits are where they were.
//
// DELAYED.  An eighth flavour: a unit at level kFlavourDelayed (uvs_camera_delayed.hip) sees
// delayed_frames_kernel(DelayedLoopArgs) with DELAYED on too.  The detector is handed the frame of step max(k - d, 0), d the OUTPUT trial's latency,
// read once before the step loop (a padding wavefront: that of the trial it shadows).  Frames are not kept: the DETECTION of every step goes
// through s_ring[trial slot][disc][k mod 9] (delay_line, vision_device.hpp), written and read by lane 0 of the wavefront that finished
// detect_pair for that disc -- in the one-trial form each disc still belongs to exactly one wavefront -- between detect_pair and noisy_centre.
// Occluders, paints and motion are evaluated at step k as before; the ring carries their effect.  No barrier and no exit is added.
//
// ALIGNED.  A ninth flavour: a unit at level kFlavourAligned (uvs_camera_aligned.hip) sees
// aligned_frames_kernel(AlignedLoopArgs) with ALIGNED on too.  The controller is told a latency: each OUTPUT trial has an ASSUMED latency a (the
// rule: plant.aligned_regressor_step), read once before the step loop by the estimator-side lanes for their etrial (lanes beyond G L and a
// padding slot: that of the trial they shadow).  The estimator's regressor at step k is the command of step k - 1 - a, or zeros before there
// was one; the command integrated into the joints stays dq_{k-1}.  Wavefront 0 keeps the last nine commands per trial slot in
// s_cmd[slot][k mod 9][N], written by the trial's sub == 0 lane next to the s_dq store and read by the trial's L lanes (and their shadows)
// before the update: the end-of-step barrier stands between a write and every later read, and for a == 8 the slot read at step k is the one
// written at step k, after the read in the one wavefront's program order.  The regressor is formed anew in every step, so dq[N] is not
// live across the step here.  The rings start as zeros (all 256 threads, before the barrier that precedes step 0): for k - 1 - a < 0 the slot
// (k - 1 - a + 9) mod 9 >= k has not been written yet, so "the zero vector" is a plain read and needs no select.  The six freshly read
// doubles cost the register allocation 12 to 15 registers against the delayed twin, whose regressor is last step's cmd left where it was
// -- MCKF at (8,6), four trials per workgroup, spilled 36 B -- so this flavour keeps the error sums where they end up, in this lane's own
// words of s_sum, updated by the same three operations per step: 3 R doubles fewer per lane, 0 B of scratch in all 22.  No barrier and no
// exit is added.
//
// PREDICTED.  A tenth flavour: a unit at level kFlavourPredicted (uvs_camera_predicted.hip)
// sees predicted_frames_kernel(PredictedLoopArgs) with PREDICTED on too.  The control law no longer servoes on a stale row: each OUTPUT trial has a
// prediction HORIZON p (the rule: plant.prediction_steps; uvs_vision.h, FEATURE PREDICTION), read once before the step loop by the lanes
// that read `assumed`, and after the update the error is err_r = (f_r + sum_j X_k[r][j] s[j]) - desired_r, s = cmd_{k-1} + ... + cmd_{k-p}
// summed newest first from s = 0, a step before 0 being the zero vector -- the Smith form: X absorbs t_s, so X s is what the commands issued
// since the frame shown must have done to the features.  The dot product is the unit's own form, acc = fma(X[r][j], s[j], acc) from acc = 0
// with j ascending (Rows::update's); f + acc is one rounded add.  z, f_prev, kappa, the f log, the regressor and the joints are untouched.
// The trial's sub == 0 lane forms s for step k + 1 right after it writes cmd into slot k mod 9 of the command ring -- a step before 0 is a slot
// not written yet, zeros, so no select -- and leaves it in s_pred[slot][N]; the end-of-step barrier stands between that store and the reads
// of step k + 1, which take one word per fma: no lane holds s in registers across the update.  The reported row is read again from s_f
// after the update for the same reason.  No barrier and no exit is added.
//
// LOGGED.  An eleventh flavour: a unit at level kFlavourLogged (uvs_camera_logged.hip) sees
// logged_frames_kernel(LoggedLoopArgs) with LOGGED on too: the highest level.  The estimate itself is a log: x_log [K][T][M N], row k = X_k, the matrix AFTER step k's
// update -- the one step k's law and prediction read -- element i N + j = X[i][j], the layout of x0.  Each owner lane of wavefront 0 stores the
// R rows it holds, R N contiguous doubles, next to the step's dq row and under the condition of the err, kappa and dq rows (alive && estore:
// rows k < k_done of valid trials that are not void); shadow lanes and padding slots store nothing.  One cursor, x_at, advances with err_at;
// nothing else is carried across the step.  The R N stores are written as one 8-byte vector store each, in inline assembly, ON PURPOSE: as
// plain assignments the compiler merges them into 16-byte stores, which need the rows in aligned register quadruples, and MCKF at (8,6,4)
// -- 509 of 512 registers in the predicted flavour -- then spills 156 to 192 B per lane (and 60 B at (2,6,1)); unmerged, all 22 have 0 B.
// No barrier, no exit and no LDS is added.  x_log == NULL: the predicted kernel's bits in every output.
#ifndef UVS_CAMERA_LOOP_DEVICE_HPP
#define UVS_CAMERA_LOOP_DEVICE_HPP

#include "camera_sensor_device.hpp"

namespace uvs_vision {

struct LoopArgs {
    uvs_filter_params fp;
    uvs_camera cam;
    long long T;
    const double *q_start, *noise, *x0, *f0;
    double *q_log, *f_log, *dq_log, *err_log, *kappa_log;        // [K][T][comp], each or NULL
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels;
};
// uvs_camera_closed_loop_grid_f64: the per-trial block rides in a derived argument block that only camera_grid_kernel takes
struct GridLoopArgs : LoopArgs {
    uvs_camera_trial_params tp;
};

// uvs_camera_closed_loop_occluded_f64: the per-trial block and the occluders, [T][n_occ] by output trial; only camera_occluded_kernel takes it
struct OccludedLoopArgs : GridLoopArgs {
    const uvs_occluder *occ;
    int32_t n_occ;
};

// uvs_camera_closed_loop_held_f64: the occluded block, the longest hold and the held-step counts; only camera_held_kernel takes it
struct HeldLoopArgs : OccludedLoopArgs {
    int32_t hold;
    int32_t *held;                                               // [T][n_points] or NULL
};

// uvs_camera_closed_loop_painted_f64: the held block and the occluders' paints, [T][n_occ] by output trial or NULL; only camera_painted_kernel takes it
struct PaintedLoopArgs : HeldLoopArgs {
    const int32_t *paint;
};

// uvs_camera_closed_loop_scenes_f64: the painted block (whose `cam` is then the shape alone) and the scenes; only camera_scene_kernel takes it
struct ScenesLoopArgs : PaintedLoopArgs {
    Scenes S;
};

// uvs_camera_closed_loop_moving_f64: the scenes block and the motions, [T] by output trial or NULL; only moving_target_kernel takes it
struct MovingLoopArgs : ScenesLoopArgs {
    const uvs_target_motion *motion;
};

// uvs_camera_closed_loop_delayed_f64: the moving block and the latencies, [T] by output trial or NULL; only delayed_frames_kernel takes it
struct DelayedLoopArgs : MovingLoopArgs {
    const int32_t *latency;
};

// uvs_camera_closed_loop_aligned_f64: the delayed block and the assumed latencies, [T] by output trial or NULL; only aligned_frames_kernel takes it
struct AlignedLoopArgs : DelayedLoopArgs {
    const int32_t *assumed;
};

// uvs_camera_closed_loop_predicted_f64: the aligned block and the prediction horizons, [T] by output trial or NULL; only predicted_frames_kernel takes it
struct PredictedLoopArgs : AlignedLoopArgs {
    const int32_t *predict;
};

// uvs_camera_closed_loop_logged_f64: the predicted block and the log of the estimate, [K][T][M N] or NULL; only logged_frames_kernel takes it
struct LoggedLoopArgs : PredictedLoopArgs {
    double *x_log;
};

// The unit's flavour: the value it gave UVS_CAMERA_FLAVOUR.  Row f of the three tables below -- level, argument block, kernel name -- is one flavour.
enum CameraFlavour {
    kFlavourUniform, kFlavourPerTrial, kFlavourOccluded, kFlavourHeld, kFlavourPainted, kFlavourScenes, kFlavourMoving, kFlavourDelayed,
    kFlavourAligned, kFlavourPredicted, kFlavourLogged
};
using CameraLoopArgsList = std::tuple<LoopArgs, GridLoopArgs, OccludedLoopArgs, HeldLoopArgs, PaintedLoopArgs, ScenesLoopArgs, MovingLoopArgs,
                                      DelayedLoopArgs, AlignedLoopArgs, PredictedLoopArgs, LoggedLoopArgs>;
#define UVS_CAMERA_KERNEL_0 camera_loop_kernel
#define UVS_CAMERA_KERNEL_1 camera_grid_kernel
#define UVS_CAMERA_KERNEL_2 camera_occluded_kernel
#define UVS_CAMERA_KERNEL_3 camera_held_kernel
#define UVS_CAMERA_KERNEL_4 camera_painted_kernel
#define UVS_CAMERA_KERNEL_5 camera_scene_kernel
#define UVS_CAMERA_KERNEL_6 moving_target_kernel
#define UVS_CAMERA_KERNEL_7 delayed_frames_kernel
#define UVS_CAMERA_KERNEL_8 aligned_frames_kernel
#define UVS_CAMERA_KERNEL_9 predicted_frames_kernel
#define UVS_CAMERA_KERNEL_10 logged_frames_kernel

#ifndef UVS_CAMERA_FLAVOUR
#error "state the unit's flavour before including this header: #define UVS_CAMERA_FLAVOUR <0 .. 10>, a value of CameraFlavour"
#endif
constexpr int kCameraFlavour = UVS_CAMERA_FLAVOUR;
static_assert(kCameraFlavour >= kFlavourUniform && kCameraFlavour <= kFlavourLogged, "UVS_CAMERA_FLAVOUR is a value of CameraFlavour");
constexpr bool kCameraPerTrial = kCameraFlavour >= kFlavourPerTrial, kCameraOccluded = kCameraFlavour >= kFlavourOccluded;
constexpr bool kCameraHeld = kCameraFlavour >= kFlavourHeld, kCameraPainted = kCameraFlavour >= kFlavourPainted;
constexpr bool kCameraScenes = kCameraFlavour >= kFlavourScenes, kCameraMoving = kCameraFlavour >= kFlavourMoving;
constexpr bool kCameraDelayed = kCameraFlavour >= kFlavourDelayed, kCameraAligned = kCameraFlavour >= kFlavourAligned;
constexpr bool kCameraPredicted = kCameraFlavour >= kFlavourPredicted, kCameraLogged = kCameraFlavour >= kFlavourLogged;
using CameraLoopKernelArgs = std::tuple_element_t<kCameraFlavour, CameraLoopArgsList>;
#define UVS_CAMERA_LOOP_KERNEL UVS_PASTE(UVS_CAMERA_KERNEL_, UVS_CAMERA_FLAVOUR)

__device__ __forceinline__ const uvs_camera_trial_params *trial_params_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const uvs_camera_trial_params *trial_params_of(const GridLoopArgs &a) { return &a.tp; }
// the occluders of output trial `trial` and their number (never called on the other two blocks: OCC is off there)
__device__ __forceinline__ const uvs_occluder *occluders_of(const LoopArgs &, long long, int &n_occ) { n_occ = 0; return nullptr; }
__device__ __forceinline__ const uvs_occluder *occluders_of(const OccludedLoopArgs &a, long long trial, int &n_occ) {
    n_occ = a.n_occ;
    return a.occ + trial * a.n_occ;
}
// the longest hold and where the held-step counts go (never called on the other three blocks: HOLD is off there)
__device__ __forceinline__ int hold_of(const LoopArgs &, int32_t *&held) { held = nullptr; return 0; }
__device__ __forceinline__ int hold_of(const HeldLoopArgs &a, int32_t *&held) { held = a.held; return a.hold; }
// the paints of the launch, or NULL (never called on the other four blocks: PAINT is off there)
__device__ __forceinline__ const int32_t *paints_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const int32_t *paints_of(const PaintedLoopArgs &a) { return a.paint; }
// the scenes of the launch (never called on the other five blocks: SCENES is off there)
__device__ __forceinline__ Scenes scenes_of(const LoopArgs &) { return Scenes{nullptr, 0, nullptr}; }
__device__ __forceinline__ Scenes scenes_of(const ScenesLoopArgs &a) { return a.S; }
// the motions of the launch, or NULL (never called on the other six blocks: MOVING is off there)
__device__ __forceinline__ const uvs_target_motion *motions_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const uvs_target_motion *motions_of(const MovingLoopArgs &a) { return a.motion; }
// the latencies of the launch, or NULL (never called on the first seven blocks: DELAYED is off there)
__device__ __forceinline__ const int32_t *latencies_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const int32_t *latencies_of(const DelayedLoopArgs &a) { return a.latency; }
// the assumed latencies of the launch, or NULL (never called on the first eight blocks: ALIGNED is off there)
__device__ __forceinline__ const int32_t *assumed_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const int32_t *assumed_of(const AlignedLoopArgs &a) { return a.assumed; }
// the prediction horizons of the launch, or NULL (never called on the first nine blocks: PREDICTED is off there)
__device__ __forceinline__ const int32_t *horizons_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ const int32_t *horizons_of(const PredictedLoopArgs &a) { return a.predict; }
// the log of the estimate, or NULL (never called on the first ten blocks: LOGGED is off there)
__device__ __forceinline__ double *x_log_of(const LoopArgs &) { return nullptr; }
__device__ __forceinline__ double *x_log_of(const LoggedLoopArgs &a) { return a.x_log; }

template <int M, int N, int L, int METHOD_T, int G>
__global__ __launch_bounds__(kLoopThreads) void UVS_CAMERA_LOOP_KERNEL(const CameraLoopKernelArgs A) {
    constexpr bool PTP = kCameraPerTrial, OCC = kCameraOccluded, HOLD = kCameraHeld, PAINT = kCameraPainted, SCENES = kCameraScenes;
    constexpr bool MOVING = kCameraMoving, DELAYED = kCameraDelayed, ALIGNED = kCameraAligned, PREDICTED = kCameraPredicted;
    constexpr bool LOGGED = kCameraLogged;
    constexpr int R = M / L, W = kLoopThreads / 64;
    static_assert((G == 1 || G == W) && W == kColours && G * L <= 64 && N <= UVS_CAMERA_MAX_JOINTS && M <= 2 * kColours, "one or four trials per workgroup");
    __shared__ double s_sin[W][UVS_CAMERA_MAX_JOINTS], s_cos[W][UVS_CAMERA_MAX_JOINTS];   // per wavefront (G = 1: four copies of one trial's)
    __shared__ double s_disc[W][kColours * 3];
    __shared__ double s_f[G][M];                                 // this step's features, sensor side -> estimator side
    __shared__ double s_dq[G][N];                                // this step's command, estimator side -> sensor side
    __shared__ int s_alive[G];                                   // trial has not FAILed, as of the end of this step
    __shared__ int s_pix[G][kColours];                           // smallest mask so far
    __shared__ double s_sum[G][3][M];                            // per-feature ISE, IAE, ITAE after the loop
    // Three rows per lane, (6,6,2): X, P and the careful solve's two n x n matrices do not fit 512 registers together.  The control law reads X
    // alone, so wavefront 0 parks P in LDS around it (plane [entry][lane]: consecutive lanes, consecutive banks).
    constexpr bool PARK = R * uvs::Sym<N>::NP > 42;
    __shared__ double s_park[PARK ? R * uvs::Sym<N>::NP : 1][PARK ? 64 : 1];
    __shared__ double s_tp[PTP ? G : 1][4];                      // PTP: the trial's kernel_bw, gain, reg, fpi_threshold
    __shared__ uint32_t s_occ[OCC ? W : 1][kOccluders];          // OCC: this step's rectangles of the wavefront's trial (occluder_rect's packing)
    __shared__ uint32_t s_paint[PAINT ? W : 1];                  // PAINT: the paints of those rectangles, a byte each (paint_slot)
    __shared__ int s_miss[HOLD ? G : 1][kColours];               // HOLD: steps in a row, up to this one, at which the disc's pair was held
    __shared__ int s_held[HOLD ? G : 1][kColours];               // HOLD: steps at which it was held, while the trial's rows were due
    __shared__ uvs_camera s_cam[SCENES ? G : 1];                 // SCENES: the cameras that render the workgroup's trials, staged once below
    __shared__ uvs_target_motion s_mot[MOVING ? G : 1];          // MOVING: the motions of those trials, staged next to them
    __shared__ DelayCell s_ring[DELAYED ? G : 1][DELAYED ? kColours : 1][DELAYED ? kDelaySlots : 1];   // DELAYED: the last nine detections of every disc
    __shared__ double s_cmd[ALIGNED ? G : 1][ALIGNED ? kDelaySlots : 1][ALIGNED ? N : 1];   // ALIGNED: the last nine commands of every trial
    __shared__ double s_pred[PREDICTED ? G : 1][PREDICTED ? N : 1];   // PREDICTED: s of this step, the sum of the trial's last p commands

    const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const uvs_filter_params &fp = A.fp;
    const uvs_camera &cam = A.cam;
    const long long T = A.T;
    const int K = fp.steps, npts = cam.n_points;

    // sensor side: this wavefront's trial, and the feature pairs it detects: all of its own trial's, or every fourth of the workgroup's one trial
    const int ws = G == 1 ? 0 : w;
    const uvs_camera &scene = SCENES ? s_cam[ws] : cam;          // the camera that renders this trial's frames
    const bool writer = G == W || w == 0;                        // G = 1: the four wavefronts hold the same joints; the first one logs them
    const int j_first = G == 1 ? w : 0, j_step = G == 1 ? W : 1;
    long long trial = static_cast<long long>(blockIdx.x) * G + ws;
    bool valid = trial < T;
    if (!valid) trial = T - 1;                                   // a padding wavefront shadows the last trial and stores nothing
    long long src = trial;                                       // the input trial: q_start and the noise rows come from there
    long long in_rows = T;                                       // trials per noise row
    if constexpr (PTP) {
        const uvs_camera_trial_params &tp = *trial_params_of(A);
        if (tp.source != nullptr) {
            src = tp.source[trial];
            in_rows = tp.n_in;
            if (src < 0 || src >= in_rows) {                     // names no input trial: void.  Never an address; nothing of it is stored
                src = 0;
                valid = false;
            }
        }
    }
    if constexpr (SCENES) {                                      // the scene of the OUTPUT trial (a padding wavefront: of the one it shadows)
        stage_scenes<G, kLoopThreads>(scenes_of(A), cam, static_cast<long long>(blockIdx.x) * G, T, s_cam);
        if (model_of(scenes_of(A), trial) < 0) valid = false;    // names no scene: void.  Never an address; nothing of it is stored
    }
    if constexpr (MOVING) stage_motions<G, kLoopThreads>(motions_of(A), static_cast<long long>(blockIdx.x) * G, T, s_mot);   // by OUTPUT trial too
    int delay = 0;                                               // DELAYED: the latency of the OUTPUT trial (a padding wavefront: of the one it shadows)
    if constexpr (DELAYED) delay = latency_of(latencies_of(A), trial);
    const uvs_occluder *occ_at = nullptr;                        // OCC: the occluders of the OUTPUT trial (a padding wavefront: of the one it shadows)
    int n_occ = 0;
    if constexpr (OCC) occ_at = occluders_of(A, trial, n_occ);
    double q = lane < N ? A.q_start[src * N + lane] : 0.0;
    // Row k of a [K][T][comp] log is step_rows * comp doubles past row k - 1.  The cursors below are this lane's own addresses in row 0 (NULL for
    // a log that is not wanted, or where this lane has nothing to store), kept in vector registers: fifteen pointers as scalars did not fit.
    const long long step_rows = T;
    double *q_at = (valid && writer && lane < N && A.q_log != nullptr) ? A.q_log + trial * N + lane : nullptr;
    double *f_at = (valid && lane == 0 && A.f_log != nullptr) ? A.f_log + trial * M : nullptr;
    const double *noise_at = A.noise != nullptr ? A.noise + src * M : nullptr;
    bool seen = true;                                            // this trial has not FAILed before this step: its rows q[k], f[k] are due
    if (lane < kColours) s_pix[ws][lane] = INT_MAX;
    int hold = 0;
    int32_t *held_out = nullptr;
    if constexpr (HOLD) {
        hold = hold_of(A, held_out);
        if (lane < kColours) {
            s_miss[ws][lane] = 0;
            s_held[ws][lane] = 0;
        }
    }

    // estimator side (wavefront 0): this lane's trial and rows
    const int slot = (lane / L) & (G - 1), sub = lane % L;
    long long etrial = static_cast<long long>(blockIdx.x) * G + slot;
    const bool owner = lane < G * L;                             // the lanes beyond shadow these
    bool evalid = owner && etrial < T;
    if (etrial >= T) etrial = T - 1;
    long long esrc = etrial;                                     // the input trial: x0 and f0 come from there
    bool evoid = false;
    if constexpr (PTP) {
        const uvs_camera_trial_params &tp = *trial_params_of(A);
        if (tp.source != nullptr) {
            esrc = tp.source[etrial];
            if (esrc < 0 || esrc >= tp.n_in) {
                esrc = 0;
                evoid = true;
            }
        }
        if (w == 0 && owner && sub == 0) {                       // read back by this lane and its trial's other lanes after the first barrier
            s_tp[slot][0] = tp.kernel_bw != nullptr ? tp.kernel_bw[etrial] : fp.kernel_bw;
            s_tp[slot][1] = tp.gain != nullptr ? tp.gain[etrial] : fp.gain;
            s_tp[slot][2] = tp.reg != nullptr ? tp.reg[etrial] : fp.reg;
            s_tp[slot][3] = tp.fpi_threshold != nullptr ? tp.fpi_threshold[etrial] : fp.fpi_threshold;
        }
    }
    if constexpr (SCENES) {
        if (model_of(scenes_of(A), etrial) < 0) evoid = true;
    }
    const bool estore = evalid && !evoid;                        // this lane's trial has rows to log
    double *err_at = (estore && A.err_log != nullptr) ? A.err_log + etrial * M + sub * R : nullptr;
    double *kappa_at = (estore && A.kappa_log != nullptr) ? A.kappa_log + etrial * M + sub * R : nullptr;
    double *dq_at = (estore && sub == 0 && A.dq_log != nullptr) ? A.dq_log + etrial * N : nullptr;
    double *x_at = nullptr;                                      // LOGGED: this lane's R rows of X in row 0 of the log
    if constexpr (LOGGED) x_at = (estore && x_log_of(A) != nullptr) ? x_log_of(A) + (etrial * M + sub * R) * N : nullptr;
    int assumed = 0;                                             // ALIGNED: the assumed latency of this lane's trial (a shadow lane: of the one it shadows)
    if constexpr (ALIGNED) {
        if (w == 0) assumed = latency_of(assumed_of(A), etrial);
        // the rings start as zeros: "no such step" is then a slot that has not been written.  The step's first barrier is before the first read.
        for (int i = threadIdx.x; i < G * kDelaySlots * N; i += kLoopThreads) (&s_cmd[0][0][0])[i] = 0;
    }
    int horizon = 0;                                             // PREDICTED: the prediction horizon of this lane's trial (a shadow lane: of the one it shadows)
    if constexpr (PREDICTED) {
        if (w == 0) horizon = latency_of(horizons_of(A), etrial);
        for (int i = threadIdx.x; i < G * N; i += kLoopThreads) (&s_pred[0][0])[i] = 0;   // step 0: no command has been issued
    }
    uvs::Rows<M, N, L> st;
    st.init_cov();
    double f_prev[R], des[R], dq[N], ise[R], iae[R], itae[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = sub * R + r;
        des[r] = fp.desired[row];
        if constexpr (PTP) {
            const double *tp_des = trial_params_of(A)->desired;
            if (tp_des != nullptr) des[r] = tp_des[etrial * M + row];
        }
        f_prev[r] = A.f0[esrc * M + row];
        ise[r] = iae[r] = itae[r] = 0.0;
        if constexpr (ALIGNED) {                                 // the sums are kept where they end up, s_sum: the ring's reads take their registers
            if (w == 0 && owner) s_sum[slot][0][row] = s_sum[slot][1][row] = s_sum[slot][2][row] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) st.x[r][j] = A.x0[(esrc * M + row) * N + j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) dq[j] = 0.0;                     // first step: H = 0 (experiment.py:183)
    double t = 0.0 + fp.dt;                                      // engine._loop_times: t_s accumulated in floating point
    int status = UVS_STATUS_SUCCESS, k_done = K;
    bool alive = true;
    const bool strict = (fp.reserved & UVS_OPT_STRICT_PINV) != 0;
    uvs_filter_params fp_trial;                                  // PTP: the launch's block with the trial's own reg and fpi_threshold, per lane
    if constexpr (PTP) fp_trial = A.fp;
    const uvs_filter_params &fpe = PTP ? fp_trial : A.fp;        // what the estimator update reads
    if constexpr (SCENES) __syncthreads();                       // the staged scenes: step 0's sines read them before the step's first barrier

    for (int k = 0; k < K; ++k) {
        // ---- the sensor side of the step (camera_sensor_device.hpp): joints, projection, detection
        if (lane < N) {
            advance_joint(lane, k, s_dq[ws], fp.dt, q);
            joint_sincos_rows(scene, lane, q, s_sin[w], s_cos[w]);
            if (seen && q_at != nullptr) *q_at = q;              // after the sines: where this text measured fastest
        }
        __syncthreads();
        if constexpr (MOVING) {                                  // the disc where step k of the trial's motion has taken it
            if (lane < npts) project_lane_disc_at(scene, lane, s_mot[ws], k, s_sin[w], s_cos[w], s_disc[w]);
        } else {
            if (lane < npts) project_lane_disc(scene, lane, s_sin[w], s_cos[w], s_disc[w]);
        }
        if constexpr (OCC) {                                     // lane o: rectangle o of this step, next to the projection
            if (lane < kOccluders) s_occ[w][lane] = lane < n_occ ? occluder_rect(occ_at[lane], k) : kNoRect;
        }
        if constexpr (PAINT) {                                   // and its paint: byte o of the trial's dword
            if (lane < kOccluders) {
                const int32_t *paint = paints_of(A);
                const bool given = paint != nullptr && lane < n_occ;
                reinterpret_cast<uint8_t *>(&s_paint[w])[lane] = static_cast<uint8_t>(given ? paint_slot(paint[trial * n_occ + lane], npts) : kOpaque);
            }
        }
        __syncthreads();
        Rects rects;                                             // OCC off: never read
        if constexpr (OCC) {
#pragma unroll
            for (int o = 0; o < kOccluders; ++o) rects.r[o] = s_occ[w][o];
        }
        uint32_t paints = kNoPaints;                             // PAINT off: never read
        if constexpr (PAINT) paints = s_paint[w];
#pragma unroll 1
        for (int j = j_first; j < npts; j += j_step) {
            ColourSum sum = detect_pair<OCC, PAINT>(s_disc[w], npts, j, lane, rects, paints);
            if (lane == 0) {                                     // the lane the shuffle tree ends in
                if constexpr (DELAYED) delay_line(s_ring[ws][j], sum, k, delay);   // in place: the detection of step max(k - delay, 0)
                double u, v;
                noisy_centre(sum, noise_at, j, u, v);
                if constexpr (HOLD) {                            // the integer count decides, never the pair
                    if (sum.count != 0) {
                        s_miss[ws][j] = 0;
                    } else if (k >= 1 && s_miss[ws][j] < hold) { // lost, and the hold is not used up: step k - 1's reported pair, no noise of step k
                        u = s_f[ws][2 * j];
                        v = s_f[ws][2 * j + 1];
                        s_miss[ws][j] += 1;
                        if (seen) s_held[ws][j] += 1;
                    }                                            // lost otherwise: the NaN pair, which FAILs the trial at this step
                }
                report_pair(sum.count, j, u, v, seen, s_f[ws], s_pix[ws], f_at);
            }
        }
        __syncthreads();
        // ---- estimator and control law of the workgroup's four trials (step_kernel's sequence)
        if (w == 0) {
            double z[R], err[R], kap[R], cmd[N];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double fv = s_f[slot][sub * R + r];
                z[r] = fv - f_prev[r];
                f_prev[r] = fv;
                err[r] = fv - des[r];
            }
            double sigma, gain;
            if constexpr (PTP) {                                 // the trial's scalars wait in LDS and are read where a step needs them
                asm volatile("" ::: "memory");
                sigma = uvs::bandwidth_of(fp, s_tp[slot][0], k);
                gain = s_tp[slot][1];
                fp_trial.reg = s_tp[slot][2];
                fp_trial.fpi_threshold = s_tp[slot][3];
            } else {
                sigma = uvs::bandwidth(fp, k);
                gain = fp.gain;
            }
            if constexpr (ALIGNED) {                             // the regressor: the command of step k - 1 - assumed, or zeros where there is none
                const int kr = aligned_regressor_step(k, assumed);  // >= -kDelaySlots.  Negative: slot kr + 9 >= k has not been written: zeros
                const double *told = s_cmd[slot][(kr + kDelaySlots) % kDelaySlots];
#pragma unroll
                for (int j = 0; j < N; ++j) dq[j] = told[j];
            }
            st.template update<METHOD_T>(fpe, z, dq, sigma, kap);   // h = the previous command; zero on k = 0
            const int bad = st.any_nonfinite();
            if (alive && bad) {                                  // FAIL at this step; the trial stops
                alive = false;
                status = UVS_STATUS_FAIL;
                k_done = k;
            }
            if constexpr (PREDICTED) {                           // the law's error: the reported row advanced by X_k s, against the target
                const double *s = s_pred[slot];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < N; ++j) acc = fma(st.x[r][j], s[j], acc);
                    const double predicted = s_f[slot][sub * R + r] + acc;
                    err[r] = predicted - des[r];
                }
            }
            if constexpr (PARK) {
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int e = 0; e < uvs::Sym<N>::NP; ++e) s_park[r * uvs::Sym<N>::NP + e][lane] = st.p[r][e];
                asm volatile("" ::: "memory");                   // the loads below are loads: nothing of P is carried in registers
            }
            const bool suspect = strict || uvs::control_law<M, N, L, false>(st, kap, err, gain, sub, cmd);
            if (__any(suspect)) {                                // the careful solve for a filter whose watch fires, or for every one when strict
                double careful[N];
                uvs::control_law<M, N, L, true>(st, kap, err, gain, sub, careful);
#pragma unroll
                for (int j = 0; j < N; ++j) cmd[j] = suspect ? careful[j] : cmd[j];
            }
            if constexpr (PARK) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int e = 0; e < uvs::Sym<N>::NP; ++e) st.p[r][e] = s_park[r * uvs::Sym<N>::NP + e][lane];
            }
            if (alive && estore) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (err_at != nullptr) err_at[r] = err[r];
                    if (kappa_at != nullptr) kappa_at[r] = kap[r];
                    const double ae = fabs(err[r]);              // stats_kernel's sums, in its order over k
                    if constexpr (ALIGNED) {                     // the same three operations, on this lane's own words of s_sum
                        double *sum = &s_sum[slot][0][sub * R + r];
                        sum[0] = fma(err[r], err[r], sum[0]);
                        sum[M] += ae;
                        sum[2 * M] = fma(t, ae, sum[2 * M]);
                    } else {
                        ise[r] = fma(err[r], err[r], ise[r]);
                        iae[r] += ae;
                        itae[r] = fma(t, ae, itae[r]);
                    }
                }
                if (dq_at != nullptr) {
#pragma unroll
                    for (int j = 0; j < N; ++j) dq_at[j] = cmd[j];
                }
                if constexpr (LOGGED) {                          // X_k, the matrix this step's update left and its law read: the lane's R rows
                    if (x_at != nullptr) {                       // one 8-byte store each, not to be merged (see LOGGED above)
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int j = 0; j < N; ++j) asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(x_at + r * N + j), "v"(st.x[r][j]) : "memory");
                    }
                }
            }
            if constexpr (!ALIGNED) {
#pragma unroll
                for (int j = 0; j < N; ++j) dq[j] = cmd[j];
            }
            if (owner && sub == 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) s_dq[slot][j] = cmd[j];
                if constexpr (ALIGNED) {                         // slot k mod 9 of the trial's ring; the end-of-step barrier comes before every later read
                    double *cell = s_cmd[slot][k % kDelaySlots];
#pragma unroll
                    for (int j = 0; j < N; ++j) cell[j] = cmd[j];
                }
                if constexpr (PREDICTED) {                       // s of step k + 1: cmd_k, cmd_{k-1}, ... newest first; a slot not written yet is zeros
                    double *s = s_pred[slot];
#pragma unroll
                    for (int j = 0; j < N; ++j) s[j] = 0.0;
#pragma unroll 1
                    for (int i = 1; i <= horizon; ++i) {
                        const double *cell = s_cmd[slot][(k + 1 - i + kDelaySlots) % kDelaySlots];
#pragma unroll
                        for (int j = 0; j < N; ++j) s[j] += cell[j];
                    }
                }
                s_alive[slot] = (alive && !evoid) ? 1 : 0;
            }
        }
        __syncthreads();
        t += fp.dt;
        if (q_at != nullptr) q_at += step_rows * N;
        if (f_at != nullptr) f_at += step_rows * M;
        if (noise_at != nullptr) noise_at += in_rows * M;
        if (err_at != nullptr) err_at += step_rows * M;
        if (kappa_at != nullptr) kappa_at += step_rows * M;
        if (dq_at != nullptr) dq_at += step_rows * N;
        if constexpr (LOGGED) {
            if (x_at != nullptr) x_at += step_rows * (M * N);
        }
        seen = s_alive[ws] != 0;
        int any_alive = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) any_alive |= s_alive[g];
        if (any_alive == 0) break;                               // the same G words in all 256 threads: a uniform exit
    }

    if (w == 0 && owner) {
        if constexpr (!ALIGNED) {                                // ALIGNED: they are there already
#pragma unroll
            for (int r = 0; r < R; ++r) {
                s_sum[slot][0][sub * R + r] = ise[r];
                s_sum[slot][1][sub * R + r] = iae[r];
                s_sum[slot][2][sub * R + r] = itae[r];
            }
        }
        if (evalid && sub == 0) {
            A.status[etrial] = evoid ? UVS_STATUS_FAIL : status;
            A.k_done[etrial] = evoid ? 0 : k_done;
        }
    }
    __syncthreads();
    store_norms_and_pixels<M>(valid && writer, lane, npts, trial, s_sum[ws], s_pix[ws], A.stats, A.pixels);
    if constexpr (HOLD) {
        if (lane < npts && valid && writer && held_out != nullptr) held_out[trial * npts + lane] = s_held[ws][lane];
    }
}

// MCKF: the fixed-point iteration's working set next to three rows per lane spills at (6,6,2) (684 B of scratch per lane), so that one
// instantiation is not built in either flavour and the entry points refuse it; at (8,6,4) and (2,6,1) it has none and is built.
template <int M, int N, int L, bool WITH_MCKF>
bool launch_loop(int method, hipStream_t s, const CameraLoopKernelArgs &A) {
    const LoopLaunch at = loop_launch(A.T);
#define UVS_LOOP_METHOD(METHOD)                                                                                                          \
    if (method == METHOD) {                                                                                                              \
        if (at.small) hipLaunchKernelGGL((UVS_CAMERA_LOOP_KERNEL<M, N, L, METHOD, 1>), dim3(at.blocks), dim3(kLoopThreads), 0, s, A);     \
        else hipLaunchKernelGGL((UVS_CAMERA_LOOP_KERNEL<M, N, L, METHOD, kLoopTrials>), dim3(at.blocks), dim3(kLoopThreads), 0, s, A);    \
        return true;                                                                                                                     \
    }
    UVS_LOOP_METHOD(UVS_METHOD_GMCKF)
    UVS_LOOP_METHOD(UVS_METHOD_KF)
    UVS_LOOP_METHOD(UVS_METHOD_IMCCKF)
    if constexpr (WITH_MCKF) {
        UVS_LOOP_METHOD(UVS_METHOD_MCKF)
    }
#undef UVS_LOOP_METHOD
    return false;
}

// The refusals uvs_camera_closed_loop_f64 and uvs_camera_closed_loop_grid_f64 share, in the order the former always made them; UVS_OK = go on.
inline int check_loop_args(const uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start, const double *x0, const double *f0,
                           const int32_t *status, const int32_t *k_done, const double *stats) {
    if (fp == nullptr || cam == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp or cam");
    if (q_start == nullptr || x0 == nullptr || f0 == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL q_start, x0 or f0");
    if (status == nullptr || k_done == nullptr || stats == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL status, k_done or stats");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (fp->steps < 1 || fp->k_max <= 0) return fail(UVS_ERR_ARG, "%s", "steps must be >= 1 and k_max > 0");
    if (cam->n_joints < 1 || cam->n_joints > UVS_CAMERA_MAX_JOINTS) return fail(UVS_ERR_ARG, "%s", "n_joints must be 1 .. 8");
    if (!colours_ok(cam->n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (fp->method != UVS_METHOD_KF && fp->method != UVS_METHOD_MCKF && fp->method != UVS_METHOD_IMCCKF && fp->method != UVS_METHOD_GMCKF)
        return fail(UVS_ERR_METHOD, "%s", "method must be KF, MCKF, IMCCKF or GMCKF (the calibrated baseline's pixel loop is uvs_camera_analytical_loop_f64)");
    if (fp->method == UVS_METHOD_MCKF && fp->fpi_epoch_max < 1) return fail(UVS_ERR_ARG, "%s", "MCKF needs fpi_epoch_max >= 1");
    if (fp->lanes_per_filter != 0) return fail(UVS_ERR_SHAPE, "%s", "lanes_per_filter must be 0: the loop kernel has one mapping per shape");
    if (fp->m != 2 * cam->n_points) return fail(UVS_ERR_SHAPE, "%s", "fp->m must be 2 * cam->n_points");
    if (fp->n != cam->n_joints) return fail(UVS_ERR_SHAPE, "%s", "fp->n must be cam->n_joints");
    if (fp->n != kJoints || (fp->m != 8 && fp->m != 6 && fp->m != 2)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    if (fp->method == UVS_METHOD_MCKF && fp->m == 6) return fail(UVS_ERR_METHOD, "%s", "MCKF is not built at (6, 6): use the two-launch loop");
    return UVS_OK;
}

// the lane counts uvs_rmckf_step_f64 resolves for lanes_per_filter == 0
inline bool launch_loop_shape(const uvs_filter_params &fp, hipStream_t s, const CameraLoopKernelArgs &A) {
    if (fp.m == 8) return launch_loop<8, 6, 4, true>(fp.method, s, A);
    if (fp.m == 6) return launch_loop<6, 6, 2, false>(fp.method, s, A);
    if (fp.m == 2) return launch_loop<2, 6, 1, true>(fp.method, s, A);
    return false;
}

// ---------------------------------------------------------------------------------------------------------------- the one host path
// Every operand an estimator loop can take.  An entry point fills the ones it has from its parameters; the others stay NULL / 0 and are
// not read at its unit's flavour.  `cam` belongs to the flavours below kFlavourScenes, (cams, n_cams, cam_index) to those from it on.
struct LoopRequest {
    const uvs_filter_params *fp;
    const uvs_camera *cam;
    const uvs_camera *cams;
    int64_t n_cams;
    const int32_t *cam_index;
    const uvs_target_motion *motion;
    const int32_t *latency, *assumed, *predict;
    int64_t T;
    const uvs_camera_trial_params *tp;
    const uvs_occluder *occ;
    const int32_t *paint;
    int32_t n_occ, hold;
    const double *q_start, *noise, *x0, *f0;
    double *q_log, *f_log, *dq_log, *err_log, *kappa_log, *x_log;
    int32_t *status, *k_done;
    double *stats;
    int32_t *pixels, *held;
    void *stream;
};

// The unit's argument block from the request, member by name.  A template so that the members are dependent: a branch for a member the
// unit's block does not have is discarded, not compiled.  `cam`: the camera of the launch, or from kFlavourScenes on its shape alone.
// static, like run_camera_loop below: the body reads the unit's own constants.
template <class Args>
static void fill_loop_args(Args &A, const LoopRequest &r, const uvs_camera &cam) {
    A.fp = *r.fp; A.cam = cam; A.T = r.T;
    A.q_start = r.q_start; A.noise = r.noise; A.x0 = r.x0; A.f0 = r.f0;
    A.q_log = r.q_log; A.f_log = r.f_log; A.dq_log = r.dq_log; A.err_log = r.err_log; A.kappa_log = r.kappa_log;
    A.status = r.status; A.k_done = r.k_done; A.stats = r.stats; A.pixels = r.pixels;
    if constexpr (kCameraPerTrial) A.tp = r.tp != nullptr ? *r.tp : uvs_camera_trial_params{};   // NULL tp: every member NULL
    if constexpr (kCameraOccluded) { A.occ = r.occ; A.n_occ = r.n_occ; }
    if constexpr (kCameraHeld) { A.hold = r.hold; A.held = r.held; }
    if constexpr (kCameraPainted) A.paint = r.paint;             // NULL: every rectangle opaque
    if constexpr (kCameraScenes) { A.S.models = r.cams; A.S.n = r.n_cams; A.S.index = r.cam_index; }
    if constexpr (kCameraMoving) A.motion = r.motion;            // NULL is legal: nothing moves
    if constexpr (kCameraDelayed) A.latency = r.latency;         // NULL is legal: no latency
    if constexpr (kCameraAligned) A.assumed = r.assumed;         // NULL is legal: the controller is not told
    if constexpr (kCameraPredicted) A.predict = r.predict;       // NULL is legal: no prediction
    if constexpr (kCameraLogged) A.x_log = r.x_log;              // NULL is legal: no log of X, the predicted namesake bit for bit
}

// What every estimator loop entry point does, at the unit's flavour: the refusals that apply there, in the order the entry points always made
// them and before the first HIP call; T == 0 is a call that does nothing; the argument block; the launch.  Two orders exist: the flavours
// that take a `cam` hand it to check_loop_args, those that take scenes refuse a NULL fp first and derive the shape from fp.
// static: the body differs from unit to unit under one signature, so it must not be merged across the library's units at link time.
static int run_camera_loop(const LoopRequest &r) {
    g_err[0] = '\0';
    uvs_camera shape;
    const uvs_camera *cam = r.cam;
    if constexpr (kCameraScenes) {
        if (r.fp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL fp");
        shape = scene_shape(r.fp->n, r.fp->m / 2);               // the shape is fp's: no struct's own n_joints / n_points is read
        cam = &shape;
    }
    if (const int rc = check_loop_args(r.fp, cam, r.T, r.q_start, r.x0, r.f0, r.status, r.k_done, r.stats)) return rc;
    if constexpr (kCameraFlavour == kFlavourPerTrial) {          // the grid call alone insists on its block; from kFlavourOccluded on NULL is "no block"
        if (r.tp == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL tp (a block whose members are all NULL is the uniform call)");
    }
    if constexpr (kCameraPerTrial) {
        if (r.tp != nullptr && r.tp->source != nullptr && r.tp->n_in < 1)
            return fail(UVS_ERR_ARG, "%s", "source needs n_in >= 1: the trials q_start, noise, x0 and f0 hold");
    }
    if constexpr (kCameraOccluded) {
        if (const int rc = check_occluders(r.occ, r.n_occ)) return rc;
    }
    if constexpr (kCameraHeld) {
        if (r.hold < 0) return fail(UVS_ERR_ARG, "%s", "hold must be >= 0");
    }
    if constexpr (kCameraScenes) {
        if (const int rc = check_scenes(r.cams, r.n_cams, r.cam_index, r.T)) return rc;
    }
    if (r.T == 0) return UVS_OK;
    CameraLoopKernelArgs A{};
    fill_loop_args(A, r, *cam);
    if (!launch_loop_shape(*r.fp, static_cast<hipStream_t>(r.stream), A)) return fail(UVS_ERR_SHAPE, "%s", "(m, n) must be (8, 6), (6, 6) or (2, 6)");
    return launched(UVS_STR(UVS_CAMERA_LOOP_KERNEL) " launch: %s");
}

}  // namespace uvs_vision
#endif  // UVS_CAMERA_LOOP_DEVICE_HPP
