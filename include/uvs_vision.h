/*
 * uvs_vision.h -- C ABI of libuvs_vision.so: the perception front-end of the live route
 * (colour-threshold + centre-of-mass circle detectors) on AMD MI355X (gfx950).
 *
 * The reference detects its circles on the host, one 256x256 RGB frame per loop iteration
 * (utils.py:11-166, called from experiment.py:89 and :129).  This library does the same on the
 * device for a batch of T frames, so that the detector and the estimator step
 * (uvs_rmckf_step_f64 of uvs_rmckf.h) are two launches on one stream with one synchronisation.
 * It is a library of its own: nothing here touches the RMCKF kernels or their fingerprint.
 *
 * Conventions (those of uvs_rmckf.h)
 *   - All data pointers are owned by the caller; nothing is allocated, freed or synchronised
 *     inside the library.  Work is enqueued on the hipStream_t passed as `stream` (void* here;
 *     NULL = default stream).
 *   - Every pointer may name device memory (HBM) or pinned host memory mapped to the device
 *     (hipHostMalloc / a pinned torch tensor): the kernel reads and writes it in place.  No
 *     managed memory, nothing that needs XNACK.
 *   - Returns 0 on success, <0 on error (never throws); uvs_vision_last_error() gives the text
 *     for the calling thread.  Arguments are validated before the first HIP call.
 */
#ifndef UVS_VISION_H
#define UVS_VISION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes: the values of uvs_rmckf.h */
#ifndef UVS_OK
#define UVS_OK 0
#define UVS_ERR_ARG (-1)      /* NULL/ill-formed argument                   */
#define UVS_ERR_SHAPE (-2)    /* frame size other than 256 x 256            */
#define UVS_ERR_HIP (-3)      /* HIP runtime error (see last_error)         */
#endif

#define UVS_VISION_SIDE 256   /* utils.py:7-9: the pixel grid is np.linspace(0, 1, 256), whatever the image */

const char *uvs_vision_version(void);
const char *uvs_vision_last_error(void);

/*
 * Centre-of-mass circle detection of T camera frames: detectGreenCircle (utils.py:11-51),
 * detectRGBCircles (:53-124) and detect4Circles (:126-166) with method CENTER_OF_MASS, and the
 * measurement-noise line of the loop (experiment.py:127-135).
 *   frames [T][256][256][3] uint8 RGB in, frame t at frames + t * frame_stride_bytes, rows dense
 *     (768 B).  The frames are UNFLIPPED, as the vision sensor hands them over: the kernel
 *     applies cv2.flip(image, 0) (utils.py:13) by indexing.  frames must be 16-byte aligned and
 *     frame_stride_bytes a multiple of 16 (rows are read with 16-byte loads), at least
 *     height * width * 3.
 *   n_colours: 1 = green -> f = [u, v]; 3 = red, green, blue; 4 = red, green, blue, pink.
 *   noise [T][2*n_colours] in or NULL: f += noise (experiment.py:133-135), in the same launch.
 *   f_out [T][2*n_colours] out; pixels_out [T][n_colours] int32 out or NULL: the number of
 *     pixels in each colour's mask (exact).
 * Arithmetic.  The masks are thresholded in integers as the reference does (a channel is above
 * at > 250 and below at < 250, utils.py:15-24; 250 itself is neither).  Per colour the kernel
 * counts mask pixels per column and per flipped row in int32 -- independent of any order -- and
 * forms S_u = sum_c colcount[c] * p[c], S_v = sum_r rowcount[r] * p[r] in fp64 with
 * p[i] = fl(g[i] * 255.0), g = np.linspace(0, 1, 256) (g[i] = fl(i * fl(1/255)), g[255] = 1): the
 * products the reference's `X * mask` holds (utils.py:25-27), 24 of which are not integers.
 * u = (255.0 * S_u) / (double)(255 * count), v likewise; an empty mask gives 0.0/0.0 = NaN as
 * the reference does -- no special case and no error.  Against numpy's pairwise sum over the
 * 65 536 products the result differs by under 1e-11 pixel.
 * Errors: UVS_ERR_ARG for NULL frames / f_out, T < 0, n_colours not in {1, 3, 4}, a height or
 * width < 1, a misaligned frames pointer, a stride below height * width * 3 or not a multiple of
 * 16; UVS_ERR_SHAPE for a size other than 256 x 256 (np broadcasting fails on it in the
 * reference).  T == 0 returns UVS_OK and launches nothing.  One workgroup per frame.
 */
int uvs_detect_circles_u8(int64_t T, const uint8_t *frames, int64_t frame_stride_bytes,
                          int32_t height, int32_t width, int32_t n_colours,
                          const double *noise, double *f_out, int32_t *pixels_out,
                          void *stream);

/*
 * The synthetic camera: the sensor side of the same 256 x 256 frames.  A DH arm carries a pinhole camera that looks at up to four
 * coloured discs; the entry points below project the discs, rasterise them into frames the detector above can read, and -- the loop's
 * hot path -- return what the detector would return for those frames without ever writing them.
 *
 * The camera is this library's own description (nothing of uvs_rmckf.h is needed): the DH table as the uvs_plant struct of that header
 * holds it (cos_alpha / sin_alpha computed by the host), the world points, the pinhole, and the physical disc radii in metres.
 * Colour order of the points: red, green, blue, pink; with n_points == 1 the one disc is the green one.
 */
#define UVS_CAMERA_MAX_JOINTS 8
#define UVS_CAMERA_MAX_POINTS 4

typedef struct uvs_camera {
    int32_t n_joints;                               /* 1 .. UVS_CAMERA_MAX_JOINTS */
    int32_t n_points;                               /* 1, 3 or 4 */
    double theta_offset[UVS_CAMERA_MAX_JOINTS];
    double d[UVS_CAMERA_MAX_JOINTS];
    double a[UVS_CAMERA_MAX_JOINTS];
    double cos_alpha[UVS_CAMERA_MAX_JOINTS];
    double sin_alpha[UVS_CAMERA_MAX_JOINTS];
    double points[UVS_CAMERA_MAX_POINTS][3];        /* world coordinates */
    double focal, center;                           /* pixels */
    double radius[UVS_CAMERA_MAX_POINTS];           /* metres */
} uvs_camera;

/*
 * Joint update and disc projection of T trials.
 *   q_prev [T][n_joints] in; dq [T][n_joints] in or NULL.  With dq the joints are q = q_prev + dq * dt (one rounded multiply, then one
 *     rounded add: the loop's new_q = q_now + dq * t_s), without it q = q_prev and dt is ignored.
 *   q_out [T][n_joints] out or NULL: q.  It must not overlap q_prev.
 *   discs_out [T][n_points][3] out: (u, v, r) in pixels of the flipped frame (u right, v down).  The camera pose is the product of the DH
 *     links Rz(theta) Tz(d) Rx(alpha) Tx(a); per point pc = R^T (w - t), u = center + focal * pc0 / pc2, v = center + focal * pc1 / pc2,
 *     r = focal * radius / pc2.  A point with pc2 <= 0 or a non-finite pc2 (behind the camera, NaN joints) gets r = -1: it is not drawn.
 *     A disc renders as a circle of that radius: no perspective-correct ellipse.
 * Errors: UVS_ERR_ARG for NULL cam / q_prev / discs_out, T < 0, n_joints outside 1 .. 8, n_points not in {1, 3, 4}, q_out overlapping
 * q_prev.  T == 0 returns UVS_OK and launches nothing.
 */
int uvs_camera_project_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt,
                           double *q_out, double *discs_out, void *stream);

/*
 * Rasteriser: T frames [256][256][3] uint8 of n_colours discs, written UNFLIPPED as the sensor hands them over (flipped row i is stored
 * at row 255 - i), frame t at frames + t * frame_stride_bytes.  Alignment and stride rules are the detector's: frames 16-byte aligned,
 * frame_stride_bytes a multiple of 16 and at least 256 * 256 * 3; bytes beyond a frame's 196 608 are not written.
 *   discs [T][n_colours][3] in: (u, v, r) as uvs_camera_project_f64 writes them.
 * The pixel rule is part of the contract.  Pixel (flipped row i, column j) belongs to disc c iff r_c >= 0 and
 *   fl(fl(dx * dx) + fl(dy * dy)) <= fl(r_c * r_c),   dx = (double)j - u_c,  dy = (double)i - v_c;
 * a NaN anywhere gives nothing.  The painter's order is the colour order (a later disc overwrites an earlier one); the colours are
 * (255,0,0), (0,255,0), (0,0,255), (255,0,255), with n_colours == 1 the one disc is green; every other pixel is `background` in all
 * three channels.
 * The rule holds for every disc, whatever its size: u, v and r may be huge or infinite (a point that grazes the camera's focal plane
 * projects to some 1e7 px and beyond), and the frames are those of the rule evaluated at all 65 536 pixels.  The kernels here and
 * below visit a disc's bounding box only, [centre - r - 1, centre + r + 1] clipped to the frame, while |u|, |v| and r are all below
 * 1e9; any other disc -- from 2^54 on the rule's rounded dx reaches past that box -- is given the whole frame as its box.
 * Errors: UVS_ERR_ARG for NULL discs / frames, T < 0, n_colours not in {1, 3, 4}, background outside 0 .. 249 (250 and above would
 * enter a mask of the detector), a misaligned frames pointer, a stride below 256 * 256 * 3 or not a multiple of 16.  T == 0 returns
 * UVS_OK and launches nothing.  One workgroup per frame, 16-byte stores.
 */
int uvs_render_discs_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, uint8_t *frames,
                        int64_t frame_stride_bytes, void *stream);

/*
 * The frame-free detector: what uvs_detect_circles_u8 returns for the frames uvs_render_discs_u8 writes from `discs`, bit for bit
 * (features, NaN pairs of empty masks, mask sizes, noise epilogue), without the frames.  Thread (colour c, index i) counts the rows at
 * which c is the topmost disc in column i and the columns at which it is topmost in row i, visiting only the disc's bounding box
 * [centre - r - 1, centre + r + 1] clipped to the frame (the whole frame for a disc with |u|, |v| or r not below 1e9, see the pixel
 * rule above); the sums that follow are the detector's own code.
 *   discs [T][n_colours][3] in; noise [T][2*n_colours] in or NULL; f_out [T][2*n_colours] out; pixels_out [T][n_colours] int32 out or NULL.
 * Errors: UVS_ERR_ARG for NULL discs / f_out, T < 0, n_colours not in {1, 3, 4}.  T == 0 returns UVS_OK and launches nothing.
 */
int uvs_disc_features_f64(int64_t T, const double *discs, int32_t n_colours, const double *noise, double *f_out,
                          int32_t *pixels_out, void *stream);

/*
 * uvs_camera_project_f64 and uvs_disc_features_f64 in one launch (one workgroup per trial), bit-identical to the two calls in a row:
 * joints in, noisy detected features out.  Arguments as above with n_colours = cam->n_points; discs_out [T][n_points][3] out or NULL.
 * Errors: those of the two calls (f_out takes the place of discs_out as the mandatory output).
 */
int uvs_camera_features_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt,
                            double *q_out, const double *noise, double *f_out, int32_t *pixels_out, double *discs_out,
                            void *stream);

/*
 * Occluders: opaque rectangles that slide in front of the discs while the loop runs -- the event that gives a centre-of-mass detector its
 * heavy-tailed errors (the mask loses a side and the centroid jumps).  The rule, in integers, is part of the pixel rule above:
 *   - At step k >= 0 an occluder is ACTIVE iff k_on <= k < k_off, w > 0 and h > 0.  It then covers columns [x_k, x_k + w - 1] and flipped
 *     rows [y_k, y_k + h - 1], clipped to the frame, with x_k = x + vx * k and y_k = y + vy * k formed in 64-bit integers: with k < 2^31
 *     nothing overflows, whatever the int32 fields hold, and the clip to [0, 255] comes before any narrowing.
 *   - A covered pixel belongs to NO disc, whatever the painter's order; the rasteriser gives it `shade` in all three channels (0 .. 249,
 *     for background's reason).  Occluders may overlap: the covered set is the union.  Everything else is the rule above, unchanged.
 * plant.occluder_rects and plant.render_discs (Python) state the rule once in numpy; every kernel below is held to it byte for byte.
 * The operand of every entry point: occ [T][n_occ] structs in device (or pinned host) memory, trial t's at occ + t * n_occ; n_occ in
 * 0 .. UVS_CAMERA_MAX_OCCLUDERS (occ may be NULL only with 0); the step k >= 0.
 */
#define UVS_CAMERA_MAX_OCCLUDERS 4
typedef struct uvs_occluder {      /* 8 x int32, 32 bytes */
    int32_t x, y;                  /* column and FLIPPED row of the top-left pixel at step 0 */
    int32_t w, h;                  /* size in pixels; w <= 0 or h <= 0 covers nothing */
    int32_t vx, vy;                /* pixels per step */
    int32_t k_on, k_off;           /* active at steps k_on <= k < k_off */
} uvs_occluder;

/*
 * The three entry points above with occluders at step k; without any (n_occ == 0) each gives the bits of its namesake.  The detectors
 * decide per disc: when no active rectangle meets the disc's bounding box the walk is the unoccluded one, so an unoccluded disc costs what
 * it costs there.  A disc that is covered completely has an empty mask: a NaN pair and a mask size of 0, like a disc outside the frame.
 * Errors: those of the namesake, then UVS_ERR_ARG for n_occ outside 0 .. 4, a NULL occ with n_occ > 0, k < 0, or (rasteriser) shade
 * outside 0 .. 249.  T == 0 returns UVS_OK and launches nothing.
 */
int uvs_render_discs_occluded_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, const uvs_occluder *occ,
                                 int32_t n_occ, int32_t k, int32_t shade, uint8_t *frames, int64_t frame_stride_bytes, void *stream);
int uvs_disc_features_occluded_f64(int64_t T, const double *discs, int32_t n_colours, const uvs_occluder *occ, int32_t n_occ, int32_t k,
                                   const double *noise, double *f_out, int32_t *pixels_out, void *stream);
int uvs_camera_features_occluded_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                     const uvs_occluder *occ, int32_t n_occ, int32_t k, const double *noise, double *f_out,
                                     int32_t *pixels_out, double *discs_out, void *stream);

/*
 * The pixel closed loop in ONE launch: K steps of { joints, projection, frame-free detection, estimator, control law } for T trials, with the
 * filter state resident in registers.  Step for step it is the loop a caller writes with the camera-features entry point above and the
 * single-step entry point of libuvs_rmckf (state in HBM, two launches per step), and since both libraries compile with -ffp-contract=off
 * every output has that loop's bits.  The estimator code is libuvs_rmckf's own device header, compiled into this library.
 *   fp: the uvs_filter_params struct of uvs_rmckf.h (K = fp->steps >= 1; dt, gain, method, kernel_bw, annealing, desired, option bit
 *     UVS_OPT_STRICT_PINV as there).  (fp->m, fp->n) must be (8, 6), (6, 6) or (2, 6) with fp->m == 2 * cam->n_points and fp->n ==
 *     cam->n_joints, and fp->lanes_per_filter 0: the kernel runs the lane counts the single-step entry point resolves for 0 (4, 2, 1).
 *   q_start [T][n] in.  noise [K][T][m] in or NULL.  x0 [T][m*n] in: the initial estimate.  f0 [T][m] in: the first step's f_old -- the
 *     noise-free detection at q_start when fp->initial_guess, zeros otherwise.
 *   q_log [K][T][n], f_log [K][T][m], dq_log [K][T][n], err_log [K][T][m], kappa_log [K][T][m] out, each or NULL (not written).
 *   status [T], k_done [T] int32 out; stats [T][3] out: ||ISE||, ||IAE||, ||ITAE|| of the error rows k < k_done with the clock t_k = dt
 *     accumulated in floating point, summed in the order of libuvs_rmckf's statistics kernel.  pixels [T][n_points] int32 out or NULL: the
 *     smallest mask per colour over the steps k <= k_done.
 * Step k: q_k = q_{k-1} + dq_{k-1} * dt (one rounded multiply, one rounded add; q_0 = q_start), f_k = detection at q_k + noise_k,
 * z = f_k - f_{k-1}, err = f_k - desired, estimator update with regressor dq_{k-1} (zero at k = 0) and bandwidth sigma_k, then the control
 * law: the plain least-squares solve, and the careful one (numpy's pinv) for a filter whose watch fires, or for all under UVS_OPT_STRICT_PINV.
 * A non-finite state after the update -- a disc left the frame: NaN features -- gives status FAIL and k_done = k, and the trial stops.
 * Rows q_log[k], f_log[k] are written for k <= k_done, rows dq_log[k], err_log[k], kappa_log[k] for k < k_done; the rest is left as it was.
 * Estimators: GMCKF, KF and IMCC-KF at all three shapes.  MCKF at (8, 6) and (2, 6); at (6, 6) its instantiation spills to scratch memory,
 * is not built, and is refused with UVS_ERR_METHOD (-4, as in uvs_rmckf.h), like UVS_METHOD_ANALYTICAL at every shape
 * (the calibrated baseline has its own pixel loop, uvs_camera_analytical_loop_f64 below).
 * Errors, all before the first HIP call: UVS_ERR_ARG for NULL fp / cam / q_start / x0 / f0 / status / k_done / stats, T < 0, fp->steps < 1,
 * fp->k_max < 1, n_joints outside 1 .. 8, n_points not in {1, 3, 4}, MCKF with fpi_epoch_max < 1; UVS_ERR_METHOD as above; UVS_ERR_SHAPE
 * for lanes_per_filter != 0, m != 2 * n_points, n != n_joints, or another (m, n).  T == 0 returns UVS_OK and launches nothing.
 * One workgroup of 256 threads per trial up to 256 trials, per four trials beyond; the results do not depend on which.
 */
#ifndef UVS_ERR_METHOD
#define UVS_ERR_METHOD (-4)
#endif
struct uvs_filter_params;
int uvs_camera_closed_loop_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start,
                               const double *noise, const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log,
                               double *err_log, double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                               void *stream);

/*
 * The same loop with PER-TRIAL estimator parameters: a hyperparameter grid over the same starts and noise in one launch, as
 * uvs_rmckf_closed_loop_grid_f64 of uvs_rmckf.h runs one on ideal features.  The block is this library's own struct:
 *   kernel_bw, gain, reg, fpi_threshold [T] in: trial t runs with its own sigma_0, gain, regulariser and fixed-point threshold.
 *   desired [T][m] in: trial t's desired features.
 *   A NULL member means fp's value for every trial.  The arrays are device (or pinned host) memory.  fp->annealing, anneal_span, dt,
 *     steps, k_max, fpi_epoch_max, initial_guess, method and UVS_OPT_STRICT_PINV stay launch-wide.
 *   source [T] int32 in or NULL: trial t reads q_start[source[t]], the noise rows noise[k][source[t]] -- noise is then [K][n_in][m], its
 *     row stride n_in * m, not T * m -- x0[source[t]] and f0[source[t]]: those four hold n_in trials.  NULL: trial t reads trial t, the
 *     four hold T trials, and n_in is not read.  Every output of trial t is written at t; the logs are [K][T][comp].
 *   An index outside [0, n_in) never becomes an address (the rule of believed_index below).  That trial writes status FAIL and
 *     k_done = 0 and nothing else -- no log row, no stats, no pixels -- and its neighbours keep their bits.
 * Every value is used exactly where uvs_camera_closed_loop_f64 uses fp's, by the same operations in the same order (the two kernels are
 * one text): trial t's results are bit-identical to those of that call with t's values, and a block whose members are all NULL is that
 * call.  The other arguments are that call's.
 * Built: GMCKF, KF and IMCC-KF at (8, 6), (6, 6) and (2, 6), MCKF at (8, 6) and (2, 6), each in both workgroup forms (chosen by T, the
 * number of output trials) with 0 B of scratch memory.  MCKF at (6, 6) would spill here as it does there: it is not built and is refused
 * with UVS_ERR_METHOD.  No other flavour is missing.
 * Errors, all before the first HIP call: those of uvs_camera_closed_loop_f64, in its order, then UVS_ERR_ARG for a NULL tp or for source
 * with n_in < 1.  T == 0 returns UVS_OK and launches nothing.
 */
typedef struct uvs_camera_trial_params {
    const double *kernel_bw, *gain, *reg, *fpi_threshold;  /* [T] device or pinned; NULL = fp's value for every trial */
    const double *desired;                                 /* [T][m]; NULL = fp->desired */
    const int32_t *source;                                 /* [T]; NULL = t */
    int64_t n_in;                                          /* trials that q_start / noise / x0 / f0 hold; read only with source */
} uvs_camera_trial_params;
int uvs_camera_closed_loop_grid_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T,
                                    const uvs_camera_trial_params *tp, const double *q_start, const double *noise, const double *x0,
                                    const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log,
                                    int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream);

/*
 * The same loop with OCCLUDERS in front of the camera, per output trial: the detection of step k is that of the frame with trial t's
 * occluders at step k (the rule at uvs_occluder above).  One flavour carries both the per-trial block and the occluders -- the study it
 * serves is occlusion scenario x bandwidth x estimator over the same starts and noise.
 *   tp: the block of uvs_camera_closed_loop_grid_f64, or NULL = every member NULL.
 *   occ [T][n_occ]: indexed by OUTPUT trial, like every output (not by source); n_occ 0 .. 4, occ NULL only with 0.
 *   The fourteen operands that follow are those of uvs_camera_closed_loop_grid_f64, in its order.  f0 is the caller's: for the loop of the
 *     reference it is the noise-free detection of the step-0 frame, occluders at k = 0 included.
 * A trial without an active occluder near its discs has the bits of uvs_camera_closed_loop_grid_f64; a padding or void trial evaluates
 * the rectangles of the trial it shadows and stores nothing.  FULL OCCLUSION: an occluder that covers a disc completely gives an empty
 * mask, a NaN pair, a non-finite X and FAIL at that step -- the loop's behaviour for a disc that leaves the frame, and the documented
 * meaning of full occlusion; the last feature is not held here (uvs_camera_closed_loop_held_f64 below holds it).
 * Built: what uvs_camera_closed_loop_grid_f64 builds (MCKF at (6, 6) is refused with UVS_ERR_METHOD), each in both workgroup forms with
 * 0 B of scratch memory.
 * Errors, all before the first HIP call: those of uvs_camera_closed_loop_grid_f64, in its order, except that a NULL tp is allowed; then
 * UVS_ERR_ARG for n_occ outside 0 .. 4 or a NULL occ with n_occ > 0.  T == 0 returns UVS_OK and launches nothing.
 */
int uvs_camera_closed_loop_occluded_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T,
                                        const uvs_camera_trial_params *tp, const uvs_occluder *occ, int32_t n_occ, const double *q_start,
                                        const double *noise, const double *x0, const double *f0, double *q_log, double *f_log,
                                        double *dq_log, double *err_log, double *kappa_log, int32_t *status, int32_t *k_done,
                                        double *stats, int32_t *pixels, void *stream);

/*
 * The same loop HOLDING a lost disc's last detection, as a servo loop reuses the last detection when its detector returns nothing for a
 * few frames.  The rule (plant.hold_features states it in numpy; every kernel is held to it bit for bit):
 *   hold >= 0, one for the launch: the largest number of consecutive steps for which a disc's pair may be held.
 *   Disc j of a trial is LOST at step k iff its mask count at step k is 0 -- covered completely, out of the frame, behind the camera or a
 *     NaN projection alike: the integer count decides, never the floating-point pair.  Each trial keeps a counter miss[j], 0 at the start.
 *   detected: miss[j] = 0 and the pair is the detector's, noise included.
 *   lost, k >= 1 and miss[j] < hold: the reported pair of step k is the reported pair of step k - 1 -- row k - 1 of the f log, with that
 *     step's noise in it and no noise of step k added; miss[j] += 1; the disc counts as HELD at step k.
 *   lost otherwise (step 0, where f0 is the same empty frame, or a hold that is used up): the NaN pair, which FAILs the trial at this step.
 * A held pair is an ordinary input to the estimator: z = f_k - f_{k-1} is exactly +0.0 in its two rows, err repeats, the statistics sum it.
 *   The twenty operands of uvs_camera_closed_loop_occluded_f64, in its order, with two more: hold after n_occ, held after pixels.
 *   held [T][n_points] out or NULL: the number of steps k <= k_done (and k < K) at which the disc was held -- the steps pixels looks at;
 *     pixels is the smallest mask seen, as before, so a trial that SUCCEEDs after a hold shows 0 there.
 * occ = NULL with n_occ = 0 and hold > 0 is legal: a disc that leaves the frame is held too.  hold = 0 gives the bits of
 * uvs_camera_closed_loop_occluded_f64 (and held = 0 everywhere).  A padding or void trial stores nothing, held included.
 * Built: what uvs_camera_closed_loop_occluded_f64 builds (MCKF at (6, 6) is refused with UVS_ERR_METHOD), each in both workgroup forms
 * with 0 B of scratch memory.
 * Errors, all before the first HIP call: those of uvs_camera_closed_loop_occluded_f64, in its order; then UVS_ERR_ARG for hold < 0.
 * T == 0 returns UVS_OK and launches nothing.
 */
int uvs_camera_closed_loop_held_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T,
                                    const uvs_camera_trial_params *tp, const uvs_occluder *occ, int32_t n_occ, int32_t hold,
                                    const double *q_start, const double *noise, const double *x0, const double *f0, double *q_log,
                                    double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status, int32_t *k_done,
                                    double *stats, int32_t *pixels, int32_t *held, void *stream);

/*
 * The rule above for the stepwise loops: one small launch, one thread per (trial, disc), applied to the row that
 * uvs_camera_features_f64 or uvs_camera_features_occluded_f64 has just written on the same stream.
 *   k: the step; f_prev_row [T][2*n_points] in: the reported row of step k - 1 (read only where a pair is held; may be NULL at k == 0).
 *   f_row [T][2*n_points] in, out: the detector's row of step k; a held pair is overwritten with f_prev_row's, nothing else is written.
 *   pixels_row [T][n_points] in: the mask counts of step k.
 *   miss [T][4] in, out: the loop's counters of consecutive held steps, zero before step 0 (disc j of trial t at 4 t + j).
 *   held_row [T][n_points] out or NULL: 1 where the disc was held at this step, else 0.
 * hold == 0 holds nothing (and still resets miss).  Errors, before the HIP call: UVS_ERR_ARG for a NULL f_row, pixels_row or miss, T < 0,
 * n_points not in {1, 3, 4}, hold < 0, k < 0, or a NULL f_prev_row with k >= 1.  T == 0 returns UVS_OK and launches nothing.
 */
int uvs_hold_features_f64(int64_t T, int32_t n_points, int32_t hold, int32_t k, const double *f_prev_row, double *f_row,
                          const int32_t *pixels_row, int32_t *miss, int32_t *held_row, void *stream);

/*
 * PAINTED occluders: distractors.  A colour-threshold detector's best-known outlier ADDS pixels to a mask -- something else in the scene has
 * the target's colour -- where the occluders above only remove them.  An occluder may therefore carry a PAINT, a parallel operand; the
 * uvs_occluder struct is as it was:
 *   paint [T][n_occ] int32 in, device (or pinned host) memory, trial t's values at paint + t * n_occ, or NULL = every rectangle opaque.
 *   A value p in 0 .. n_colours - 1 paints the rectangle the colour of disc p (n_colours == 1: 0 is the green one).  EVERY other int32
 *   (-1 by convention) is opaque, as above: the device rule is total and validates nothing.
 * Order: the rectangles are in front of every disc, and rectangle o' is in front of rectangle o when o' > o.  A pixel belongs to the
 * highest-index ACTIVE rectangle that contains it; otherwise to the topmost disc by the painter's order; otherwise to the background.
 *   Rasteriser: a pixel of a rectangle painted p gets disc p's colour in its three channels, a pixel of an opaque one `shade`.
 *   Detectors: the mask of colour c is { pixels of disc c } + { pixels of the rectangles painted c } -- disjoint sets, so the integer
 *     column and row counts add; the sums, the centre and the noise add are those of the pixel rule above.  The mask size includes the
 *     distractor's pixels.  A colour whose disc draws nothing (r < 0, out of the frame, NaN) still has a mask where a rectangle is painted it.
 *   Hold: "lost iff the count is 0" stays the rule, so a disc that is gone while a distractor of its colour is visible is NOT lost: it
 *     reports the distractor's centroid.
 * plant.render_discs(..., occluder_colours=) states the rule once in numpy; every kernel below is held to it byte for byte.
 * Bit for bit: paint == NULL, or every paint opaque, gives the occluded (or held) namesake -- for opaque rectangles "a later one in front"
 * is the union of above -- and n_occ == 0 the unoccluded one.
 * The three stand-alone entry points and the loop: each its occluded (held) namesake's operands with `paint` directly after `occ`, its
 * refusals in its order (a NULL paint is legal with any n_occ), its instantiations (the loop: GMCKF, KF and IMCC-KF at (8, 6), (6, 6) and
 * (2, 6), MCKF at (8, 6) and (2, 6), each in both workgroup forms with 0 B of scratch memory; MCKF at (6, 6) is refused with
 * UVS_ERR_METHOD).  In the loop paints are indexed by OUTPUT trial, like occluders; f0 is the caller's: for the loop of the reference the
 * noise-free detection of the step-0 frame, painted rectangles included.
 */
int uvs_render_discs_painted_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, const uvs_occluder *occ,
                                const int32_t *paint, int32_t n_occ, int32_t k, int32_t shade, uint8_t *frames, int64_t frame_stride_bytes,
                                void *stream);
int uvs_disc_features_painted_f64(int64_t T, const double *discs, int32_t n_colours, const uvs_occluder *occ, const int32_t *paint,
                                  int32_t n_occ, int32_t k, const double *noise, double *f_out, int32_t *pixels_out, void *stream);
int uvs_camera_features_painted_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                    const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t k, const double *noise,
                                    double *f_out, int32_t *pixels_out, double *discs_out, void *stream);
int uvs_camera_closed_loop_painted_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T,
                                       const uvs_camera_trial_params *tp, const uvs_occluder *occ, const int32_t *paint, int32_t n_occ,
                                       int32_t hold, const double *q_start, const double *noise, const double *x0, const double *f0,
                                       double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status,
                                       int32_t *k_done, double *stats, int32_t *pixels, int32_t *held, void *stream);

/*
 * The analytic initial guess X0 of the loop (experiment.py:94-114) for T trials, one lane each: the geometric Jacobian of the DH chain in the
 * camera frame at q_start, the depths |camera - point|, and the image-Jacobian rows at the DETECTED features f0 (raw pixels).
 *   q_start [T][6] in; f0 [T][2*n_points] in; x0_out [T][2*n_points*6] out.
 * The same formula as the host's numpy statement, in another order of operations: equal to about 1e-13 relative, not bit for bit.
 * Errors: UVS_ERR_ARG for a NULL pointer, T < 0, n_points not in {1, 3, 4}; UVS_ERR_SHAPE for n_joints != 6.  T == 0 returns UVS_OK.
 */
int uvs_camera_guess_f64(const uvs_camera *cam, int64_t T, const double *q_start, const double *f0, double *x0_out, void *stream);

/*
 * The calibrated IBVS baseline (Method.ANALYTICAL, experiment.py:145-162 and :300-320) through pixels: the control law whose interaction
 * matrix is evaluated from the model at every step instead of estimated -- what the estimators of the loop above are compared against.
 * The two entry points below are that loop's single step and its one launch.  The step, defined once for both:
 *   (rot, pos, Jc) = the camera pose and the geometric Jacobian of the DH chain in the camera frame at the joints q;
 *   depth_p = |pos - points[p]|, the true camera-disc distance (computeZ(recalculate_fkine=True));
 *   rows 2p, 2p+1 of J = the image-Jacobian rows at the NOISY DETECTED u = f[2p], v = f[2p+1] (raw pixels) and depth_p, times Jc;
 *   err = f - desired; kappa = 1;
 *   status FAIL when an entry of J is not finite (numpy's pinv raises there, :313-316): a disc left the frame (NaN pair) or the noise
 *     row holds a NaN;
 *   dq = -gain * pinv(J) err by the solver sequence of the loop above: the plain least-squares solve with its watches, and the careful
 *     one (numpy's pinv) for a solve whose watch fires, or for every solve under UVS_OPT_STRICT_PINV.
 * Both kernels form every value through the same device functions (libuvs_rmckf's device header, compiled into this library with
 * -ffp-contract=off) in the same order: K x (uvs_camera_features_f64, uvs_camera_analytical_step_f64) on rows of the logs and the one
 * launch give the same bits.
 * Both entry points, before the first HIP call: fp->method must be UVS_METHOD_ANALYTICAL (else UVS_ERR_METHOD); fp->lanes_per_filter 0,
 * (fp->m, fp->n) one of (8, 6), (6, 6), (2, 6) with fp->m == 2 * cam->n_points and fp->n == cam->n_joints == 6 (else UVS_ERR_SHAPE; the
 * kernels run 4, 2, 1 lanes per trial); fp->reserved 0 or UVS_OPT_STRICT_PINV (else UVS_ERR_ARG); m, n, gain, desired, reserved -- and
 * for the loop steps and dt -- are read, the estimator fields are ignored.  UVS_ERR_ARG for a NULL mandatory pointer, T < 0, n_joints
 * outside 1 .. 8, n_points not in {1, 3, 4}.  T == 0 returns UVS_OK and launches nothing.  All three shapes are built, in every form,
 * with 0 B of scratch memory.
 *
 * uvs_camera_analytical_step_f64: one step for T trials.
 *   q [T][n] in; f [T][m] in: detected features, noise already added.
 *   dq_out [T][n] out; err_out [T][m] out; j_out [T][m*n] out or NULL: J, row-major; status [T] int32 out: UVS_STATUS_SUCCESS or _FAIL.
 *   On FAIL the trial's dq_out row is unspecified; err_out and j_out are still written.
 * 64 / lanes trials per wavefront.
 */
int uvs_camera_analytical_step_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q, const double *f,
                                   double *dq_out, double *err_out, double *j_out, int32_t *status, void *stream);

/*
 * uvs_camera_analytical_loop_f64: the pixel closed loop of the calibrated law in ONE launch, K = fp->steps >= 1 (else UVS_ERR_ARG).
 *   q_start [T][n] in.  noise [K][T][m] in or NULL.
 *   q_log [K][T][n], f_log [K][T][m], dq_log [K][T][n], err_log [K][T][m] out, each or NULL (not written).
 *   status [T], k_done [T] int32 out; stats [T][3] out; pixels [T][n_points] int32 out or NULL: as uvs_camera_closed_loop_f64 writes them.
 * Step k: q_k = q_{k-1} + dq_{k-1} * dt (one rounded multiply, one rounded add; q_0 = q_start), f_k = the frame-free detection at q_k
 * + noise_k, then the step above.  The rules are those of uvs_camera_closed_loop_f64: rows q_log[k], f_log[k] are written for
 * k <= k_done, rows dq_log[k], err_log[k] for k < k_done, the rest is left as it was; the clock t_k = dt accumulated in floating point
 * and the order of the statistics' sums; pixels = the smallest mask per colour over k <= k_done; a FAILed trial (k_done = the failing
 * step) stops alone.  There is no x0, f0 or kappa_log.
 * One workgroup of 256 threads per trial up to 256 trials, per four trials beyond; the results do not depend on which.
 */
int uvs_camera_analytical_loop_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const double *q_start,
                                   const double *noise, double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status,
                                   int32_t *k_done, double *stats, int32_t *pixels, void *stream);

/*
 * The calibrated law on a WRONG model, per trial.  The loop above hands its control side the camera that renders the frames; the entry
 * points below take the control side's model as a second operand, so that the baseline can be miscalibrated, differently in every trial:
 *   believed [n_believed] in: uvs_camera structs IN DEVICE (or pinned host) MEMORY, unlike `cam`, which stays a host struct passed by value
 *     into the launch.  A wrong model is a uvs_camera with other numbers in it -- focal: the intrinsics; points: the depth assumption;
 *     theta_offset: encoder zeros (joint 6: camera roll); d, a, cos_alpha, sin_alpha: link and hand-eye geometry.  n_joints and n_points
 *     of a believed struct are ignored (the shape is fp's, and cam's where there is one), and so are center and radius, which the law
 *     does not read.
 *   believed_index [T] int32 in (device or pinned) or NULL.  With an index trial t uses believed[believed_index[t]].  Without one
 *     n_believed must be 1 (every trial uses believed[0]) or T (trial t uses believed[t]), else UVS_ERR_ARG.
 *   An index outside [0, n_believed) never becomes an address.  That trial reads no model and FAILs: the step writes its status FAIL and
 *     nothing else; the loop writes status FAIL and k_done = 0 and nothing else (no log row, no stats, no pixels); the guess writes
 *     nothing.  Its neighbours are untouched.
 * The step is the one of uvs_camera_analytical_step_f64, the same device function on the same operands: with believed == the true camera
 * every entry point here gives the bits of its calibrated counterpart, and K x (uvs_camera_features_f64 on the true camera,
 * uvs_camera_believed_step_f64) on rows of the logs gives the bits of uvs_camera_believed_loop_f64.
 * Refusals, before the first HIP call: those of the calibrated entry points (method, reserved, lanes_per_filter, shape, NULL mandatory
 * pointers, T, and for the loop steps), UVS_ERR_ARG for NULL believed, n_believed < 1, or n_believed not in {1, T} without an index.
 * T == 0 (with n_believed == 1 or an index) returns UVS_OK and launches nothing.  All three shapes are built, in every form, with 0 B of
 * scratch memory: the kernels stage their trials' models through LDS (472 B per trial) instead of holding them in registers.
 *
 * uvs_camera_believed_step_f64: uvs_camera_analytical_step_f64 without `cam` (n_points = fp->m / 2, n_joints = fp->n), 64 / lanes trials
 * per wavefront.
 * uvs_camera_believed_loop_f64: uvs_camera_analytical_loop_f64; the sensor side (projection, detection) uses `cam`, the law `believed`.
 * uvs_camera_believed_guess_f64: uvs_camera_guess_f64 on the trial's believed model, so that an estimator can start from the same wrong
 *   model the baseline is stuck with.  There is no true camera among its operands, so the number of points is an argument of its own;
 *   six joints.  f0 are the features detected on the true camera.  UVS_ERR_ARG for a NULL pointer, T < 0, n_points not in {1, 3, 4}.
 */
int uvs_camera_believed_step_f64(const struct uvs_filter_params *fp, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                 const int32_t *believed_index, const double *q, const double *f, double *dq_out, double *err_out,
                                 double *j_out, int32_t *status, void *stream);
int uvs_camera_believed_loop_f64(const struct uvs_filter_params *fp, const uvs_camera *cam, int64_t T, const uvs_camera *believed,
                                 int64_t n_believed, const int32_t *believed_index, const double *q_start, const double *noise,
                                 double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done,
                                 double *stats, int32_t *pixels, void *stream);
int uvs_camera_believed_guess_f64(int64_t T, int32_t n_points, const uvs_camera *believed, int64_t n_believed,
                                  const int32_t *believed_index, const double *q_start, const double *f0, double *x0_out, void *stream);

/*
 * A SCENE PER TRIAL: Monte-Carlo over true cameras in one launch.  Every entry point above that takes `cam` renders the frames of all T
 * trials with that one host struct.  Below, a SCENE is the uvs_camera that renders a trial's frames, and every trial has its own.  The
 * scene operand is a triple, with the rules of the believed operand above word for word:
 *   cams [n_cams] in: uvs_camera structs IN DEVICE (or pinned host) MEMORY.
 *   cam_index [T] int32 in (device or pinned) or NULL.  With an index trial t is rendered by cams[cam_index[t]].  Without one n_cams must
 *     be 1 (every trial cams[0]) or T (trial t cams[t]), else UVS_ERR_ARG.
 *   An index outside [0, n_cams) never becomes an address.  That trial is VOID: a stand-alone call writes nothing for it; a loop writes
 *     status FAIL and k_done = 0 and nothing else (no log row, no stats, no pixels, no held); its neighbours keep their bits.
 *   The index is by OUTPUT trial, like occluders and paints (not by trial_params' source).
 *   Shapes come from fp (n_points = fp->m / 2), or from the n_points argument where there is no fp; six joints everywhere.  The structs'
 *     own n_joints / n_points are not read.  Read per trial: theta_offset, d, a, cos_alpha, sin_alpha, points, focal, center, radius.
 * Each entry point has its namesake's operands with `cam` replaced by the triple (the two without an fp: by the triple and n_points), its
 * namesake's refusals in their order on that shape, then the triple's: UVS_ERR_ARG for NULL cams, n_cams outside 1 .. 2^31 - 1, or
 * n_cams not in {1, T} without an index.  T == 0 (with n_cams == 1 or an index) returns UVS_OK and launches nothing.  Every value is
 * formed by the namesake's operations in its order: trial t has the bits of the namesake called with cam = the scene of t.
 *
 * uvs_camera_project_scenes_f64: uvs_camera_project_f64 per trial, so that the frames of a scene batch can be rendered with the
 *   rasterisers above.
 * uvs_camera_features_scenes_f64: uvs_camera_features_painted_f64 per trial, the step of the stepwise loops; occ, paint and n_occ = 0 stay
 *   legal as they are there (n_occ = 0: the bits of uvs_camera_features_f64).
 * uvs_camera_closed_loop_scenes_f64: uvs_camera_closed_loop_painted_f64 per trial, with tp, occluders, paints, hold and held; f0 and x0
 *   are the caller's (for the loop of the reference: from the step-0 frame of the trial's own scene).  Built: GMCKF, KF and IMCC-KF at
 *   (8, 6), (6, 6) and (2, 6), MCKF at (8, 6) and (2, 6), each in both workgroup forms with 0 B of scratch memory -- what the painted
 *   flavour builds, no instantiation is missing beyond MCKF at (6, 6), which is refused with UVS_ERR_METHOD as everywhere.  The kernel
 *   stages its workgroup's scenes through LDS (472 B per trial) once, before the first step.
 * uvs_camera_believed_loop_scenes_f64: uvs_camera_believed_loop_f64 with the sensor side on the trial's scene and the law on its believed
 *   model; a trial without a scene or without a model is void.  No occluders and no hold, as there.  With believed == cams and
 *   believed_index == cam_index it is the calibrated law on every trial's own camera.  All three shapes, both forms, 0 B of scratch.
 */
int uvs_camera_project_scenes_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int32_t n_points, int64_t T,
                                  const double *q_prev, const double *dq, double dt, double *q_out, double *discs_out, void *stream);
int uvs_camera_features_scenes_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int32_t n_points, int64_t T,
                                   const double *q_prev, const double *dq, double dt, double *q_out, const uvs_occluder *occ,
                                   const int32_t *paint, int32_t n_occ, int32_t k, const double *noise, double *f_out, int32_t *pixels_out,
                                   double *discs_out, void *stream);
int uvs_camera_closed_loop_scenes_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                      int64_t T, const uvs_camera_trial_params *tp, const uvs_occluder *occ, const int32_t *paint,
                                      int32_t n_occ, int32_t hold, const double *q_start, const double *noise, const double *x0,
                                      const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log,
                                      int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, int32_t *held, void *stream);
int uvs_camera_believed_loop_scenes_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                        int64_t T, const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index,
                                        const double *q_start, const double *noise, double *q_log, double *f_log, double *dq_log,
                                        double *err_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, void *stream);

/*
 * MOVING TARGETS: the discs move while the loop runs.  Every scene above is static -- the world points a trial looks at at step 0 are the
 * ones it looks at at step K - 1.  Below each OUTPUT trial may carry a motion, the one disturbance that breaks the estimators'
 * measurement model z = J dq continuously, and the one the calibrated law is not immune to: its model of the points stays where it was.
 * The rule (plant.target_at states it once in numpy; every kernel below is held to it bit for bit):
 *   Each disc p has a world velocity v[p] in metres per step, and one window (k_on, k_off) applies to all discs of the trial.
 *   At step k >= 0 the target has moved s(k) = clamp(k - k_on, 0, max(k_off - k_on, 0)) steps, formed in 64-bit integers: nothing
 *     overflows, whatever the int32 fields hold.
 *   If s == 0 the world point of disc p is points[p] itself, bits untouched, with no arithmetic at all -- also for a -0.0 coordinate
 *     and for a velocity that is not finite.  Otherwise, per coordinate, points[p][c] + (double)s * v[p][c]: one rounded multiply, then
 *     one rounded add, as the joint step does it.  On the device the choice is a select, not a branch.
 *   Everything downstream is the text above on that point: projection, apparent radius focal * radius / zc, the pixel rule, occluders,
 *     paints and hold.
 * The operand: motion [T] structs in device (or pinned host) memory, indexed by OUTPUT trial like occluders, paints and cam_index;
 * NULL = nothing moves.  The struct's values are not validated: the device rule is total.
 * Each entry point has its *_scenes_* namesake's operands in its order with `motion` directly after cam_index (the project call, which
 * has no k, also takes the step k after dt), its namesake's refusals in their order, all before the first HIP call; the project call
 * then adds UVS_ERR_ARG for k < 0.  T == 0 returns UVS_OK and launches nothing.
 * Bit for bit: (a) motion == NULL, or a trial whose s(k) == 0 at every step, has the bits of the *_scenes_* namesake; (b) at a given k a
 * stand-alone call has the bits of the scenes namesake on a camera whose points were moved on the host by the numpy rule; (c) a padding
 * wavefront reads the motion of the trial it shadows and stores nothing; (d) a void trial (no scene, or a void source) is void as
 * before, and its motion never forms an output.
 * The loops stage their trials' motions through LDS (104 B per trial) once, next to the scenes, and form a moved point in registers
 * where it is projected; nothing is written back.  uvs_camera_believed_loop_moving_f64 moves the SENSOR side's points alone: the law's
 * model (believed, or the trial's own scene) stays where it was -- the controller does not know the target's motion.
 * Built: what the scenes namesakes build -- the estimator loop for GMCKF, KF and IMCC-KF at (8, 6), (6, 6) and (2, 6), MCKF at (8, 6)
 * and (2, 6) (at (6, 6) refused with UVS_ERR_METHOD as everywhere), the baseline loop at the three shapes, each in both workgroup forms
 * with 0 B of scratch memory.
 */
typedef struct uvs_target_motion {          /* 104 bytes */
    double  v[UVS_CAMERA_MAX_POINTS][3];    /* world metres per step */
    int32_t k_on, k_off;
} uvs_target_motion;

int uvs_camera_project_moving_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                  int32_t n_points, int64_t T, const double *q_prev, const double *dq, double dt, int32_t k, double *q_out,
                                  double *discs_out, void *stream);
int uvs_camera_features_moving_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                   int32_t n_points, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                   const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t k, const double *noise,
                                   double *f_out, int32_t *pixels_out, double *discs_out, void *stream);
int uvs_camera_closed_loop_moving_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                      const uvs_target_motion *motion, int64_t T, const uvs_camera_trial_params *tp, const uvs_occluder *occ,
                                      const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start, const double *noise,
                                      const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                                      double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, int32_t *held,
                                      void *stream);
int uvs_camera_believed_loop_moving_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                        const uvs_target_motion *motion, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                        const int32_t *believed_index, const double *q_start, const double *noise, double *q_log,
                                        double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done, double *stats,
                                        int32_t *pixels, void *stream);

/*
 * CAMERA LATENCY: the frame the detector is handed is not the newest one.  In every loop above frame k reaches the detector at step k;
 * below each OUTPUT trial may carry a latency d, in control periods, between the pose a frame shows and the command computed from it.
 * The rule (plant.delayed_step states it once in numpy; every kernel below is held to it bit for bit):
 *   latency [T] int32 by output trial, in device (or pinned host) memory; NULL = none.  The device uses clamp(d, 0,
 *     UVS_CAMERA_MAX_LATENCY): the rule is total and the operand is not validated.
 *   At step k the detector is handed the frame of step kk = max(k - d, 0): joints q_kk, occluders and paints at kk, target motion at kk.
 *     The delay line is primed with the step-0 frame.
 *   Everything after the detector is the text above on that detection, in this order: the centre; plus the noise of step k (NOT kk), one
 *     rounded add; then the hold rule on the delayed integer counts; then the estimator or the law.
 *   The law's joints are the current q_k (encoders are not delayed), the regressor is dq_{k-1} as before: the controller is not told the
 *     latency.  f logs the reported row; pixels is the smallest mask among the detections that were reported while the trial's rows were
 *     due; held counts as before.  f0 and the initial guess come from the step-0 frame.  With d == 0 the pair is the one just detected.
 * The two loops have their *_moving_* namesake's operands in its order with `latency` directly after `motion`, its refusals in their
 * order, all before the first HIP call; T == 0 returns UVS_OK and launches nothing.  Each keeps the detections (the integer count and the
 * two sums of a mask, before the centre is formed) of the last UVS_CAMERA_MAX_LATENCY + 1 steps in an LDS ring per disc, written and
 * read by the one lane that holds the detection: no barrier and no exit is added.
 * uvs_delay_features_f64 is the stepwise loops' companion, like uvs_hold_features_f64: sensed_log [K][T][2 n_points] and count_log
 * [K][T][n_points] hold the noise-free sensed rows and mask sizes of steps 0 .. k (what the features calls write without noise); the
 * reported row of step k is, per trial t, row max(k - d_t, 0) of the sensed log plus noise_row (step k's [T][2 n_points], or NULL: no
 * add), and its counts those of that row.  It refuses NULL sensed_log, count_log, f_row or pixels_row, T outside 0 .. 2^31 - 1, an
 * n_points that is not 1, 3 or 4, and k < 0, before any HIP call.  f_row and pixels_row must not overlap the logs.
 * Bit for bit: (a) latency == NULL, or all zeros, gives the bits of the moving namesake; (b) a trial of a mixed-latency launch has the
 * bits of the uniform launch at its own latency; (c) the one launch has the stepwise loop's bits; (d) a padding wavefront reads the
 * latency of the trial it shadows and stores nothing; (e) void trials stay void.
 * Built: what the moving namesakes build, each in both workgroup forms with 0 B of scratch memory.
 */
#define UVS_CAMERA_MAX_LATENCY 8

int uvs_camera_closed_loop_delayed_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                       const uvs_target_motion *motion, const int32_t *latency, int64_t T,
                                       const uvs_camera_trial_params *tp, const uvs_occluder *occ, const int32_t *paint, int32_t n_occ,
                                       int32_t hold, const double *q_start, const double *noise, const double *x0, const double *f0,
                                       double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status,
                                       int32_t *k_done, double *stats, int32_t *pixels, int32_t *held, void *stream);
int uvs_camera_believed_loop_delayed_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, int64_t T, const uvs_camera *believed,
                                         int64_t n_believed, const int32_t *believed_index, const double *q_start, const double *noise,
                                         double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done,
                                         double *stats, int32_t *pixels, void *stream);
int uvs_delay_features_f64(int64_t T, int32_t n_points, int32_t k, const int32_t *latency, const double *sensed_log, const int32_t *count_log,
                           const double *noise_row, double *f_row, int32_t *pixels_row, void *stream);

/*
 * ASSUMED LATENCY: the controller is told a camera latency.  In the loops above the frame may be delayed (`latency`) but the controller is
 * not told: the estimators pair f_k - f_{k-1} with dq_{k-1} although, at latency d, that difference belongs to dq_{k-1-d}, and the law
 * evaluates its interaction matrix at q_k on features of q_{k-d}.  Below each OUTPUT trial also carries an ASSUMED latency a, in control
 * periods, independent of its true latency d: a != d is the mismatch experiment, and a > 0 without any latency is legal.  The rule
 * (plant.aligned_regressor_step and plant.delayed_step state it once in numpy; every kernel below is held to it bit for bit):
 *   assumed [T] int32 by output trial, in device (or pinned host) memory, directly after `latency`; NULL = none.  The device uses
 *     clamp(a, 0, UVS_CAMERA_MAX_LATENCY): the rule is total and the operand is not validated.
 *   Estimators: the regressor of step k is the command of step k - 1 - a when k - 1 - a >= 0, and the zero vector otherwise, which goes
 *     through the same update with h = 0 that step 0 always ran.  Everything else in the step is the text above: z, err, sigma, the
 *     control law on the updated X, the logs, the hold rule, FAIL.  Only the regressor moves: the command integrated into the joints
 *     stays dq_{k-1}.
 *   Calibrated and believed law: the joints handed to the law at step k are q_{max(k - a, 0)}, so the camera Jacobian, the depths and the
 *     interaction matrix are those of the pose the assumed frame shows.  The features stay the reported (delayed, noisy) row of step k;
 *     the model's points do not move; the q log and the joint integration stay current.
 * The two loops have their *_delayed_* namesake's operands in its order with `assumed` directly after `latency`, its refusals in their
 * order, all before the first HIP call; T == 0 returns UVS_OK and launches nothing.  The estimator loop keeps the last
 * UVS_CAMERA_MAX_LATENCY + 1 commands of every trial in an LDS ring, the baseline loop the joints of as many steps; the barriers that were
 * there cover both: no barrier and no exit is added.  The stepwise loops gather the step call's dq_prev (or joints) row per trial from the
 * dq (or q) log.
 * Bit for bit: (a) assumed == NULL, or all zeros, gives the bits of the delayed namesake (with latency NULL too: of the moving one);
 * (b) a trial of a launch that mixes (d, a) pairs has the bits of the uniform launch at its own pair; (c) the one launch has the
 * stepwise loop's bits; (d) padding wavefronts and shadow lanes read the assumed latency of the trial they shadow and store nothing;
 * (e) void trials stay void; (f) values outside 0 .. UVS_CAMERA_MAX_LATENCY are clamped on the device.
 * Built: what the delayed namesakes build, each in both workgroup forms with 0 B of scratch memory.
 */
int uvs_camera_closed_loop_aligned_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                       const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed, int64_t T,
                                       const uvs_camera_trial_params *tp, const uvs_occluder *occ, const int32_t *paint, int32_t n_occ,
                                       int32_t hold, const double *q_start, const double *noise, const double *x0, const double *f0,
                                       double *q_log, double *f_log, double *dq_log, double *err_log, double *kappa_log, int32_t *status,
                                       int32_t *k_done, double *stats, int32_t *pixels, int32_t *held, void *stream);
int uvs_camera_believed_loop_aligned_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed, int64_t T,
                                         const uvs_camera *believed, int64_t n_believed, const int32_t *believed_index, const double *q_start,
                                         const double *noise, double *q_log, double *f_log, double *dq_log, double *err_log, int32_t *status,
                                         int32_t *k_done, double *stats, int32_t *pixels, void *stream);

/*
 * FEATURE PREDICTION: the control law predicts the features over the camera latency.  Above, an assumed latency repairs the MODEL, but the
 * law still servoes on a feature row that is d steps old.  Below each OUTPUT trial also carries a prediction HORIZON p, in control periods,
 * independent of its latency d and its assumed latency a: p != d is the mismatch experiment, and p > 0 without any latency is legal.  The
 * law acts on the reported row advanced by what the commands issued since that frame must have done to it (a predictor in the Smith form).
 * The rule (plant.prediction_steps states the steps once in numpy; every kernel below is held to it bit for bit):
 *   predict [T] int32 by output trial, in device (or pinned host) memory, directly after `assumed`; NULL = none.  The device uses
 *     clamp(p, 0, UVS_CAMERA_MAX_LATENCY): the rule is total and the operand is not validated.
 *   The steps whose commands count at step k, newest first: k - 1, k - 2, ..., max(k - p, 0).
 *   Estimators, at step k after the update and before the control law:
 *     1. s = 0, then s += cmd_{k-i} for i = 1 .. p in that order; a term with k - i < 0 is the zero vector (s is never -0.0).
 *     2. for each row r: acc_r = sum_j X_k[r][j] s[j] as acc = fma(X_k[r][j], s[j], acc) from acc = 0 with j ascending -- the form of the
 *        update's own dot products -- on the X just updated.
 *     3. f^_r = f_r + acc_r, one rounded add; err_r = f^_r - desired_r.
 *     X absorbs t_s (z = X dq), so X sum dq is the feature displacement between the frame shown and now; for k < p the frame shown is
 *     frame 0, so dropping the missing terms is exact.  The control law, the err log and the three error sums see this err.  Everything
 *     else is the text above: z and f_prev come from the reported row, kappa from the innovation, the f log is the reported row; the hold
 *     rule, FAIL, the regressor (aligned to a) and the command integrated into the joints are unchanged.
 *   Calibrated and believed law: f^ = f_reported + (h(q_k) - h(q_{max(k - p, 0)})), two rounded operations per component, the difference
 *     first.  h(q) is the (u, v) uvs_camera_project_f64 gives for the law's own model at joints q; the model's points do not move.  The
 *     law is handed f^ as its feature row and is otherwise untouched: the interaction matrix is evaluated at the predicted pixels, err and
 *     the sums are f^ - f*, the joints it is handed stay q_{max(k - a, 0)}, the f log stays the reported row.  A non-finite f^ FAILs the
 *     trial through the check that is there.
 * The two loops have their *_aligned_* namesake's operands in its order with `predict` directly after `assumed`, its refusals in their
 * order, all before the first HIP call; T == 0 returns UVS_OK and launches nothing.  The estimator loop forms s for the next step from its
 * ring of commands where the command is written; the baseline loop keeps h at the joints of the last UVS_CAMERA_MAX_LATENCY + 1 steps in an
 * LDS ring, written once per step by the projection kernel's text.  No barrier and no exit is added.  The stepwise baseline loop calls
 * uvs_camera_project_f64 (or its scenes namesake) on rows k and max(k - p, 0) of the q log and applies the two operations.
 * Bit for bit: (a) predict == NULL, or all zeros, gives the bits of the aligned namesake; (b) a trial of a launch that mixes (d, a, p)
 * triples has the bits of the uniform launch at its own triple; (c) the baseline's one launch has the stepwise loop's bits; (d) padding
 * wavefronts and shadow lanes read the horizon of the trial they shadow and store nothing; (e) void trials stay void; (f) values outside
 * 0 .. UVS_CAMERA_MAX_LATENCY are clamped on the device.
 * Built: what the aligned namesakes build, each in both workgroup forms with 0 B of scratch memory.
 */
int uvs_camera_closed_loop_predicted_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                         const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed,
                                         const int32_t *predict, int64_t T, const uvs_camera_trial_params *tp, const uvs_occluder *occ,
                                         const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start, const double *noise,
                                         const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                                         double *kappa_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels, int32_t *held,
                                         void *stream);
int uvs_camera_believed_loop_predicted_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                           const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed,
                                           const int32_t *predict, int64_t T, const uvs_camera *believed, int64_t n_believed,
                                           const int32_t *believed_index, const double *q_start, const double *noise, double *q_log,
                                           double *f_log, double *dq_log, double *err_log, int32_t *status, int32_t *k_done, double *stats,
                                           int32_t *pixels, void *stream);

/*
 * THE ESTIMATE AS A LOG: the one-launch estimator loop stores X itself.  The product of the estimators is a Jacobian estimate; above it
 * lives in registers for all K steps and is never seen.  uvs_camera_closed_loop_logged_f64 has its *_predicted_* namesake's operands in
 * its order with `x_log` directly after `kappa_log`, its refusals in their order, all before the first HIP call; T == 0 returns UVS_OK and
 * launches nothing; MCKF at (6, 6) is UVS_ERR_METHOD as everywhere.
 *   x_log [K][T][m n] doubles in device memory, or NULL.  Element i n + j of a record is X[i][j]: the layout of x0 and of the X tensor of
 *     uvs_rmckf_step_f64.  Row k holds X_k, the matrix AFTER step k's update -- the one step k's control law (and prediction) reads.
 *   Row k of trial t is written under the condition of the err, kappa and dq rows: k < k_done[t], t a valid trial that is not void.  Nothing
 *     else of x_log is touched: rows from k_done on, void trials, padding wavefronts and shadow lanes store nothing.
 * Bit for bit: (a) x_log == NULL gives the bits of the predicted namesake in every output; (b) with the log every other output keeps those
 * bits; (c) rows k < k_done are the X tensor of the stepwise loop after its step call k.
 * Built: what the predicted namesake builds (22 instantiations), each with 0 B of scratch memory.
 */
int uvs_camera_closed_loop_logged_f64(const struct uvs_filter_params *fp, const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index,
                                      const uvs_target_motion *motion, const int32_t *latency, const int32_t *assumed,
                                      const int32_t *predict, int64_t T, const uvs_camera_trial_params *tp, const uvs_occluder *occ,
                                      const int32_t *paint, int32_t n_occ, int32_t hold, const double *q_start, const double *noise,
                                      const double *x0, const double *f0, double *q_log, double *f_log, double *dq_log, double *err_log,
                                      double *kappa_log, double *x_log, int32_t *status, int32_t *k_done, double *stats, int32_t *pixels,
                                      int32_t *held, void *stream);

/*
 * THE TRUE IMAGE JACOBIAN, and an X stream scored against it.  h(q) is the (u, v) row uvs_camera_project_moving_f64 gives for a trial's
 * scene at joints q and step k (a moving target's points stand where step k of its motion has taken them).  The rule
 * (plant.projection_jacobian states it once in numpy): with T6 the camera pose at q, R and c its rotation and origin, [v_j; w_j] column j
 * of the arm's geometric Jacobian (w_j = z_{j-1}, v_j = z_{j-1} x (c - o_{j-1}), frame 0 the base), w a world point and p = R^T (w - c),
 *   dp/dq_j = -R^T (w_j x (w - c) + v_j) = -R^T (z_{j-1} x (w - o_{j-1}))       (the device evaluates the right-hand form)
 *   du/dq_j = focal (dp_x / p_z - p_x dp_z / p_z^2),  dv/dq_j likewise with p_y.
 * The unit is pixels per radian: there is no t_s in it.  (The interaction row at the CENTRED pixels with the depth ALONG THE OPTICAL AXIS,
 * applied to the camera-frame twist, is this matrix; the initial guess of the loops -- raw pixels, camera-disc distance -- is not.)
 * The arms have six joints: q rows are six doubles, a record is [2 n_points][6], and no struct's own n_joints / n_points is read.
 * Operand conventions are those of the scenes / moving project calls: (cams, n_cams, cam_index) picks the scene of trial t, cam_index
 * NULL with n_cams == 1 or n_cams == T; motion [T] by trial or NULL: nothing moves.  A trial whose index names no scene gets a record of
 * NaNs and reads no struct.
 *
 * uvs_camera_jacobian_f64: q [rows][T][6], j_out [rows][T][2 n_points][6].  The record at (r, t) is dh/dq at q[r][t] of trial t's scene at
 *   step k0 + r.  Refused before any HIP call, in this order: NULL q or j_out; T outside 0 .. 2^31 - 1; rows outside 0 .. 2^31 - 1; an
 *   n_points that is not 1, 3 or 4; the scene triple's refusals; k0 < 0 or k0 + rows > 2^31 - 1.  T == 0 or rows == 0 returns UVS_OK and
 *   launches nothing.
 * uvs_camera_jacobian_score_f64: x_log [K][T][2 n_points 6] (the layout of the log above), q_log [K][T][6], dq_log [K][T][6] or NULL,
 *   k_done [T] int32 or NULL, score [K][T][6].  With J the record of the call above at (k, t) with k0 = 0, Js[i][j] = dt J[i][j] (one rounded
 *   multiply per entry), X the record of x_log and dq that of dq_log, the six doubles of a record are
 *     nx2 = sum X^2, nj2 = sum Js^2, dot = sum X Js, diff2 = sum (X - Js)^2, xd_xd = |X dq|^2, xd_jd = (X dq) . (Js dq)
 *   each product and each add rounded once.  The sums over (i, j) run row-major within a disc's two rows from 0.0; the discs' partial sums
 *   are then added in disc order from the first disc's.  (X dq)_i sums j ascending from 0.0.  dq_log == NULL: the last two are 0.0.  A record
 *   with k >= k_done[t] is six NaNs, written without reading x_log, q_log or dq_log there.  A record does not depend on T, K or where it
 *   stands in the launch.  Refused before any HIP call, in this order: NULL x_log, q_log or score; T outside 0 .. 2^31 - 1; K outside
 *   0 .. 2^31 - 1; an n_points that is not 1, 3 or 4; the scene triple's refusals.  T == 0 or K == 0 returns UVS_OK and launches nothing.
 * Either call refuses more than 2^36 records (rows T, K T) with UVS_ERR_ARG, also before any HIP call.
 * Both kernels give four lanes to a record, one per disc: a lane reads or writes the 96 contiguous bytes of its disc's two rows, so a
 * wavefront covers sixteen whole records; one device function forms J in both.
 */
int uvs_camera_jacobian_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                            int32_t n_points, int64_t T, int64_t rows, int32_t k0, const double *q, double *j_out, void *stream);
int uvs_camera_jacobian_score_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                  int32_t n_points, int64_t T, int64_t K, double dt, const double *x_log, const double *q_log,
                                  const double *dq_log, const int32_t *k_done, double *score, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UVS_VISION_H */
