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

#ifdef __cplusplus
}
#endif
#endif /* UVS_VISION_H */
