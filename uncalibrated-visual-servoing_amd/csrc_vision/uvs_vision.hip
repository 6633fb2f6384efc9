// libuvs_vision.so: centre-of-mass circle detectors of the live route (utils.py:11-166 of the reference) as one HIP kernel for gfx950.
// One workgroup of 1024 threads per 256x256 RGB frame.  Phase 1 reads the frame with 16-byte loads (16 lanes x 48 B per row, 64 rows per
// pass, all 12 loads of a thread issued before the first use), thresholds in integers and leaves integer counts in LDS; phase 2 gives
// every (colour, grid index) its own thread, which sums the column and the flipped-row count, multiplies by the grid product in fp64 and
// joins a wavefront reduction.  Nothing is atomic and no sum depends on timing: the same frame gives the same bits in every launch.
// The synthetic camera (second half of the file) is the sensor side: disc projection of a DH arm's pinhole camera, a rasteriser with the
// detector's lane unit, and frame-free detectors that count mask pixels from the disc geometry and then run the same phase 2.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "uvs_vision.h"
#include "vision_device.hpp"

namespace uvs_vision {

constexpr int kRowBytes = kSide * 3;            // 768 B = 16 lanes x 48 B = 16 lanes x 16 whole pixels
static_assert(kThreads == 16 * 64, "16 column groups x 64 row groups");
constexpr int kPasses = kSide / 64;             // rows per thread
constexpr int kThreshold = 250;                 // utils.py:15
// LDS pitches in dwords, chosen so that the 16-byte reads of phase 2 spread over all banks: column-count records of 64 row groups (+4),
// row records of 16 column groups (+4).
constexpr int kColPitch = 68, kRowPitch = 20;

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[12], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// centre_of_mass (vision_device.hpp) for the kernels of this unit, whose trial is the workgroup: [T][2 n_colours] noise and features, [T][n_colours] masks
__device__ __forceinline__ void centre_of_mass_of_block(int cc, int rc, int n_colours, const double *__restrict__ noise, double *__restrict__ f_out,
                                                        int32_t *__restrict__ pixels_out) {
    const int64_t o = static_cast<int64_t>(blockIdx.x) * (2 * n_colours);
    centre_of_mass(cc, rc, n_colours, noise != nullptr ? noise + o : nullptr, f_out + o,
                   pixels_out != nullptr ? pixels_out + static_cast<int64_t>(blockIdx.x) * n_colours : nullptr);
}

__global__ __launch_bounds__(kThreads) void detect_circles_kernel(const uint8_t *__restrict__ frames, int64_t frame_stride, int n_colours,
                                                                  const double *__restrict__ noise, double *__restrict__ f_out,
                                                                  int32_t *__restrict__ pixels_out) {
    // colcnt[colour][half][column group][row group]: eight 4-bit counters per dword, pixel p of the thread's 16 in dword p >> 3, nibble p & 7
    __shared__ __attribute__((aligned(16))) uint32_t colcnt[kColours * 2 * 16 * kColPitch];
    // rowcnt[flipped row][column group]: the four colours' counts (<= 16 each) in the four bytes
    __shared__ __attribute__((aligned(16))) uint32_t rowcnt[kSide * kRowPitch];

    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    const uint8_t *frame = frames + static_cast<int64_t>(blockIdx.x) * frame_stride;

    uint4 w[kPasses][3];
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const uint4 *src = reinterpret_cast<const uint4 *>(frame + (j * 64 + rg) * kRowBytes + cg * 48);
        w[j][0] = src[0];
        w[j][1] = src[1];
        w[j][2] = src[2];
    }

    uint32_t cnt[kColours][2] = {};
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const uint32_t d[12] = {w[j][0].x, w[j][0].y, w[j][0].z, w[j][0].w, w[j][1].x, w[j][1].y, w[j][1].z, w[j][1].w,
                                w[j][2].x, w[j][2].y, w[j][2].z, w[j][2].w};
        uint32_t m[kColours][2] = {};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const uint32_t r = byte_of(d, 3 * p), g = byte_of(d, 3 * p + 1), b = byte_of(d, 3 * p + 2);
            const bool ra = r > kThreshold, rb = r < kThreshold, ga = g > kThreshold, gb = g < kThreshold, ba = b > kThreshold, bb = b < kThreshold;
            const uint32_t bit = 1u << (4 * (p & 7));
            m[0][p >> 3] |= (ra && gb && bb) ? bit : 0u;         // red   (utils.py:130-132)
            m[1][p >> 3] |= (rb && ga && bb) ? bit : 0u;         // green (:134-136)
            m[2][p >> 3] |= (rb && gb && ba) ? bit : 0u;         // blue  (:138-140)
            m[3][p >> 3] |= (ra && gb && ba) ? bit : 0u;         // pink  (:142-144)
        }
        uint32_t packed = 0;
#pragma unroll
        for (int c = 0; c < kColours; ++c) {
            packed |= static_cast<uint32_t>(__popc(m[c][0]) + __popc(m[c][1])) << (8 * c);
            cnt[c][0] += m[c][0];                                // at most kPasses = 4 per nibble
            cnt[c][1] += m[c][1];
        }
        rowcnt[(kSide - 1 - (j * 64 + rg)) * kRowPitch + cg] = packed;   // cv2.flip(image, 0) (utils.py:13): row r of the sensor is row 255 - r
    }
#pragma unroll
    for (int c = 0; c < kColours; ++c) {
        colcnt[((c * 2 + 0) * 16 + cg) * kColPitch + rg] = cnt[c][0];
        colcnt[((c * 2 + 1) * 16 + cg) * kColPitch + rg] = cnt[c][1];
    }
    __syncthreads();

    // phase 2: thread (c, i) owns grid index i of colour c
    const int c = tid >> 8, i = tid & 255;
    int cc = 0, rc = 0;
    {
        const uint4 *q = reinterpret_cast<const uint4 *>(&colcnt[((c * 2 + ((i >> 3) & 1)) * 16 + (i >> 4)) * kColPitch]);
        const int sh = 4 * (i & 7);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint4 v = q[k];
            cc += static_cast<int>(((v.x >> sh) & 15u) + ((v.y >> sh) & 15u) + ((v.z >> sh) & 15u) + ((v.w >> sh) & 15u));
        }
        const uint4 *r = reinterpret_cast<const uint4 *>(&rowcnt[i * kRowPitch]);
        const int rs = 8 * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = r[k];
            rc += static_cast<int>(((v.x >> rs) & 255u) + ((v.y >> rs) & 255u) + ((v.z >> rs) & 255u) + ((v.w >> rs) & 255u));
        }
    }
    centre_of_mass_of_block(cc, rc, n_colours, noise, f_out, pixels_out);
}

// ---------------------------------------------------------------------------------------------------------------- synthetic camera
// colour word (R in the low byte) of disc k of n: red, green, blue, pink; the one disc of n == 1 is green
__device__ __forceinline__ uint32_t colour_word(int k, int n) {
    const int slot = n == 1 ? 1 : k;
    return slot == 0 ? 0x0000ffu : slot == 1 ? 0x00ff00u : slot == 2 ? 0xff0000u : 0xff00ffu;
}

// The occluder operand of the OCC flavours below: nothing at all in the kernels that always were
template <bool OCC>
struct OccluderArgs {};
template <>
struct OccluderArgs<true> {
    const uvs_occluder *occ;                                     // [T][n_occ]
    int n_occ, k;
    uint32_t shade;                                              // the rasteriser's
};
// the rectangles of this workgroup's trial at the launch's step
__device__ __forceinline__ Rects rects_of_block(const OccluderArgs<true> &oa) {
    Rects rects = occluder_rects(oa.occ + static_cast<int64_t>(blockIdx.x) * oa.n_occ, oa.n_occ, oa.k);
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) rects.r[o] = __builtin_amdgcn_readfirstlane(rects.r[o]);   // the same in every thread: scalar registers
    return rects;
}

template <bool OCC>
__global__ __launch_bounds__(kThreads) void render_discs_kernel(const double *__restrict__ discs, int n_colours, uint32_t background,
                                                                uint8_t *__restrict__ frames, int64_t frame_stride, const OccluderArgs<OCC> oa) {
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;                      // the detector's lane unit: 16 pixels = 48 B of row j * 64 + rg
    uint8_t *frame = frames + static_cast<int64_t>(blockIdx.x) * frame_stride;
    const double *mine = discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours);
    Disc d[kColours];
    int x0[kColours], x1[kColours], y0[kColours], y1[kColours];
#pragma unroll
    for (int k = 0; k < kColours; ++k) {
        d[k] = load_disc(mine + 3 * (k < n_colours ? k : 0), k < n_colours);
        disc_box(d[k], x0[k], x1[k], y0[k], y1[k]);
    }
    const uint32_t bg = background * 0x010101u;
    Rects rects;
    if constexpr (OCC) rects = rects_of_block(oa);
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const int row = j * 64 + rg, i = kSide - 1 - row;        // stored row, flipped row
        const double fi = static_cast<double>(i);
        double dy2[kColours];
        bool any = false;
#pragma unroll
        for (int k = 0; k < kColours; ++k) {
            const double dy = fi - d[k].v;
            dy2[k] = dy * dy;
            any = any || (d[k].r2 >= 0.0 && i >= y0[k] && i <= y1[k] && x0[k] <= 16 * cg + 15 && x1[k] >= 16 * cg);
        }
        if constexpr (OCC) any = any || rects_meet(rects, 16 * cg, 16 * cg + 15, i, i);   // a run an active rectangle meets is not skipped
        uint32_t px[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) px[p] = bg;
        if (any) {
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const double fj = static_cast<double>(16 * cg + p);
#pragma unroll
                for (int k = 0; k < kColours; ++k) {             // painter's order: a later disc overwrites an earlier one
                    const double dx = fj - d[k].u;
                    if (dx * dx + dy2[k] <= d[k].r2) px[p] = colour_word(k, n_colours);
                }
                if constexpr (OCC) {                             // a covered pixel belongs to no disc, whatever the painter's order
                    if (rects_cover(rects, 16 * cg + p, i)) px[p] = oa.shade * 0x010101u;
                }
            }
        }
        uint4 *dst = reinterpret_cast<uint4 *>(frame + row * kRowBytes + cg * 48);
#pragma unroll
        for (int g = 0; g < 3; ++g) {                            // 16 pixels of 3 bytes are three 16-byte stores; four pixels fill three dwords
            uint32_t w[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int e = 4 * g + h;                         // dword e of the twelve holds bytes 4 e .. 4 e + 3
                const int q = (4 * e) / 3, s = (4 * e) % 3;      // first pixel in it and the byte of that pixel it starts at
                w[h] = s == 0 ? (px[q] | (px[q + 1] << 24)) : s == 1 ? ((px[q] >> 8) | (px[q + 1] << 16)) : ((px[q] >> 16) | (px[q + 1] << 8));
            }
            dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

template <bool OCC>
__global__ __launch_bounds__(kThreads) void disc_features_kernel(const double *__restrict__ discs, int n_colours, const double *__restrict__ noise,
                                                                 double *__restrict__ f_out, int32_t *__restrict__ pixels_out,
                                                                 const OccluderArgs<OCC> oa) {
    int cc, rc;
    if constexpr (OCC)
        disc_counts<true>(discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours), n_colours, cc, rc, rects_of_block(oa));
    else
        disc_counts(discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours), n_colours, cc, rc);
    centre_of_mass_of_block(cc, rc, n_colours, noise, f_out, pixels_out);
}

constexpr int kProjectThreads = 64;

__global__ __launch_bounds__(kProjectThreads) void camera_project_kernel(const uvs_camera cam, int64_t T, const double *__restrict__ q_prev,
                                                                         const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                         double *__restrict__ discs_out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kProjectThreads + threadIdx.x;
    if (t >= T) return;
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    for (int i = 0; i < cam.n_joints; ++i) {
        double s, c;
        joint_sincos(cam, t, i, q_prev, dq, dt, q_out, s, c);
        chain_link(cam, i, s, c, pose);
    }
    for (int p = 0; p < cam.n_points; ++p) project_disc(cam, p, pose, discs_out + (t * cam.n_points + p) * 3);
}

// The loop's hot path: one workgroup per trial.  Lane i of the first wavefront takes joint i (the sincos calls, the long part of the chain,
// run side by side), the first n_points lanes then each multiply the links (lanes of one wavefront: the time of one) and project their own
// point into LDS; then every thread counts against those discs and the detector's phase 2 follows.  Same arithmetic on the same operands
// as camera_project_kernel, so the same bits.
template <bool OCC>
__global__ __launch_bounds__(kThreads) void camera_features_kernel(const uvs_camera cam, const double *__restrict__ q_prev,
                                                                   const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                   const double *__restrict__ noise, double *__restrict__ f_out,
                                                                   int32_t *__restrict__ pixels_out, double *__restrict__ discs_out,
                                                                   const OccluderArgs<OCC> oa) {
    __shared__ double sdisc[kColours * 3];
    __shared__ double ssin[UVS_CAMERA_MAX_JOINTS], scos[UVS_CAMERA_MAX_JOINTS];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    if (tid < cam.n_joints) joint_sincos(cam, t, tid, q_prev, dq, dt, q_out, ssin[tid], scos[tid]);
    __syncthreads();
    if (tid < cam.n_points) {
        double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        for (int i = 0; i < cam.n_joints; ++i) chain_link(cam, i, ssin[i], scos[i], pose);
        project_disc(cam, tid, pose, &sdisc[3 * tid]);
        if (discs_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) discs_out[(t * cam.n_points + tid) * 3 + k] = sdisc[3 * tid + k];
        }
    }
    __syncthreads();
    int cc, rc;
    if constexpr (OCC)
        disc_counts<true>(sdisc, cam.n_points, cc, rc, rects_of_block(oa));
    else
        disc_counts(sdisc, cam.n_points, cc, rc);
    centre_of_mass_of_block(cc, rc, cam.n_points, noise, f_out, pixels_out);
}

// ---------------------------------------------------------------------------------------------------------------- painted occluders
// The three kernels above with PAINTED rectangles (vision_device.hpp): kernels of their own names and texts, so that the six above keep
// their code and their resource figures; what they compute with is the shared device functions.
struct PaintArgs {
    OccluderArgs<true> oa;
    const int32_t *paint;                                        // [T][n_occ] or NULL: every rectangle opaque
};
// the paints of this workgroup's trial, in scalar registers like its rectangles
__device__ __forceinline__ uint32_t paints_of_block(const PaintArgs &pa, int n_colours) {
    const int32_t *mine = pa.paint != nullptr ? pa.paint + static_cast<int64_t>(blockIdx.x) * pa.oa.n_occ : nullptr;
    return __builtin_amdgcn_readfirstlane(occluder_paints(mine, pa.oa.n_occ, n_colours));
}
// colour word of a slot (colour_word's, without the n == 1 mapping that paint_slot has already made)
__device__ __forceinline__ uint32_t slot_word(uint32_t slot) { return colour_word(static_cast<int>(slot), kColours); }

// render_discs_kernel<true>'s lane unit and skips; then the rectangles in index order, a later one in front: painted ones in their colour
__global__ __launch_bounds__(kThreads) void paint_frames_kernel(const double *__restrict__ discs, int n_colours, uint32_t background,
                                                                uint8_t *__restrict__ frames, int64_t frame_stride, const PaintArgs pa) {
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    uint8_t *frame = frames + static_cast<int64_t>(blockIdx.x) * frame_stride;
    const double *mine = discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours);
    Disc d[kColours];
    int x0[kColours], x1[kColours], y0[kColours], y1[kColours];
#pragma unroll
    for (int k = 0; k < kColours; ++k) {
        d[k] = load_disc(mine + 3 * (k < n_colours ? k : 0), k < n_colours);
        disc_box(d[k], x0[k], x1[k], y0[k], y1[k]);
    }
    const uint32_t bg = background * 0x010101u;
    const Rects rects = rects_of_block(pa.oa);
    const uint32_t paints = paints_of_block(pa, n_colours);
    uint32_t ink[kOccluders];                                    // what each rectangle shows
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) ink[o] = paint_of(paints, o) == kOpaque ? pa.oa.shade * 0x010101u : slot_word(paint_of(paints, o));
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const int row = j * 64 + rg, i = kSide - 1 - row;        // stored row, flipped row
        const double fi = static_cast<double>(i);
        double dy2[kColours];
        bool any = rects_meet(rects, 16 * cg, 16 * cg + 15, i, i);
#pragma unroll
        for (int k = 0; k < kColours; ++k) {
            const double dy = fi - d[k].v;
            dy2[k] = dy * dy;
            any = any || (d[k].r2 >= 0.0 && i >= y0[k] && i <= y1[k] && x0[k] <= 16 * cg + 15 && x1[k] >= 16 * cg);
        }
        const LineCover cover(rects, i, true);                   // the columns each rectangle covers of this row
        uint32_t px[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) px[p] = bg;
        if (any) {
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int x = 16 * cg + p;
                const double fj = static_cast<double>(x);
#pragma unroll
                for (int k = 0; k < kColours; ++k) {             // painter's order among the discs
                    const double dx = fj - d[k].u;
                    if (dx * dx + dy2[k] <= d[k].r2) px[p] = colour_word(k, n_colours);
                }
#pragma unroll
                for (int o = 0; o < kOccluders; ++o)             // then among the rectangles: the highest index that holds the pixel owns it
                    if (x >= cover.lo[o] && x <= cover.hi[o]) px[p] = ink[o];
            }
        }
        uint4 *dst = reinterpret_cast<uint4 *>(frame + row * kRowBytes + cg * 48);
#pragma unroll
        for (int g = 0; g < 3; ++g) {                            // render_discs_kernel's three 16-byte stores
            uint32_t w[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int e = 4 * g + h;
                const int q = (4 * e) / 3, s = (4 * e) % 3;
                w[h] = s == 0 ? (px[q] | (px[q + 1] << 24)) : s == 1 ? ((px[q] >> 8) | (px[q + 1] << 16)) : ((px[q] >> 16) | (px[q + 1] << 8));
            }
            dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

__global__ __launch_bounds__(kThreads) void paint_detect_kernel(const double *__restrict__ discs, int n_colours, const double *__restrict__ noise,
                                                                double *__restrict__ f_out, int32_t *__restrict__ pixels_out, const PaintArgs pa) {
    int cc, rc;
    painted_counts(discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours), n_colours, cc, rc, rects_of_block(pa.oa), paints_of_block(pa, n_colours));
    centre_of_mass_of_block(cc, rc, n_colours, noise, f_out, pixels_out);
}

// camera_features_kernel's joints and projection, on the same operands in the same order, then the painted counts
__global__ __launch_bounds__(kThreads) void paint_camera_detect_kernel(const uvs_camera cam, const double *__restrict__ q_prev,
                                                                       const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                       const double *__restrict__ noise, double *__restrict__ f_out,
                                                                       int32_t *__restrict__ pixels_out, double *__restrict__ discs_out,
                                                                       const PaintArgs pa) {
    __shared__ double sdisc[kColours * 3];
    __shared__ double ssin[UVS_CAMERA_MAX_JOINTS], scos[UVS_CAMERA_MAX_JOINTS];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    if (tid < cam.n_joints) joint_sincos(cam, t, tid, q_prev, dq, dt, q_out, ssin[tid], scos[tid]);
    __syncthreads();
    if (tid < cam.n_points) {
        double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        for (int i = 0; i < cam.n_joints; ++i) chain_link(cam, i, ssin[i], scos[i], pose);
        project_disc(cam, tid, pose, &sdisc[3 * tid]);
        if (discs_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) discs_out[(t * cam.n_points + tid) * 3 + k] = sdisc[3 * tid + k];
        }
    }
    __syncthreads();
    int cc, rc;
    painted_counts(sdisc, cam.n_points, cc, rc, rects_of_block(pa.oa), paints_of_block(pa, cam.n_points));
    centre_of_mass_of_block(cc, rc, cam.n_points, noise, f_out, pixels_out);
}

// ---------------------------------------------------------------------------------------------------------------- a scene per trial
// camera_project_kernel and paint_camera_detect_kernel with the camera of THEIR trial, read from memory where a value is used (DESIGN.md
// 4.22): kernels of their own names and texts, so that the ones above keep their code and their resource figures.  The arithmetic is the
// shared device functions' on the same operands in the same order, so trial t has the bits of the call with cam = its scene.  The shape is
// the launch's (six joints, n_points), never a struct's; a trial whose index names no scene reads none and stores nothing.
__global__ __launch_bounds__(kProjectThreads) void scene_project_kernel(const Scenes S, int n_points, int64_t T, const double *__restrict__ q_prev,
                                                                        const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                        double *__restrict__ discs_out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kProjectThreads + threadIdx.x;
    if (t >= T) return;
    const long long scene = model_of(S, t);
    if (scene < 0) return;
    const uvs_camera &cam = S.models[scene];
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    for (int i = 0; i < kSceneJoints; ++i) {
        double s, c;
        scene_joint_sincos(cam, t, i, q_prev, dq, dt, q_out, s, c);
        chain_link(cam, i, s, c, pose);
    }
    for (int p = 0; p < n_points; ++p) project_disc(cam, p, pose, discs_out + (t * n_points + p) * 3);
}

__global__ __launch_bounds__(kThreads) void scene_camera_detect_kernel(const Scenes S, int n_points, const double *__restrict__ q_prev,
                                                                       const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                       const double *__restrict__ noise, double *__restrict__ f_out,
                                                                       int32_t *__restrict__ pixels_out, double *__restrict__ discs_out,
                                                                       const PaintArgs pa) {
    __shared__ double sdisc[kColours * 3];
    __shared__ double ssin[UVS_CAMERA_MAX_JOINTS], scos[UVS_CAMERA_MAX_JOINTS];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const long long scene = model_of(S, t);                      // the same word in all 1024 threads: the workgroup leaves as one
    if (scene < 0) return;
    const uvs_camera &cam = S.models[scene];
    if (tid < kSceneJoints) scene_joint_sincos(cam, t, tid, q_prev, dq, dt, q_out, ssin[tid], scos[tid]);
    __syncthreads();
    if (tid < n_points) {
        double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        for (int i = 0; i < kSceneJoints; ++i) chain_link(cam, i, ssin[i], scos[i], pose);
        project_disc(cam, tid, pose, &sdisc[3 * tid]);
        if (discs_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) discs_out[(t * n_points + tid) * 3 + k] = sdisc[3 * tid + k];
        }
    }
    __syncthreads();
    int cc, rc;
    painted_counts(sdisc, n_points, cc, rc, rects_of_block(pa.oa), paints_of_block(pa, n_points));
    centre_of_mass_of_block(cc, rc, n_points, noise, f_out, pixels_out);
}

// The two kernels above on MOVING targets: every disc projected where step k of its trial's motion has taken it
// (project_moved_disc: the rule of uvs_target_motion).  motion [T] by trial, or NULL: nothing moves, and the bits are those of the kernels above.
__global__ __launch_bounds__(kProjectThreads) void moving_project_kernel(const Scenes S, const uvs_target_motion *__restrict__ motion, int n_points,
                                                                         int64_t T, const double *__restrict__ q_prev,
                                                                         const double *__restrict__ dq, double dt, int k,
                                                                         double *__restrict__ q_out, double *__restrict__ discs_out) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kProjectThreads + threadIdx.x;
    if (t >= T) return;
    const long long scene = model_of(S, t);
    if (scene < 0) return;
    const uvs_camera &cam = S.models[scene];
    const uvs_target_motion *mot = motion != nullptr ? motion + t : nullptr;
    double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    for (int i = 0; i < kSceneJoints; ++i) {
        double s, c;
        scene_joint_sincos(cam, t, i, q_prev, dq, dt, q_out, s, c);
        chain_link(cam, i, s, c, pose);
    }
    for (int p = 0; p < n_points; ++p) project_moved_disc_of(cam, p, mot, k, pose, discs_out + (t * n_points + p) * 3);
}

__global__ __launch_bounds__(kThreads) void moving_detect_kernel(const Scenes S, const uvs_target_motion *__restrict__ motion, int n_points,
                                                                 const double *__restrict__ q_prev, const double *__restrict__ dq, double dt,
                                                                 double *__restrict__ q_out, const double *__restrict__ noise,
                                                                 double *__restrict__ f_out, int32_t *__restrict__ pixels_out,
                                                                 double *__restrict__ discs_out, const PaintArgs pa) {
    __shared__ double sdisc[kColours * 3];
    __shared__ double ssin[UVS_CAMERA_MAX_JOINTS], scos[UVS_CAMERA_MAX_JOINTS];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const long long scene = model_of(S, t);                      // the same word in all 1024 threads: the workgroup leaves as one
    if (scene < 0) return;
    const uvs_camera &cam = S.models[scene];
    if (tid < kSceneJoints) scene_joint_sincos(cam, t, tid, q_prev, dq, dt, q_out, ssin[tid], scos[tid]);
    __syncthreads();
    if (tid < n_points) {
        const uvs_target_motion *mot = motion != nullptr ? motion + t : nullptr;
        double pose[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
        for (int i = 0; i < kSceneJoints; ++i) chain_link(cam, i, ssin[i], scos[i], pose);
        project_moved_disc_of(cam, tid, mot, pa.oa.k, pose, &sdisc[3 * tid]);
        if (discs_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) discs_out[(t * n_points + tid) * 3 + k] = sdisc[3 * tid + k];
        }
    }
    __syncthreads();
    int cc, rc;
    painted_counts(sdisc, n_points, cc, rc, rects_of_block(pa.oa), paints_of_block(pa, n_points));
    centre_of_mass_of_block(cc, rc, n_points, noise, f_out, pixels_out);
}

thread_local char g_err[256] = "";

int fail(int code, const char *fmt, const char *detail) {
    std::snprintf(g_err, sizeof g_err, fmt, detail);
    return code;
}

bool colours_ok(int32_t n) { return n == 1 || n == 3 || n == 4; }

int check_camera(const uvs_camera *cam, int64_t T, const double *q_prev, const double *q_out) {
    if (cam == nullptr || q_prev == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL cam or q_prev");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (cam->n_joints < 1 || cam->n_joints > UVS_CAMERA_MAX_JOINTS) return fail(UVS_ERR_ARG, "%s", "n_joints must be 1 .. 8");
    if (!colours_ok(cam->n_points)) return fail(UVS_ERR_ARG, "%s", "n_points must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (q_out != nullptr) {                                      // every trial reads its own row only, but the contract is the simple one
        const uintptr_t a = reinterpret_cast<uintptr_t>(q_prev), b = reinterpret_cast<uintptr_t>(q_out);
        const uintptr_t bytes = static_cast<uintptr_t>(T > 0 ? T : 1) * cam->n_joints * sizeof(double);
        if (a < b + bytes && b < a + bytes) return fail(UVS_ERR_ARG, "%s", "q_out overlaps q_prev");
    }
    return UVS_OK;
}

int check_occluders(const uvs_occluder *occ, int32_t n_occ) {
    if (n_occ < 0 || n_occ > UVS_CAMERA_MAX_OCCLUDERS) return fail(UVS_ERR_ARG, "%s", "n_occ must be 0 .. 4");
    if (occ == nullptr && n_occ > 0) return fail(UVS_ERR_ARG, "%s", "NULL occ with n_occ > 0");
    return UVS_OK;
}

int check_scenes(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int64_t T) {
    if (cams == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL cams");
    if (n_cams < 1 || n_cams > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "n_cams must be 1 .. 2^31 - 1");
    if (cam_index == nullptr && n_cams != 1 && n_cams != T) return fail(UVS_ERR_ARG, "%s", "without cam_index, n_cams must be 1 or T");
    return UVS_OK;
}

uvs_camera scene_shape(int32_t n_joints, int32_t n_points) {
    uvs_camera shape{};
    shape.n_joints = n_joints;
    shape.n_points = n_points;
    return shape;
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UVS_ERR_HIP, what, hipGetErrorString(e));
    return UVS_OK;
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

const char *uvs_vision_version(void) { return "uvs_vision 0.2.0 (gfx950, uint8 frames, fp64 features, synthetic camera)"; }
const char *uvs_vision_last_error(void) { return g_err; }

int uvs_detect_circles_u8(int64_t T, const uint8_t *frames, int64_t frame_stride_bytes, int32_t height, int32_t width, int32_t n_colours,
                          const double *noise, double *f_out, int32_t *pixels_out, void *stream) {
    g_err[0] = '\0';
    if (frames == nullptr || f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL frames or f_out");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (n_colours != 1 && n_colours != 3 && n_colours != 4) return fail(UVS_ERR_ARG, "%s", "n_colours must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (height < 1 || width < 1) return fail(UVS_ERR_ARG, "%s", "height and width must be positive");
    if (frame_stride_bytes < static_cast<int64_t>(height) * width * 3) return fail(UVS_ERR_ARG, "%s", "frame stride below height * width * 3");
    if (frame_stride_bytes % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frame stride must be a multiple of 16 bytes");
    if (reinterpret_cast<uintptr_t>(frames) % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frames must be 16-byte aligned");
    if (height != kSide || width != kSide) return fail(UVS_ERR_SHAPE, "%s", "frames must be 256 x 256 (utils.py:7-9 fixes the pixel grid)");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(detect_circles_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), frames,
                       frame_stride_bytes, static_cast<int>(n_colours), noise, f_out, pixels_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(UVS_ERR_HIP, "detect_circles_kernel launch: %s", hipGetErrorString(e));
    return UVS_OK;
}

int uvs_camera_project_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out, double *discs_out,
                           void *stream) {
    g_err[0] = '\0';
    if (discs_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs_out");
    if (const int rc = check_camera(cam, T, q_prev, q_out)) return rc;
    if (T == 0) return UVS_OK;
    const unsigned blocks = static_cast<unsigned>((T + kProjectThreads - 1) / kProjectThreads);
    hipLaunchKernelGGL(camera_project_kernel, dim3(blocks), dim3(kProjectThreads), 0, static_cast<hipStream_t>(stream), *cam, T, q_prev, dq, dt,
                       q_out, discs_out);
    return launched("camera_project_kernel launch: %s");
}

static int check_render(int64_t T, const double *discs, int32_t n_colours, int32_t background, const uint8_t *frames, int64_t frame_stride_bytes) {
    if (discs == nullptr || frames == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs or frames");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_colours)) return fail(UVS_ERR_ARG, "%s", "n_colours must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (background < 0 || background >= kThreshold) return fail(UVS_ERR_ARG, "%s", "background must be 0 .. 249 (250 and above would enter a mask)");
    if (frame_stride_bytes < static_cast<int64_t>(kSide) * kRowBytes) return fail(UVS_ERR_ARG, "%s", "frame stride below 256 * 256 * 3");
    if (frame_stride_bytes % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frame stride must be a multiple of 16 bytes");
    if (reinterpret_cast<uintptr_t>(frames) % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frames must be 16-byte aligned");
    return UVS_OK;
}

int uvs_render_discs_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, uint8_t *frames, int64_t frame_stride_bytes,
                        void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_render(T, discs, n_colours, background, frames, frame_stride_bytes)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(render_discs_kernel<false>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), static_cast<uint32_t>(background), frames, frame_stride_bytes, OccluderArgs<false>{});
    return launched("render_discs_kernel launch: %s");
}

int uvs_render_discs_occluded_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, const uvs_occluder *occ, int32_t n_occ,
                                 int32_t k, int32_t shade, uint8_t *frames, int64_t frame_stride_bytes, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_render(T, discs, n_colours, background, frames, frame_stride_bytes)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (shade < 0 || shade >= kThreshold) return fail(UVS_ERR_ARG, "%s", "shade must be 0 .. 249 (250 and above would enter a mask)");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(render_discs_kernel<true>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), static_cast<uint32_t>(background), frames, frame_stride_bytes,
                       OccluderArgs<true>{occ, n_occ, k, static_cast<uint32_t>(shade)});
    return launched("render_discs_kernel<occluded> launch: %s");
}

static int check_disc_features(int64_t T, const double *discs, int32_t n_colours, const double *f_out) {
    if (discs == nullptr || f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs or f_out");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_colours)) return fail(UVS_ERR_ARG, "%s", "n_colours must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    return UVS_OK;
}

int uvs_disc_features_f64(int64_t T, const double *discs, int32_t n_colours, const double *noise, double *f_out, int32_t *pixels_out,
                          void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_disc_features(T, discs, n_colours, f_out)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(disc_features_kernel<false>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), noise, f_out, pixels_out, OccluderArgs<false>{});
    return launched("disc_features_kernel launch: %s");
}

int uvs_disc_features_occluded_f64(int64_t T, const double *discs, int32_t n_colours, const uvs_occluder *occ, int32_t n_occ, int32_t k,
                                   const double *noise, double *f_out, int32_t *pixels_out, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_disc_features(T, discs, n_colours, f_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(disc_features_kernel<true>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), noise, f_out, pixels_out, OccluderArgs<true>{occ, n_occ, k, 0u});
    return launched("disc_features_kernel<occluded> launch: %s");
}

int uvs_camera_features_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                            const double *noise, double *f_out, int32_t *pixels_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    if (const int rc = check_camera(cam, T, q_prev, q_out)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(camera_features_kernel<false>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), *cam,
                       q_prev, dq, dt, q_out, noise, f_out, pixels_out, discs_out, OccluderArgs<false>{});
    return launched("camera_features_kernel launch: %s");
}

int uvs_camera_features_occluded_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                     const uvs_occluder *occ, int32_t n_occ, int32_t k, const double *noise, double *f_out,
                                     int32_t *pixels_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    if (const int rc = check_camera(cam, T, q_prev, q_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(camera_features_kernel<true>, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), *cam,
                       q_prev, dq, dt, q_out, noise, f_out, pixels_out, discs_out, OccluderArgs<true>{occ, n_occ, k, 0u});
    return launched("camera_features_kernel<occluded> launch: %s");
}

// The three occluded entry points with `paint` after `occ`: their refusals, in their order; a NULL paint is legal (every rectangle opaque)
int uvs_render_discs_painted_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, const uvs_occluder *occ,
                                const int32_t *paint, int32_t n_occ, int32_t k, int32_t shade, uint8_t *frames, int64_t frame_stride_bytes,
                                void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_render(T, discs, n_colours, background, frames, frame_stride_bytes)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (shade < 0 || shade >= kThreshold) return fail(UVS_ERR_ARG, "%s", "shade must be 0 .. 249 (250 and above would enter a mask)");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(paint_frames_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), static_cast<uint32_t>(background), frames, frame_stride_bytes,
                       PaintArgs{{occ, n_occ, k, static_cast<uint32_t>(shade)}, paint});
    return launched("paint_frames_kernel launch: %s");
}

int uvs_disc_features_painted_f64(int64_t T, const double *discs, int32_t n_colours, const uvs_occluder *occ, const int32_t *paint, int32_t n_occ,
                                  int32_t k, const double *noise, double *f_out, int32_t *pixels_out, void *stream) {
    g_err[0] = '\0';
    if (const int rc = check_disc_features(T, discs, n_colours, f_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(paint_detect_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), noise, f_out, pixels_out, PaintArgs{{occ, n_occ, k, 0u}, paint});
    return launched("paint_detect_kernel launch: %s");
}

int uvs_camera_features_painted_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                    const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t k, const double *noise,
                                    double *f_out, int32_t *pixels_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    if (const int rc = check_camera(cam, T, q_prev, q_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(paint_camera_detect_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), *cam,
                       q_prev, dq, dt, q_out, noise, f_out, pixels_out, discs_out, PaintArgs{{occ, n_occ, k, 0u}, paint});
    return launched("paint_camera_detect_kernel launch: %s");
}

// The scene per trial: the namesakes' refusals in their order on the launch's shape (six joints, n_points), then the triple's
int uvs_camera_project_scenes_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int32_t n_points, int64_t T,
                                  const double *q_prev, const double *dq, double dt, double *q_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (discs_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs_out");
    const uvs_camera shape = scene_shape(kSceneJoints, n_points);
    if (const int rc = check_camera(&shape, T, q_prev, q_out)) return rc;
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0) return UVS_OK;
    const unsigned blocks = static_cast<unsigned>((T + kProjectThreads - 1) / kProjectThreads);
    hipLaunchKernelGGL(scene_project_kernel, dim3(blocks), dim3(kProjectThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, static_cast<int>(n_points), T, q_prev, dq, dt, q_out, discs_out);
    return launched("scene_project_kernel launch: %s");
}

int uvs_camera_features_scenes_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int32_t n_points, int64_t T,
                                   const double *q_prev, const double *dq, double dt, double *q_out, const uvs_occluder *occ,
                                   const int32_t *paint, int32_t n_occ, int32_t k, const double *noise, double *f_out, int32_t *pixels_out,
                                   double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    const uvs_camera shape = scene_shape(kSceneJoints, n_points);
    if (const int rc = check_camera(&shape, T, q_prev, q_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(scene_camera_detect_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, static_cast<int>(n_points), q_prev, dq, dt, q_out, noise, f_out, pixels_out, discs_out,
                       PaintArgs{{occ, n_occ, k, 0u}, paint});
    return launched("scene_camera_detect_kernel launch: %s");
}

// Moving targets: the scenes namesakes' refusals in their order; a NULL motion is legal (nothing moves).  The project call has a k of its own.
int uvs_camera_project_moving_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                  int32_t n_points, int64_t T, const double *q_prev, const double *dq, double dt, int32_t k, double *q_out,
                                  double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (discs_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs_out");
    const uvs_camera shape = scene_shape(kSceneJoints, n_points);
    if (const int rc = check_camera(&shape, T, q_prev, q_out)) return rc;
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (T == 0) return UVS_OK;
    const unsigned blocks = static_cast<unsigned>((T + kProjectThreads - 1) / kProjectThreads);
    hipLaunchKernelGGL(moving_project_kernel, dim3(blocks), dim3(kProjectThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, motion, static_cast<int>(n_points), T, q_prev, dq, dt, static_cast<int>(k), q_out,
                       discs_out);
    return launched("moving_project_kernel launch: %s");
}

int uvs_camera_features_moving_f64(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, const uvs_target_motion *motion,
                                   int32_t n_points, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                                   const uvs_occluder *occ, const int32_t *paint, int32_t n_occ, int32_t k, const double *noise,
                                   double *f_out, int32_t *pixels_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    const uvs_camera shape = scene_shape(kSceneJoints, n_points);
    if (const int rc = check_camera(&shape, T, q_prev, q_out)) return rc;
    if (const int rc = check_occluders(occ, n_occ)) return rc;
    if (k < 0) return fail(UVS_ERR_ARG, "%s", "k must be >= 0");
    if (const int rc = check_scenes(cams, n_cams, cam_index, T)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(moving_detect_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       Scenes{cams, n_cams, cam_index}, motion, static_cast<int>(n_points), q_prev, dq, dt, q_out, noise, f_out, pixels_out,
                       discs_out, PaintArgs{{occ, n_occ, k, 0u}, paint});
    return launched("moving_detect_kernel launch: %s");
}

}  // extern "C"
