// libuvs_vision.so: centre-of-mass circle detectors of the live route (utils.py:11-166 of the reference) as one HIP kernel for gfx950.
// One workgroup of 1024 threads per 256x256 RGB frame.  Phase 1 reads the frame with 16-byte loads (16 lanes x 48 B per row, 64 rows per
// pass, all 12 loads of a thread issued before the first use), thresholds in integers and leaves integer counts in LDS; phase 2 gives
// every (colour, grid index) its own thread, which sums the column and the flipped-row count, multiplies by the grid product in fp64 and
// joins a wavefront reduction.  Nothing is atomic and no sum depends on timing: the same frame gives the same bits in every launch.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "uvs_vision.h"

namespace uvs_vision {

constexpr int kSide = UVS_VISION_SIDE;          // rows = columns = grid points (utils.py:7-9)
constexpr int kRowBytes = kSide * 3;            // 768 B = 16 lanes x 48 B = 16 lanes x 16 whole pixels
constexpr int kThreads = 1024;                  // 16 column groups x 64 row groups
constexpr int kPasses = kSide / 64;             // rows per thread
constexpr int kThreshold = 250;                 // utils.py:15
// LDS pitches in dwords, chosen so that the 16-byte reads of phase 2 spread over all banks: column-count records of 64 row groups (+4),
// row records of 16 column groups (+4).
constexpr int kColPitch = 68, kRowPitch = 20;
constexpr int kColours = 4;                     // red, green, blue, pink (utils.py:126-166)

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[12], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// p[i] = fl(g[i] * 255.0) with g = np.linspace(0, 1, 256): g[i] = fl(i * fl(1/255)), g[255] = 1.0 (the endpoint is assigned, not computed)
__device__ __forceinline__ double grid_product(int i) {
    const double step = 1.0 / 255.0;
    const double g = i < kSide - 1 ? static_cast<double>(i) * step : 1.0;
    return g * 255.0;
}

__global__ __launch_bounds__(kThreads) void detect_circles_kernel(const uint8_t *__restrict__ frames, int64_t frame_stride, int n_colours,
                                                                  const double *__restrict__ noise, double *__restrict__ f_out,
                                                                  int32_t *__restrict__ pixels_out) {
    // colcnt[colour][half][column group][row group]: eight 4-bit counters per dword, pixel p of the thread's 16 in dword p >> 3, nibble p & 7
    __shared__ __attribute__((aligned(16))) uint32_t colcnt[kColours * 2 * 16 * kColPitch];
    // rowcnt[flipped row][column group]: the four colours' counts (<= 16 each) in the four bytes
    __shared__ __attribute__((aligned(16))) uint32_t rowcnt[kSide * kRowPitch];
    __shared__ double part_u[kThreads / 64], part_v[kThreads / 64];
    __shared__ int part_n[kThreads / 64];

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
    const double p = grid_product(i);
    double su = static_cast<double>(cc) * p, sv = static_cast<double>(rc) * p;   // X * mask, Y * mask (utils.py:25-27), summed by count
    int n = cc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                     // a wavefront holds one colour: 64 consecutive grid indices
        su += __shfl_down(su, off, 64);
        sv += __shfl_down(sv, off, 64);
        n += __shfl_down(n, off, 64);
    }
    if ((tid & 63) == 0) {
        part_u[tid >> 6] = su;
        part_v[tid >> 6] = sv;
        part_n[tid >> 6] = n;
    }
    __syncthreads();

    if (tid < n_colours) {
        const int colour = n_colours == 1 ? 1 : tid;             // detectGreenCircle: green alone
        double s_u = 0.0, s_v = 0.0;
        int count = 0;
        for (int k = 0; k < 4; ++k) {
            s_u += part_u[4 * colour + k];
            s_v += part_v[4 * colour + k];
            count += part_n[4 * colour + k];
        }
        const double total = static_cast<double>(255 * count);   // np.sum of the uint8 mask of 255s (utils.py:26)
        double u = (255.0 * s_u) / total, v = (255.0 * s_v) / total;   // 0.0 / 0.0 = NaN for an empty mask, like the reference
        const int64_t o = static_cast<int64_t>(blockIdx.x) * (2 * n_colours) + 2 * tid;
        if (noise != nullptr) {                                  // f += noise (experiment.py:135)
            u += noise[o];
            v += noise[o + 1];
        }
        f_out[o] = u;
        f_out[o + 1] = v;
        if (pixels_out != nullptr) pixels_out[static_cast<int64_t>(blockIdx.x) * n_colours + tid] = count;
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char *fmt, const char *detail = "") {
    std::snprintf(g_err, sizeof g_err, fmt, detail);
    return code;
}

}  // namespace uvs_vision

using namespace uvs_vision;

extern "C" {

const char *uvs_vision_version(void) { return "uvs_vision 0.1.0 (gfx950, uint8 frames, fp64 features)"; }
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

}  // extern "C"
