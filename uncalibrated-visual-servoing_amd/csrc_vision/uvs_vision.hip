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

// Phase 2 of every detector here, from the integer counts on: thread (colour tid >> 8, grid index tid & 255) brings the number of mask pixels
// of its colour in column i (cc) and in flipped row i (rc).  The bits of the result depend on the order below, so the frame detector and the
// frame-free ones share this one function.  Called by all kThreads threads of the workgroup (it synchronises).
__device__ __forceinline__ void centre_of_mass(int cc, int rc, int n_colours, const double *__restrict__ noise, double *__restrict__ f_out,
                                               int32_t *__restrict__ pixels_out) {
    __shared__ double part_u[kThreads / 64], part_v[kThreads / 64];
    __shared__ int part_n[kThreads / 64];
    const int tid = threadIdx.x;
    const int i = tid & 255;
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
    centre_of_mass(cc, rc, n_colours, noise, f_out, pixels_out);
}

// ---------------------------------------------------------------------------------------------------------------- synthetic camera
// A disc as the kernels hold it: centre, and r2 = fl(r * r) -- or -1 for a disc that draws nothing (r < 0, NaN r, or no such disc), which no
// squared distance is below.  The pixel rule of the header is `dx2 + dy2 <= r2` with each square rounded once (-ffp-contract=off).
struct Disc {
    double u, v, r, r2;
};

__device__ __forceinline__ Disc load_disc(const double *d, bool present) {
    Disc o;
    o.u = present ? d[0] : 0.0;
    o.v = present ? d[1] : 0.0;
    o.r = present ? d[2] : -1.0;
    o.r2 = o.r >= 0.0 ? o.r * o.r : -1.0;
    return o;
}

// Inclusive pixel range [lo, hi] of [centre - r - 1, centre + r + 1] clipped to the frame: conservative against the exact rule by a whole
// pixel.  fmax / fmin drop a NaN operand, so a bound that is NaN (inf - inf) becomes the frame edge, never an unconverted NaN.
__device__ __forceinline__ void pixel_range(double centre, double r, int &lo, int &hi) {
    lo = static_cast<int>(fmin(fmax(ceil(centre - r - 1.0), 0.0), static_cast<double>(kSide)));
    hi = static_cast<int>(fmax(fmin(floor(centre + r + 1.0), static_cast<double>(kSide - 1)), -1.0));
}

// colour word (R in the low byte) of disc k of n: red, green, blue, pink; the one disc of n == 1 is green
__device__ __forceinline__ uint32_t colour_word(int k, int n) {
    const int slot = n == 1 ? 1 : k;
    return slot == 0 ? 0x0000ffu : slot == 1 ? 0x00ff00u : slot == 2 ? 0xff0000u : 0xff00ffu;
}

__global__ __launch_bounds__(kThreads) void render_discs_kernel(const double *__restrict__ discs, int n_colours, uint32_t background,
                                                                uint8_t *__restrict__ frames, int64_t frame_stride) {
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;                      // the detector's lane unit: 16 pixels = 48 B of row j * 64 + rg
    uint8_t *frame = frames + static_cast<int64_t>(blockIdx.x) * frame_stride;
    const double *mine = discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours);
    Disc d[kColours];
    int x0[kColours], x1[kColours], y0[kColours], y1[kColours];
#pragma unroll
    for (int k = 0; k < kColours; ++k) {
        d[k] = load_disc(mine + 3 * (k < n_colours ? k : 0), k < n_colours);
        pixel_range(d[k].u, d[k].r, x0[k], x1[k]);
        pixel_range(d[k].v, d[k].r, y0[k], y1[k]);
    }
    const uint32_t bg = background * 0x010101u;
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

// Counts of thread (colour c = tid >> 8, index i = tid & 255) for the frame the rasteriser above would write from the n_colours discs at
// `discs` (global memory or LDS): cc = rows at which c's disc is the topmost one in column i, rc = columns at which it is in flipped row i.
__device__ __forceinline__ void disc_counts(const double *discs, int n_colours, int &cc, int &rc) {
    const int c = threadIdx.x >> 8, i = threadIdx.x & 255;
    const int own = n_colours == 1 ? (c == 1 ? 0 : -1) : (c < n_colours ? c : -1);   // wavefront-uniform
    cc = 0;
    rc = 0;
    if (own < 0) return;
    const Disc me = load_disc(discs + 3 * own, true);
    if (!(me.r2 >= 0.0)) return;
    Disc over[kColours - 1];                                     // the discs painted after mine; absent ones never cover a pixel
#pragma unroll
    for (int k = 0; k < kColours - 1; ++k) {
        const int other = own + 1 + k;
        over[k] = load_disc(discs + 3 * (other < n_colours ? other : own), other < n_colours);
    }
    int x0, x1, y0, y1;
    pixel_range(me.u, me.r, x0, x1);
    pixel_range(me.v, me.r, y0, y1);
    const double fi = static_cast<double>(i);
    if (i >= x0 && i <= x1) {                                    // column i: walk the rows of the box
        const double dx = fi - me.u, dx2 = dx * dx;
        double ox2[kColours - 1];
#pragma unroll
        for (int k = 0; k < kColours - 1; ++k) {
            const double o = fi - over[k].u;
            ox2[k] = o * o;
        }
        for (int y = y0; y <= y1; ++y) {
            const double fy = static_cast<double>(y), dy = fy - me.v;
            bool top = dx2 + dy * dy <= me.r2;
#pragma unroll
            for (int k = 0; k < kColours - 1; ++k) {
                const double o = fy - over[k].v;
                top = top && !(ox2[k] + o * o <= over[k].r2);
            }
            cc += top ? 1 : 0;
        }
    }
    if (i >= y0 && i <= y1) {                                    // flipped row i: walk the columns of the box
        const double dy = fi - me.v, dy2 = dy * dy;
        double oy2[kColours - 1];
#pragma unroll
        for (int k = 0; k < kColours - 1; ++k) {
            const double o = fi - over[k].v;
            oy2[k] = o * o;
        }
        for (int x = x0; x <= x1; ++x) {
            const double fx = static_cast<double>(x), dx = fx - me.u;
            bool top = dx * dx + dy2 <= me.r2;
#pragma unroll
            for (int k = 0; k < kColours - 1; ++k) {
                const double o = fx - over[k].u;
                top = top && !(o * o + oy2[k] <= over[k].r2);
            }
            rc += top ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kThreads) void disc_features_kernel(const double *__restrict__ discs, int n_colours, const double *__restrict__ noise,
                                                                 double *__restrict__ f_out, int32_t *__restrict__ pixels_out) {
    int cc, rc;
    disc_counts(discs + static_cast<int64_t>(blockIdx.x) * (3 * n_colours), n_colours, cc, rc);
    centre_of_mass(cc, rc, n_colours, noise, f_out, pixels_out);
}

// Joint i of trial t -- q = q_prev + dq * dt when dq is given, written to q_out when that is given -- and the sine and cosine of its DH angle.
__device__ __forceinline__ void joint_sincos(const uvs_camera &cam, int64_t t, int i, const double *__restrict__ q_prev,
                                             const double *__restrict__ dq, double dt, double *__restrict__ q_out, double &s, double &c) {
    const int n = cam.n_joints;
    double q = q_prev[t * n + i];
    if (dq != nullptr) {
        const double step = dq[t * n + i] * dt;                  // one rounded multiply, then one rounded add
        q = q + step;
    }
    if (q_out != nullptr) q_out[t * n + i] = q;
    sincos(q + cam.theta_offset[i], &s, &c);
}

// One more link of the chain: T <- T * Rz(theta) Tz(d) Rx(alpha) Tx(a), summed left to right as a plain matrix product.
__device__ __forceinline__ void chain_link(const uvs_camera &cam, int i, double s, double c, double (&T)[3][4]) {
    const double ca = cam.cos_alpha[i], sa = cam.sin_alpha[i], aa = cam.a[i], dd = cam.d[i];
    const double l01 = -s * ca, l02 = s * sa, l03 = aa * c;
    const double l11 = c * ca, l12 = -c * sa, l13 = aa * s;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double t0 = T[r][0], t1 = T[r][1], t2 = T[r][2], t3 = T[r][3];
        T[r][0] = t0 * c + t1 * s;
        T[r][1] = t0 * l01 + t1 * l11 + t2 * sa;
        T[r][2] = t0 * l02 + t1 * l12 + t2 * ca;
        T[r][3] = t0 * l03 + t1 * l13 + t2 * dd + t3;
    }
}

// (u, v, r) of world point p seen from the camera pose T = [R | t]: pc = R^T (w - t); r = -1 for a point that is not in front of the camera
__device__ __forceinline__ void project_disc(const uvs_camera &cam, int p, const double (&T)[3][4], double *out) {
    const double dx = cam.points[p][0] - T[0][3], dy = cam.points[p][1] - T[1][3], dz = cam.points[p][2] - T[2][3];
    const double xc = T[0][0] * dx + T[1][0] * dy + T[2][0] * dz;
    const double yc = T[0][1] * dx + T[1][1] * dy + T[2][1] * dz;
    const double zc = T[0][2] * dx + T[1][2] * dy + T[2][2] * dz;
    out[0] = cam.center + cam.focal * xc / zc;
    out[1] = cam.center + cam.focal * yc / zc;
    out[2] = (zc > 0.0 && isfinite(zc)) ? cam.focal * cam.radius[p] / zc : -1.0;
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
__global__ __launch_bounds__(kThreads) void camera_features_kernel(const uvs_camera cam, const double *__restrict__ q_prev,
                                                                   const double *__restrict__ dq, double dt, double *__restrict__ q_out,
                                                                   const double *__restrict__ noise, double *__restrict__ f_out,
                                                                   int32_t *__restrict__ pixels_out, double *__restrict__ discs_out) {
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
    disc_counts(sdisc, cam.n_points, cc, rc);
    centre_of_mass(cc, rc, cam.n_points, noise, f_out, pixels_out);
}

thread_local char g_err[256] = "";

int fail(int code, const char *fmt, const char *detail = "") {
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

int uvs_render_discs_u8(int64_t T, const double *discs, int32_t n_colours, int32_t background, uint8_t *frames, int64_t frame_stride_bytes,
                        void *stream) {
    g_err[0] = '\0';
    if (discs == nullptr || frames == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs or frames");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_colours)) return fail(UVS_ERR_ARG, "%s", "n_colours must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (background < 0 || background >= kThreshold) return fail(UVS_ERR_ARG, "%s", "background must be 0 .. 249 (250 and above would enter a mask)");
    if (frame_stride_bytes < static_cast<int64_t>(kSide) * kRowBytes) return fail(UVS_ERR_ARG, "%s", "frame stride below 256 * 256 * 3");
    if (frame_stride_bytes % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frame stride must be a multiple of 16 bytes");
    if (reinterpret_cast<uintptr_t>(frames) % 16 != 0) return fail(UVS_ERR_ARG, "%s", "frames must be 16-byte aligned");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(render_discs_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), static_cast<uint32_t>(background), frames, frame_stride_bytes);
    return launched("render_discs_kernel launch: %s");
}

int uvs_disc_features_f64(int64_t T, const double *discs, int32_t n_colours, const double *noise, double *f_out, int32_t *pixels_out,
                          void *stream) {
    g_err[0] = '\0';
    if (discs == nullptr || f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL discs or f_out");
    if (T < 0 || T > INT32_MAX) return fail(UVS_ERR_ARG, "%s", "T out of range");
    if (!colours_ok(n_colours)) return fail(UVS_ERR_ARG, "%s", "n_colours must be 1 (green), 3 (RGB) or 4 (RGB + pink)");
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(disc_features_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), discs,
                       static_cast<int>(n_colours), noise, f_out, pixels_out);
    return launched("disc_features_kernel launch: %s");
}

int uvs_camera_features_f64(const uvs_camera *cam, int64_t T, const double *q_prev, const double *dq, double dt, double *q_out,
                            const double *noise, double *f_out, int32_t *pixels_out, double *discs_out, void *stream) {
    g_err[0] = '\0';
    if (f_out == nullptr) return fail(UVS_ERR_ARG, "%s", "NULL f_out");
    if (const int rc = check_camera(cam, T, q_prev, q_out)) return rc;
    if (T == 0) return UVS_OK;
    hipLaunchKernelGGL(camera_features_kernel, dim3(static_cast<unsigned>(T)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), *cam, q_prev,
                       dq, dt, q_out, noise, f_out, pixels_out, discs_out);
    return launched("camera_features_kernel launch: %s");
}

}  // extern "C"
