// Device code shared by all twenty translation units of libuvs_vision.so (uvs_vision.hip and uvs_camera_jacobian.hip directly, the eighteen loop and baseline units through camera_sensor_device.hpp): the detector's phase 2 in the two
// forms its callers need, the disc geometry of the synthetic camera with its occluders and their paints, and the DH chain.  The summation order of the phase 2 is a contract
// (see centre_of_mass): every unit that sums mask pixels goes through wave_partial and ColourSum, so they all give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "uvs_vision.h"

namespace uvs_vision {

constexpr int kSide = UVS_VISION_SIDE;          // rows = columns = grid points (utils.py:7-9)
constexpr int kThreads = 1024;                  // one workgroup per frame: 4 colours x 256 grid indices
constexpr int kColours = 4;                     // red, green, blue, pink (utils.py:126-166)

// p[i] = fl(g[i] * 255.0) with g = np.linspace(0, 1, 256): g[i] = fl(i * fl(1/255)), g[255] = 1.0 (the endpoint is assigned, not computed)
__device__ __forceinline__ double grid_product(int i) {
    const double step = 1.0 / 255.0;
    const double g = i < kSide - 1 ? static_cast<double>(i) * step : 1.0;
    return g * 255.0;
}

// First stage of the phase 2: the 64 lanes of a wavefront hold 64 consecutive grid indices of one colour, lane l the index i = 64 k + l with
// cc mask pixels in column i and rc in flipped row i.  Lane 0 receives the wavefront's sums of cc * p[i], rc * p[i] and cc through the
// __shfl_down tree (32, 16, .., 1); the other lanes receive partial trees nobody reads.  All 64 lanes must call it.
__device__ __forceinline__ void wave_partial(int cc, int rc, int i, double &su, double &sv, int &n) {
    const double p = grid_product(i);
    su = static_cast<double>(cc) * p;                            // X * mask, Y * mask (utils.py:25-27), summed by count
    sv = static_cast<double>(rc) * p;
    n = cc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        su += __shfl_down(su, off, 64);
        sv += __shfl_down(sv, off, 64);
        n += __shfl_down(n, off, 64);
    }
}

// Second stage: the four partials of one colour are added in index order, starting from 0.0, then (255 S) / (255 count).  0.0 / 0.0 = NaN
// for an empty mask, like the reference.  A wavefront whose 64 indices hold no mask pixel has the partial (+0.0, +0.0, 0): adding it is exact.
struct ColourSum {
    double s_u = 0.0, s_v = 0.0;
    int count = 0;
    __device__ __forceinline__ void add(double su, double sv, int n) {
        s_u += su;
        s_v += sv;
        count += n;
    }
    __device__ __forceinline__ void centre(double &u, double &v) const {
        const double total = static_cast<double>(255 * count);   // np.sum of the uint8 mask of 255s (utils.py:26)
        u = (255.0 * s_u) / total;
        v = (255.0 * s_v) / total;
    }
};

// Phase 2 of every one-workgroup-per-frame detector, from the integer counts on: thread (colour tid >> 8, grid index tid & 255) brings the
// number of mask pixels of its colour in column i (cc) and in flipped row i (rc).  noise, f_out and pixels_out are THE TRIAL'S OWN rows
// (2 n_colours doubles, 2 n_colours doubles, n_colours ints; noise and pixels_out may be NULL).  The bits of the result depend on the order:
// wave_partial per 64 consecutive indices, ColourSum per colour, then the noise add.  Called by all kThreads threads (it synchronises).
__device__ __forceinline__ void centre_of_mass(int cc, int rc, int n_colours, const double *__restrict__ noise, double *__restrict__ f_out,
                                               int32_t *__restrict__ pixels_out) {
    __shared__ double part_u[kThreads / 64], part_v[kThreads / 64];
    __shared__ int part_n[kThreads / 64];
    const int tid = threadIdx.x;
    double su, sv;
    int n;
    wave_partial(cc, rc, tid & 255, su, sv, n);                  // a wavefront holds one colour: 64 consecutive grid indices
    if ((tid & 63) == 0) {
        part_u[tid >> 6] = su;
        part_v[tid >> 6] = sv;
        part_n[tid >> 6] = n;
    }
    __syncthreads();

    if (tid < n_colours) {
        const int colour = n_colours == 1 ? 1 : tid;             // detectGreenCircle: green alone
        ColourSum sum;
        for (int k = 0; k < 4; ++k) sum.add(part_u[4 * colour + k], part_v[4 * colour + k], part_n[4 * colour + k]);
        double u, v;
        sum.centre(u, v);
        const int count = sum.count;
        if (noise != nullptr) {                                  // f += noise (experiment.py:135)
            u += noise[2 * tid];
            v += noise[2 * tid + 1];
        }
        f_out[2 * tid] = u;
        f_out[2 * tid + 1] = v;
        if (pixels_out != nullptr) pixels_out[tid] = count;
    }
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

// Inclusive pixel range [lo, hi] of [centre - r - slack, centre + r + slack] clipped to the frame.  fmax / fmin drop a NaN operand, so a
// bound that is NaN (inf - inf) becomes the frame edge, never an unconverted NaN: with slack = inf the range is the whole axis, whatever
// centre and r are.
__device__ __forceinline__ void pixel_range(double centre, double r, double slack, int &lo, int &hi) {
    lo = static_cast<int>(fmin(fmax(ceil(centre - r - slack), 0.0), static_cast<double>(kSide)));
    hi = static_cast<int>(fmax(fmin(floor(centre + r + slack), static_cast<double>(kSide - 1)), -1.0));
}

// A disc of ordinary size: centre and radius below 1e9 in magnitude (false for a NaN or an infinite operand)
__device__ __forceinline__ bool ordinary(const Disc &d) { return fabs(d.u) < 1e9 && fabs(d.v) < 1e9 && d.r < 1e9; }

// The box [x0, x1] x [y0, y1] that holds every pixel the rule gives the disc.  For a disc of ordinary size one pixel of slack around
// centre -+ r: doubles of that size are at most 2^-22 apart, so the slack covers every rounding of the rule's dx and of the bounds.  It
// does not from 2^54 on, where dx = x - centre itself rounds to multiples of 4 and more and the rule's pixels reach past
// centre -+ r -+ 1 (tests/test_camera_host.py: test_box_mirror_keeps_every_pixel_of_the_rule): any other disc gets the whole frame.
__device__ __forceinline__ void disc_box(const Disc &d, int &x0, int &x1, int &y0, int &y1) {
    const double slack = ordinary(d) ? 1.0 : HUGE_VAL;
    pixel_range(d.u, d.r, slack, x0, x1);
    pixel_range(d.v, d.r, slack, y0, y1);
}

// The disc of the n_colours at `discs` that colour slot c (red, green, blue, pink) shows, or -1: the one disc of n_colours == 1 is the green one
__device__ __forceinline__ int disc_of_colour(int c, int n_colours) { return n_colours == 1 ? (c == 1 ? 0 : -1) : (c < n_colours ? c : -1); }

// Could disc o cover a pixel of the box [x0, x1] x [y0, y1]?  No, when it draws nothing or when its own pixel ranges miss the box: for a disc
// of ordinary size every pixel the rule gives it lies inside its ranges (disc_box).  Anything else -- a NaN centre, a huge disc -- counts
// as "could".
__device__ __forceinline__ bool may_cover(const Disc &o, int x0, int x1, int y0, int y1) {
    if (!(o.r2 >= 0.0)) return false;
    if (!ordinary(o)) return true;
    int ox0, ox1, oy0, oy1;
    pixel_range(o.u, o.r, 1.0, ox0, ox1);
    pixel_range(o.v, o.r, 1.0, oy0, oy1);
    return ox0 <= x1 && ox1 >= x0 && oy0 <= y1 && oy1 >= y0;
}

// ---------------------------------------------------------------------------------------------------------------- occluders
// An occluder's rectangle at one step, clipped to the frame, as the kernels hold it: x0 | x1 << 8 | y0 << 16 | y1 << 24, inclusive bounds
// in 0 .. 255.  A rectangle that covers nothing -- inactive at k, no size, or wholly outside the frame -- is kNoRect: x0 = 1 > x1 = 0.
constexpr int kOccluders = UVS_CAMERA_MAX_OCCLUDERS;
constexpr uint32_t kNoRect = 0x00010001u;

struct Rects {
    uint32_t r[kOccluders] = {kNoRect, kNoRect, kNoRect, kNoRect};
};

__device__ __forceinline__ int rect_x0(uint32_t r) { return static_cast<int>(r & 255u); }
__device__ __forceinline__ int rect_x1(uint32_t r) { return static_cast<int>((r >> 8) & 255u); }
__device__ __forceinline__ int rect_y0(uint32_t r) { return static_cast<int>((r >> 16) & 255u); }
__device__ __forceinline__ int rect_y1(uint32_t r) { return static_cast<int>(r >> 24); }

// THE rectangle of the rule (uvs_vision.h, uvs_occluder), shared by every kernel: position in 64-bit integers -- |x + vx * k| < 2^62 + 2^31
// for any int32 fields and 0 <= k < 2^31 -- and the clip to the frame before the narrowing.
__device__ __forceinline__ uint32_t occluder_rect(const uvs_occluder &o, int k) {
    if (!(k >= o.k_on && k < o.k_off && o.w > 0 && o.h > 0)) return kNoRect;
    const long long xk = static_cast<long long>(o.x) + static_cast<long long>(o.vx) * k;
    const long long yk = static_cast<long long>(o.y) + static_cast<long long>(o.vy) * k;
    const long long last = kSide - 1;
    const long long x0 = xk > 0 ? xk : 0, x1 = xk + o.w - 1 < last ? xk + o.w - 1 : last;
    const long long y0 = yk > 0 ? yk : 0, y1 = yk + o.h - 1 < last ? yk + o.h - 1 : last;
    if (x0 > x1 || y0 > y1) return kNoRect;                      // here 0 <= x0 <= x1 <= 255, and likewise y
    return static_cast<uint32_t>(x0) | static_cast<uint32_t>(x1) << 8 | static_cast<uint32_t>(y0) << 16 | static_cast<uint32_t>(y1) << 24;
}

// The rectangles of one trial at step k: occ names the trial's n_occ structs (read only when n_occ > 0)
__device__ __forceinline__ Rects occluder_rects(const uvs_occluder *occ, int n_occ, int k) {
    Rects out;
#pragma unroll
    for (int o = 0; o < kOccluders; ++o)
        if (o < n_occ) out.r[o] = occluder_rect(occ[o], k);
    return out;
}

// Does a rectangle of `rects` hold a pixel of the box [x0, x1] x [y0, y1]?
__device__ __forceinline__ bool rects_meet(const Rects &rects, int x0, int x1, int y0, int y1) {
    bool meets = false;
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) {
        const uint32_t r = rects.r[o];
        meets = meets || (rect_x0(r) <= rect_x1(r) && rect_x0(r) <= x1 && rect_x1(r) >= x0 && rect_y0(r) <= y1 && rect_y1(r) >= y0);
    }
    return meets;
}

__device__ __forceinline__ bool rects_cover(const Rects &rects, int x, int y) {
    bool covered = false;
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) {
        const uint32_t r = rects.r[o];
        covered = covered || (x >= rect_x0(r) && x <= rect_x1(r) && y >= rect_y0(r) && y <= rect_y1(r));
    }
    return covered;
}

// The same test for a walk along one line of the frame: what each rectangle covers of column x (along = false: flipped rows [lo, hi]) or
// of flipped row y (along = true: columns [lo, hi]), formed once per line; a rectangle that misses the line leaves lo = 1 > hi = 0.
struct LineCover {
    int lo[kOccluders], hi[kOccluders];
    __device__ __forceinline__ LineCover(const Rects &rects, int line, bool along) {
#pragma unroll
        for (int o = 0; o < kOccluders; ++o) {
            const uint32_t r = rects.r[o];
            const bool on = along ? (line >= rect_y0(r) && line <= rect_y1(r)) : (line >= rect_x0(r) && line <= rect_x1(r));
            lo[o] = on ? (along ? rect_x0(r) : rect_y0(r)) : 1;
            hi[o] = on ? (along ? rect_x1(r) : rect_y1(r)) : 0;
        }
    }
    __device__ __forceinline__ bool at(int p) const {
        bool covered = false;
#pragma unroll
        for (int o = 0; o < kOccluders; ++o) covered = covered || (p >= lo[o] && p <= hi[o]);
        return covered;
    }
};

// The walks of disc_counts_at over the box of `me`; OVER = false leaves the tests against the discs painted later out (none can cover a
// pixel of the box), which is three of the four distance tests of every pixel.  OCC = true adds the occluders: a pixel counts when it is
// the topmost disc's AND no rectangle covers it -- integer compares; OCC = false is the walk as it always was and never reads `rects`.
template <bool OVER, bool OCC = false>
__device__ __forceinline__ void box_counts(const Disc &me, const Disc (&over)[kColours - 1], int x0, int x1, int y0, int y1, int i, int &cc, int &rc,
                                           const Rects &rects = Rects{}) {
    const double fi = static_cast<double>(i);
    if (i >= x0 && i <= x1) {                                    // column i: walk the rows of the box
        const double dx = fi - me.u, dx2 = dx * dx;
        double ox2[kColours - 1];
        if constexpr (OVER) {
#pragma unroll
            for (int k = 0; k < kColours - 1; ++k) {
                const double o = fi - over[k].u;
                ox2[k] = o * o;
            }
        }
        const LineCover cover(rects, i, false);                  // OCC = false: never read
        for (int y = y0; y <= y1; ++y) {
            const double fy = static_cast<double>(y), dy = fy - me.v;
            bool top = dx2 + dy * dy <= me.r2;
            if constexpr (OVER) {
#pragma unroll
                for (int k = 0; k < kColours - 1; ++k) {
                    const double o = fy - over[k].v;
                    top = top && !(ox2[k] + o * o <= over[k].r2);
                }
            }
            if constexpr (OCC) top = top && !cover.at(y);
            cc += top ? 1 : 0;
        }
    }
    if (i >= y0 && i <= y1) {                                    // flipped row i: walk the columns of the box
        const double dy = fi - me.v, dy2 = dy * dy;
        double oy2[kColours - 1];
        if constexpr (OVER) {
#pragma unroll
            for (int k = 0; k < kColours - 1; ++k) {
                const double o = fi - over[k].v;
                oy2[k] = o * o;
            }
        }
        const LineCover cover(rects, i, true);
        for (int x = x0; x <= x1; ++x) {
            const double fx = static_cast<double>(x), dx = fx - me.u;
            bool top = dx * dx + dy2 <= me.r2;
            if constexpr (OVER) {
#pragma unroll
                for (int k = 0; k < kColours - 1; ++k) {
                    const double o = fx - over[k].u;
                    top = top && !(o * o + oy2[k] <= over[k].r2);
                }
            }
            if constexpr (OCC) top = top && !cover.at(x);
            rc += top ? 1 : 0;
        }
    }
}

// Counts of index i for disc `own` of the n_colours at `discs` (global memory or LDS) in the frame the rasteriser would write: cc = rows at
// which it is the topmost one in column i, rc = columns at which it is in flipped row i.  `me` is that disc, loaded (me.r2 >= 0), and
// [x0, x1] x [y0, y1] its disc_box: a caller that has both in hand -- the closed loops, which skip whole blocks of indices by the box --
// passes them on instead of having them formed again.  The discs are the same in all lanes of a wavefront (every caller's are), so which
// of the two walks runs is a scalar branch.  OCC: so are the trial's rectangles, and so is the decision whether one of them meets the box;
// when none does the walks are the unoccluded ones -- an unoccluded disc costs what it always cost and trivially has those bits.
template <bool OCC = false>
__device__ __forceinline__ void disc_counts_in_box(const double *discs, int n_colours, int own, const Disc &me, int x0, int x1, int y0, int y1, int i,
                                                   int &cc, int &rc, const Rects &rects = Rects{}) {
    cc = 0;
    rc = 0;
    Disc over[kColours - 1];                                     // the discs painted after mine; absent ones never cover a pixel
    bool covered = false;
#pragma unroll
    for (int k = 0; k < kColours - 1; ++k) {
        const int other = own + 1 + k;
        over[k] = load_disc(discs + 3 * (other < n_colours ? other : own), other < n_colours);
        covered = covered || may_cover(over[k], x0, x1, y0, y1);
    }
    if constexpr (OCC) {
        if (__builtin_amdgcn_readfirstlane(static_cast<int>(rects_meet(rects, x0, x1, y0, y1)))) {
            if (__builtin_amdgcn_readfirstlane(static_cast<int>(covered)))
                box_counts<true, true>(me, over, x0, x1, y0, y1, i, cc, rc, rects);
            else
                box_counts<false, true>(me, over, x0, x1, y0, y1, i, cc, rc, rects);
            return;
        }
    }
    if (__builtin_amdgcn_readfirstlane(static_cast<int>(covered)))
        box_counts<true>(me, over, x0, x1, y0, y1, i, cc, rc);
    else
        box_counts<false>(me, over, x0, x1, y0, y1, i, cc, rc);
}

// Counts of (colour c, index i) from the discs alone; c is the same in all lanes of a wavefront.
template <bool OCC = false>
__device__ __forceinline__ void disc_counts_at(const double *discs, int n_colours, int c, int i, int &cc, int &rc, const Rects &rects = Rects{}) {
    const int own = disc_of_colour(c, n_colours);
    cc = 0;
    rc = 0;
    if (own < 0) return;
    const Disc me = load_disc(discs + 3 * own, true);
    if (!(me.r2 >= 0.0)) return;
    int x0, x1, y0, y1;
    disc_box(me, x0, x1, y0, y1);
    disc_counts_in_box<OCC>(discs, n_colours, own, me, x0, x1, y0, y1, i, cc, rc, rects);
}

// The same for thread (colour c = tid >> 8, index i = tid & 255) of a one-workgroup-per-frame kernel; c is wavefront-uniform there.
template <bool OCC = false>
__device__ __forceinline__ void disc_counts(const double *discs, int n_colours, int &cc, int &rc, const Rects &rects = Rects{}) {
    disc_counts_at<OCC>(discs, n_colours, threadIdx.x >> 8, threadIdx.x & 255, cc, rc, rects);
}

// ---------------------------------------------------------------------------------------------------------------- painted occluders
// The paints of a trial's rectangles as the kernels hold them: one dword, byte o = the colour SLOT (red, green, blue, pink: 0 .. 3) that
// rectangle o is painted, or kOpaque.  paint_slot is THE rule of the header (uvs_vision.h, "paint"), total: a value p in
// 0 .. n_colours - 1 is the colour of disc p (n_colours == 1: the green one), every other int32 is opaque.
constexpr uint32_t kOpaque = 0xffu;
constexpr uint32_t kNoPaints = 0xffffffffu;                     // four opaque rectangles

__device__ __forceinline__ uint32_t paint_slot(int32_t p, int n_colours) {
    if (p < 0 || p >= n_colours) return kOpaque;
    return n_colours == 1 ? 1u : static_cast<uint32_t>(p);
}
__device__ __forceinline__ uint32_t paint_of(uint32_t paints, int o) { return (paints >> (8 * o)) & 0xffu; }

// The paints of one trial: paint names the trial's n_occ values (read only when it is not NULL and n_occ > 0)
__device__ __forceinline__ uint32_t occluder_paints(const int32_t *paint, int n_occ, int n_colours) {
    uint32_t out = kNoPaints;
    if (paint == nullptr) return out;
#pragma unroll
    for (int o = 0; o < kOccluders; ++o)
        if (o < n_occ) out = (out & ~(0xffu << (8 * o))) | (paint_slot(paint[o], n_colours) << (8 * o));
    return out;
}

// Rectangle o is active and painted slot c
__device__ __forceinline__ bool painted(const Rects &rects, uint32_t paints, int o, int c) {
    return paint_of(paints, o) == static_cast<uint32_t>(c) && rect_x0(rects.r[o]) <= rect_x1(rects.r[o]);
}

// Does an active rectangle painted slot c reach the indices [lo, hi], in columns or in flipped rows?  (All of them: lo = 0, hi = 255.)
__device__ __forceinline__ bool paint_reaches(const Rects &rects, uint32_t paints, int c, int lo, int hi) {
    bool reaches = false;
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) {
        const uint32_t r = rects.r[o];
        reaches = reaches || (painted(rects, paints, o, c) && ((rect_x0(r) <= hi && rect_x1(r) >= lo) || (rect_y0(r) <= hi && rect_y1(r) >= lo)));
    }
    return reaches;
}

// Pixels of [a, b] on one line that the rectangles in front of rectangle o (those of a higher index) leave to it.  lo / hi: what each
// rectangle covers of the line (LineCover's members).  Inclusion and exclusion over the at most three ranges in front, each clipped to
// [a, b]; an empty range has lo > hi, stays empty in every intersection and counts 0.  Integers only.
__device__ __forceinline__ int owned_on_line(const int (&lo)[kOccluders], const int (&hi)[kOccluders], int o, int a, int b) {
    int l[kOccluders - 1], h[kOccluders - 1];
#pragma unroll
    for (int k = 0; k < kOccluders - 1; ++k) {
        const int f = o + 1 + k;                                 // in front of o, or no rectangle at all: nothing
        const bool is_rect = f >= 0 && f < kOccluders;
        l[k] = is_rect ? max(lo[is_rect ? f : o], a) : 1;
        h[k] = is_rect ? min(hi[is_rect ? f : o], b) : 0;
    }
    const auto len = [](int x, int y) { return y >= x ? y - x + 1 : 0; };
    const int two = len(max(l[0], l[1]), min(h[0], h[1])) + len(max(l[0], l[2]), min(h[0], h[2])) + len(max(l[1], l[2]), min(h[1], h[2]));
    const int three = len(max(max(l[0], l[1]), l[2]), min(min(h[0], h[1]), h[2]));
    return len(a, b) - (len(l[0], h[0]) + len(l[1], h[1]) + len(l[2], h[2]) - two + three);
}

// What the rectangles painted slot c add to the counts of index i: for every such rectangle that meets column i the rows of it that no
// rectangle in front of it takes, and likewise for flipped row i.  A pixel has one owner, so nothing is counted twice -- neither among the
// rectangles nor with the disc's own walk, which leaves out every pixel an active rectangle covers.
__device__ __forceinline__ void paint_counts(const Rects &rects, uint32_t paints, int c, int i, int &cc, int &rc) {
    const LineCover column(rects, i, false), row(rects, i, true);    // formed once per line
#pragma unroll
    for (int o = 0; o < kOccluders; ++o) {
        const bool mine = painted(rects, paints, o, c);
        if (mine && column.lo[o] <= column.hi[o]) cc += owned_on_line(column.lo, column.hi, o, column.lo[o], column.hi[o]);
        if (mine && row.lo[o] <= row.hi[o]) rc += owned_on_line(row.lo, row.hi, o, row.lo[o], row.hi[o]);
    }
}

// Counts of index i for colour slot c = the colour of disc `own` in the frame with painted rectangles: the disc's pixels behind ALL active
// rectangles (the occluded walk as it is, when the disc draws anything: me.r2 >= 0), and the pixels of the rectangles painted c.
// `any_painted` = painted_at_all(rects, paints, c), formed ONCE per colour by the caller: a colour no active rectangle is painted takes
// exactly the occluded path, and pays one test per colour for it, not one per index block.  Both decisions are wavefront-uniform.
__device__ __forceinline__ int painted_at_all(const Rects &rects, uint32_t paints, int c) {
    return __builtin_amdgcn_readfirstlane(static_cast<int>(paint_reaches(rects, paints, c, 0, kSide - 1)));
}
__device__ __forceinline__ void painted_counts_in_box(const double *discs, int n_colours, int own, int c, const Disc &me, int x0, int x1, int y0, int y1,
                                                      int i, int &cc, int &rc, const Rects &rects, uint32_t paints, int any_painted) {
    cc = 0;
    rc = 0;
    if (__builtin_amdgcn_readfirstlane(static_cast<int>(me.r2 >= 0.0)))
        disc_counts_in_box<true>(discs, n_colours, own, me, x0, x1, y0, y1, i, cc, rc, rects);
    if (any_painted) paint_counts(rects, paints, c, i, cc, rc);
}

// disc_counts<true> for thread (colour c = tid >> 8, index i = tid & 255) of a one-workgroup-per-frame kernel, with paints
__device__ __forceinline__ void painted_counts(const double *discs, int n_colours, int &cc, int &rc, const Rects &rects, uint32_t paints) {
    const int c = threadIdx.x >> 8, i = threadIdx.x & 255;
    const int own = disc_of_colour(c, n_colours);
    cc = 0;
    rc = 0;
    if (own < 0) return;                                         // no disc of this colour, so no paint of it either (paint_slot)
    const Disc me = load_disc(discs + 3 * own, true);
    int x0, x1, y0, y1;
    disc_box(me, x0, x1, y0, y1);
    painted_counts_in_box(discs, n_colours, own, c, me, x0, x1, y0, y1, i, cc, rc, rects, paints, painted_at_all(rects, paints, c));
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

// The same for a camera whose own n_joints is not read (a scene in memory): the arms of this project have six joints.
constexpr int kSceneJoints = 6;
__device__ __forceinline__ void scene_joint_sincos(const uvs_camera &cam, int64_t t, int i, const double *__restrict__ q_prev,
                                                   const double *__restrict__ dq, double dt, double *__restrict__ q_out, double &s, double &c) {
    constexpr int n = kSceneJoints;
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

// ---------------------------------------------------------------------------------------------------------------- cameras in memory
// The operand (structs, number, index) of every entry point that reads a uvs_camera PER TRIAL from device memory: the believed models of the
// calibrated law (uvs_camera_believed.hip) and the scenes that render a trial's frames.  One rule for both: an index outside
// [0, n) never becomes an address.
constexpr int kCamWords = static_cast<int>(sizeof(uvs_camera) / 8);
static_assert(sizeof(uvs_camera) % 8 == 0, "copied as doubles");

struct Believed {
    const uvs_camera *models;                                    // [n]
    long long n;
    const int32_t *index;                                        // [T] or NULL: n == 1 (all trials the one model) or n == T (trial t model t)
};
using Scenes = Believed;                                         // the same triple, naming the cameras of the sensor side

// The model of `trial`, or -1 when its index names none.
__device__ __forceinline__ long long model_of(const Believed &B, long long trial) {
    const long long i = B.index != nullptr ? static_cast<long long>(B.index[trial]) : (B.n == 1 ? 0 : trial);
    return (i >= 0 && i < B.n) ? i : -1;
}

// The models of the trials first .. first + COUNT - 1 (clamped to the last trial: padding shadows it) into s_cam[COUNT], by all THREADS threads;
// zeros for a trial without a model.  The caller's next barrier stands between this and the first read.
template <int COUNT, int THREADS>
__device__ __forceinline__ void stage_models(const Believed &B, long long first, long long T, uvs_camera *s_cam) {
    for (int i = threadIdx.x; i < COUNT * kCamWords; i += THREADS) {
        const int slot = i / kCamWords, word = i - slot * kCamWords;
        long long trial = first + slot;
        if (trial >= T) trial = T - 1;
        const long long model = model_of(B, trial);
        reinterpret_cast<double *>(s_cam)[i] = model >= 0 ? reinterpret_cast<const double *>(B.models + model)[word] : 0.0;
    }
}

// The same for the SCENES of those trials, whose structs' own n_joints / n_points are not read: word 0 of every staged struct is `shape`'s
// (the launch's n_joints and n_points, from fp), also for a trial without a scene, whose other words are zeros.
template <int COUNT, int THREADS>
__device__ __forceinline__ void stage_scenes(const Scenes &S, const uvs_camera &shape, long long first, long long T, uvs_camera *s_cam) {
    for (int i = threadIdx.x; i < COUNT * kCamWords; i += THREADS) {
        const int slot = i / kCamWords, word = i - slot * kCamWords;
        long long trial = first + slot;
        if (trial >= T) trial = T - 1;
        const long long model = model_of(S, trial);
        double value = model >= 0 ? reinterpret_cast<const double *>(S.models + model)[word] : 0.0;
        if (word == 0) value = reinterpret_cast<const double *>(&shape)[0];
        reinterpret_cast<double *>(s_cam)[i] = value;
    }
}

// ---------------------------------------------------------------------------------------------------------------- moving targets
// THE rule of uvs_target_motion (uvs_vision.h), shared by every kernel that moves a disc.  The steps the target has moved
// at step k, in 64-bit integers: |k - k_on| and k_off - k_on are below 2^33 for any int32 fields.
__device__ __forceinline__ long long motion_steps(int32_t k_on, int32_t k_off, int k) {
    const long long span = static_cast<long long>(k_off) - k_on, most = span > 0 ? span : 0;
    const long long since = static_cast<long long>(k) - k_on, s = since > 0 ? since : 0;
    return s < most ? s : most;
}

// One coordinate of a world point after s steps at velocity v: one rounded multiply, then one rounded add (-ffp-contract=off), as the
// joint step; for s == 0 the coordinate itself, bits untouched -- a select over both values, so a -0.0 stays -0.0 and a velocity that is
// not finite moves nothing.
__device__ __forceinline__ double moved_coordinate(double x, double v, long long s) {
    const double step = static_cast<double>(s) * v;
    const double moved = x + step;
    return s == 0 ? x : moved;
}

// project_disc for disc p of `cam` standing at the world point w instead of cam.points[p]: its operations in its order
__device__ __forceinline__ void project_disc_at(const uvs_camera &cam, int p, double wx, double wy, double wz, const double (&T)[3][4], double *out) {
    const double dx = wx - T[0][3], dy = wy - T[1][3], dz = wz - T[2][3];
    const double xc = T[0][0] * dx + T[1][0] * dy + T[2][0] * dz;
    const double yc = T[0][1] * dx + T[1][1] * dy + T[2][1] * dz;
    const double zc = T[0][2] * dx + T[1][2] * dy + T[2][2] * dz;
    out[0] = cam.center + cam.focal * xc / zc;
    out[1] = cam.center + cam.focal * yc / zc;
    out[2] = (zc > 0.0 && isfinite(zc)) ? cam.focal * cam.radius[p] / zc : -1.0;
}

// project_disc for disc p of `cam` at step k of the motion `mot` (global memory or LDS)
__device__ __forceinline__ void project_moved_disc(const uvs_camera &cam, int p, const uvs_target_motion &mot, int k, const double (&T)[3][4],
                                                   double *out) {
    const long long s = motion_steps(mot.k_on, mot.k_off, k);
    project_disc_at(cam, p, moved_coordinate(cam.points[p][0], mot.v[p][0], s), moved_coordinate(cam.points[p][1], mot.v[p][1], s),
                    moved_coordinate(cam.points[p][2], mot.v[p][2], s), T, out);
}

// The same for a motion in memory that may be absent (NULL: nothing moves, s == 0 and no velocity is read)
__device__ __forceinline__ void project_moved_disc_of(const uvs_camera &cam, int p, const uvs_target_motion *mot, int k, const double (&T)[3][4],
                                                      double *out) {
    const long long s = mot != nullptr ? motion_steps(mot->k_on, mot->k_off, k) : 0;
    double w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = moved_coordinate(cam.points[p][c], mot != nullptr ? mot->v[p][c] : 0.0, s);
    project_disc_at(cam, p, w[0], w[1], w[2], T, out);
}

// The motions of the trials first .. first + COUNT - 1 (clamped to the last trial: padding shadows it) into s_mot[COUNT], by all THREADS
// threads; zeros -- nothing moves -- for a NULL operand.  The caller's next barrier stands between this and the first read.
constexpr int kMotionWords = static_cast<int>(sizeof(uvs_target_motion) / 8);
static_assert(sizeof(uvs_target_motion) == 104, "copied as 13 eight-byte words");
template <int COUNT, int THREADS>
__device__ __forceinline__ void stage_motions(const uvs_target_motion *motion, long long first, long long T, uvs_target_motion *s_mot) {
    for (int i = threadIdx.x; i < COUNT * kMotionWords; i += THREADS) {
        const int slot = i / kMotionWords, word = i - slot * kMotionWords;
        long long trial = first + slot;
        if (trial >= T) trial = T - 1;
        reinterpret_cast<uint64_t *>(s_mot)[i] = motion != nullptr ? reinterpret_cast<const uint64_t *>(motion + trial)[word] : 0ull;
    }
}

// ---------------------------------------------------------------------------------------------------------------- camera latency
// THE rule of the latency operand (uvs_vision.h), shared by every kernel that delays a frame: the latency the device
// uses, and the step whose frame the detector is handed at step k.
__device__ __forceinline__ int clamped_latency(int32_t d) { return d < 0 ? 0 : (d > UVS_CAMERA_MAX_LATENCY ? UVS_CAMERA_MAX_LATENCY : d); }
__device__ __forceinline__ int delayed_step(int k, int d) { return k - d > 0 ? k - d : 0; }
// the latency of `trial`, clamped; NULL: none
__device__ __forceinline__ int latency_of(const int32_t *latency, long long trial) { return latency != nullptr ? clamped_latency(latency[trial]) : 0; }

// THE rule of the assumed-latency operand (uvs_vision.h, ASSUMED LATENCY; plant.aligned_regressor_step): the step whose
// command is the estimator's regressor at step k when the controller assumes latency a (clamped like d); negative: the zero vector.  The
// law's joints at step k are those of delayed_step(k, a).
__device__ __forceinline__ int aligned_regressor_step(int k, int a) { return k - 1 - a; }

// The delay line of ONE disc of one trial: the detections of the last kDelaySlots steps, slot k mod kDelaySlots.  A cell is a ColourSum as
// three 64-bit integer words -- the bits of the two sums, and the count -- moved through plain integer pointers and replaced IN PLACE,
// member by member.  On purpose: with a cell of doubles stored through its struct type, or the delayed detection returned by value, the
// instantiation closest to the register limit (MCKF at (2, 6), four trials per workgroup) came out 48 registers larger and spilled 28 B
// per lane; in this form the ring costs it nothing.  The ONE lane that holds the detection of step k writes slot k and reads slot
// kk = delayed_step(k, d) -- its own words alone, in program order: no barrier.  k - kk <= UVS_CAMERA_MAX_LATENCY < kDelaySlots, so slot
// kk still holds step kk's detection (d == 0: the one just written, bits untouched), and for k < d slot 0 holds step 0's: the priming.
constexpr int kDelaySlots = UVS_CAMERA_MAX_LATENCY + 1;
struct DelayCell {
    long long s_u, s_v, count;
};
__device__ __forceinline__ void delay_line(DelayCell *ring, ColourSum &sum, int k, int d) {
    long long *in = reinterpret_cast<long long *>(ring + k % kDelaySlots);
    in[0] = __double_as_longlong(sum.s_u);
    in[1] = __double_as_longlong(sum.s_v);
    in[2] = sum.count;
    const long long *out = reinterpret_cast<const long long *>(ring + delayed_step(k, d) % kDelaySlots);
    sum.s_u = __longlong_as_double(out[0]);
    sum.s_v = __longlong_as_double(out[1]);
    sum.count = static_cast<int>(out[2]);
}

// ---------------------------------------------------------------------------------------------------------------- host side, shared
// The calling thread's error text and the two ways an entry point ends (defined in uvs_vision.hip).
extern thread_local char g_err[256];
int fail(int code, const char *fmt, const char *detail = "");
int launched(const char *what);
bool colours_ok(int32_t n);
int check_occluders(const uvs_occluder *occ, int32_t n_occ);    // UVS_ERR_ARG for n_occ outside 0 .. 4 or a NULL occ with n_occ > 0
// the scene operand: UVS_ERR_ARG for NULL cams, n_cams < 1, or n_cams not in {1, T} without an index
int check_scenes(const uvs_camera *cams, int64_t n_cams, const int32_t *cam_index, int64_t T);
uvs_camera scene_shape(int32_t n_joints, int32_t n_points);    // what a scenes launch passes where its namesake passes *cam: the shape alone

}  // namespace uvs_vision
