// Shared body of tu_closed_tuned_{a,b}.hip (which define UVS_TU_SHAPES and UVS_TU_NAME) and of tu_closed_grid_{a,b}.hip (UVS_PER_TRIAL, UVS_TU_NAME and
// UVS_TU_METHODS): there UVS_CLOSED_TUNED_KERNEL / ClosedKernelArgs are the per-trial flavour (closed_loop_grid_kernel / ClosedGridArgs, rmckf_device.hpp),
// which exists at (8,6), two lanes, DH plant only.  One launcher text, so a grid launch picks the instantiation of the uniform launch it replaces.
#include "launchers.hpp"
#include "rmckf_tuned.hpp"

#ifndef UVS_CLOSED_TUNED_HELPERS           // the unity build (uvs_unity.hip) includes this file twice
#define UVS_CLOSED_TUNED_HELPERS
namespace {
// estimator, plant kind and "X stream wanted" are compile-time in the tuned kernel
template <int M, int N, int LL, int METHOD, int PLANT, bool EMU2 = false>
void launch2(bool xo, dim3 g, hipStream_t s, const uvs::ClosedKernelArgs &A) {
    constexpr int PV = (LL == 2 ? M / LL / 2 : M / LL);      // L = 2 parks half of its blocks in LDS; 1 and 4 keep all in registers
    // UVS_OPT_STRICT_PINV on KF / IMCC-KF / MCKF: the instantiations whose control law certifies every solve (uvs_launch::tuned_certifies; a compile-time
    // switch there, see CERT in rmckf_tuned.hpp; RMCKF reads the option at run time); MCKF as whole trials.  (No per-trial CERT / XREC / XPAIR kernels.)
    if constexpr (!uvs::kPerTrial && METHOD != UVS_METHOD_GMCKF && uvs_launch::tuned_certifies(M, N, LL, METHOD, PLANT == UVS_PLANT_LINEAR, EMU2)) {
        if (A.fp.reserved & UVS_OPT_STRICT_PINV) {
            constexpr bool SEGM = (METHOD == UVS_METHOD_MCKF);
            if (xo) hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, true, false, SEGM, false, true>), g, dim3(64), 0, s, A);
            else hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, false, false, SEGM, false, true>), g, dim3(64), 0, s, A);
            return;
        }
    }
    // segmented trials (MCKF always; RMCKF through its SEGMENTED instantiation, (8,6) only): one work item per (chunk, segment), ids segment-major
    if constexpr ((METHOD == UVS_METHOD_MCKF || (METHOD == UVS_METHOD_GMCKF && M == 8 && N == 6)) && LL == 2 && PLANT != UVS_PLANT_LINEAR && !EMU2) {
        if (A.n_seg > 1) {
            uvs_launch::fill_i32(A.ws_flags, 0, (long long)g.x + 1, s);      // the chunks' counters + the fallback count (a kernel, not a memset node: launchers.hpp)
            g.x *= (unsigned)A.n_seg;
            if constexpr (METHOD == UVS_METHOD_GMCKF) {
                if (xo) hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, true, false, true>), g, dim3(64), 0, s, A);
                else hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, false, false, true>), g, dim3(64), 0, s, A);
                return;
            }
        }
    }
    // per-trial records for the X stream ([step][trial][m n]): the instantiation that writes them as whole 128-byte lines out of LDS
    // (measured, profiles/r05/record_layout.txt: KF 2.605 -> 2.54 ms, IMCC-KF 2.69 -> 2.67; RMCKF -- one wavefront per SIMD, nothing to hide the twelve
    // bank-conflicted LDS reads behind -- loses 10 % and keeps its strided stores whatever the view; 16-byte stores straight from the rows' registers,
    // without the transposition, cost KF + 25 %)
    if constexpr (!uvs::kPerTrial && M == 8 && N == 6 && LL == 2 && !EMU2 && (METHOD == UVS_METHOD_KF || METHOD == UVS_METHOD_IMCCKF) && PLANT != UVS_PLANT_LINEAR) {
        const bool aligned = (reinterpret_cast<uintptr_t>(A.x_out.p) & 15u) == 0 && A.x_out.sk % 2 == 0;
        const bool records = A.x_out.sc == 1 && A.x_out.st == M * N;
        // (round 6) trial-fastest rows -- the package's default layout -- leave LDS as 16-byte pairs of consecutive trials (XPAIR): 12 stores per lane-step
        // instead of 24; KF - 2.5 %, IMCC-KF - 2.0 % (profiles/r06/pair_stores_ab.txt; bit-identical).  Needs an even row pitch and an even T.  RMCKF -- one
        // wavefront per SIMD, nothing to hide the LDS reads and the burst of stores behind -- loses 4.6 % with it (same file) and keeps its 8-byte stores.
        const bool pairs = A.x_out.st == 1 && A.x_out.sc % 2 == 0 && A.T % 2 == 0;
        if (xo && aligned && records) {
            hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, true, false, false, true>), g, dim3(64), 0, s, A);
            return;
        }
        if (xo && aligned && pairs) {
            hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, true, false, false, true, false, true>), g, dim3(64), 0, s, A);
            return;
        }
    }
    if (xo) hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, true, EMU2>), g, dim3(64), 0, s, A);
    else hipLaunchKernelGGL((uvs::UVS_CLOSED_TUNED_KERNEL<M, N, LL, METHOD, PLANT, PV, false, EMU2>), g, dim3(64), 0, s, A);
}
// UR10-like DH table: the tuned two-lane kernel has an instantiation that knows the zeros of its first and last links per lane group
inline bool axis_aligned(const uvs_plant &p) {
    if (p.n_joints != 6) return false;
    for (int g = 0; g < 6; g += 3)
        if (!(p.sin_alpha[g] == -1.0 && p.cos_alpha[g] > -1e-15 && p.cos_alpha[g] < 1e-15 && p.cos_alpha[g + 2] == 1.0 && p.sin_alpha[g + 2] == 0.0)) return false;
    return true;
}
template <int M, int N, int LL, int METHOD, bool EMU2 = false>
void launch_dh(bool xo, dim3 g, hipStream_t s, const uvs::ClosedKernelArgs &A) {
    if constexpr ((LL == 2 || EMU2) && N == 6 && M == 8) {
        if (axis_aligned(A.plant)) { launch2<M, N, LL, METHOD, uvs::kPlantDhAxisAligned, EMU2>(xo, g, s, A); return; }
    }
    launch2<M, N, LL, METHOD, UVS_PLANT_DH_PINHOLE, EMU2>(xo, g, s, A);
}
template <int M, int N, int LL, bool EMU2 = false>
bool launch(int method, bool linear, bool xo, dim3 g, hipStream_t s, const uvs::ClosedKernelArgs &A) {
    auto go = [&](auto meth) {
        constexpr int METHOD = decltype(meth)::value;
        if (!linear) launch_dh<M, N, LL, METHOD, EMU2>(xo, g, s, A);
        else if constexpr (!EMU2) launch2<M, N, LL, METHOD, UVS_PLANT_LINEAR>(xo, g, s, A);
    };
    if constexpr (LL == 2 || EMU2)                                 // first-pass MCKF rows: two-lane kernels (and EMU2) only
        return uvs_launch::dispatch<UVS_METHOD_MCKF, UVS_METHOD_GMCKF, UVS_METHOD_IMCCKF, UVS_METHOD_KF>(method, go);
    else
        return uvs_launch::dispatch<UVS_METHOD_GMCKF, UVS_METHOD_IMCCKF, UVS_METHOD_KF>(method, go);
}
}  // namespace
#endif

#ifdef UVS_PER_TRIAL
bool uvs_launch::UVS_TU_NAME(int method, bool xo, int64_t T, hipStream_t s, const uvs::ClosedGridArgs &A) {
    return dispatch<UVS_TU_METHODS>(method, [&](auto meth) { launch_dh<8, 6, 2, decltype(meth)::value>(xo, grid_for(T, 2), s, A); });
}
#else
#ifdef UVS_TU_EMU2                      // this translation unit also carries the four-lane kernels with the two-lane kernel's bits (rmckf_tuned.hpp, EMU2)
bool uvs_launch::closed_tuned_emu2(int method, bool xo, int64_t T, hipStream_t s, const uvs::ClosedArgs &A) {
    return launch<8, 6, 4, true>(method, false, xo, grid_for(T, 4), s, A);
}
#endif

bool uvs_launch::UVS_TU_NAME(int m, int n, int L, int method, bool linear, bool xo, int64_t T, hipStream_t s, const uvs::ClosedArgs &A) {
#define X(M, N, LL) \
    if (m == M && n == N && L == LL) return launch<M, N, LL>(method, linear, xo, grid_for(T, LL), s, A);
    UVS_TU_SHAPES(X)
#undef X
    return false;
}
#endif
