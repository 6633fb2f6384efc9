// Shared body of tu_closed_grid_{a,b}.hip, which define UVS_PER_TRIAL: the per-trial-parameter flavour of the tuned closed-loop kernel
// (closed_loop_grid_kernel, rmckf_tuned.hpp) at (8,6), two lanes per filter, DH plant -- what uvs_rmckf_closed_loop_grid_f64 launches.
// UVS_TU_GRID_NAME and UVS_TU_GRID_METHODS are defined by the including file.  The choices below mirror launch2 / launch_dh of tu_closed_tuned.inc for the instantiations that exist here, so that a grid
// launch runs the arithmetic of the uniform launch it replaces: the axis-aligned chain for a UR10-like table, whole trials or segments as planned.
#include "launchers.hpp"
#include "rmckf_tuned.hpp"

#ifndef UVS_CLOSED_GRID_HELPERS            // the unity build (uvs_unity.hip) includes this file twice
#define UVS_CLOSED_GRID_HELPERS
namespace {
inline bool grid_axis_aligned(const uvs_plant &p) {              // (axis_aligned of tu_closed_tuned.inc)
    if (p.n_joints != 6) return false;
    for (int g = 0; g < 6; g += 3)
        if (!(p.sin_alpha[g] == -1.0 && p.cos_alpha[g] > -1e-15 && p.cos_alpha[g] < 1e-15 && p.cos_alpha[g + 2] == 1.0 && p.sin_alpha[g + 2] == 0.0)) return false;
    return true;
}
template <int METHOD, int PLANT>
void launch_grid(bool xo, dim3 g, hipStream_t s, const uvs::ClosedGridArgs &A) {
    constexpr int M = 8, N = 6, LL = 2, PV = 2;
    if (A.n_seg > 1) {                                           // the plan cuts MCKF and RMCKF launches only
        uvs_launch::fill_i32(A.ws_flags, 0, (long long)g.x + 1, s);
        g.x *= (unsigned)A.n_seg;
        if constexpr (METHOD == UVS_METHOD_GMCKF) {
            if (xo) hipLaunchKernelGGL((uvs::closed_loop_grid_kernel<M, N, LL, METHOD, PLANT, PV, true, false, true>), g, dim3(64), 0, s, A);
            else hipLaunchKernelGGL((uvs::closed_loop_grid_kernel<M, N, LL, METHOD, PLANT, PV, false, false, true>), g, dim3(64), 0, s, A);
            return;
        }
    }
    if (xo) hipLaunchKernelGGL((uvs::closed_loop_grid_kernel<M, N, LL, METHOD, PLANT, PV, true>), g, dim3(64), 0, s, A);
    else hipLaunchKernelGGL((uvs::closed_loop_grid_kernel<M, N, LL, METHOD, PLANT, PV, false>), g, dim3(64), 0, s, A);
}
}  // namespace
#endif

bool uvs_launch::UVS_TU_GRID_NAME(int method, bool xo, int64_t T, hipStream_t s, const uvs::ClosedGridArgs &A) {
    const bool axis = grid_axis_aligned(A.plant);
    return dispatch<UVS_TU_GRID_METHODS>(method, [&](auto meth) {
        constexpr int METHOD = decltype(meth)::value;
        if (axis) launch_grid<METHOD, uvs::kPlantDhAxisAligned>(xo, grid_for(T, 2), s, A);
        else launch_grid<METHOD, UVS_PLANT_DH_PINHOLE>(xo, grid_for(T, 2), s, A);
    });
}
