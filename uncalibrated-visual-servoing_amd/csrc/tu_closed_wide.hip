// Tuned closed-loop kernel of the wide stress shape (rmckf_wide.hpp): (32,7), 8 lanes per filter, linear plant, estimator in
// {KF, IMCCKF, GMCKF} -- and the same kernel on the DH / pinhole plant at (8,6), one row per lane: lanes_per_filter = 8.
#include "launchers.hpp"
#include "rmckf_wide.hpp"

namespace {
template <int M, int N, int LL, int METHOD>
void launch_wide(bool xo, dim3 g, hipStream_t s, const uvs::ClosedArgs &A) {
    // per-trial records ([step][trial][component]) and a whole number of wavefronts: X leaves through the LDS transposition as 1 KB stores
    // (the record path stores double2: the base must be 16-byte aligned and the step stride even, or the strided variant takes over)
    const bool rec = xo && A.x_out.sc == 1 && A.x_out.st == M * N && A.T % (64 / LL) == 0 && (uintptr_t)A.x_out.p % 16 == 0 && A.x_out.sk % 2 == 0;
    if (rec) hipLaunchKernelGGL((uvs::closed_loop_wide_kernel<M, N, LL, METHOD, true, true>), g, dim3(64), 0, s, A);
    else if (xo) hipLaunchKernelGGL((uvs::closed_loop_wide_kernel<M, N, LL, METHOD, true, false>), g, dim3(64), 0, s, A);
    else hipLaunchKernelGGL((uvs::closed_loop_wide_kernel<M, N, LL, METHOD, false, false>), g, dim3(64), 0, s, A);
}
template <int METHOD>
void launch_latency(bool xo, dim3 g, hipStream_t s, const uvs::ClosedArgs &A) {
    if (xo) hipLaunchKernelGGL((uvs::closed_loop_wide_kernel<8, 6, 8, METHOD, true, false, UVS_PLANT_DH_PINHOLE>), g, dim3(64), 0, s, A);
    else hipLaunchKernelGGL((uvs::closed_loop_wide_kernel<8, 6, 8, METHOD, false, false, UVS_PLANT_DH_PINHOLE>), g, dim3(64), 0, s, A);
}
}  // namespace

bool uvs_launch::closed_wide(int m, int n, int L, int method, bool xo, int64_t T, hipStream_t s, const uvs::ClosedArgs &A) {
    const dim3 g = grid_for(T, L);
    return dispatch<UVS_METHOD_GMCKF, UVS_METHOD_IMCCKF, UVS_METHOD_KF>(method, [&](auto meth) {
        constexpr int METHOD = decltype(meth)::value;
        if (m == 8 && n == 6 && L == 8) launch_latency<METHOD>(xo, g, s, A);   // (explicit lanes_per_filter = 8 only: measured, not faster than four lanes)
        else if (m == 32 && n == 7 && L == 8) launch_wide<32, 7, 8, METHOD>(xo, g, s, A);
        else if (m == 32 && n == 7 && L == 16) launch_wide<32, 7, 16, METHOD>(xo, g, s, A);
        else return false;
        return true;
    });
}
