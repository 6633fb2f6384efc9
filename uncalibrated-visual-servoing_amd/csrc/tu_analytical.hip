// Calibrated IBVS baseline (analytical.hpp): first pass and careful second pass, (m, n) = (8, 6) on the DH / pinhole plant.
#include "launchers.hpp"
#include "analytical.hpp"

bool uvs_launch::analytical(int m, int n, bool careful, int64_t T, hipStream_t s, const uvs::AnalyticalArgs &A) {
    if (m != 8 || n != 6) return false;
    if (careful) hipLaunchKernelGGL((uvs::analytical_kernel<8, 6, true>), grid_for(T, 1), dim3(64), 0, s, A);
    else hipLaunchKernelGGL((uvs::analytical_kernel<8, 6, false>), grid_for(T, 1), dim3(64), 0, s, A);
    return true;
}
