// The careful pass behind uvs_rmckf_closed_loop_grid_f64: the generic CAREFUL kernel at (8,6), four lanes per filter, in its per-trial flavour
// (UVS_PER_TRIAL: closed_loop_grid_generic_kernel) -- a marked trial is redone with its own parameters and inputs.
#define UVS_PER_TRIAL
#include "launchers.hpp"
#include "rmckf_generic.hpp"

bool uvs_launch::closed_grid_careful(int64_t T, hipStream_t s, const uvs::ClosedGridArgs &A) {
    hipLaunchKernelGGL((uvs::closed_loop_grid_generic_kernel<8, 6, 4, 0, true>), grid_for(T, 4), dim3(64), 0, s, A);
    return true;
}
