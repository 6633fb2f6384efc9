// Tuned replay kernels (rmckf_replay_tuned.hpp): estimator, "X stream wanted" and "control law wanted" are compile-time.
#include "launchers.hpp"
#include "rmckf_replay_tuned.hpp"

#ifndef UVS_REPLAY_PV
#define UVS_REPLAY_PV 2
#endif

#define UVS_ALL_METHODS UVS_METHOD_GMCKF, UVS_METHOD_MCKF, UVS_METHOD_IMCCKF, UVS_METHOD_KF

bool uvs_launch::replay_tuned(int m, int n, int method, bool xo, bool cmd, int64_t T, hipStream_t s, const uvs::ReplayArgs &A) {
#define XR(M, N) \
    if (m == M && n == N) return dispatch<UVS_ALL_METHODS>(method, [&](auto meth) { with_flags([&](auto x, auto c) { \
        hipLaunchKernelGGL((uvs::replay_tuned_kernel<M, N, decltype(meth)::value, UVS_REPLAY_PV, decltype(x)::value, decltype(c)::value>), \
                           grid_for(T, 2), dim3(64), 0, s, A); }, xo, cmd); });
    UVS_TUNED_REPLAY_SHAPES(XR)
#undef XR
    return false;
}

// Estimator-only replay, four lanes per filter, state in registers, two wavefronts per SIMD: (8,6) only.
// Three mappings of the same arithmetic.  Record streams (X and err both [step][trial][component], whole wavefronts of 16 trials, 16-byte
// aligned): lane groups + LDS transposition, 1 KB stores.  Otherwise KF / RMCKF at lanes_per_filter = 0: the four row groups of a filter in
// the four wavefronts of a workgroup of 64 trials (512-byte stores in the trial-fastest layout).  Otherwise four lane groups of one wavefront.
// Estimator in four row-group wavefronts + control law in two more (KF / RMCKF, X, err and the commanded dq all wanted).
bool uvs_launch::replay_rows_cmd(int m, int n, int method, int64_t T, hipStream_t s, const uvs::ReplayArgs &A) {
    if (m != 8 || n != 6) return false;
    const dim3 g((unsigned)((T + 63) / 64));
    return dispatch<UVS_METHOD_GMCKF, UVS_METHOD_KF>(method, [&](auto meth) {
        hipLaunchKernelGGL((uvs::replay_rows_kernel<8, 6, 4, decltype(meth)::value, true, true, true, false, 2>), g, dim3(384), 0, s, A); });
}

bool uvs_launch::replay_rows(int m, int n, int method, bool bywave, bool xo, bool eo, int64_t T, hipStream_t s, const uvs::ReplayArgs &A) {
    if (m != 8 || n != 6) return false;
    const bool rec = xo && eo && T % 16 == 0 && A.x_out.sc == 1 && A.x_out.st == 48 && A.err_out.sc == 1 && A.err_out.st == 8 &&
                     A.x_out.sk % 2 == 0 && A.err_out.sk % 2 == 0 && ((uintptr_t)A.x_out.p | (uintptr_t)A.err_out.p) % 16 == 0;
    if (rec)
        return dispatch<UVS_ALL_METHODS>(method, [&](auto meth) {
            hipLaunchKernelGGL((uvs::replay_rows_kernel<8, 6, 4, decltype(meth)::value, true, true, false, true>), grid_for(T, 4), dim3(64), 0, s, A); });
    if (bywave && dispatch<UVS_METHOD_GMCKF, UVS_METHOD_KF>(method, [&](auto meth) { with_flags([&](auto x, auto e) {
            hipLaunchKernelGGL((uvs::replay_rows_kernel<8, 6, 4, decltype(meth)::value, decltype(x)::value, decltype(e)::value, true>),
                               dim3((unsigned)((T + 63) / 64)), dim3(256), 0, s, A); }, xo, eo); }))
        return true;
    return dispatch<UVS_ALL_METHODS>(method, [&](auto meth) { with_flags([&](auto x, auto e) {
        hipLaunchKernelGGL((uvs::replay_rows_kernel<8, 6, 4, decltype(meth)::value, decltype(x)::value, decltype(e)::value>), grid_for(T, 4), dim3(64), 0, s, A);
    }, xo, eo); });
}
