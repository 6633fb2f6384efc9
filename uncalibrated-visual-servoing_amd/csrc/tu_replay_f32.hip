// Single-precision estimator-only replay (rmckf_replay_f32.hpp): estimator and "stream wanted" flags are compile-time.
#include "launchers.hpp"
#include "rmckf_replay_f32.hpp"

bool uvs_launch::replay_f32(int m, int n, int method, int64_t T, hipStream_t s, const uvs::ReplayArgs32 &A) {
    if (m != 8 || n != 6) return false;
    return dispatch<UVS_METHOD_GMCKF, UVS_METHOD_IMCCKF, UVS_METHOD_KF>(method, [&](auto meth) { with_flags([&](auto x, auto e) {
        hipLaunchKernelGGL((uvs::replay_f32_kernel<decltype(meth)::value, decltype(x)::value, decltype(e)::value>), grid_for(T, 2), dim3(64), 0, s, A);
    }, A.x_out.p != nullptr, A.err_out.p != nullptr); });
}
