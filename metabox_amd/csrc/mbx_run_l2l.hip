// mbx_run_l2l.hip — the L2L kernels (mbx_l2l.hpp) and their launch code, a translation unit of their own like mbx_run_les.hip; mbx.hip calls the
// l2l_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_l2l.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

static size_t l2l_lds_bytes(int D) { return (size_t)l2l_lds_doubles(D) * sizeof(double); }

hipError_t l2l_prepare(size_t lds_bytes)
{
    hipError_t e = hipSuccess;
    for (const void* k : {(const void*)k_l2l_reset, (const void*)k_l2l_step, (const void*)k_l2l_run<0>, (const void*)k_l2l_run<10>})
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void l2l_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_l2l_reset, dim3(bp.B), dim3(kThreads), l2l_lds_bytes(bp.D), stream, bp, d_state_out);
}

void l2l_launch_step(const BatchParams& bp, hipStream_t stream, const double* d_x_raw, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_l2l_step, dim3(bp.B), dim3(kThreads), l2l_lds_bytes(bp.D), stream, bp, d_x_raw, d_state_out, d_reward_out, d_done_out);
}

void l2l_launch_run(const BatchParams& bp, bool generic, hipStream_t stream, const double* d_params, const int32_t* d_set_of, int n_sets, int n_steps,
                    double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    const L2lArgs ar{d_params, d_set_of, n_sets, n_steps};
    if (bp.D == 10 && !generic)
        hipLaunchKernelGGL(k_l2l_run<10>, dim3(bp.B), dim3(kThreads), l2l_lds_bytes(bp.D), stream, bp, ar, d_state_out, d_reward_out, d_done_out);
    else
        hipLaunchKernelGGL(k_l2l_run<0>, dim3(bp.B), dim3(kThreads), l2l_lds_bytes(bp.D), stream, bp, ar, d_state_out, d_reward_out, d_done_out);
}

}  // namespace mbx
