// mbx_run_dedqn.hip — the DEDQN kernels (mbx_dedqn.hpp) and their launch code, a translation unit of their own so that `make -j` compiles them beside
// mbx.hip and the code objects of the other kernels do not depend on them; mbx.hip calls the dedqn_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_dedqn.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

hipError_t dedqn_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_dedqn_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_dedqn_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_dedqn_run, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void dedqn_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_dedqn_reset, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_state_out);
}

void dedqn_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const int32_t* d_actions, double* d_state_out, double* d_reward_out,
                       uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_dedqn_step, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_actions, d_state_out, d_reward_out, d_done_out);
}

void dedqn_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const float* d_net, int n_steps, int32_t* d_traj_actions,
                      double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_dedqn_run, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_net, n_steps,
                       DedqnTraj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out}, d_state_out, d_reward_out, d_done_out);
}

}  // namespace mbx
