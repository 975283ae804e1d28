// mbx_run_rlhpsde.hip — the RL-HPSDE kernels (mbx_rlhpsde.hpp) and their launch code, a translation unit of their own like mbx_run_nrlpso.hip; mbx.hip calls
// the rlhpsde_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_rlhpsde.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

hipError_t rlhpsde_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_rlhpsde_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_rlhpsde_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_rlhpsde_run, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void rlhpsde_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_rlhpsde_reset, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_state_out);
}

void rlhpsde_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const int32_t* d_actions, double* d_state_out, double* d_reward_out,
                         uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_rlhpsde_step, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_actions, d_state_out, d_reward_out, d_done_out);
}

void rlhpsde_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const double* d_q_table, int n_steps, int32_t* d_traj_actions,
                        double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    const HpTraj traj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out};
    hipLaunchKernelGGL(k_rlhpsde_run, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_q_table, n_steps, traj, d_state_out, d_reward_out, d_done_out);
}

}  // namespace mbx
