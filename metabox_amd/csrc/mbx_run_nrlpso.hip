// mbx_run_nrlpso.hip — the NRLPSO kernels (mbx_nrlpso.hpp) and their launch code, a translation unit of their own like mbx_run_dedqn.hip; mbx.hip calls
// the nrlpso_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_nrlpso.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

bool nrlpso_cached(int np, int dim, uint32_t flags, size_t max_lds_bytes)
{
    return !(flags & MBX_F_NRLPSO_RECOMPUTE) && (size_t)nr_lds_doubles(1, np, dim, true, true) * sizeof(double) <= max_lds_bytes;
}

hipError_t nrlpso_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_nrlpso_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_nrlpso_step<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_nrlpso_step<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void nrlpso_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_nrlpso_reset, dim3(bp.B), dim3(kThreads), (size_t)nr_lds_doubles(bp.NP, bp.NP, bp.D, false, false) * sizeof(double), stream, bp,
                       d_state_out);
}

void nrlpso_launch_steps(const BatchParams& bp, bool cached, hipStream_t stream, const int32_t* d_actions, const double* d_q_table, int n_steps,
                         int32_t* d_traj_actions, double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out,
                         double* d_reward_out, uint8_t* d_done_out)
{
    const size_t lds = (size_t)nr_lds_doubles(1, bp.NP, bp.D, true, cached) * sizeof(double);
    const NrTraj traj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out};
    if (n_steps == 1)
        hipLaunchKernelGGL(k_nrlpso_step<false>, dim3(bp.B), dim3(kThreads), lds, stream, bp, d_actions, d_q_table, 1, (int)cached, traj, d_state_out,
                           d_reward_out, d_done_out);
    else
        hipLaunchKernelGGL(k_nrlpso_step<true>, dim3(bp.B), dim3(kThreads), lds, stream, bp, d_actions, d_q_table, n_steps, (int)cached, traj, d_state_out,
                           d_reward_out, d_done_out);
}

}  // namespace mbx
