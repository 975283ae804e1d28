// mbx_run_sahlpso.hip — the SAHLPSO kernels (mbx_sahlpso.hpp) and their launch code, a translation unit of their own like mbx_run_nrlpso.hip; mbx.hip
// calls the sahlpso_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_sahlpso.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

hipError_t sahlpso_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_sahlpso_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_sahlpso_generation, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void sahlpso_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_sahlpso_reset, dim3(bp.B), dim3(kThreads), (size_t)sh_lds_doubles(MBX_SAHL_NP, bp.D, false) * sizeof(double), stream, bp, d_state_out);
}

void sahlpso_launch_generation(const BatchParams& bp, hipStream_t stream, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_sahlpso_generation, dim3(bp.B), dim3(kThreads), (size_t)sh_lds_doubles(1, bp.D, true) * sizeof(double), stream, bp, d_state_out,
                       d_reward_out, d_done_out);
}

}  // namespace mbx
