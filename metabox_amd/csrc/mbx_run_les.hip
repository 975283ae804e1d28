// mbx_run_les.hip — the LES kernels (mbx_les.hpp) and their launch code, a translation unit of their own like mbx_run_sahlpso.hip; mbx.hip calls the
// les_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_les.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

hipError_t les_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_les_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_les_run, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void les_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_les_reset, dim3(bp.B), dim3(kThreads), (size_t)les_lds_doubles(bp.D) * sizeof(double), stream, bp, d_state_out);
}

void les_launch_run(const BatchParams& bp, hipStream_t stream, const float* d_params, const int32_t* d_set_of, int n_sets, const float* d_ts, int horizon,
                    int n_gens, int skip, int step0, int skip_total, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    const LesArgs ar{d_params, d_set_of, n_sets, d_ts, horizon, n_gens, skip, step0, skip_total};
    hipLaunchKernelGGL(k_les_run, dim3(bp.B), dim3(kThreads), (size_t)les_lds_doubles(bp.D) * sizeof(double), stream, bp, ar, d_state_out, d_reward_out,
                       d_done_out);
}

}  // namespace mbx
