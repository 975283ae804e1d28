// mbx_run_symbol.hip — the SYMBOL kernels (mbx_symbol.hpp) and their launch code, a translation unit of their own like mbx_run_l2l.hip; mbx.hip calls
// the symbol_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_symbol.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

static size_t symbol_lds_bytes(const BatchParams& bp) { return (size_t)sym_lds_doubles(bp.NP, bp.D, sym_resident(bp.NP, bp.D)) * sizeof(double); }

hipError_t symbol_prepare(size_t lds_bytes)
{
    // the dynamic size was chosen with kSymStaticLdsMax bytes left for the kernels' static LDS (sym_resident): hold every kernel to that, so that a launch
    // can never ask for more than the workgroup has
    hipError_t e = hipSuccess;
    for (const void* k : {(const void*)k_symbol_reset, (const void*)k_symbol_step, (const void*)k_symbol_run}) {
        hipFuncAttributes at{};
        if (e == hipSuccess) e = hipFuncGetAttributes(&at, k);
        if (e == hipSuccess && ((int64_t)at.sharedSizeBytes > kSymStaticLdsMax || (int64_t)lds_bytes + (int64_t)at.sharedSizeBytes > kSymLdsLimit)) e = hipErrorLaunchOutOfResources;
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    }
    return e;
}

void symbol_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out)
{
    const SymArgs ar{nullptr, nullptr, nullptr, 0, 0, sym_resident(bp.NP, bp.D) ? 1 : 0, nullptr};
    hipLaunchKernelGGL(k_symbol_reset, dim3(bp.B), dim3(kThreads), symbol_lds_bytes(bp), stream, bp, ar, d_state_out);
}

void symbol_launch_run(const BatchParams& bp, hipStream_t stream, const int32_t* d_tokens, const double* d_consts, const double* d_actions, int n_sub,
                       int n_action, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, int32_t* d_n_bad)
{
    const SymArgs ar{d_tokens, d_consts, d_actions, n_sub, n_action, sym_resident(bp.NP, bp.D) ? 1 : 0, d_n_bad};
    if (n_sub == 1)
        hipLaunchKernelGGL(k_symbol_step, dim3(bp.B), dim3(kThreads), symbol_lds_bytes(bp), stream, bp, ar, d_state_out, d_reward_out, d_done_out);
    else
        hipLaunchKernelGGL(k_symbol_run, dim3(bp.B), dim3(kThreads), symbol_lds_bytes(bp), stream, bp, ar, d_state_out, d_reward_out, d_done_out);
}

}  // namespace mbx
