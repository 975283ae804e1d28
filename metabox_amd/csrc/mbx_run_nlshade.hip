// mbx_run_nlshade.hip — the NL_SHADE_LBC kernels (mbx_nlshade.hpp) and their launch code, a translation unit of their own like mbx_run_rlhpsde.hip; mbx.hip
// calls the nlshade_* functions declared in mbx_run_kernels.hpp.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_nlshade.hpp"
#include "mbx_run_kernels.hpp"

namespace mbx {

// The population schedule of an episode that runs to the budget (NLPSR, nl_shade_lbc.py:135-147): [0] = the number of updates G, [1 + g] = N after
// update g (N0 for g = 0).  N = round-half-even(N0 + (4 - N0) x^(1 - x)), x = FEs / MaxFEs, the power in long double, rounded once; FEs advances by
// the live population, which only ever shrinks.
std::vector<double> nlshade_schedule(int np, int max_fes)
{
    std::vector<double> t{0., (double)np};
    long long fes = np;
    int live = np;
    while (fes < max_fes) {
        fes += live;
        const long double x = (long double)fes / (long double)max_fes;
        const int n = (int)rintl((long double)np + (long double)(kNlNmin - np) * powl(x, 1.0L - x));
        if (n < live) live = n < 1 ? 1 : n;
        t.push_back((double)n);
    }
    t[0] = (double)(t.size() - 2);
    return t;
}

hipError_t nlshade_prepare(size_t lds_bytes)
{
    hipError_t e = hipFuncSetAttribute((const void*)k_nlshade_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_nlshade_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_nlshade_run, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e;
}

void nlshade_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out)
{
    hipLaunchKernelGGL(k_nlshade_reset, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_state_out);
}

void nlshade_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_nlshade_step, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, d_state_out, d_reward_out, d_done_out);
}

void nlshade_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, int n_updates, double* d_state_out, double* d_reward_out,
                        uint8_t* d_done_out)
{
    hipLaunchKernelGGL(k_nlshade_run, dim3(bp.B), dim3(kThreads), lds_bytes, stream, bp, n_updates, d_state_out, d_reward_out, d_done_out);
}

}  // namespace mbx
