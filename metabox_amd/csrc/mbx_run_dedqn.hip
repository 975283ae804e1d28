// mbx_run_dedqn.hip — DEDQN: the kernels (mbx_dedqn.hpp), their host code and entry point, a translation unit of their own so that `make -j` compiles
// them beside mbx.hip and the code objects of the other kernels do not depend on them; mbx.hip sees the row kDedqnOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_dedqn.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int dedqn_check(const mbx_algo_cfg& c)
{
    // the landscape analysis deals one row per lane of two waves, and LDS holds the population three times over
    if (c.np < 4 || c.np > MBX_DEDQN_NP_MAX) return fail(MBX_E_ARG, "DEDQN runs np in [4, %d], not %d", MBX_DEDQN_NP_MAX, c.np);
    if (c.dim < 2 || c.dim > MBX_DEDQN_DIM_MAX) return fail(MBX_E_ARG, "DEDQN runs dim in [2, %d], not %d", MBX_DEDQN_DIM_MAX, c.dim);
    return MBX_OK;
}

static AlgoGeom dedqn_geom(const mbx_algo_cfg& c) { return MBX_GEOM(DEDQN, dd_lds_doubles(c.np, c.dim), MBX_DEDQN_NFEAT, 1); }
static int dedqn_prepare(mbx_batch* b, const AlgoGeom& g)
{
    if (int rc = allow_lds(lds_of(g), k_dedqn_reset, k_dedqn_step, k_dedqn_run)) return rc;
    // cal_rie's frequencies are n / NP: their logarithms, correctly rounded (extended precision, then one rounding to double), so that the kernel's
    // entropies do not depend on the device's log (mbx_dedqn.hpp: dd_features); the batch's table pointer `pci` carries them
    std::vector<double> lt(b->cfg.np + 1, 0.);
    for (int n = 1; n < b->cfg.np; ++n) lt[n] = (double)std::log((long double)((double)n / (double)b->cfg.np));
    HIP_TRY(hipMalloc(&b->d_pci, lt.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(b->d_pci, lt.data(), lt.size() * sizeof(double), hipMemcpyHostToDevice));
    return MBX_OK;
}

MBX_RESET_FN(dedqn_reset) { MBX_LAUNCH(k_dedqn_reset, kThreads, b->lds_bytes, d_state_out); }
MBX_STEP_FN(dedqn_step) { MBX_LAUNCH(k_dedqn_step, kThreads, b->lds_bytes, (const int32_t*)d_actions, MBX_OUT); return MBX_OK; }

MBX_EXPORT_ROW(kDedqnOps, MBX_ALGO_DEDQN, "DEDQN", true, false, dedqn_check, dedqn_geom, dedqn_prepare, dedqn_reset, dedqn_step, nullptr);

extern "C" int mbx_dedqn_rollout(mbx_batch* b, const mbx_dedqn_net* net, int n_steps, int32_t* d_traj_actions, double* d_traj_state,
                                 double* d_traj_reward, int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out,
                                 void* stream_)
{
    if (!b || !net || !net->d_weights) return fail(MBX_E_ARG, "mbx_dedqn_rollout: bad arguments");
    if (b->cfg.algo != MBX_ALGO_DEDQN) return fail(MBX_E_UNSUPPORTED, "mbx_dedqn_rollout: the batch is not a DEDQN batch");
    if (net->in_dim != MBX_DEDQN_NFEAT || net->hidden != 10 || net->n_act != 3)
        return fail(MBX_E_UNSUPPORTED, "mbx_dedqn_rollout: only the reference's 4 -> 10 -> 10 -> 3 network is built");
    if (n_steps < 1) return fail(MBX_E_ARG, "mbx_dedqn_rollout: n_steps must be >= 1");
    if (b->d_tape && n_steps != 1) return fail(MBX_E_ARG, "mbx_dedqn_rollout: a replay tape holds one step");
    const hipStream_t stream = (hipStream_t)stream_;
    MBX_LAUNCH(k_dedqn_run, kThreads, b->lds_bytes, net->d_weights, n_steps, DedqnTraj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out}, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
