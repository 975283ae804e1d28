// mbx_run_rlhpsde.hip — RL-HPSDE: the kernels (mbx_rlhpsde.hpp), their host code and entry point, a translation unit of their own like
// mbx_run_nrlpso.hip; mbx.hip sees the row kRlhpsdeOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_rlhpsde.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int rlhpsde_check(const mbx_algo_cfg& c)
{
    // 18 dim rows shrinking towards 4, a thread owns a block of rows; the initial evaluation and the first walk (201 points) are spent by mbx_reset
    if (c.dim < 2 || c.dim > MBX_RLHPSDE_DIM_MAX) return fail(MBX_E_ARG, "RL-HPSDE runs dim in [2, %d], not %d", MBX_RLHPSDE_DIM_MAX, c.dim);
    if (c.np != MBX_RLHPSDE_NP(c.dim)) return fail(MBX_E_ARG, "RL-HPSDE runs np = 18 dim = %d, not %d", MBX_RLHPSDE_NP(c.dim), c.np);
    if (c.max_fes <= c.np + MBX_RLHPSDE_WALK)
        return fail(MBX_E_ARG, "RL-HPSDE needs max_fes > %d (the initial evaluation and the first walk), not %d", c.np + MBX_RLHPSDE_WALK, c.max_fes);
    return MBX_OK;
}

static AlgoGeom rlhpsde_geom(const mbx_algo_cfg& c) { return MBX_GEOM(RLHPSDE, hp_lds_doubles(c.np, c.dim), 1, 1); }
static int rlhpsde_prepare(mbx_batch* b, const AlgoGeom& g)
{
    if (int rc = allow_lds(lds_of(g), k_rlhpsde_reset, k_rlhpsde_step, k_rlhpsde_run)) return rc;
    // DRIE's frequencies are n / 200 (and 1e-15 for an empty class): their logarithms, correctly rounded (extended precision, then one rounding to double), so that
    // the kernel's entropies do not depend on the device's log (mbx_rlhpsde.hpp: hp_walk_state); the batch's table pointer `pci` carries them
    std::vector<double> lt(MBX_RLHPSDE_WALK, 0.);
    lt[0] = (double)std::log((long double)1e-15);
    for (int n = 1; n < MBX_RLHPSDE_WALK - 1; ++n) lt[n] = (double)std::log((long double)((double)n / (double)(MBX_RLHPSDE_WALK - 1)));
    HIP_TRY(hipMalloc(&b->d_pci, lt.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(b->d_pci, lt.data(), lt.size() * sizeof(double), hipMemcpyHostToDevice));
    return MBX_OK;
}

MBX_RESET_FN(rlhpsde_reset) { MBX_LAUNCH(k_rlhpsde_reset, kThreads, b->lds_bytes, d_state_out); }
MBX_STEP_FN(rlhpsde_step) { MBX_LAUNCH(k_rlhpsde_step, kThreads, b->lds_bytes, (const int32_t*)d_actions, MBX_OUT); return MBX_OK; }

MBX_EXPORT_ROW(kRlhpsdeOps, MBX_ALGO_RLHPSDE, "RL-HPSDE", true, false, rlhpsde_check, rlhpsde_geom, rlhpsde_prepare, rlhpsde_reset, rlhpsde_step, nullptr);

// the policy decides in the kernel: d_q_table is the 4 x 4 Q-table
extern "C" int mbx_rlhpsde_rollout(mbx_batch* b, const double* d_q_table, int n_steps, int32_t* d_traj_actions, double* d_traj_state, double* d_traj_reward,
                                   int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream_)
{
    if (!b) return fail(MBX_E_ARG, "mbx_rlhpsde_rollout: null batch");
    if (b->cfg.algo != MBX_ALGO_RLHPSDE) return fail(MBX_E_UNSUPPORTED, "mbx_rlhpsde_rollout: the batch is not an RL-HPSDE batch");
    if (!d_q_table) return fail(MBX_E_ARG, "mbx_rlhpsde_rollout: no Q-table (d_q_table is NULL)");
    if (n_steps < 1) return fail(MBX_E_ARG, "mbx_rlhpsde_rollout: n_steps must be >= 1");
    if (b->d_tape && n_steps != 1) return fail(MBX_E_ARG, "mbx_rlhpsde_rollout: a replay tape holds one step");
    const hipStream_t stream = (hipStream_t)stream_;
    MBX_LAUNCH(k_rlhpsde_run, kThreads, b->lds_bytes, d_q_table, n_steps, HpTraj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out}, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
