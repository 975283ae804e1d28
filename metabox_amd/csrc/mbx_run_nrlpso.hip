// mbx_run_nrlpso.hip — NRLPSO: the kernels (mbx_nrlpso.hpp), their host code and entry point, a translation unit of their own like mbx_run_dedqn.hip;
// mbx.hip sees the row kNrlpsoOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_nrlpso.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int nrlpso_check(const mbx_algo_cfg& c)
{
    // one lane per row of the distance matrix (two waves), k = 5 neighbours out of np - 1, and LDS holds population and pbest positions
    if (c.np < MBX_NRLPSO_NP_MIN || c.np > MBX_NRLPSO_NP_MAX) return fail(MBX_E_ARG, "NRLPSO runs np in [%d, %d], not %d", MBX_NRLPSO_NP_MIN, MBX_NRLPSO_NP_MAX, c.np);
    if (c.dim < 2 || c.dim > MBX_NRLPSO_DIM_MAX) return fail(MBX_E_ARG, "NRLPSO runs dim in [2, %d], not %d", MBX_NRLPSO_DIM_MAX, c.dim);
    return MBX_OK;
}

// the distance matrix stays in LDS (flag clear and it fits)
static bool nrlpso_cached(const mbx_algo_cfg& c)
{
    return !(c.flags & MBX_F_NRLPSO_RECOMPUTE) && (size_t)nr_lds_doubles(1, c.np, c.dim, true, true) * sizeof(double) <= (size_t)max_lds_bytes();
}

static size_t nrlpso_step_lds(const mbx_batch* b) { return (size_t)nr_lds_doubles(1, b->cfg.np, b->cfg.dim, true, b->nrlpso_cached) * sizeof(double); }

static AlgoGeom nrlpso_geom(const mbx_algo_cfg& c)
{
    // the larger of the reset's carve-up (NP evaluation rows) and the step's (one row, the resident arrays, the distance matrix where it is kept)
    return MBX_GEOM(NRLPSO, std::max(nr_lds_doubles(c.np, c.np, c.dim, false, false), nr_lds_doubles(1, c.np, c.dim, true, nrlpso_cached(c))), 1, 1);
}

static int nrlpso_prepare(mbx_batch* b, const AlgoGeom& g)
{
    b->nrlpso_cached = nrlpso_cached(b->cfg);
    return allow_lds(lds_of(g), k_nrlpso_reset, k_nrlpso_step<false>, k_nrlpso_step<true>);
}

MBX_RESET_FN(nrlpso_reset)
{
    MBX_LAUNCH(k_nrlpso_reset, kThreads, (size_t)nr_lds_doubles(b->cfg.np, b->cfg.np, b->cfg.dim, false, false) * sizeof(double), d_state_out);
}

// d_actions: the caller's actions (mbx_step), or nullptr with the Q-table: the policy decides in the kernel
static void nrlpso_launch_steps(mbx_batch* b, hipStream_t stream, const int32_t* d_actions, const double* d_q_table, int n_steps, const NrTraj& traj,
                                double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    if (n_steps == 1) MBX_LAUNCH(k_nrlpso_step<false>, kThreads, nrlpso_step_lds(b), d_actions, d_q_table, 1, (int)b->nrlpso_cached, traj, MBX_OUT);
    else MBX_LAUNCH(k_nrlpso_step<true>, kThreads, nrlpso_step_lds(b), d_actions, d_q_table, n_steps, (int)b->nrlpso_cached, traj, MBX_OUT);
}

MBX_STEP_FN(nrlpso_step) { nrlpso_launch_steps(b, stream, (const int32_t*)d_actions, nullptr, 1, NrTraj{nullptr, nullptr, nullptr, nullptr}, MBX_OUT); return MBX_OK; }

// the step kernels' LDS (the reset's carve-up is smaller at np = 100)
static void nrlpso_launch_info(const mbx_batch* b, int32_t out[4]) { out[1] = (int32_t)nrlpso_step_lds(b); }

MBX_EXPORT_ROW(kNrlpsoOps, MBX_ALGO_NRLPSO, "NRLPSO", true, false, nrlpso_check, nrlpso_geom, nrlpso_prepare, nrlpso_reset, nrlpso_step, nrlpso_launch_info);

extern "C" int mbx_nrlpso_rollout(mbx_batch* b, const double* d_q_table, int n_steps, int32_t* d_traj_actions, double* d_traj_state, double* d_traj_reward,
                                  int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream)
{
    if (!b || !d_q_table) return fail(MBX_E_ARG, "mbx_nrlpso_rollout: bad arguments");
    if (b->cfg.algo != MBX_ALGO_NRLPSO) return fail(MBX_E_UNSUPPORTED, "mbx_nrlpso_rollout: the batch is not an NRLPSO batch");
    if (n_steps < 1) return fail(MBX_E_ARG, "mbx_nrlpso_rollout: n_steps must be >= 1");
    if (b->d_tape && n_steps != 1) return fail(MBX_E_ARG, "mbx_nrlpso_rollout: a replay tape holds one step");
    nrlpso_launch_steps(b, (hipStream_t)stream, nullptr, d_q_table, n_steps, NrTraj{d_traj_actions, d_traj_state, d_traj_reward, d_actions_out}, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
