// mbx_run_l2l.hip — L2L: the kernels (mbx_l2l.hpp), their host code and entry points, a translation unit of their own like mbx_run_les.hip; mbx.hip sees
// the row kL2lOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_l2l.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int l2l_check(const mbx_algo_cfg& c)
{
    // one point per step: a single evaluation row; one lane of wave 0 per dimension
    if (c.np != 1) return fail(MBX_E_ARG, "L2L runs np = 1 (one point per step), not %d", c.np);
    if (c.dim < 2 || c.dim > MBX_L2L_DIM_MAX) return fail(MBX_E_ARG, "L2L runs dim in [2, %d], not %d", MBX_L2L_DIM_MAX, c.dim);
    return MBX_OK;
}

static size_t l2l_lds_bytes(const mbx_batch* b) { return (size_t)l2l_lds_doubles(b->cfg.dim) * sizeof(double); }
static AlgoGeom l2l_geom(const mbx_algo_cfg& c) { return MBX_GEOM(L2L, l2l_lds_doubles(c.dim), 1, c.dim); }
static int l2l_prepare(mbx_batch*, const AlgoGeom& g) { return allow_lds(lds_of(g), k_l2l_reset, k_l2l_step, k_l2l_run<0>, k_l2l_run<10>); }
MBX_RESET_FN(l2l_reset) { MBX_LAUNCH(k_l2l_reset, kThreads, l2l_lds_bytes(b), d_state_out); }
MBX_STEP_FN(l2l_step) { MBX_LAUNCH(k_l2l_step, kThreads, l2l_lds_bytes(b), (const double*)d_actions, MBX_OUT); return MBX_OK; }   // the host ran the cell: actions = x_raw [B, D]

static void l2l_launch_run(mbx_batch* b, hipStream_t stream, int n_steps, double* d_state_out, double* d_reward_out, uint8_t* d_done_out)
{
    const L2lArgs ar{(const double*)b->sets.d_params, b->sets.d_set, b->sets.n_sets, n_steps};
    if (b->cfg.dim == 10 && !generic_geometry(b)) MBX_LAUNCH(k_l2l_run<10>, kThreads, l2l_lds_bytes(b), ar, MBX_OUT);
    else MBX_LAUNCH(k_l2l_run<0>, kThreads, l2l_lds_bytes(b), ar, MBX_OUT);      // the run-time-D body, at D = 10 as well under MBX_F_GENERIC_GEOMETRY
}

MBX_EXPORT_ROW(kL2lOps, MBX_ALGO_L2L, "L2L", true, false, l2l_check, l2l_geom, l2l_prepare, l2l_reset, l2l_step, nullptr);

extern "C" int mbx_l2l_set_params(mbx_batch* b, const double* d_params, int n_sets, const int32_t* d_set_of_instance)
{
    if (!b || !d_params || n_sets < 1) return fail(MBX_E_ARG, "mbx_l2l_set_params: bad arguments");
    if (b->cfg.algo != MBX_ALGO_L2L) return fail(MBX_E_UNSUPPORTED, "mbx_l2l_set_params: the batch is not an L2L batch");
    return set_param_sets(b, "mbx_l2l_set_params", d_params, (size_t)MBX_L2L_NPARAM(b->cfg.dim) * sizeof(double), n_sets, d_set_of_instance);
}

extern "C" int mbx_l2l_rollout(mbx_batch* b, int n_steps, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream)
{
    if (!b) return fail(MBX_E_ARG, "mbx_l2l_rollout: null batch");
    if (b->cfg.algo != MBX_ALGO_L2L) return fail(MBX_E_UNSUPPORTED, "mbx_l2l_rollout: the batch is not an L2L batch");
    if (!b->sets.d_params) return fail(MBX_E_ARG, "L2L: no weights yet, call mbx_l2l_set_params first");
    if (n_steps < 1) return fail(MBX_E_ARG, "mbx_l2l_rollout: n_steps must be >= 1");
    if (b->d_tape && n_steps != 1) return fail(MBX_E_ARG, "mbx_l2l_rollout: a replay tape holds one step");
    if (b->rollout_per_generation)
        for (int g = 0; g < n_steps; ++g) l2l_launch_run(b, (hipStream_t)stream, 1, MBX_OUT);
    else l2l_launch_run(b, (hipStream_t)stream, n_steps, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
