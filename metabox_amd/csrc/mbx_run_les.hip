// mbx_run_les.hip — LES: the kernels (mbx_les.hpp), their host code and entry points, a translation unit of their own like mbx_run_sahlpso.hip; mbx.hip
// sees the row kLesOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_les.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int les_check(const mbx_algo_cfg& c)
{
    // 16 samples per generation, one lane of wave 0 per row and per dimension; the 16 initial evaluations are spent by mbx_reset
    if (c.np != MBX_LES_NP) return fail(MBX_E_ARG, "LES runs np = %d, not %d", MBX_LES_NP, c.np);
    if (c.dim < 2 || c.dim > MBX_LES_DIM_MAX) return fail(MBX_E_ARG, "LES runs dim in [2, %d], not %d", MBX_LES_DIM_MAX, c.dim);
    if (c.max_fes <= MBX_LES_NP) return fail(MBX_E_ARG, "LES needs max_fes > %d (the initial evaluation), not %d", MBX_LES_NP, c.max_fes);
    return MBX_OK;
}

static AlgoGeom les_geom(const mbx_algo_cfg& c)
{
    return AlgoGeom{MBX_LES_STATE_DOUBLES(c.np, c.dim, MBX_LES_CURVE_CAP(c.max_fes, c.log_interval, c.n_logpoint)), MBX_LES_ST_SCALARS(c.np, c.dim),
                    MBX_LES_TAPE_STRIDE(c.np, c.dim), les_lds_doubles(c.dim), 1, 0};
}

static int les_prepare(mbx_batch* b, const AlgoGeom& g)
{
    if (int rc = allow_lds(lds_of(g), k_les_reset, k_les_run)) return rc;
    // the timestamp embedding (les_optimizer.py:110): tanh(t / timestamp - 1) rounded to float32, as the reference's float64 numpy row is when it
    // enters the MLP; made in extended precision and rounded once to double, then to float, so that it does not depend on the device's tanh
    static const int stamps[MBX_LES_NTS] = {1, 3, 10, 30, 50, 100, 250, 500, 750, 1000, 1250, 1500, 2000};
    b->les_horizon = b->cfg.max_fes / MBX_LES_NP + MBX_LES_TS_MARGIN;
    std::vector<float> ts((size_t)(b->les_horizon + 1) * MBX_LES_NTS);
    for (int t = 0; t <= b->les_horizon; ++t)
        for (int k = 0; k < MBX_LES_NTS; ++k) ts[(size_t)t * MBX_LES_NTS + k] = (float)(double)std::tanh((long double)((double)t / (double)stamps[k] - 1.));
    HIP_TRY(hipMalloc(&b->d_les_ts, ts.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(b->d_les_ts, ts.data(), ts.size() * sizeof(float), hipMemcpyHostToDevice));
    return MBX_OK;
}

MBX_RESET_FN(les_reset) { MBX_LAUNCH(k_les_reset, kThreads, (size_t)les_lds_doubles(b->cfg.dim) * sizeof(double), d_state_out); }

// skip = 0: up to n_gens generations under the budget / early-stop end rule; skip = 1: steps step0 .. step0 + n_gens - 1 of a skip_step call of skip_total steps
static void les_launch_run(mbx_batch* b, hipStream_t stream, int n_gens, int skip, int step0, int skip_total, double* d_state_out, double* d_reward_out,
                           uint8_t* d_done_out)
{
    const LesArgs ar{(const float*)b->sets.d_params, b->sets.d_set, b->sets.n_sets, b->d_les_ts, b->les_horizon, n_gens, skip, step0, skip_total};
    MBX_LAUNCH(k_les_run, kThreads, (size_t)les_lds_doubles(b->cfg.dim) * sizeof(double), ar, MBX_OUT);
}

MBX_STEP_FN(les_step) { (void)d_actions; return mbx_les_rollout(b, 1, 0, MBX_OUT, stream); }   // one generation of the budget route

MBX_EXPORT_ROW(kLesOps, MBX_ALGO_LES, "LES", false, false, les_check, les_geom, les_prepare, les_reset, les_step, nullptr);

extern "C" int mbx_les_set_params(mbx_batch* b, const float* d_params, int n_sets, const int32_t* d_set_of_instance)
{
    if (!b || !d_params || n_sets < 1) return fail(MBX_E_ARG, "mbx_les_set_params: bad arguments");
    if (b->cfg.algo != MBX_ALGO_LES) return fail(MBX_E_UNSUPPORTED, "mbx_les_set_params: the batch is not an LES batch");
    return set_param_sets(b, "mbx_les_set_params", d_params, MBX_LES_NPARAM * sizeof(float), n_sets, d_set_of_instance);
}

extern "C" int mbx_les_rollout(mbx_batch* b, int n_gens, int skip, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream)
{
    if (!b) return fail(MBX_E_ARG, "mbx_les_rollout: null batch");
    if (b->cfg.algo != MBX_ALGO_LES) return fail(MBX_E_UNSUPPORTED, "mbx_les_rollout: the batch is not an LES batch");
    if (!b->sets.d_params) return fail(MBX_E_ARG, "LES: no parameters yet, call mbx_les_set_params first");
    if (n_gens < 1 || (skip != 0 && skip != 1)) return fail(MBX_E_ARG, "mbx_les_rollout: n_gens must be >= 1 and skip 0 or 1");
    if (b->d_tape && n_gens != 1) return fail(MBX_E_ARG, "mbx_les_rollout: a replay tape holds one generation");
    if (b->rollout_per_generation)
        for (int g = 0; g < n_gens; ++g) les_launch_run(b, (hipStream_t)stream, 1, skip, g, n_gens, MBX_OUT);
    else les_launch_run(b, (hipStream_t)stream, n_gens, skip, 0, n_gens, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
