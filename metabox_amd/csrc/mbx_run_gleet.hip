// mbx_run_gleet.hip — GLEET's resident rollout: the kernel (mbx_gleet_run.hpp), its host code and the two entry points of include/mbx_gleet.h, a translation
// unit of their own like mbx_run_l2l.hip.  The batch itself (reset, mbx_step, mbx_gleet_policy and the row kGleetOps) stays in mbx.hip; of the two GLEET
// headers this unit takes the device functions only, not the three kernels mbx.hip instantiates.
#include <hip/hip_runtime.h>
#define MBX_GLEET_DEVICE_FUNCTIONS_ONLY
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_gleet_run.hpp"
#include "mbx_host.hpp"

namespace mbx {

static size_t gleet_run_lds_bytes(const mbx_batch* b) { return (size_t)glr_lds_doubles(b->cfg.np, b->cfg.dim) * sizeof(double); }

static void gleet_launch_run(mbx_batch* b, hipStream_t stream, const GlrArgs& ar)
{
    if (b->fixed_geometry == 5) MBX_LAUNCH((k_gleet_run<100, 10>), kThreads, gleet_run_lds_bytes(b), ar);
    else MBX_LAUNCH(k_gleet_run<>, kThreads, gleet_run_lds_bytes(b), ar);       // the run-time-geometry body, at 100 x 10 as well under MBX_F_GENERIC_GEOMETRY
}

extern "C" int mbx_gleet_set_params(mbx_batch* b, const float* d_weights, int n_sets, const int32_t* d_set_of_instance, float min_sigma, float max_sigma)
{
    if (!b || !d_weights || n_sets < 1) return fail(MBX_E_ARG, "mbx_gleet_set_params: bad arguments");
    if (b->cfg.algo != MBX_ALGO_GLEET) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_set_params: the batch is not a GLEET batch");
    if (b->cfg.np > kGpThreads) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_set_params: np %d > %d, the actor's limit", b->cfg.np, kGpThreads);
    const size_t lds = gleet_run_lds_bytes(b);
    if (lds > (size_t)max_lds_bytes()) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_set_params: the resident kernel needs %zu bytes of LDS at np %d, dim %d", lds, b->cfg.np, b->cfg.dim);
    if (const int rc = allow_lds(lds, k_gleet_run<>, k_gleet_run<100, 10>)) return rc;
    if (const int rc = set_param_sets(b, "mbx_gleet_set_params", d_weights, (size_t)GpOff::total * sizeof(float), n_sets, d_set_of_instance)) return rc;
    b->gleet_min_sigma = min_sigma; b->gleet_max_sigma = max_sigma;
    return MBX_OK;
}

extern "C" int mbx_gleet_rollout(mbx_batch* b, int n_steps, double* d_state, float* d_traj_actions, float* d_traj_mu_sigma, double* d_traj_reward,
                                 double* d_reward_out, uint8_t* d_done_out, void* stream)
{
    if (!b || !d_state) return fail(MBX_E_ARG, "mbx_gleet_rollout: bad arguments");
    if (b->cfg.algo != MBX_ALGO_GLEET) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_rollout: the batch is not a GLEET batch");
    if (b->cfg.np > kGpThreads) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_rollout: np %d > %d, the actor's limit", b->cfg.np, kGpThreads);
    if (b->d_tape) return fail(MBX_E_UNSUPPORTED, "mbx_gleet_rollout: the batch has a replay tape (the reference's actions come from torch's generator)");
    if (!b->sets.d_params) return fail(MBX_E_ARG, "GLEET: no weights yet, call mbx_gleet_set_params first");
    if (n_steps < 1) return fail(MBX_E_ARG, "mbx_gleet_rollout: n_steps must be >= 1");
    GlrArgs ar{(const float*)b->sets.d_params, b->sets.d_set, b->gleet_min_sigma, b->gleet_max_sigma, n_steps, 0, d_state,
               d_traj_actions, d_traj_mu_sigma, d_traj_reward, d_reward_out, d_done_out};
    if (b->rollout_per_generation) {
        const int64_t row = (int64_t)b->B * b->cfg.np;
        ar.n_steps = 1;
        for (int g = 0; g < n_steps; ++g) {
            ar.accumulate = g > 0;
            ar.traj_actions = d_traj_actions ? d_traj_actions + g * row : nullptr;
            ar.traj_mu_sigma = d_traj_mu_sigma ? d_traj_mu_sigma + g * 2 * row : nullptr;
            ar.traj_reward = d_traj_reward ? d_traj_reward + (int64_t)g * b->B : nullptr;
            gleet_launch_run(b, (hipStream_t)stream, ar);
        }
    } else gleet_launch_run(b, (hipStream_t)stream, ar);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
