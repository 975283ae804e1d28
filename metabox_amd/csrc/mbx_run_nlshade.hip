// mbx_run_nlshade.hip — NL_SHADE_LBC: the kernels (mbx_nlshade.hpp), their host code and entry point, a translation unit of their own like
// mbx_run_rlhpsde.hip; mbx.hip sees the row kNlshadeOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_nlshade.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int nlshade_check(const mbx_algo_cfg& c)
{
    if (c.dim < 2 || c.dim > MBX_NLSHADE_DIM_MAX) return fail(MBX_E_ARG, "NL_SHADE_LBC runs dim in [2, %d], not %d", MBX_NLSHADE_DIM_MAX, c.dim);
    if (c.np != MBX_NLSHADE_NP(c.dim)) return fail(MBX_E_ARG, "NL_SHADE_LBC runs np = 23 dim = %d, not %d", MBX_NLSHADE_NP(c.dim), c.np);
    if (c.max_fes <= c.np) return fail(MBX_E_ARG, "NL_SHADE_LBC needs max_fes > %d (the initial evaluation), not %d", c.np, c.max_fes);
    return MBX_OK;
}

// The population schedule of an episode that runs to the budget (NLPSR, nl_shade_lbc.py:135-147): [0] = the number of updates G, [1 + g] = N after
// update g (N0 for g = 0).  N = round-half-even(N0 + (4 - N0) x^(1 - x)), x = FEs / MaxFEs, the power in long double, rounded once; FEs advances by
// the live population, which only ever shrinks.
static std::vector<double> nlshade_schedule(int np, int max_fes)
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

static AlgoGeom nlshade_geom(const mbx_algo_cfg& c) { return MBX_GEOM(NLSHADE, nl_lds_doubles(c.np, c.dim), 1, 0); }
static int nlshade_prepare(mbx_batch* b, const AlgoGeom& g)
{
    if (int rc = allow_lds(lds_of(g), k_nlshade_reset, k_nlshade_step, k_nlshade_run)) return rc;
    // the population schedule is a function of (dim, max_fes) alone (mbx_nlshade.hpp, quirk 11); the batch's table pointer `pci` carries it
    const std::vector<double> t = nlshade_schedule(b->cfg.np, b->cfg.max_fes);
    HIP_TRY(hipMalloc(&b->d_pci, t.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(b->d_pci, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return MBX_OK;
}

MBX_RESET_FN(nlshade_reset) { MBX_LAUNCH(k_nlshade_reset, kThreads, b->lds_bytes, d_state_out); }
MBX_STEP_FN(nlshade_step) { MBX_LAUNCH(k_nlshade_step, kThreads, b->lds_bytes, MBX_OUT); return MBX_OK; }

MBX_EXPORT_ROW(kNlshadeOps, MBX_ALGO_NLSHADE, "NL_SHADE_LBC", false, false, nlshade_check, nlshade_geom, nlshade_prepare, nlshade_reset, nlshade_step, nullptr);

extern "C" int mbx_nlshade_run(mbx_batch* b, int n_updates, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream_)
{
    if (!b) return fail(MBX_E_ARG, "mbx_nlshade_run: null batch");
    if (b->cfg.algo != MBX_ALGO_NLSHADE) return fail(MBX_E_UNSUPPORTED, "mbx_nlshade_run: the batch is not an NL_SHADE_LBC batch");
    if (n_updates < 1) return fail(MBX_E_ARG, "mbx_nlshade_run: n_updates must be >= 1");
    if (b->d_tape && n_updates != 1) return fail(MBX_E_ARG, "mbx_nlshade_run: a replay tape holds one update");
    const hipStream_t stream = (hipStream_t)stream_;
    MBX_LAUNCH(k_nlshade_run, kThreads, b->lds_bytes, n_updates, MBX_OUT);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
