// mbx_run_symbol.hip — SYMBOL: the kernels (mbx_symbol.hpp), their host code and entry point, a translation unit of their own like mbx_run_l2l.hip;
// mbx.hip sees the row kSymbolOps (mbx_host.hpp) and nothing else.
#include <hip/hip_runtime.h>
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"
#include "mbx_symbol.hpp"
#include "mbx_host.hpp"

namespace mbx {

static int symbol_check(const mbx_algo_cfg& c)
{
    // the index rows are bytes and one lane owns a row in the bookkeeping; the rule's operand gathers and the evaluator share two position buffers.
    // dim >= 2 is the library's common lower bound (check_dim: the evaluator's 2-wide tiles and FastDiv are built for D >= 2), stated here so that SYMBOL's own message names it
    // (a geometry outside these limits is a valid request this build does not implement, like a protein batch: MBX_E_UNSUPPORTED, the code every SYMBOL refusal carries)
    if (c.np < 4 || c.np > MBX_SYM_NP_MAX) return fail(MBX_E_UNSUPPORTED, "SYMBOL runs np in [4, %d], not %d", MBX_SYM_NP_MAX, c.np);
    if (c.dim < 2 || c.dim > MBX_SYM_DIM_MAX) return fail(MBX_E_UNSUPPORTED, "SYMBOL runs dim in [2, %d], not %d", MBX_SYM_DIM_MAX, c.dim);
    return MBX_OK;
}

static size_t symbol_lds_bytes(const mbx_batch* b) { return (size_t)sym_lds_doubles(b->cfg.np, b->cfg.dim, sym_resident(b->cfg.np, b->cfg.dim)) * sizeof(double); }
static AlgoGeom symbol_geom(const mbx_algo_cfg& c) { return MBX_GEOM(SYMBOL, sym_lds_doubles(c.np, c.dim, sym_resident(c.np, c.dim)), MBX_SYM_NFEAT, 2 * MBX_SYM_SLOTS); }

static int symbol_prepare(mbx_batch* b, const AlgoGeom& g)
{
    for (int i = 0; i < b->B; ++i)
        if (b->suite->h_problems[b->h_problem_idx[i]].kind == MBX_KIND_PROTEIN) return fail(MBX_E_UNSUPPORTED, "SYMBOL: protein docking problems are not supported");
    // the dynamic size was chosen with kSymStaticLdsMax bytes left for the kernels' static LDS (sym_resident): hold every kernel to that, so that a launch
    // can never ask for more than the workgroup has
    for (const void* k : {(const void*)k_symbol_reset, (const void*)k_symbol_step, (const void*)k_symbol_run}) {
        hipFuncAttributes at{};
        HIP_TRY(hipFuncGetAttributes(&at, k));
        if ((int64_t)at.sharedSizeBytes > kSymStaticLdsMax || (int64_t)lds_of(g) + (int64_t)at.sharedSizeBytes > kSymLdsLimit)
            return fail(MBX_E_HIP, "symbol_prepare failed: %s", hipGetErrorString(hipErrorLaunchOutOfResources));
        if (int rc = allow_lds(lds_of(g), k)) return rc;
    }
    return MBX_OK;
}

// n_sub sub-steps of an action of n_action; the program as (d_tokens, d_consts) or as d_actions [B, 126] float64
static void symbol_launch(mbx_batch* b, hipStream_t stream, const int32_t* d_tokens, const double* d_consts, const double* d_actions, int n_sub, int n_action,
                          double* d_state_out, double* d_reward_out, uint8_t* d_done_out, int32_t* d_n_bad)
{
    const SymArgs ar{d_tokens, d_consts, d_actions, n_sub, n_action, sym_resident(b->cfg.np, b->cfg.dim) ? 1 : 0, d_n_bad};
    if (n_sub == 1) MBX_LAUNCH(k_symbol_step, kThreads, symbol_lds_bytes(b), ar, MBX_OUT);
    else MBX_LAUNCH(k_symbol_run, kThreads, symbol_lds_bytes(b), ar, MBX_OUT);
}

// all n_action sub-steps in one launch, or one launch each on the host-loop route
static void symbol_launch_action(mbx_batch* b, hipStream_t stream, const int32_t* d_tokens, const double* d_consts, const double* d_actions, int n_action,
                                 double* d_state_out, double* d_reward_out, uint8_t* d_done_out, int32_t* d_n_bad)
{
    if (b->rollout_per_generation)
        for (int g = 0; g < n_action; ++g) symbol_launch(b, stream, d_tokens, d_consts, d_actions, 1, n_action, MBX_OUT, d_n_bad);
    else symbol_launch(b, stream, d_tokens, d_consts, d_actions, n_action, n_action, MBX_OUT, d_n_bad);
}

MBX_RESET_FN(symbol_reset)
{
    const SymArgs ar{nullptr, nullptr, nullptr, 0, 0, sym_resident(b->cfg.np, b->cfg.dim) ? 1 : 0, nullptr};
    MBX_LAUNCH(k_symbol_reset, kThreads, symbol_lds_bytes(b), ar, d_state_out);
}
// the program as actions: MBX_SYM_SKIP sub-steps
MBX_STEP_FN(symbol_step) { symbol_launch_action(b, stream, nullptr, nullptr, (const double*)d_actions, MBX_SYM_SKIP, MBX_OUT, nullptr); return MBX_OK; }

MBX_EXPORT_ROW(kSymbolOps, MBX_ALGO_SYMBOL, "SYMBOL", true, false, symbol_check, symbol_geom, symbol_prepare, symbol_reset, symbol_step, nullptr);

extern "C" int mbx_symbol_rollout(mbx_batch* b, const int32_t* d_tokens, const double* d_consts, int n_substeps, double* d_state_out, double* d_reward_out,
                                  uint8_t* d_done_out, int32_t* d_n_bad, void* stream)
{
    if (!b || !d_tokens || !d_consts) return fail(MBX_E_ARG, "mbx_symbol_rollout: bad arguments");
    if (b->cfg.algo != MBX_ALGO_SYMBOL) return fail(MBX_E_UNSUPPORTED, "mbx_symbol_rollout: the batch is not a SYMBOL batch");
    if (n_substeps < 1 || n_substeps > MBX_SYM_SUB_MAX) return fail(MBX_E_ARG, "mbx_symbol_rollout: n_substeps must be in [1, %d]", MBX_SYM_SUB_MAX);
    symbol_launch_action(b, (hipStream_t)stream, d_tokens, d_consts, nullptr, n_substeps, MBX_OUT, d_n_bad);
    HIP_TRY(hipGetLastError());
    return MBX_OK;
}

}  // namespace mbx
