/* mbx_symbol.h -- the SYMBOL entry point of libmbx.so (MBX_ALGO_SYMBOL = 27; layouts, tokens and the tape: include/mbx_layout.h section 22).  A header
 * of its own beside include/mbx.h, like include/mbx_l2l.h, whose conventions hold here too: device pointers are named d_*, every function returns 0
 * or a negative MBX_E_* code and mbx_last_error() describes the failure.  A batch is created with mbx_batch_create (np in [4, 128], dim in [2, 40] -- 2 is the library's common lower bound; any other
 * geometry and a protein problem are MBX_E_UNSUPPORTED) and reset with mbx_reset as for every other algorithm; mbx_state_dim is 9.  mbx_step takes the program as
 * [n_instances, 126] float64 actions -- 63 tokens, then 63 constants -- and runs MBX_SYM_SKIP = 5 sub-steps. */
#ifndef MBX_SYMBOL_H
#define MBX_SYMBOL_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One action of Symbol_Optimizer.update (symbol_optimizer.py:122-200) for every instance, each under ITS OWN update rule: d_tokens
 * [n_instances, 63] int32 is the heap-ordered expression tree (-1 = empty slot), d_consts [n_instances, 63] float64 the value of every constant leaf
 * (already scaled by its power of ten).  The n_substeps (1 .. 8; the reference: 5) sub-steps run in ONE launch with the population in LDS
 * (MBX_F_ROLLOUT_PER_GENERATION: one launch per sub-step, same outputs), then the nine features go to d_state_out [n_instances, 9], the reward
 * (pre_gbest - gbest) / init_cost to d_reward_out and is_done to d_done_out.  A finished instance stays frozen.  A malformed program leaves its
 * instance untouched (features of the previous action, reward 0) and sets d_n_bad [n_instances] int32 (optional) to 1, else 0.  The index rows the
 * randx leaves drew are kept in the state block: fed back as a tape they reproduce the action bit for bit. */
int mbx_symbol_rollout(mbx_batch* b, const int32_t* d_tokens, const double* d_consts, int n_substeps, double* d_state_out, double* d_reward_out,
                       uint8_t* d_done_out, int32_t* d_n_bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_SYMBOL_H */
