/* mbx_les.h -- the LES entry points of libmbx.so (MBX_ALGO_LES = 21; layouts: include/mbx_layout.h section 18).  A header of its own beside
 * include/mbx.h, whose conventions hold here too: device pointers are named d_*, every function returns 0 or a negative MBX_E_* code and
 * mbx_last_error() describes the failure.  A batch is created with mbx_batch_create and reset with mbx_reset as for every other algorithm. */
#ifndef MBX_LES_H
#define MBX_LES_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* LES (include/mbx_layout.h section 18): the 246 float32 parameters of the attention module and the learning-rate MLP, PER INSTANCE.  d_params is
 * [n_sets, 246] float32 in the reference's vector2nn order (attn[0:68] = Wq.weight (8x3), Wq.bias, Wk.weight, Wk.bias, Wv.weight (1x3), Wv.bias;
 * mlp[68:246] = ln1.weight (8x19), ln1.bias, ln2.weight (2x8), ln2.bias), d_set_of_instance [n_instances] int32 names the set of every instance (NULL: set 0
 * for all; an index outside [0, n_sets) is MBX_E_ARG).  Both are copied: the caller's buffers may go away afterwards.  Synchronises the device. */
int mbx_les_set_params(mbx_batch* b, const float* d_params, int n_sets, const int32_t* d_set_of_instance);

/* LES, generations of les_optimizer.py's update() loop (:128-178) in ONE launch with parents, costs, mu, sigma, the evolution paths, the counters and the
 * instance's parameters in LDS in between (MBX_F_ROLLOUT_PER_GENERATION: one launch per generation, same outputs).
 *   skip = 0: up to n_gens generations under the budget / early-stop end rule; a finished instance stays frozen.  n one-generation calls, one n-generation
 *             call and n calls of mbx_step (actions = NULL) leave bit-identical state blocks.
 *   skip = 1: the reference's call with action['skip_step'] = n_gens: exactly n_gens generations, the end rule REPLACED by step >= n_gens (budget, early
 *             stop and the done flag are ignored; FEs may pass max_fes; the call closes the cost curve as :174-178 does).
 * d_state_out [n_instances] = gbest, d_reward_out = (init_y - gbest) / init_y with init_y the gbest after the first generation of the reference's call (skip = 0:
 * the first generation after mbx_reset; skip = 1: the first generation of this call), d_done_out = is_end.  With a replay tape n_gens must be 1.
 * MBX_E_ARG before mbx_les_set_params. */
int mbx_les_rollout(mbx_batch* b, int n_gens, int skip, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_LES_H */
