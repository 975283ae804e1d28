/* mbx_gleet.h -- GLEET's resident rollout, two entry points of libmbx.so (MBX_ALGO_GLEET; layouts: include/mbx_layout.h).  A header of its own beside
 * include/mbx.h, like include/mbx_l2l.h, whose conventions hold here too: device pointers are named d_*, every function returns 0 or a negative MBX_E_* code
 * and mbx_last_error() describes the failure.  A batch is created with mbx_batch_create and reset with mbx_reset as for every other algorithm; mbx_step and
 * mbx_gleet_policy (include/mbx.h) remain the two-launch route these functions are bit-compatible with. */
#ifndef MBX_GLEET_H
#define MBX_GLEET_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The actor's 5426 float32 weights, PER INSTANCE SET: d_weights [n_sets, 5426] in the order mbx_gleet_actor documents;
 * d_set_of_instance [n_instances] int32 or NULL (set 0 for all; an index outside [0, n_sets) is MBX_E_ARG).  Copied. */
int mbx_gleet_set_params(mbx_batch* b, const float* d_weights, int n_sets, const int32_t* d_set_of_instance,
                         float min_sigma, float max_sigma);

/* Up to n_steps env steps in ONE launch: actor -> sample -> generation -> features, the swarm's features staying on chip.
 * d_state [n_instances, np, 27] float64 is IN/OUT: on entry what mbx_reset / mbx_step / the previous call wrote, on return
 * the state after the last executed step (untouched for an instance that was already done).
 * Per-step records, each may be NULL, rows of steps after an instance's termination are not written:
 *   d_traj_actions [n_steps, n_instances, np] float32, d_traj_mu_sigma [n_steps, n_instances, 2, np] float32,
 *   d_traj_reward [n_steps, n_instances] float64.
 * d_reward_out: SUM of the rewards of the executed steps; d_done_out: is_done after the last one. */
int mbx_gleet_rollout(mbx_batch* b, int n_steps, double* d_state, float* d_traj_actions, float* d_traj_mu_sigma,
                      double* d_traj_reward, double* d_reward_out, uint8_t* d_done_out, void* stream);

/* Every step is mbx_gleet_policy followed by mbx_step, Philox counters included (the policy draw is (i, MBX_SITE_POLICY, gen + 1, episode)); the float64
 * generation is bit-identical to mbx_step fed the recorded actions.  One n-step call, n one-step calls and any split of n leave bit-identical state blocks,
 * d_state, cost curves and records; MBX_F_ROLLOUT_PER_GENERATION: one launch per step, same outputs.  A finished instance (budget, or gbest <= 1e-8 under
 * cfg.early_stop) stays frozen.  MBX_E_UNSUPPORTED: not a GLEET batch, np > 128 (the actor's limit), a batch with a replay tape (the reference's actions come
 * from torch's generator: a policy-inside replay has nothing to be compared with).  MBX_E_ARG: rollout before mbx_gleet_set_params, n_steps < 1. */

#ifdef __cplusplus
}
#endif
#endif /* MBX_GLEET_H */
