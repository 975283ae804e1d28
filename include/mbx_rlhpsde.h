/* mbx_rlhpsde.h -- the RL-HPSDE entry point of libmbx.so (MBX_ALGO_RLHPSDE = 24; layouts: include/mbx_layout.h section 19).  A header of its own beside
 * include/mbx.h, like include/mbx_les.h, whose conventions hold here too: device pointers are named d_*, every function returns 0 or a negative
 * MBX_E_* code and mbx_last_error() describes the failure.  A batch is created with mbx_batch_create, reset with mbx_reset and stepped with the
 * caller's int32 actions by mbx_step as for every other algorithm. */
#ifndef MBX_RLHPSDE_H
#define MBX_RLHPSDE_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* RL-HPSDE, up to n_steps updates of rl_hpsde_optimizer.py's update() (:231-287) per instance in ONE launch, the agent's choice (rl_hpsde_agent.py:31-34:
 * softmax over the row of the 4 x 4 float64 Q-table d_q_table that the landscape state names, one uniform) made in the kernel.  Semantics are those of
 * mbx_nrlpso_rollout: n one-step calls, one n-step call and n calls of mbx_step fed the same actions leave bit-identical state blocks; a finished instance stays
 * frozen.  d_traj_actions / d_traj_state / d_traj_reward [n_steps, n_instances] (each may be NULL) take the per-step records (rows after an instance's
 * termination are not written), d_actions_out [n_instances] the last action, d_state_out the landscape state after the last executed update, d_reward_out the
 * rewards summed over the executed updates, d_done_out the done flag.  With a replay tape n_steps must be 1 and the choice uniform comes from the tape.
 * MBX_E_ARG without a Q-table. */
int mbx_rlhpsde_rollout(mbx_batch* b, const double* d_q_table, int n_steps, int32_t* d_traj_actions, double* d_traj_state, double* d_traj_reward,
                        int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_RLHPSDE_H */
