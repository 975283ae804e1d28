/* mbx_l2l.h -- the L2L entry points of libmbx.so (MBX_ALGO_L2L = 26; layouts: include/mbx_layout.h section 21).  A header of its own beside
 * include/mbx.h, like include/mbx_les.h, whose conventions hold here too: device pointers are named d_*, every function returns 0 or a negative
 * MBX_E_* code and mbx_last_error() describes the failure.  A batch is created with mbx_batch_create (np = 1) and reset with mbx_reset as for every
 * other algorithm; mbx_step takes x_raw [n_instances, dim] float64 as its actions (the host ran the LSTM cell) and does the box map, the evaluation
 * and the bookkeeping. */
#ifndef MBX_L2L_H
#define MBX_L2L_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The weights of nn.LSTM(input dim + 2, hidden 32, proj dim), float64, PER INSTANCE SET.  d_params is [n_sets, MBX_L2L_NPARAM(dim)] in torch's order
 * (weight_ih_l0 [128][dim + 2], weight_hh_l0 [128][dim], bias_ih_l0 [128], bias_hh_l0 [128], weight_hr_l0 [dim][32]; gate rows i, f, g, o),
 * d_set_of_instance [n_instances] int32 names the set of every instance (NULL: set 0 for all; an index outside [0, n_sets) is MBX_E_ARG).  Both are
 * copied: the caller's buffers may go away afterwards.  Synchronises the device. */
int mbx_l2l_set_params(mbx_batch* b, const double* d_params, int n_sets, const int32_t* d_set_of_instance);

/* Up to n_steps steps of rollout_episode (l2l_agent.py:114-132) in ONE launch -- cell, box map, one evaluation, bookkeeping -- with the input, h, c,
 * the counters and the curve in LDS in between (MBX_F_ROLLOUT_PER_GENERATION: one launch per step, same outputs).  A finished instance (y <= 1e-8
 * with a known optimum and cfg.early_stop, or 100 steps) stays frozen.  One n-step call, n one-step calls and mbx_step fed the x_raw the kernel
 * produced leave bit-identical bookkeeping.  d_state_out [n_instances] = the last y, d_reward_out = sum y / y_0, d_done_out = is_done.  With a replay
 * tape n_steps must be 1.  MBX_E_ARG before mbx_l2l_set_params. */
int mbx_l2l_rollout(mbx_batch* b, int n_steps, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_L2L_H */
