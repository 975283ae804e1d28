/* mbx_nlshade.h -- the NL_SHADE_LBC entry point of libmbx.so (MBX_ALGO_NLSHADE = 25; layouts: include/mbx_layout.h section 20).  A header of its own beside
 * include/mbx.h, like include/mbx_rlhpsde.h, whose conventions hold here too: device pointers are named d_*, every function returns 0 or a negative
 * MBX_E_* code and mbx_last_error() describes the failure.  A batch is created with mbx_batch_create, reset with mbx_reset and stepped one update at a
 * time by mbx_step (actions = NULL) as for every other classic baseline. */
#ifndef MBX_NLSHADE_API_H
#define MBX_NLSHADE_API_H
#include "mbx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* NL_SHADE_LBC, up to n_updates updates of nl_shade_lbc.py's __update (:163-273) per instance in ONE launch.  n one-update calls, one n-update call and
 * n calls of mbx_step leave bit-identical state blocks; a finished instance stays frozen.  d_state_out [n_instances] takes fes / max_fes, d_reward_out
 * zeros, d_done_out the done flag (each may be NULL).  With a replay tape n_updates must be 1. */
int mbx_nlshade_run(mbx_batch* b, int n_updates, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_NLSHADE_API_H */
