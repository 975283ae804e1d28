// mbx_run_kernels.hpp — the resident-rollout kernels that are compiled in translation units of their own (mbx_run_rlepso*.hip, mbx_run_lde.hip): mbx.hip sees
// explicit instantiation DECLARATIONS (no device code, the host-side launch stub is resolved at link time), the other files hold the definitions.
#pragma once
#ifndef MBX_RUN10_THREADS
#define MBX_RUN10_THREADS 256           // workgroup size of the headline resident kernel k_rlepso_run<., 100, 10, 5> (A/B knob; 128 threads at 3 waves per SIMD, no spills: 158.9 against 117.1 us per generation)
#endif
// k_rlepso_run<THREADS, NP, D, groups, TIE>: TIE = true is the exact FDR scan (default), false the MBX_F_FDR_FAST form (BASELINE configs 2 / 5 only)
#define MBX_RUN_RLEPSO_EXACT(X)                                                                          \
    X template __global__ void k_rlepso_run<MBX_RUN10_THREADS, 100, 10, 5, true>(BatchParams, const float*, int, int, RunOut); \
    X template __global__ void k_rlepso_run<512, 100, 30, 5, true>(BatchParams, const float*, int, int, RunOut);                \
    X template __global__ void k_rlepso_run<256, 100, 12, 5, true>(BatchParams, const float*, int, int, RunOut);      /* protein docking (src/config.py:86-90: dim 12), any-kind body */
#define MBX_RUN_RLEPSO_C5(X) X template __global__ void k_rlepso_run<1024, 128, 40, 5, true>(BatchParams, const float*, int, int, RunOut);
#define MBX_RUN_RLEPSO_D40(X) X template __global__ void k_rlepso_run<1024, 100, 40, 5, true>(BatchParams, const float*, int, int, RunOut);      /* the reference's NP at --dim 40 */
#define MBX_RUN_RLEPSO_FAST(X)                                                                           \
    X template __global__ void k_rlepso_run<MBX_RUN10_THREADS, 100, 10, 5, false>(BatchParams, const float*, int, int, RunOut); \
    X template __global__ void k_rlepso_run<1024, 128, 40, 5, false>(BatchParams, const float*, int, int, RunOut);
#ifdef MBX_RUN_KERNELS_EXTERN
namespace mbx {
MBX_RUN_RLEPSO_EXACT(extern)
MBX_RUN_RLEPSO_C5(extern)
MBX_RUN_RLEPSO_D40(extern)
MBX_RUN_RLEPSO_FAST(extern)
extern template __global__ void k_lde_run<100, 30>(LdeRunArgs);
extern template __global__ void k_lde_run<50, 30>(LdeRunArgs);
extern template __global__ void k_lde_run<50, 10>(LdeRunArgs);
extern template __global__ void k_lde_run<50, 30, 50, true>(LdeRunArgs);
}  // namespace mbx
#endif
// DEDQN (mbx_dedqn.hpp): kernels AND launch code live in mbx_run_dedqn.hip; mbx.hip reaches them through these host functions
namespace mbx {
hipError_t dedqn_prepare(size_t lds_bytes);         // the kernels' dynamic-LDS limit, once per batch
void dedqn_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out);
void dedqn_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const int32_t* d_actions, double* d_state_out, double* d_reward_out,
                       uint8_t* d_done_out);
void dedqn_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const float* d_net, int n_steps, int32_t* d_traj_actions,
                      double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// NRLPSO (mbx_nrlpso.hpp): likewise in mbx_run_nrlpso.hip
namespace mbx {
bool nrlpso_cached(int np, int dim, uint32_t flags, size_t max_lds_bytes);     // the distance matrix stays in LDS (flag clear and it fits)
hipError_t nrlpso_prepare(size_t lds_bytes);
void nrlpso_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out);
// d_actions: the caller's actions (mbx_step), or nullptr with the Q-table: the policy decides in the kernel
void nrlpso_launch_steps(const BatchParams& bp, bool cached, hipStream_t stream, const int32_t* d_actions, const double* d_q_table, int n_steps,
                         int32_t* d_traj_actions, double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out,
                         double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// SAHLPSO (mbx_sahlpso.hpp): likewise in mbx_run_sahlpso.hip
namespace mbx {
hipError_t sahlpso_prepare(size_t lds_bytes);
void sahlpso_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out);
void sahlpso_launch_generation(const BatchParams& bp, hipStream_t stream, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// LES (mbx_les.hpp): likewise in mbx_run_les.hip
namespace mbx {
hipError_t les_prepare(size_t lds_bytes);
void les_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out);
// skip = 0: up to n_gens generations under the budget / early-stop end rule; skip = 1: steps step0 .. step0 + n_gens - 1 of a skip_step call of skip_total steps
void les_launch_run(const BatchParams& bp, hipStream_t stream, const float* d_params, const int32_t* d_set_of, int n_sets, const float* d_ts, int horizon,
                    int n_gens, int skip, int step0, int skip_total, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// L2L (mbx_l2l.hpp): likewise in mbx_run_l2l.hip
namespace mbx {
hipError_t l2l_prepare(size_t lds_bytes);
void l2l_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out);
// the host ran the cell: d_x_raw [B, D] is the action
void l2l_launch_step(const BatchParams& bp, hipStream_t stream, const double* d_x_raw, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
// generic: the run-time-D body at D = 10 as well (MBX_F_GENERIC_GEOMETRY)
void l2l_launch_run(const BatchParams& bp, bool generic, hipStream_t stream, const double* d_params, const int32_t* d_set_of, int n_sets, int n_steps,
                    double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// SYMBOL (mbx_symbol.hpp): likewise in mbx_run_symbol.hip
namespace mbx {
hipError_t symbol_prepare(size_t lds_bytes);
void symbol_launch_reset(const BatchParams& bp, hipStream_t stream, double* d_state_out);
// n_sub sub-steps of an action of n_action; the program as (d_tokens, d_consts) or as d_actions [B, 126] float64
void symbol_launch_run(const BatchParams& bp, hipStream_t stream, const int32_t* d_tokens, const double* d_consts, const double* d_actions, int n_sub,
                       int n_action, double* d_state_out, double* d_reward_out, uint8_t* d_done_out, int32_t* d_n_bad);
}  // namespace mbx
// RL-HPSDE (mbx_rlhpsde.hpp): likewise in mbx_run_rlhpsde.hip
namespace mbx {
hipError_t rlhpsde_prepare(size_t lds_bytes);
void rlhpsde_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out);
void rlhpsde_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const int32_t* d_actions, double* d_state_out, double* d_reward_out,
                         uint8_t* d_done_out);
// the policy decides in the kernel: d_q_table is the 4 x 4 Q-table
void rlhpsde_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, const double* d_q_table, int n_steps, int32_t* d_traj_actions,
                        double* d_traj_state, double* d_traj_reward, int32_t* d_actions_out, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
}  // namespace mbx
// NL_SHADE_LBC (mbx_nlshade.hpp): likewise in mbx_run_nlshade.hip
#include <vector>
namespace mbx {
std::vector<double> nlshade_schedule(int np, int max_fes);      // the batch's table bp.pci: the update count, then N after update 0 .. G
hipError_t nlshade_prepare(size_t lds_bytes);
void nlshade_launch_reset(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out);
void nlshade_launch_step(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, double* d_state_out, double* d_reward_out, uint8_t* d_done_out);
void nlshade_launch_run(const BatchParams& bp, size_t lds_bytes, hipStream_t stream, int n_updates, double* d_state_out, double* d_reward_out,
                        uint8_t* d_done_out);
}  // namespace mbx
