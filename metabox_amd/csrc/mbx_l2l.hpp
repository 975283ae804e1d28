// mbx_l2l.hpp — L2L (RNN-OI), an LSTM that proposes one point per step, as a resident episode kernel (reference: src/agent/l2l_agent.py:92-135,
// src/optimizer/l2l_optimizer.py; layout, weight order and tape: include/mbx_layout.h section 21).
//
// rollout_episode is 100 strictly sequential steps: one cell of nn.LSTM(D + 2 -> 32, proj D) in float64, the sigmoid box map, ONE evaluation, and the
// next input (x_raw, y, 1).  It draws no random number and takes no gradient, so on a noise-free problem an episode is a pure function of
// (weights, problem).  One workgroup owns an instance (through bp.order) and keeps in, h, c, the curve and the counters on chip for the n_steps of a
// launch; the weights belong to the instance's SET (mbx_l2l_set_params) and are read from memory, or -- at the reference's D = 10 -- sit in the
// registers of the lane that owns the gate row.  The 128 gate rows go one per lane on waves 0 and 1; the 32 cell entries and the D projections run
// on wave 0 and hand over inside that wave; the single-row objective is the evaluator every kernel here shares (eval_rows with a RowPost: noise, then
// the optimum).  Block barriers per step: two of this file's (the gates go to the cell, the position to the evaluator) plus the evaluator's own.
// Every thread keeps the counters, y and best in registers and updates them from the evaluator's result, so the loop's exit is uniform.
//
// One body, three kernels: k_l2l_reset (MODE 0) zeroes the block; k_l2l_step (MODE 1) takes x_raw [B, D] as the action -- the host ran the cell, as
// the reference's agent does -- and does the box map, the evaluation and the bookkeeping; k_l2l_run (MODE 2) puts the cell in front.
//
// The reference's own behaviour, kept on purpose:
//  * the first input is all zeros: the constant slot is 0 at step 0 and 1 from step 1 on (l2l_agent.py:104, :129).
//  * np_scale (l2l_optimizer.py:10-13): lb + (ub - lb) * (1 / (1 + exp(-x))), the reciprocal first.
//  * y = problem.eval(x) - optimum, or problem.eval(x) where the optimum is None (:36-39); best updates with strict < (:40-43).
//  * done = (optimum known and y <= 1e-8) or fes >= 100 (:48-52): the 100 is a literal, max_fes plays no part.  The stop on y needs cfg.early_stop.
//  * the agent returns cost[::2] (l2l_agent.py:135): best after steps 1, 3, 5, ...; return = sum y / y_0.
// Arithmetic: float64, no contraction (the build passes -ffp-contract=off); the summation orders are fixed in include/mbx_layout.h section 21.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"

namespace mbx {

constexpr int kL2lHid = MBX_L2L_HID, kL2lGates = MBX_L2L_GATES;

struct L2lArgs {
    const double* params;       // [n_sets][MBX_L2L_NPARAM(D)]
    const int32_t* set_of;      // [B] or nullptr = set 0
    int n_sets;
    int n_steps;                // steps of this launch at most
};

__device__ __forceinline__ double l2l_sigmoid(double v) { return 1. / (1. + m_exp(-v)); }

// DC: the dimension as a compile-time constant (10: a gate row's 22 weights stay in the lane's registers), 0 = bp.D
template <int DC, int MODE>
__device__ __forceinline__ void l2l_body(const BatchParams& bp, const L2lArgs& ar, const double* __restrict__ actions, double* __restrict__ state_out,
                                         double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int D = DC ? DC : bp.D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_L2L_ST_SCALARS(1, D);
    if (MODE == 0) {                                                 // ---- reset (init_population :20-23, rollout_episode :104-112)
        for (int e = tid; e < MBX_L2L_ST_SCALARS(1, D); e += kThreads) S[e] = 0.;
        if (tid < MBX_L2L_CURVE) sc[MBX_NSCALAR + tid] = 0.;
        if (tid == 0) {
            const double episode = (double)((int)sc[MBX_SC_EPISODE] + 1);
            for (int k = 0; k < MBX_NSCALAR; ++k) sc[k] = 0.;
            sc[MBX_SC_EPISODE] = episode;
            if (state_out) state_out[b] = 0.;
        }
        return;
    }
    // every scalar is read here, before the first barrier, by every thread; thread 0 writes them back after the last one
    int steps = (int)sc[MBX_SC_GEN];
    double best = sc[MBX_SC_GBEST], ysum = sc[MBX_SC_L2L_YSUM], y0 = sc[MBX_SC_L2L_Y0], y = sc[MBX_SC_L2L_Y];
    if (sc[MBX_SC_DONE] != 0.) {                                     // a finished instance stays as it is
        if (tid == 0) {
            if (state_out) state_out[b] = y;
            if (reward_out) reward_out[b] = ysum / y0;
            if (done_out) done_out[b] = 1;
        }
        return;
    }
    steps = min(max(steps, 0), MBX_L2L_T - 1);                       // (clamped: mbx_debug_write_state is caller data; a live instance has run fewer than 100 steps)
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const L2lLds L = l2l_carve(smem, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const uint32_t episode = (uint32_t)(int)sc[MBX_SC_EPISODE];
    const bool stop_rule = !isnan(P.optimum) && bp.early_stop;
    const double lb = P.lb, ub = P.ub;
    double in_y = S[MBX_L2L_ST_IN(1, D) + D], in_one = S[MBX_L2L_ST_IN(1, D) + D + 1];   // the input's last two slots, in registers

    stage_problem(P, L.eval());
    if (tid < D) { L.IN[tid] = S[MBX_L2L_ST_IN(1, D) + tid]; L.H[tid] = S[MBX_L2L_ST_H(1, D) + tid]; L.XR[tid] = S[MBX_L2L_ST_X(1, D) + tid]; }
    if (tid < kL2lHid) L.C[tid] = S[MBX_L2L_ST_C(1, D) + tid];
    if (tid < MBX_L2L_CURVE) L.CURVE[tid] = sc[MBX_NSCALAR + tid];

    // the instance's weight set; the row of this lane
    const double* W = nullptr;
    double wi[DC ? DC + 2 : 1], wh[DC ? DC : 1], bi = 0., bh = 0.;
    if (MODE == 2) {
        const int set = ar.set_of ? min(max(ar.set_of[b], 0), ar.n_sets - 1) : 0;     // (clamped: the host has checked the table)
        W = ar.params + (int64_t)set * MBX_L2L_NPARAM(D);
        if (tid < kL2lGates) {
            bi = W[MBX_L2L_B_IH(D) + tid]; bh = W[MBX_L2L_B_HH(D) + tid];
            if constexpr (DC != 0) {
#pragma unroll
                for (int j = 0; j < DC + 2; ++j) wi[j] = W[MBX_L2L_W_IH(D) + tid * (DC + 2) + j];
#pragma unroll
                for (int j = 0; j < DC; ++j) wh[j] = W[MBX_L2L_W_HH(D) + tid * DC + j];
            }
        }
    }
    __syncthreads();

    bool done = false;
    const int n = MODE == 1 ? 1 : ar.n_steps;
    for (int it = 0; it < n && !done; ++it) {
        if (MODE == 2) {
            if (tid < kL2lGates) {                                   // ---- the gates (row tid), waves 0 and 1
                double s1 = 0., s2 = 0.;
                if constexpr (DC != 0) {
#pragma unroll
                    for (int j = 0; j < DC; ++j) s1 = s1 + wi[j] * L.IN[j];
                    s1 = s1 + wi[DC] * in_y; s1 = s1 + wi[DC + 1] * in_one;
#pragma unroll
                    for (int j = 0; j < DC; ++j) s2 = s2 + wh[j] * L.H[j];
                } else {
                    const double* wr = W + MBX_L2L_W_IH(D) + (int64_t)tid * (D + 2);
                    for (int j = 0; j < D; ++j) s1 = s1 + wr[j] * L.IN[j];
                    s1 = s1 + wr[D] * in_y; s1 = s1 + wr[D + 1] * in_one;
                    const double* hr = W + MBX_L2L_W_HH(D) + (int64_t)tid * D;
                    for (int j = 0; j < D; ++j) s2 = s2 + hr[j] * L.H[j];
                }
                const double g = ((s1 + bi) + s2) + bh;
                L.ACT[tid] = (tid >> 5) == 2 ? tanh(g) : l2l_sigmoid(g);      // rows i | f | g | o
            }
            __syncthreads();                                          // the gates go to the cell
        }
        if (tid < 64) {                                              // ---- cell, projection and box map, wave 0
            if (MODE == 2) {
                if (tid < kL2lHid) {
                    const double c2 = L.ACT[kL2lHid + tid] * L.C[tid] + L.ACT[tid] * L.ACT[2 * kL2lHid + tid];
                    L.C[tid] = c2;
                    L.HO[tid] = L.ACT[3 * kL2lHid + tid] * tanh(c2);
                }
                wave_lds_fence();
            }
            if (tid < D) {
                double xr;
                if (MODE == 2) {
                    const double* pr = W + MBX_L2L_W_HR(D) + (int64_t)tid * kL2lHid;
                    xr = 0.;
#pragma unroll 8
                    for (int k = 0; k < kL2lHid; ++k) xr = xr + pr[k] * L.HO[k];
                } else xr = actions[(int64_t)b * D + tid];
                L.IN[tid] = xr; L.H[tid] = xr;
                const double sg = 1. / (1. + m_exp(-xr));            // np_scale: the reciprocal, then the box
                L.XR[tid] = lb + (ub - lb) * sg;
            }
        }
        __syncthreads();                                              // the position goes to the evaluator
        {
            const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(steps + 1), episode};
            const RowPost post{&rng, tape ? tape + MBX_L2L_TAPE_NOISE(1, D) : nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B, 1, 0};
            eval_rows(P, L.eval(), 1, &post);                        // its last barrier hands y to every thread
        }
        y = L.NC[0];
        steps += 1;
        ysum = steps == 1 ? y : ysum + y;                             // y_sum = 0; y_sum += y
        if (steps == 1) { y0 = y; best = y; }
        else if (y < best) best = y;
        if ((steps & 1) && tid == 0) L.CURVE[steps >> 1] = best;      // cost[::2]: steps <= 100, slot <= 49
        in_y = y; in_one = 1.;
        done = (stop_rule && y <= 1e-8) || steps >= MBX_L2L_T;
    }
    __syncthreads();
    // ---- the state block, once per launch
    if (tid < D) { S[MBX_L2L_ST_IN(1, D) + tid] = L.IN[tid]; S[MBX_L2L_ST_H(1, D) + tid] = L.H[tid]; S[MBX_L2L_ST_X(1, D) + tid] = L.XR[tid]; }
    if (tid < kL2lHid) S[MBX_L2L_ST_C(1, D) + tid] = L.C[tid];
    if (tid < MBX_L2L_CURVE) sc[MBX_NSCALAR + tid] = L.CURVE[tid];
    if (tid == 0) {
        S[MBX_L2L_ST_IN(1, D) + D] = in_y; S[MBX_L2L_ST_IN(1, D) + D + 1] = in_one;
        const double ret = ysum / y0;
        sc[MBX_SC_GBEST] = best; sc[MBX_SC_FES] = steps; sc[MBX_SC_GEN] = steps; sc[MBX_SC_COST_LEN] = (steps + 1) >> 1;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_RETURN] = ret;
        sc[MBX_SC_L2L_YSUM] = ysum; sc[MBX_SC_L2L_Y0] = y0; sc[MBX_SC_L2L_Y] = y;
        if (state_out) state_out[b] = y;
        if (reward_out) reward_out[b] = ret;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_l2l_reset(BatchParams bp, double* __restrict__ state_out)
{
    l2l_body<0, 0>(bp, L2lArgs{}, nullptr, state_out, nullptr, nullptr);
}

__global__ __launch_bounds__(kThreads) void k_l2l_step(BatchParams bp, const double* __restrict__ actions, double* __restrict__ state_out,
                                                       double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    l2l_body<0, 1>(bp, L2lArgs{}, actions, state_out, reward_out, done_out);
}

template <int DC>
__global__ __launch_bounds__(kThreads) void k_l2l_run(BatchParams bp, L2lArgs ar, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                      uint8_t* __restrict__ done_out)
{
    l2l_body<DC, 2>(bp, ar, nullptr, state_out, reward_out, done_out);
}

}  // namespace mbx
