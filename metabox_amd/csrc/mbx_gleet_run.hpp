// mbx_gleet_run.hpp — GLEET's resident rollout for gfx950: up to n_steps env steps of every instance in ONE launch, the attention actor inside the step kernel.
//
// One step is what mbx_gleet_policy followed by mbx_step does, from the same device functions: the actor's blocks (mbx_gleet_policy.hpp: gp_embed,
// gp_encoder_layer, gp_head / gp_mu_sigma, sample_action) and the generation (mbx_gleet.hpp: gl_generation, gl_epilogue, gl_bookkeeping), with the same Philox
// counters.  What the two-launch route hands over through the [B, np, 27] float64 state tensor -- 88 MB written and read again per generation of 4096 swarms --
// stays in registers here: the epilogue's 9 features, the particle's memory row and the gbest memory go straight into the next step's embedding.  The state
// tensor is read once when the launch starts and written once, after the last executed step.
//
// One 256-thread workgroup per instance, as k_gleet_step has it; thread i < np <= 128 owns particle i in the generation AND in the actor, so waves 0 and 1 run the
// actor and waves 2 and 3 only meet its barriers.  (The alternative, two threads per particle with the heads split between them, keeps all four waves busy
// but needs gp_encoder_layer rewritten around a lane exchange; this kernel shares the encoder with k_gleet_policy unchanged.)  The weights are scalar loads
// through the constant cache: the base pointer is the instance's set, one per workgroup and therefore wave-uniform.  The actor's keys / values lie in the
// evaluator's scratch, dead while the actor runs (glr_layout, mbx_lds.hpp); positions, velocities and pbest rows stay in the state block in HBM / L2 as in
// k_gleet_step: they are L2-resident between the steps of a launch, and another 24 KB of LDS (at 100 x 10) buys nothing while the registers decide the occupancy.
#pragma once
#include "mbx_gleet.hpp"
#include "mbx_gleet_policy.hpp"

namespace mbx {

struct GlrArgs {
    const float* weights;           // [n_sets][GpOff::total]
    const int32_t* set;             // [B] set of every instance, or null: set 0
    float min_sigma, max_sigma;
    int n_steps;
    int accumulate;                 // reward_out is added to instead of overwritten (the later launches of the one-launch-per-step route)
    double* state;                  // [B][NP][27] in / out
    float* traj_actions;            // [n_steps][B][NP], [n_steps][B][2][NP], [n_steps][B]: the records of THIS launch's steps; each may be null
    float* traj_mu_sigma;
    double* traj_reward;
    double* reward_out;
    uint8_t* done_out;
};

// Left alone the compiler takes 237 (NP 100 / D 10) and 230 (run-time geometry) VGPRs: two waves per SIMD, two workgroups per CU, no scratch.  Capped at three waves
// (168 VGPRs) it spills 89 / 75 registers to scratch, which this kernel does not accept; the 34 KB of LDS would hold four workgroups.
#ifndef MBX_GLR_WAVES
#define MBX_GLR_WAVES
#endif

template <int NPC = 0, int DC = 0>
__global__ __launch_bounds__(kThreads) MBX_GLR_WAVES void k_gleet_run(BatchParams bp0, GlrArgs ar)
{
    const BatchParams& bp = bp0;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid0 = threadIdx.x;
    const int NP0 = NPC ? NPC : bp.NP, D0 = DC ? DC : bp.D;
    double* S0 = bp.state + (int64_t)b * bp.state_stride;
    if (S0[MBX_GLEET_ST_SCALARS(NP0, D0) + MBX_SC_DONE] != 0.) {     // frozen: the state tensor and the records stay as they are
        if (tid0 == 0) { if (ar.reward_out && !ar.accumulate) ar.reward_out[b] = 0.; if (ar.done_out) ar.done_out[b] = 1; }
        return;
    }
    const DevProblem* P0 = bp.problems + bp.problem_idx[b];
    const float* W0 = ar.weights + (int64_t)(ar.set ? ar.set[b] : 0) * GpOff::total;      // uniform, constant-indexed reads through GpConstW: scalar loads
    const uint64_t seed0 = bp.seeds[b];
    float h[kGpE] = {}, dq[kGpE] = {};
    if (tid0 < NP0) {
        const double* si = ar.state + ((int64_t)b * NP0 + tid0) * 27;
        float xi[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) xi[k] = (float)si[k];
        gp_embed(xi, (GpConstW)(uintptr_t)W0, h, dq);
    }
    double rsum = 0.;                                               // thread 0's
    if (tid0 == 0 && ar.accumulate && ar.reward_out) rsum = ar.reward_out[b];
    for (int t = 0;; ++t) {
        // Nothing below may look loop-invariant to the compiler: what it hoists out of a loop this long -- the weights' loads, every per-thread address into the
        // state block, the LDS pointers of the run-time geometry -- it keeps alive across the actor, whose 168 registers leave no room, and spills.  Behind an
        // empty asm the bases and the thread's index are new values every step: loads and address arithmetic stay where they are used.
        const float* Wt = W0; double* S = S0; const DevProblem* Pt = P0; double* lds = smem; int NP = NP0, D = D0;
        asm volatile("" : "+s"(Wt), "+s"(S), "+s"(Pt), "+s"(lds));
        if (!NPC) asm volatile("" : "+s"(NP));
        if (!DC) asm volatile("" : "+s"(D));
        uint32_t k0 = (uint32_t)seed0, k1 = (uint32_t)(seed0 >> 32);
        asm volatile("" : "+s"(k0), "+s"(k1));
        const uint64_t seed = (uint64_t)k1 << 32 | k0;
        BatchParams bp = bp0;                                        // (the budget: its conversions and quotients are hoisted like everything else)
        asm volatile("" : "+s"(bp.max_fes));
        const int tid = opaque_tid();
        const bool live = tid < NP;
        const GpConstW W = (GpConstW)(uintptr_t)Wt;
        ConstProblem& P = *(ConstProblem*)Pt;
        double* sc = S + MBX_GLEET_ST_SCALARS(NP, D);
        const GlrLds R = glr_carve(lds, NP, D);
        const GlLds& L = R.g;
        // ---- the actor: encoder, decoder, heads, draw (k_gleet_policy's sequence).  Its swarm size is a run-time value in every instantiation, as in
        // k_gleet_policy: with a constant the loops over the keys unroll completely.
        int NPa = NP;
        asm volatile("" : "+s"(NPa));
        gp_encoder_layer(h, h, W + GpOff::enc, R.KL, R.VL, live, NPa, tid, R.PRED);
        __syncthreads();                                             // every lane is done with the encoder's keys / values
        gp_encoder_layer(h, dq, W + GpOff::dec, R.KL, R.VL, live, NPa, tid, R.PRED);
        float a = 0.f;
        if (live) {
            float mu, sigma;
            gp_mu_sigma(h, W, ar.min_sigma, ar.max_sigma, mu, sigma);
            const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)((int)sc[MBX_SC_GEN] + 1), (uint32_t)(int)sc[MBX_SC_EPISODE]};
            a = sample_action(rng, tid, mu, sigma, MBX_POLICY_RLEPSO);
            const int64_t row = (int64_t)t * bp.B + b;
            if (ar.traj_actions) ar.traj_actions[row * NP + tid] = a;
            if (ar.traj_mu_sigma) { ar.traj_mu_sigma[(row * 2) * NP + tid] = mu; ar.traj_mu_sigma[(row * 2 + 1) * NP + tid] = sigma; }
        }
        // ---- the generation (the block sums of the second layer's normalisation are behind every lane: the keys / values are dead, T | Z free again)
        const GlGen g = gl_generation<DC>(bp, P, L, S, sc, nullptr, seed, a, tid, NP, D);
        double f[MBX_GLEET_NFEAT], pf[MBX_GLEET_NFEAT];
        gl_epilogue(bp, P, L, S, g, tid, NP, D, f, pf);
        if (tid == 0) {
            double reward;
            const bool d = gl_bookkeeping(bp, P, sc, g, reward);
            rsum = t == 0 && !ar.accumulate ? reward : rsum + reward;
            if (ar.traj_reward) ar.traj_reward[(int64_t)t * bp.B + b] = reward;
            L.RED[2] = d ? 1. : 0.;                                  // block_argmin uses RED[0 .. 1]
        }
        __syncthreads();                                             // publishes the flag and thread 0's scalars
        const bool done = L.RED[2] != 0.;
        const bool last = done || t + 1 >= ar.n_steps;
        if (last) {
            if (live) {
                double* so = ar.state + ((int64_t)b * NP + tid) * 27;
#pragma unroll
                for (int k = 0; k < 9; ++k) { so[k] = f[k]; so[9 + k] = pf[k]; so[18 + k] = L.GF[k]; }
            }
            if (tid == 0) { if (ar.reward_out) ar.reward_out[b] = rsum; if (ar.done_out) ar.done_out[b] = done ? 1 : 0; }
            break;
        }
        if (live) {                                                  // features -> embedding, no trip through memory
            float xi[27];
#pragma unroll
            for (int k = 0; k < 9; ++k) { xi[k] = (float)f[k]; xi[9 + k] = (float)pf[k]; xi[18 + k] = (float)L.GF[k]; }
            gp_embed(xi, W, h, dq);
        } else {                                                     // (assigned on every path: nothing of the actor is alive across the generation)
#pragma unroll
            for (int k = 0; k < kGpE; ++k) h[k] = dq[k] = 0.f;
        }
    }
}

}  // namespace mbx
