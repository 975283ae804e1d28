// mbx_rlhpsde.hpp — RL-HPSDE as batched kernels (reference: src/optimizer/rl_hpsde_optimizer.py:7-287, operators/mutate.py:12-33, 148-157,
// 184-188, crossover.py:6-18, boundary_control.py:5-9, and the tabular policy of src/agent/rl_hpsde_agent.py:31-34).
//
// SHADE-style DE: every row draws a memory slot, Cr = clip(N(MCr[slot], 0.1)) and F = MF[slot] + 0.1 x with x a standard Cauchy or Levy variate,
// mutates by cur_to_rand_1 or cur_to_best_1 (best = row 0 of the sorted population), is clipped, crossed binomially and evaluated; the improved
// rows update one memory slot by weighted Lehmer means; the population is sorted and cut linearly from N0 = 18 D rows towards 4 (LPSR).  The
// action in 0..3 picks the mutation (action & 1) and the law of F (action >> 1).  After the reset and after EVERY update, the last one of an
// episode included, a progressive random walk of 201 points is drawn, evaluated and billed (fes += 201), and two landscape bits make the state:
//   DFDC (:172-183)  the correlation r of the walk costs [1:] with the distances to row 0, bit = 0.15 < r <= 1;
//   DRIE (:186-217)  the largest base-6 entropy of the six kinds of unequal symbol transitions over nine thresholds scale * max|diff|, the 199
//                    transition counts divided by 200 and floored at 1e-15, bit = 0.5 <= entropy <= 1.
//
// k_rlhpsde_reset is init_population, k_rlhpsde_step one update with the caller's action, k_rlhpsde_run n_steps updates per launch with the 4 x 4
// Q-table in the workgroup; step and run are the same body (hp_steps), so they are bit-identical by construction.  A finished instance stays
// frozen.  One workgroup of 256 threads per instance, dispatched through bp.order; state block and tape: include/mbx_layout.h section 19.  As in
// MadDE and NL_SHADE_LBC (the three share mbx_depop.hpp: carve-up, prefix scan, numpy's pairwise sums, the bitonic (cost, row) sort, and the phases
// chunked evaluation, sorted first population, ranks of the improved rows, the memory update's sums, replacement and row move; this file holds the
// algorithm's own draws, mutation, crossover, walk and bookkeeping) a thread owns a contiguous block of ceil(NP / 256) rows; population, trial rows, costs, F, Cr, the indices and the walk points stay in
// the state block (HBM / L2); LDS holds the evaluator's chunk, the (cost, row) pairs of the sort, the compacted vectors of the long sums, and the
// walk's costs, distances, differences and transition counts.  The walk is one lane per coordinate with 200 sequential steps.  The means, the
// variances, the covariance and the row norms follow numpy's pairwise order (mbx_npsum.hpp).  The logarithms of the frequencies n / 200 come from
// the batch's table of correctly rounded values (bp.pci, built on the host as DEDQN's is), not from the device's log.
//
// Decisions taken where the reference leaves the result open, or cannot be followed:
//   a. sort (:45): the reference's argsort is introsort, whose order among equal costs depends on numpy's SIMD dispatch; the kernel orders by
//      (cost, row before the sort), numpy's kind='stable' order, as MadDE does;
//   b. generate_random_int's redraw loops are unbounded; on the Philox route every column redraws kHpTries times at most and then keeps what it
//      has (kDdRedrawMax of DEDQN is the precedent).  The tape carries the reference's resolved indices;
//   c. where the reference raises -- r is NaN, r == 0.15, r or the entropy outside their ranges (:183, :217) -- the bit is 0 and nothing is raised;
//   d. on the Philox route the Levy variate is x = 1 / s^2 with s a standard normal, the law of scipy's 1 / isf(u / 2)^2; on the tape route x
//      comes from the tape.
// Quirks of the reference kept on purpose:
//   1. F below 0 is reflected about its location once (2 loc - F, :65) and may stay negative; then min(1, F);
//   2. k advances only when some row improved; otherwise MF[k] = MCr[k] = 0.5 (:79-87); a weighted sum not above 1e-6 gives 0.5;
//   3. N = max(int(N0 + (4 - N0) fes / maxFEs), 1), truncated, with fes counting every walk so far (:92); the last N can be 3;
//   4. the reward is the share of improved rows of the population BEFORE the reduction (:277);
//   5. at most one log point per update (:273), so steps that bill more than log_interval skip points; the curve is closed on done (:282-286);
//   6. the walk after the update is billed AFTER the done test, also on the step that ends the episode (:287);
//   7. a reflected walk coordinate flips its zone; both bound tests look at the point before either reflection (:164-168).
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off).
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate
#include "mbx_depop.hpp"    // the carve-up and the phases shared with MadDE and NL_SHADE_LBC
#include "mbx_npsum.hpp"
#include "mbx_qchoose.hpp"

namespace mbx {

constexpr int kHpTries = 25, kHpWalk = MBX_RLHPSDE_WALK, kHpSteps = MBX_RLHPSDE_WALK - 1;
static_assert(kHpWalk <= kThreads, "one thread per walk point");

// per-step records of k_rlhpsde_run (each may be nullptr) and the last action of every instance
struct HpTraj { int32_t* actions; double* state; double* reward; int32_t* last_action; };

__host__ __device__ inline int hp_h(int D) { return D / 2 < 1 ? 1 : D / 2; }

// population size after `fes` evaluations (:92): int(N0 + ((4 - N0) fes) / max_fes), the product exact, truncated
__host__ __device__ inline int hp_np_at(int N0, double fes, double max_fes)
{
    const int n = (int)((double)N0 + ((double)(4 - N0) * fes) / max_fes);
    return n < 1 ? 1 : n;
}

// __get_state (:219-229): the walk into the state block, its costs, the two bits.  best: row 0 of the sorted population.  tape: the instance's
// tape or nullptr.  The state goes to L.RED[12], the features to the state block.  All threads call; ends with a barrier.
template <class PT>
__device__ void hp_walk_state(const PT& P, const MdLds& L, double* FT, double* S, int N0, int D, const Rng& rng, const double* tape,
                              const double* best, const double* __restrict__ logtab)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* W = S + MBX_RLHPSDE_ST_WALK(N0, D);
    double* gWC = S + MBX_RLHPSDE_ST_WCOST(N0, D);
    double* gFT = S + MBX_RLHPSDE_ST_FEAT(N0, D);
    double *WC = FT, *DIST = FT + 202, *DIFF = FT + 402, *HS = FT + 604;
    int* CNT = reinterpret_cast<int*>(FT + 616);
    const double lb = P.lb, ub = P.ub;
    // ---- __progressive_random_walk (:150-169)
    if (tid < D) {
        double uz, uo;
        int rD;
        if (tape) {
            uz = tape[MBX_RLHPSDE_TAPE_ZONE(N0, D) + tid]; uo = tape[MBX_RLHPSDE_TAPE_OFF(N0, D) + tid];
            rD = (int)tape[MBX_RLHPSDE_TAPE_RD(N0, D)];
        } else {
            const U4 w = rng.draw((uint32_t)tid, MBX_SITE_HP_WALK);
            uz = u53(w.x, w.y); uo = u53(w.z, w.w);
            rD = (int)__umulhi(rng.draw((uint32_t)(kHpWalk * D), MBX_SITE_HP_WALK).x, (uint32_t)D);
        }
        double zone = uz < 0.5 ? -1. : 1.;
        const double r = uo * (ub - lb) / 2;
        double x = (ub + lb) / 2 + zone * r;
        if (tid == rD) x = zone == -1. ? lb : ub;
        W[tid] = x;
        for (int s = 1; s <= kHpSteps; ++s) {
            double u;
            if (tape) u = tape[MBX_RLHPSDE_TAPE_STEPU(N0, D) + (int64_t)(s - 1) * D + tid];
            else { const U4 w = rng.draw((uint32_t)(D + (s - 1) * D + tid), MBX_SITE_HP_WALK); u = u53(w.x, w.y); }
            x = x + u * (-10.) * zone;
            const bool cu = x > ub, cl = x < lb;
            if (cu) x = 2 * ub - x;
            if (cl) x = 2 * lb - x;
            if (cu || cl) zone *= -1.;
            W[(int64_t)s * D + tid] = x;
        }
    }
    __syncthreads();
    // ---- the walk's costs, in row chunks
    md_eval_rows(P, L, kHpWalk, kHpWalk, D, [&](int e) { return W[e]; }, WC, rng, tape ? tape + MBX_RLHPSDE_TAPE_WNOISE(N0, D) : nullptr,
                 MBX_SITE_HP_WNOISE_A, MBX_SITE_HP_WNOISE_B);
    if (tid < kHpWalk) gWC[tid] = WC[tid];
    // ---- distances to row 0 (np.linalg.norm(., axis=-1): sqrt of a pairwise row sum) and the first differences
    static_assert(MBX_RLHPSDE_DIM_MAX <= 128 && kHpSteps <= 256, "np_sum_block / np_sum are numpy's order for n <= 128 / 256: D by rlhpsde_check, the walk by its constant");
    if (tid < kHpSteps) {
        const double* x = W + (int64_t)(tid + 1) * D;
        DIST[tid] = sqrt(np_sum_block([&](int d) { const double t = x[d] - best[d]; return t * t; }, D));
        DIFF[tid] = WC[tid + 1] - WC[tid];
    }
    __syncthreads();
    // ---- the two means (waves 0, 1), max |diff| (wave 3)
    if (tid == 0) L.RED[1] = np_sum([&](int i) { return WC[1 + i]; }, kHpSteps) / kHpSteps;
    if (tid == 64) L.RED[2] = np_sum([&](int i) { return DIST[i]; }, kHpSteps) / kHpSteps;
    if (wave == 3) {
        double m = 0.;
        for (int i = lane; i < kHpSteps; i += 64) m = fmax(m, fabs(DIFF[i]));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        if (lane == 0) L.RED[3] = m;
    }
    __syncthreads();
    // ---- covariance and variances (lane 0 of waves 0-2); the transition counts of the nine levels as ballots (every wave)
    const double mc = L.RED[1], md = L.RED[2], star = L.RED[3];
    if (tid == 0) L.RED[4] = np_sum([&](int i) { return (WC[1 + i] - mc) * (DIST[i] - md); }, kHpSteps) / kHpSteps;
    if (tid == 64) L.RED[5] = np_sum([&](int i) { const double t = WC[1 + i] - mc; return t * t; }, kHpSteps) / kHpSteps;
    if (tid == 128) L.RED[6] = np_sum([&](int i) { const double t = DIST[i] - md; return t * t; }, kHpSteps) / kHpSteps;
    {
        const bool on = tid < kHpSteps - 1;
        const double d0 = on ? DIFF[tid] : 0., d1 = on ? DIFF[tid + 1] : 0.;
        for (int k = 0; k < MBX_RLHPSDE_NLEVEL; ++k) {
            const double eps = k == 0 ? 0. : star * (1. / (double)(1 << (MBX_RLHPSDE_NLEVEL - 1 - k)));      // scale in 0, 1/128 .. 1: powers of two, one rounding
            const int s0 = (d0 < -eps ? -1 : 0) + (eps < d0 ? 1 : 0), s1 = (d1 < -eps ? -1 : 0) + (eps < d1 ? 1 : 0);
            const int cls = s0 == s1 ? -1 : s0 == -1 ? (s1 == 0 ? 0 : 1) : s0 == 0 ? (s1 == -1 ? 2 : 3) : (s1 == -1 ? 4 : 5);
#pragma unroll
            for (int c = 0; c < MBX_RLHPSDE_NCLASS; ++c) {
                const int n = __popcll(__ballot(on && cls == c));
                if (lane == 0) CNT[wave * 64 + k * MBX_RLHPSDE_NCLASS + c] = n;
            }
        }
    }
    __syncthreads();
    // ---- the entropy of every level (:206-211), one lane each: (prob * log(prob)) / log(6) summed left to right
    if (tid < MBX_RLHPSDE_NLEVEL) {
        double s = 0.;
        for (int c = 0; c < MBX_RLHPSDE_NCLASS; ++c) {
            const int j = tid * MBX_RLHPSDE_NCLASS + c, n = min(CNT[j] + CNT[64 + j] + CNT[128 + j] + CNT[192 + j], kHpSteps);
            const double f = n == 0 ? 1e-15 : (double)n / (double)kHpSteps;
            s += f * logtab[n] / 1.791759469228055;                  // np.log(6)
            gFT[MBX_RLHPSDE_FEAT_COUNTS + j] = n;
        }
        HS[tid] = -s;
    }
    __syncthreads();
    if (tid == 0) {
        int level = 0;
        for (int k = 1; k < MBX_RLHPSDE_NLEVEL; ++k) if (HS[k] > HS[level]) level = k;
        const double r = L.RED[4] / (sqrt(L.RED[5]) * sqrt(L.RED[6])), h = HS[level];
        const int dfdc = (0.15 < r && r <= 1.) ? 1 : 0, drie = (0.5 <= h && h <= 1.) ? 1 : 0;
        gFT[MBX_RLHPSDE_FEAT_R] = r; gFT[MBX_RLHPSDE_FEAT_H] = h; gFT[MBX_RLHPSDE_FEAT_LEVEL] = level;
        L.RED[12] = dfdc + 2 * drie;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ reset (init_population :123-131)
__global__ __launch_bounds__(kThreads) void k_rlhpsde_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = hp_h(D);
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const MdLds L = md_carve(smem, N0, D);
    double* FT = smem + md_lds_hand_doubles(N0, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_RLHPSDE_ST_SCALARS(N0, D);
    double* gU = S + MBX_RLHPSDE_ST_U(N0, D);
    double* gNC = S + MBX_RLHPSDE_ST_NCOST(N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(CH, D, L.TC));
    // the rows are drawn chunk by chunk on their way into the evaluator
    auto draw = [&](int g) -> double {
        double u;
        if (tape) u = tape[MBX_RLHPSDE_TAPE_POS(N0, D) + g];
        else { const U4 w = rng.draw((uint32_t)g, MBX_SITE_HP_CROSS); u = u53(w.x, w.y); }
        return gU[g] = u * (ub - lb) + lb;
    };
    md_eval_rows(P, L, N0, N0, D, draw, gNC, rng, tape ? tape + MBX_RLHPSDE_TAPE_NOISE_INIT(N0, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    // sort by (cost, row) and move the rows into buffer 0
    double* pop = S + MBX_RLHPSDE_ST_POP(N0, D);
    md_init_sorted(L, gU, gNC, pop, S + MBX_RLHPSDE_ST_COST(N0, D), N0, D);
    for (int t = tid; t < N0; t += kThreads) {
        S[MBX_RLHPSDE_ST_F(N0, D) + t] = 0.;
        S[MBX_RLHPSDE_ST_CR(N0, D) + t] = 0.;
        S[MBX_RLHPSDE_ST_Z(N0, D) + t] = 0.;
        S[MBX_RLHPSDE_ST_X(N0, D) + t] = 0.;
        for (int c = 0; c < 3; ++c) S[MBX_RLHPSDE_ST_R(N0, D) + 3 * t + c] = 0.;
    }
    for (int t = tid; t < H; t += kThreads) { S[MBX_RLHPSDE_ST_MF(N0, D) + t] = 0.5; S[MBX_RLHPSDE_ST_MCR(N0, D) + t] = 0.5; }
    if (tid < MBX_RLHPSDE_FEAT_SLOTS) S[MBX_RLHPSDE_ST_FEAT(N0, D) + tid] = 0.;
    const double gb = L.KEY[0];
    __syncthreads();
    hp_walk_state(P, L, FT, S, N0, D, rng, tape, pop, bp.pci);
    if (tid == 0) {
        const double state = L.RED[12];
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = N0 + kHpWalk; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_HP_NP] = N0; sc[MBX_SC_HP_K] = 0; sc[MBX_SC_HP_LIVE] = 0; sc[MBX_SC_HP_STATE] = state;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = state;
    }
}

// ------------------------------------------------------------------------------------------------ update (:231-287)
// RUN = false: one update with the caller's action (k_rlhpsde_step); RUN = true: up to n_steps updates, the policy decides (k_rlhpsde_run).
template <bool RUN>
__device__ __forceinline__ void hp_steps(const BatchParams& bp, const int32_t* __restrict__ actions, const double* __restrict__ q_table, int n_steps,
                                         const HpTraj& traj, double* __restrict__ state_out, double* __restrict__ reward_out,
                                         uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = hp_h(D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_RLHPSDE_ST_SCALARS(N0, D);
    if (sc[MBX_SC_DONE] != 0.) {                                     // a finished instance stays frozen: the outputs repeat what its last update left
        if (tid == 0) {
            if (reward_out) reward_out[b] = 0.;
            if (done_out) done_out[b] = 1;
            if (state_out) state_out[b] = sc[MBX_SC_HP_STATE];
            if (traj.last_action) traj.last_action[b] = (int)sc[MBX_SC_HP_ACTION];
        }
        return;
    }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const MdLds L = md_carve(smem, N0, D);
    double* FT = smem + md_lds_hand_doubles(N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const double lb = P.lb, ub = P.ub, mf = (double)bp.max_fes;
    double* gC = S + MBX_RLHPSDE_ST_COST(N0, D);
    double* gMF = S + MBX_RLHPSDE_ST_MF(N0, D);
    double* gMCr = S + MBX_RLHPSDE_ST_MCR(N0, D);
    double* gU = S + MBX_RLHPSDE_ST_U(N0, D);
    double* gNC = S + MBX_RLHPSDE_ST_NCOST(N0, D);
    double* gF = S + MBX_RLHPSDE_ST_F(N0, D);
    double* gCr = S + MBX_RLHPSDE_ST_CR(N0, D);
    double* gR = S + MBX_RLHPSDE_ST_R(N0, D);
    stage_problem(P, L.eval(CH, D, L.TC));
    const int episode = (int)sc[MBX_SC_EPISODE];
    double reward_sum = 0.;
    int done = 0, last_action = 0;
    for (int it = 0; it < (RUN ? n_steps : 1) && !done; ++it) {
        const int gen = (int)sc[MBX_SC_GEN] + 1;
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)episode};
        const double fes0 = sc[MBX_SC_FES], ret0 = sc[MBX_SC_RETURN];
        // (clamped: the state block can be caller data, mbx_debug_write_state)
        const int NP = min(max((int)sc[MBX_SC_HP_NP], 1), N0), k_mem = min(max((int)sc[MBX_SC_HP_K], 0), H - 1);
        const int live = sc[MBX_SC_HP_LIVE] != 0. ? 1 : 0;
        const int log_index0 = (int)sc[MBX_SC_LOG_INDEX], cost_len0 = (int)sc[MBX_SC_COST_LEN];
        const double* pop = S + MBX_RLHPSDE_ST_POP(N0, D) + (int64_t)live * N0 * D;
        double* npop = S + MBX_RLHPSDE_ST_POP(N0, D) + (int64_t)(1 - live) * N0 * D;
        const int per = (NP + kThreads - 1) / kThreads, row0 = min(tid * per, NP), row1 = min(row0 + per, NP);
        int action;
        if (RUN) {                                                   // RL_HPSDE_Agent.__get_action (rl_hpsde_agent.py:31-34)
            if (tid == 0) {
                double u;
                if (tape) u = tape[MBX_RLHPSDE_TAPE_CHOICE(N0, D)];
                else { const U4 w = rng.draw(0u, MBX_SITE_POLICY); u = u53(w.x, w.y); }
                L.RED[8] = ql_choose(q_table + 4 * min(max((int)sc[MBX_SC_HP_STATE], 0), 3), u);
            }
            __syncthreads();
            action = (int)L.RED[8];
        } else action = actions[b];
        action = min(max(action, 0), 3);
        last_action = action;
        const bool to_best = (action & 1) != 0, levy = (action >> 1) != 0;
        const int cols = to_best ? 2 : 3;
        // ---- choose_F_Cr (:52-67), generate_random_int (mutate.py:12-33), mutation, np.clip, binomial crossover: trial rows into the state block
        for (int i = row0; i < row1; ++i) {
            int mem, jr, r[3] = {0, 0, 0};
            double z, x;
            if (tape) {
                mem = (int)tape[MBX_RLHPSDE_TAPE_MEM(N0, D) + i]; z = tape[MBX_RLHPSDE_TAPE_Z(N0, D) + i]; x = tape[MBX_RLHPSDE_TAPE_X(N0, D) + i];
                jr = (int)tape[MBX_RLHPSDE_TAPE_JRAND(N0, D) + i];
                for (int c = 0; c < cols; ++c) r[c] = (int)tape[MBX_RLHPSDE_TAPE_R(N0, D) + 3 * i + c];
            } else {
                const U4 v = rng.draw((uint32_t)i, MBX_SITE_HP_PAR);
                mem = (int)__umulhi(v.x, (uint32_t)H); jr = (int)__umulhi(v.y, (uint32_t)D);
                const U4 w = rng.draw((uint32_t)i, MBX_SITE_HP_NORM);
                double s;
                box_muller(u53(w.x, w.y), u53(w.z, w.w), z, s);
                if (levy) x = 1. / (s * s);
                else { const U4 c = rng.draw((uint32_t)i, MBX_SITE_HP_CAUCHY); x = tan(3.141592653589793 * (u53(c.x, c.y) - 0.5)); }
                // the redraw loops, column by column: one draw, then at most kHpTries redraws while the column repeats an earlier one or the row
                for (int c = 0; c < cols; ++c)
                    for (int a = 0; a <= kHpTries; ++a) {
                        const U4 q = rng.draw((uint32_t)(i * 32 + a), MBX_SITE_HP_IDX);
                        r[c] = (int)__umulhi(c == 0 ? q.x : c == 1 ? q.y : q.z, (uint32_t)NP);
                        if (!(r[c] == i || (c > 0 && r[c] == r[0]) || (c > 1 && r[c] == r[1]))) break;
                    }
            }
            mem = min(max(mem, 0), H - 1); jr = min(max(jr, 0), D - 1);
            for (int c = 0; c < 3; ++c) r[c] = min(max(r[c], 0), NP - 1);               // a tape cannot send a read outside the population
            const double Cr = fmin(1., fmax(0., gMCr[mem] + 0.1 * z)), loc = gMF[mem];
            double F = x * 0.1 + loc;
            if (F < 0.) F = 2 * loc - F;
            F = fmin(1., F);
            gF[i] = F; gCr[i] = Cr;
            S[MBX_RLHPSDE_ST_Z(N0, D) + i] = z; S[MBX_RLHPSDE_ST_X(N0, D) + i] = x;
            for (int c = 0; c < 3; ++c) gR[3 * i + c] = r[c];
            const double* xi = pop + (int64_t)i * D;
            const double* x0 = pop + (int64_t)r[0] * D;
            const double* x1 = pop + (int64_t)r[1] * D;
            const double* x2 = pop + (int64_t)r[2] * D;
            for (int d = 0; d < D; ++d) {
                double cu;
                if (tape) cu = tape[MBX_RLHPSDE_TAPE_CROSS(N0, D) + (int64_t)i * D + d];
                else { const U4 w = rng.draw((uint32_t)(i * D + d), MBX_SITE_HP_CROSS); cu = u53(w.x, w.y); }
                double v;
                if (to_best) v = xi[d] + F * (pop[d] - xi[d] + x0[d] - x1[d]);
                else v = xi[d] + F * (x0[d] - xi[d] + x1[d] - x2[d]);
                v = fmin(fmax(v, lb), ub);
                gU[(int64_t)i * D + d] = (cu < Cr || d == jr) ? v : xi[d];
            }
        }
        __syncthreads();
        // ---- evaluation of the trials in row chunks
        md_eval_rows(P, L, NP, N0, D, [&](int e) { return gU[e]; }, gNC, rng, tape ? tape + MBX_RLHPSDE_TAPE_NOISE(N0, D) : nullptr, MBX_SITE_HP_NOISE_A,
                     MBX_SITE_HP_NOISE_B);
        // ---- selection (:259): ranks of the improved rows
        int obase, n_opt;
        md_rank_improved(L, gC, gNC, row0, row1, obase, n_opt);
        // ---- memory (:70-87): weighted Lehmer means over the improved rows, compacted in rank order, numpy's pairwise sums
        double newMF = 0.5, newMCr = 0.5;
        if (n_opt > 0) {
            // pass 0: df;  1: w SF;  2: w SF^2;  3: w SCr;  4: w SCr^2
            double sums[5];
            md_weighted_sums(L, gC, gNC, row0, row1, obase, n_opt, [](double c, double nc) { return fmax(0., c - nc); },
                             [&](int pass, double w, int i) { const double s = pass <= 2 ? gF[i] : gCr[i]; return (pass & 1) ? w * s : w * (s * s); }, sums);
            newMF = sums[1] > 0.000001 ? sums[2] / sums[1] : 0.5;
            newMCr = sums[3] > 0.000001 ? sums[4] / sums[3] : 0.5;
        }
        // ---- replacement, LPSR, sort (:265-271, :90-98): rows into the other buffer in (cost, row) order
        const double fes = fes0 + NP;
        const int NPn = min(hp_np_at(N0, fes, mf), NP);
        md_replace_sorted(L, gC, gNC, gU, pop, npop, NP, NPn, D);
        // ---- bookkeeping (:273-286)
        if (tid == 0) {
            const double gbest = L.KEY[0], reward = (double)n_opt / (double)NP;
            gMF[k_mem] = newMF; gMCr[k_mem] = newMCr;
            int log_index = log_index0, cost_len = cost_len0;
            const bool dn = log_and_terminate(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
            sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
            sc[MBX_SC_DONE] = dn ? 1. : 0.; sc[MBX_SC_GEN] = gen; sc[MBX_SC_GBEST_IDX] = 0; sc[MBX_SC_RETURN] = ret0 + reward;
            sc[MBX_SC_HP_NP] = NPn; sc[MBX_SC_HP_K] = n_opt > 0 ? (k_mem + 1) % H : k_mem; sc[MBX_SC_HP_LIVE] = 1 - live;
            sc[MBX_SC_HP_ACTION] = action;
            S[MBX_RLHPSDE_ST_FEAT(N0, D) + MBX_RLHPSDE_FEAT_NOPT] = n_opt;
            L.RED[9] = reward; L.RED[10] = dn ? 1. : 0.;
        }
        __syncthreads();
        // ---- __get_state (:287): the walk is billed after the done test
        hp_walk_state(P, L, FT, S, N0, D, rng, tape, npop, bp.pci);
        const double reward = L.RED[9], state = L.RED[12];
        done = L.RED[10] != 0.;
        reward_sum += reward;
        if (tid == 0) {
            sc[MBX_SC_FES] = fes + kHpWalk; sc[MBX_SC_HP_STATE] = state;
            if (RUN) {
                const int64_t row = (int64_t)it * bp.B + b;
                if (traj.actions) traj.actions[row] = action;
                if (traj.reward) traj.reward[row] = reward;
                if (traj.state) traj.state[row] = state;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (state_out) state_out[b] = sc[MBX_SC_HP_STATE];
        if (reward_out) reward_out[b] = reward_sum;
        if (done_out) done_out[b] = done ? 1 : 0;
        if (traj.last_action) traj.last_action[b] = last_action;
    }
}

__global__ __launch_bounds__(kThreads) void k_rlhpsde_step(BatchParams bp, const int32_t* __restrict__ actions, double* __restrict__ state_out,
                                                           double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    hp_steps<false>(bp, actions, nullptr, 1, HpTraj{}, state_out, reward_out, done_out);
}

__global__ __launch_bounds__(kThreads) void k_rlhpsde_run(BatchParams bp, const double* __restrict__ q_table, int n_steps, HpTraj traj,
                                                          double* __restrict__ state_out, double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    hp_steps<true>(bp, nullptr, q_table, n_steps, traj, state_out, reward_out, done_out);
}

}  // namespace mbx
