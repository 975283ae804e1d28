// mbx_dedqn.hpp — DEDQN step kernels for gfx950 (reference: src/optimizer/dedqn_optimizer.py:8-206, src/optimizer/operators/mutate.py:5-9,
// 36-39, 88-91, 178-181, crossover.py:6-18, boundary_control.py:5-9, and the greedy policy of src/agent/dedqn_agent.py:44-53, 89-98).
//
// One env step builds ONE trial vector for the row `pointer` (rand_1 / cur_to_rand_1 / best_2, F = 0.5, clipping, binomial crossover with
// Cr = 0.5), evaluates it, selects (`u_cost <= cost[pointer]`), and then runs the landscape analysis of __cal_feature (:130-142): the WHOLE
// population is evaluated again, a random walk of NP points through the population's bounding box is drawn, and four features pair walk
// point i with the cost of population row i (the reference's own pairing; the fresh costs are never written back):
//   fdc (:8-12)   fitness-distance correlation over the distances to the walk point of the cheapest row;
//   rie (:15-52)  the largest base-6 entropy of the six kinds of symbol transitions over nine ruggedness thresholds epsilon_star / 2^k, 0;
//   acf (:55-62)  lag-1 autocorrelation, a sequential sum over a pairwise-summed denominator;
//   nop (:65-76)  descents of the cost along the order of the distances (ties among equal distances: by index), over NP.
// A step bills NP evaluations for the trial and NP for the walk (:178, :141), so a D = 10 episode is 99 steps.  The reward (:92-100) is a
// sequential sum over the survival counters.  `gbest` is a numpy view of the initial best row until the first strict improvement (:151,
// :183-185): a row index plus an alias flag in the scalars.
//
// (bp.pci, RLEPSO's per-batch table pointer, carries DEDQN's per-batch table instead: logtab[0 .. NP], see dd_features.)
// One instance per workgroup of 256 threads.  Population, costs, survival counters and the last features stay in LDS for every step of a
// launch: k_dedqn_step (one step, action from the caller) and k_dedqn_run (n_steps steps, the 4 -> 10 -> 10 -> 3 Q-network evaluated in the
// workgroup) are the same body, so they are bit-identical by construction.  Means, variances and the row norms follow numpy's pairwise
// order (mbx_npsum.hpp); sums that the reference writes as Python loops are sequential on one lane.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"

namespace mbx {

constexpr int kDdLevels = 9, kDdClasses = 6;
constexpr int kDdQnetFloats = 4 * 10 + 10 + 10 * 10 + 10 + 10 * 3 + 3;      // W1t b1 W2t b2 W3t b3
constexpr int kDdRedrawMax = 1024;

// per-step records of k_dedqn_run (each may be nullptr) and the last action of every instance
struct DedqnTraj { int32_t* actions; double* state; double* reward; int32_t* last_action; };

// The LDS layout (DdLds, dd_lds_doubles, dd_carve) lives in mbx_lds.hpp.

// __cal_feature (:130-142) for the population in L.POP: costs into L.SCOST, the four features and the diagnostics into L.FEAT.
// tape_walk / tape_noise: the step's (or the reset's) slots of the replay tape, or nullptr.  All threads call; ends with a barrier.
template <class PT>
__device__ void dd_features(const PT& P, const DdLds& L, int NP, int D, const Rng& rng, const double* tape_walk, const double* tape_noise,
                            const double* __restrict__ logtab)
{
    const int tid = threadIdx.x, NE = NP * D, lane = tid & 63, wave = tid >> 6;
    population_costs(P, L.eval(L.POP, L.SCOST), NP, rng, tape_noise, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    // ---- random_walk_sampling (:79-89): the uniforms by every thread, then one lane per coordinate walks its chain (a sequential sum modulo 1)
    // (uniforms in Z, walk points in T -- both the evaluator's scratch, free now: loads of the chain do not wait for its stores)
    double* __restrict__ U = L.Z;
    double* __restrict__ W = L.T;
    for (int e = tid; e < NE; e += MBX_NT) {
        double u;
        if (tape_walk) u = tape_walk[e];
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_DD_WALK); u = u53(w.x, w.y); }
        U[e] = u;
    }
    __syncthreads();
    if (tid < D) {
        double pmin = L.POP[tid], pmax = pmin;
#pragma unroll 4
        for (int i = 1; i < NP; ++i) { const double x = L.POP[i * D + tid]; pmin = fmin(pmin, x); pmax = fmax(pmax, x); }
        const double span = pmax - pmin;
        double w = U[tid];
        W[tid] = pmin + span * w;
#pragma unroll 4
        for (int i = 1; i < NP; ++i) {
            w = w + U[i * D + tid];
            if (w >= 1.) w -= 1.;                                    // (start + move) % 1 on [0, 2): exact
            W[i * D + tid] = pmin + span * w;
        }
    }
    double fbest; int best;
    block_argmin(L.SCOST, NP, L.RED, fbest, best);                  // np.argmin: first minimum
    // ---- distances to the walk point of the cheapest row (np.linalg.norm(., axis=-1): sqrt of a pairwise row sum) and the first differences
    if (tid < NP) {
        const double *x = W + tid * D, *xb = W + best * D;
        L.DIST[tid] = sqrt(np_sum([&](int d) { const double t = x[d] - xb[d]; return t * t; }, D));
        L.DIFF[tid] = tid < NP - 1 ? L.SCOST[tid + 1] - L.SCOST[tid] : 0.;
    }
    __syncthreads();
    // ---- A: the order of the distances (waves 0-1), the two means (waves 2 and 3, numpy's pairwise sums over eight lanes), epsilon_star (wave 3)
    if (tid < NP) {
        const double di = L.DIST[tid];
        int rank = 0;
        for (int j = 0; j < NP; ++j) { const double dj = L.DIST[j]; rank += (dj < di) || (dj == di && j < tid); }
        L.SORTED[rank] = L.SCOST[tid];
    }
    static_assert(MBX_DEDQN_NP_MAX <= 128, "np_sum_lanes8 is numpy's order for n <= 128: the NP sums below rest on dedqn_check's np <= MBX_DEDQN_NP_MAX");
    if (wave == 2) {
        const double m = np_sum_lanes8([&](int i) { return L.SCOST[i]; }, NP) / NP;
        if (lane == 0) L.RED[2] = m;
    }
    if (wave == 3) {                                                 // ... and the largest positive first difference, 0 if there is none (:16-19)
        const double mean_d = np_sum_lanes8([&](int i) { return L.DIST[i]; }, NP) / NP;
        if (lane == 0) L.RED[3] = mean_d;
        double m = 0.;
        for (int i = lane; i < NP - 1; i += 64) m = fmax(m, L.DIFF[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        if (lane == 0) L.RED[4] = m;
    }
    __syncthreads();
    // ---- B: descents and the transition counts of the nine levels as ballots (waves 0-1); the pairwise sums (wave 2); the lag-1 sum (wave 3)
    const double mf = L.RED[2], md = L.RED[3], star = L.RED[4];
    if (tid < 128) {
        const bool desc = tid < NP - 1 && L.SORTED[tid + 1] < L.SORTED[tid];
        const int ndesc = __popcll(__ballot(desc));
        if (lane == 0) L.CNT[wave * 64 + kDdLevels * kDdClasses] = ndesc;
        const bool on = tid < NP - 2;
        const double d0 = on ? L.DIFF[tid] : 0., d1 = on ? L.DIFF[tid + 1] : 0.;
        for (int k = 0; k < kDdLevels; ++k) {
            const double eps = k == kDdLevels - 1 ? 0. : star * (1. / (double)(1 << k));      // epsilon_star / 2 ** k: one rounding, like the division
            const int s0 = d0 < -eps ? -1 : (d0 > eps ? 1 : 0), s1 = d1 < -eps ? -1 : (d1 > eps ? 1 : 0);
            const int cls = (s0 == -1 && s1 == 0) ? 0 : (s0 == -1 && s1 == 1) ? 1 : (s0 == 0 && s1 == 1) ? 2 : (s0 == 0 && s1 == -1) ? 3 : (s0 == 1 && s1 == -1) ? 4 : 5;
#pragma unroll
            for (int c = 0; c < kDdClasses; ++c) {
                const int n = __popcll(__ballot(on && cls == c));
                if (lane == 0) L.CNT[wave * 64 + k * kDdClasses + c] = n;
            }
        }
    }
    if (wave == 2) {
        const double cfd = np_sum_lanes8([&](int i) { return (L.SCOST[i] - mf) * (L.DIST[i] - md); }, NP) / NP;
        const double vd = np_sum_lanes8([&](int i) { const double t = L.DIST[i] - md; return t * t; }, NP) / NP;              // np.var(distance)
        if (lane == 0) { L.RED[5] = cfd; L.RED[6] = vd; }
    }
    if (wave == 3) {
        const double ss = np_sum_lanes8([&](int i) { const double t = L.SCOST[i] - mf; return t * t; }, NP);                  // sum of squares: np.var(fitness) * NP, cal_acf's a - 1e-6
        if (lane == 0) {
            double acc = 0.;
#pragma unroll 4
            for (int i = 0; i < NP - 1; ++i) acc += (L.SCOST[i] - mf) * (L.SCOST[i + 1] - mf);
            L.RED[7] = ss; L.RED[8] = acc;
        }
    }
    __syncthreads();
    // ---- C: the entropy of every level (:48-51), one lane each.  A frequency is n / NP with n <= NP <= 128: its logarithm comes from the batch's table of
    // CORRECTLY ROUNDED values (logtab[n] = log(n / NP), built on the host in extended precision, mbx.hip), not from the device's log, so that
    // the entropy is the same double wherever the reference's log is correctly rounded on these arguments (numpy's is at NP = 100); the product, the
    // quotient and the six-term sum are IEEE operations in numpy's order.
    if (tid < kDdLevels) {
        double s = 0.;
        for (int c = 0; c < kDdClasses; ++c) {
            const int n = L.CNT[tid * kDdClasses + c] + L.CNT[64 + tid * kDdClasses + c];
            const int m = n == 0 ? NP : n;
            const double f = (double)m / (double)NP;
            s += f * logtab[m] / 1.791759469228055;                  // np.log(6)
        }
        L.HS[tid] = -s;
    }
    __syncthreads();
    if (tid == 0) {
        int level = 0;
        for (int k = 1; k < kDdLevels; ++k) if (L.HS[k] > L.HS[level]) level = k;
        const double ss = L.RED[7];
        L.FEAT[0] = L.RED[5] / (L.RED[6] * (ss / NP) + 1e-6);
        L.FEAT[1] = L.HS[level];
        L.FEAT[2] = L.RED[8] / (ss + 1e-6);
        L.FEAT[3] = (double)(L.CNT[kDdLevels * kDdClasses] + L.CNT[64 + kDdLevels * kDdClasses]) / (double)NP;
        L.FEAT[MBX_DEDQN_FEAT_LEVEL] = level;
        for (int c = 0; c < kDdClasses; ++c) L.FEAT[MBX_DEDQN_FEAT_COUNTS + c] = L.CNT[level * kDdClasses + c] + L.CNT[64 + level * kDdClasses + c];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ reset (init_population :144-157)
__global__ __launch_bounds__(kThreads) void k_dedqn_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const DdLds L = dd_carve(smem, NP, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_DEDQN_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const double pointer = sc[MBX_SC_DEDQN_POINTER];               // survives the reset, as in the reference (:118)
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(L.POP, L.COST));
    for (int e = tid; e < NE; e += kThreads) {
        double u;
        if (tape) u = tape[MBX_DEDQN_TAPE_POS(NP, D) + e];
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_LDE_ELEM); u = u53(w.x, w.y); }
        const double x = u * (ub - lb) + lb;
        L.POP[e] = x; S[MBX_DEDQN_ST_POP(NP, D) + e] = x;
    }
    __syncthreads();
    population_costs(P, L.eval(L.POP, L.COST), NP, rng, tape ? tape + MBX_DEDQN_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_DD_NOISE_A, MBX_SITE_DD_NOISE_B);
    double gb; int g0;
    block_argmin(L.COST, NP, L.RED, gb, g0);
    dd_features(P, L, NP, D, rng, tape ? tape + MBX_DEDQN_TAPE_WALK_INIT(NP, D) : nullptr, tape ? tape + MBX_DEDQN_TAPE_NOISE_FEAT0(NP, D) : nullptr, bp.pci);
    for (int i = tid; i < NP; i += kThreads) {
        S[MBX_DEDQN_ST_COST(NP, D) + i] = L.COST[i]; S[MBX_DEDQN_ST_SURVIVAL(NP, D) + i] = 1.; S[MBX_DEDQN_ST_SCOST(NP, D) + i] = L.SCOST[i];
    }
    if (tid < D) S[MBX_DEDQN_ST_GBPOS(NP, D) + tid] = L.POP[g0 * D + tid];
    if (tid < MBX_DEDQN_FEAT_SLOTS) S[MBX_DEDQN_ST_FEAT(NP, D) + tid] = tid < MBX_DEDQN_FEAT_UCOST ? L.FEAT[tid] : 0.;
    if (tid < MBX_DEDQN_NFEAT && state_out) state_out[(int64_t)b * MBX_DEDQN_NFEAT + tid] = L.FEAT[tid];
    if (tid == 0) {
        for (int k = 0; k < MBX_NSCALAR; ++k) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = 2 * NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = g0; sc[MBX_SC_DEDQN_POINTER] = pointer; sc[MBX_SC_DEDQN_G0] = g0; sc[MBX_SC_DEDQN_ALIAS] = 1.;
        sc[MBX_NSCALAR] = gb;
    }
}

// DEDQN_Agent.__get_action without exploration (dedqn_agent.py:44-53): Q = MLP(float32(state)), argmax (first maximum).  float32, one fma chain
// per unit in ascending k starting at the bias, like the other in-kernel policies.  Every lane of the calling wave takes part and gets the answer.
__device__ __forceinline__ int dd_qnet(const float* __restrict__ w, const double* feat, float q[3])
{
    const int lane = threadIdx.x & 63;
    float a1 = lane < 10 ? w[40 + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) a1 = lane < 10 ? __builtin_fmaf(w[k * 10 + lane], (float)feat[k], a1) : 0.f;
    const float h1 = fmaxf(a1, 0.f);
    float a2 = lane < 10 ? w[150 + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) { const float h = __shfl(h1, k, 64); a2 = lane < 10 ? __builtin_fmaf(w[50 + k * 10 + lane], h, a2) : 0.f; }
    const float h2 = fmaxf(a2, 0.f);
    float a3 = lane < 3 ? w[190 + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) { const float h = __shfl(h2, k, 64); a3 = lane < 3 ? __builtin_fmaf(w[160 + k * 3 + lane], h, a3) : 0.f; }
    q[0] = __shfl(a3, 0, 64); q[1] = __shfl(a3, 1, 64); q[2] = __shfl(a3, 2, 64);
    int a = 0;
    if (q[1] > q[a]) a = 1;
    if (q[2] > q[a]) a = 2;
    return a;
}

// ------------------------------------------------------------------------------------------------ step (update :159-206)
// RUN = false: one step with the caller's action (k_dedqn_step); RUN = true: up to n_steps steps with the Q-network in the workgroup (k_dedqn_run).
template <bool RUN>
__device__ __forceinline__ void dd_steps(const BatchParams& bp, const int32_t* __restrict__ actions, const float* __restrict__ net, int n_steps,
                                         const DedqnTraj& traj, double* __restrict__ state_out, double* __restrict__ reward_out,
                                         uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_DEDQN_ST_SCALARS(NP, D);
    if (sc[MBX_SC_DONE] != 0.) {
        if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; }
        return;
    }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const DdLds L = dd_carve(smem, NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const double lb = P.lb, ub = P.ub, F = 0.5, Cr = 0.5;

    stage_problem(P, L.eval(L.POP, L.SCOST));
    for (int e = tid; e < NE; e += kThreads) L.POP[e] = S[MBX_DEDQN_ST_POP(NP, D) + e];
    for (int i = tid; i < NP; i += kThreads) { L.COST[i] = S[MBX_DEDQN_ST_COST(NP, D) + i]; L.SURV[i] = S[MBX_DEDQN_ST_SURVIVAL(NP, D) + i]; }
    if (tid < D) L.GB[tid] = S[MBX_DEDQN_ST_GBPOS(NP, D) + tid];
    if (tid < MBX_DEDQN_FEAT_SLOTS) L.FEAT[tid] = S[MBX_DEDQN_ST_FEAT(NP, D) + tid];
    if (tid < MBX_NSCALAR) L.SC[tid] = sc[tid];
    __syncthreads();
    const int episode = (int)L.SC[MBX_SC_EPISODE];
    double reward_sum = 0.;
    int done = 0, last_action = 0;
    for (int it = 0; it < (RUN ? n_steps : 1) && !done; ++it) {
        const int step = (int)L.SC[MBX_SC_GEN] + 1, p = (int)L.SC[MBX_SC_DEDQN_POINTER], g0 = (int)L.SC[MBX_SC_DEDQN_G0];
        const bool alias = L.SC[MBX_SC_DEDQN_ALIAS] != 0.;
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)episode, true};
        int action;
        float q[3] = {0.f, 0.f, 0.f};
        if (RUN) action = dd_qnet(net, L.FEAT, q);                   // every wave evaluates the 193 weights for itself: no broadcast, no barrier
        else action = actions[b];
        last_action = action;
        if (tid == 0) {                                              // generate_random_int_single (mutate.py:5-9), binomial's jrand (crossover.py:11)
            const int cols = (action == 0 || action == 1) ? 3 : 4;
            int r[4];
            if (tape) { for (int j = 0; j < 4; ++j) r[j] = (int)tape[MBX_DEDQN_TAPE_R(NP, D) + j]; }
            else {
                for (int a = 0; a < kDdRedrawMax; ++a) {
                    const U4 w = rng.draw((uint32_t)a, MBX_SITE_DD_R);
                    r[0] = (int)__umulhi(w.x, (uint32_t)NP); r[1] = (int)__umulhi(w.y, (uint32_t)NP);
                    r[2] = (int)__umulhi(w.z, (uint32_t)NP); r[3] = (int)__umulhi(w.w, (uint32_t)NP);
                    if (!(r[0] == p || r[1] == p || r[2] == p || (cols == 4 && r[3] == p))) break;
                }
            }
            int jr;
            if (tape) jr = (int)tape[MBX_DEDQN_TAPE_JRAND(NP, D)];
            else { const U4 w = rng.draw(0u, MBX_SITE_DQ_JRAND); jr = (int)__umulhi(w.x, (uint32_t)D); }
            for (int j = 0; j < 4; ++j) L.IR[j] = min(max(r[j], 0), NP - 1);            // a tape cannot send a read outside the population
            L.IR[4] = min(max(jr, 0), D - 1);
        }
        __syncthreads();
        // ---- mutation (left to right as written), np.clip, binomial crossover
        if (tid < D) {
            const int d = tid;
            const double x0 = L.POP[L.IR[0] * D + d], x1 = L.POP[L.IR[1] * D + d], x2 = L.POP[L.IR[2] * D + d], x3 = L.POP[L.IR[3] * D + d];
            const double xp = L.POP[p * D + d], best = alias ? L.POP[g0 * D + d] : L.GB[d];
            double v;
            if (action == 0) v = x0 + F * (x1 - x2);
            else if (action == 1) v = xp + F * (x0 - xp + x1 - x2);
            else v = best + F * (x0 - x1 + x2 - x3);
            v = fmin(fmax(v, lb), ub);
            double cu;
            if (tape) cu = tape[MBX_DEDQN_TAPE_CROSS(NP, D) + d];
            else { const U4 w = rng.draw((uint32_t)d, MBX_SITE_LDE_ELEM); cu = u53(w.x, w.y); }
            L.TRIAL[d] = (cu < Cr || d == L.IR[4]) ? v : xp;
        }
        __syncthreads();
        {
            const RowPost post{&rng, tape ? tape + MBX_DEDQN_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B, 1};
            eval_rows(P, L.eval(L.TRIAL, L.RED + 16), 1, &post);
        }
        // ---- selection (:179-187)
        const double u_cost = L.RED[16];
        const bool sel = u_cost <= L.COST[p], better = sel && u_cost < L.SC[MBX_SC_GBEST];
        __syncthreads();
        if (sel && tid < D) { L.POP[p * D + tid] = L.TRIAL[tid]; if (better) L.GB[tid] = L.TRIAL[tid]; }
        if (tid == 0) {
            if (sel) {
                L.COST[p] = u_cost; L.SURV[p] = 1.;
                if (better) { L.SC[MBX_SC_GBEST] = u_cost; L.SC[MBX_SC_DEDQN_ALIAS] = 0.; L.SC[MBX_SC_GBEST_IDX] = p; }
            } else L.SURV[p] += 1.;
        }
        __syncthreads();
        dd_features(P, L, NP, D, rng, tape ? tape + MBX_DEDQN_TAPE_WALK(NP, D) : nullptr, tape ? tape + MBX_DEDQN_TAPE_NOISE_FEAT(NP, D) : nullptr, bp.pci);
        if (tid < NP) L.DIST[tid] = 1. / L.SURV[tid];                // cal_reward's quotients side by side; their sum stays sequential
        __syncthreads();
        if (tid == 0) {
            const double fes = L.SC[MBX_SC_FES] + 2 * NP, gbest = L.SC[MBX_SC_GBEST];
            int log_index = (int)L.SC[MBX_SC_LOG_INDEX], cost_len = (int)L.SC[MBX_SC_COST_LEN];
            const bool dn = log_and_terminate(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
            double acc = 0.;                                         // cal_reward (:92-100), before the pointer moves on
#pragma unroll 4
            for (int i = 0; i < NP; ++i) {
                if (i == p) { if (L.SURV[i] == 1.) acc += 1.; }
                else acc += L.DIST[i];
            }
            const double reward = acc / NP;
            L.SC[MBX_SC_FES] = fes; L.SC[MBX_SC_LOG_INDEX] = log_index; L.SC[MBX_SC_COST_LEN] = cost_len; L.SC[MBX_SC_DONE] = dn ? 1. : 0.;
            L.SC[MBX_SC_RETURN] += reward; L.SC[MBX_SC_GEN] = step; L.SC[MBX_SC_DEDQN_POINTER] = (p + 1) % NP;
            L.RED[17] = reward;
            L.FEAT[MBX_DEDQN_FEAT_UCOST] = u_cost;                      // diagnostics: the trial's cost and the Q values behind the action
            for (int k = 0; k < 3; ++k) L.FEAT[MBX_DEDQN_FEAT_Q + k] = q[k];
            if (RUN) {
                const int64_t row = (int64_t)it * bp.B + b;
                if (traj.actions) traj.actions[row] = action;
                if (traj.reward) traj.reward[row] = reward;
            }
        }
        __syncthreads();
        reward_sum += L.RED[17];
        done = L.SC[MBX_SC_DONE] != 0.;
        if (RUN && traj.state && tid < MBX_DEDQN_NFEAT) traj.state[((int64_t)it * bp.B + b) * MBX_DEDQN_NFEAT + tid] = L.FEAT[tid];
    }
    // ---- the state block, once per launch
    for (int e = tid; e < NE; e += kThreads) S[MBX_DEDQN_ST_POP(NP, D) + e] = L.POP[e];
    for (int i = tid; i < NP; i += kThreads) {
        S[MBX_DEDQN_ST_COST(NP, D) + i] = L.COST[i]; S[MBX_DEDQN_ST_SURVIVAL(NP, D) + i] = L.SURV[i]; S[MBX_DEDQN_ST_SCOST(NP, D) + i] = L.SCOST[i];
    }
    if (tid < D) S[MBX_DEDQN_ST_GBPOS(NP, D) + tid] = L.SC[MBX_SC_DEDQN_ALIAS] != 0. ? L.POP[(int)L.SC[MBX_SC_DEDQN_G0] * D + tid] : L.GB[tid];
    if (tid < MBX_DEDQN_FEAT_SLOTS) S[MBX_DEDQN_ST_FEAT(NP, D) + tid] = L.FEAT[tid];
    if (tid < MBX_NSCALAR) sc[tid] = L.SC[tid];
    if (tid < MBX_DEDQN_NFEAT && state_out) state_out[(int64_t)b * MBX_DEDQN_NFEAT + tid] = L.FEAT[tid];
    if (tid == 0) {
        if (reward_out) reward_out[b] = reward_sum;
        if (done_out) done_out[b] = done ? 1 : 0;
        if (RUN && traj.last_action) traj.last_action[b] = last_action;
    }
}

// Registers: the compiler takes 228 / 236 VGPRs (two workgroups per CU, although 32 KB of LDS at NP = 100 / D = 10 would admit five).  A cap applies to the
// three kernels together (the evaluator and dd_features are out-of-line functions they share).  Measured, us per env step, k_dedqn_step / k_dedqn_run:
// D = 10, 4096 instances: no cap 499 / 457, 168 registers 387 / 424, 128 registers 353 / 443 (k_dedqn_run then spills 122 registers around its step loop);
// D = 30, 1024 instances: 388 / 361, 398 / 414, 416 / 433.  (Wall times of tools/kbench_algos.py in one session, launch gaps included; the per-launch
// medians of a kernel trace of the uncapped build are 513 / 450 and 400 / 360, docs/EXPERIMENTS.md.)  The resident kernel is the one rollouts run: without
// a cap it is the fastest at D = 30 and within 7 % of its best (the 168-register build) at D = 10, so none is set.
__global__ __launch_bounds__(kThreads) void k_dedqn_step(BatchParams bp, const int32_t* __restrict__ actions, double* __restrict__ state_out,
                                                         double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    dd_steps<false>(bp, actions, nullptr, 1, DedqnTraj{}, state_out, reward_out, done_out);
}

__global__ __launch_bounds__(kThreads) void k_dedqn_run(BatchParams bp, const float* __restrict__ net, int n_steps, DedqnTraj traj,
                                                        double* __restrict__ state_out, double* __restrict__ reward_out, uint8_t* __restrict__ done_out)
{
    dd_steps<true>(bp, nullptr, net, n_steps, traj, state_out, reward_out, done_out);
}

}  // namespace mbx
