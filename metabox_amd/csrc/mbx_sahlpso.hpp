// mbx_sahlpso.hpp — SAHLPSO, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/sahlpso.py:6-161; layout, tape
// and Philox sites: include/mbx_layout.h section 17).
//
// Self-adaptive PSO with two learning strategies: 40 particles, of which 8 fixed "exploration" particles learn from the better of two random
// live particles and the others from one of the best 20 %, blended with gBest; a crossover rate cr out of 8 (5 in use) and a history depth ls
// out of 15 are picked per move with probabilities re-estimated every 5 generations from their success rates; a failed move redraws the
// particle's inertia weight; the population shrinks linearly from 40 to 4 by initial rank.
//
// The reference moves its particles ONE AFTER THE OTHER inside a generation (:50-124): gBest is a view of a row of X, pBest rows are written in
// place by the crossover, f_X of earlier particles decides the exemplar of later ones, and `done` is looked at after every move.  One mbx_step
// is nevertheless one launch for the whole pass: one workgroup per instance (through bp.order) keeps X, V and pBest in LDS (3 x 40 x D doubles,
// 38.4 KB at D = 40) and walks remain_index strictly in order.  The D-wide work of a move -- exemplar, crossover, velocity, the clips -- is
// done by the lanes of wave 0, the single-row objective by all four waves (eval_rows with one row), and the move's bookkeeping by wave 0
// again, so that consecutive moves hand over inside one wave.  Block barriers per move: ONE of this file's (the new row is handed to the
// evaluator) plus the evaluator's own; its last one hands the cost back.  success, gBest_cost, g, fes, the log and `done` are recomputed by every
// thread from the cost alone, so the loop's exit is uniform without another barrier.  A move's draws are keyed by (pass, slot, element): no
// serial generator state.
//
// The reference's own behaviour, kept on purpose (line numbers of sahlpso.py):
//  * pBest_cost is never written after :31.  Success is f_X[i] < pBest_cost0[i] (:93); np.argsort(pBest_cost) (:68, :153) is ONE fixed ranking,
//    stored at reset (cost, then the lower index).  remain_index is 0..39 until the first reduction and rank[:NP] afterwards -- the iteration
//    order is then rank order (:50, :153) -- and best_p_index is rank[:max(1, int(0.2 NP))] (:68).
//  * every entry of A[i] is a view of the row pBest[i] (:33, :108), so history_pbest is that row whatever ls is (:63-66, :70): ls changes
//    nothing but the draw count and the nf_ls / ns_ls statistics.  e[mask] = o[mask] (:73-74) therefore writes INTO pBest[i], whether or not the
//    move succeeds, and touches no cost.
//  * gBest is a view of X[g] (:34, :96): the row index g is kept and X[g] read wherever gBest is used (:77), also after row g has moved on;
//    gBest_cost (:35, :97) is a scalar of its own and goes stale when row g moves without improving.
//  * in generations with G % 5 == 0 and G != 1 nothing is chosen: cr = 0, no crossover (the rand(D) of :72 is drawn all the same), and both
//    counters go to index 0 (:51-57, :80-81, :99-100).  nf / ns are never zeroed.
//  * exploration particles take o by the CURRENT f_X[m] < f_X[n], not by pbest cost; m and n come from the current remain_index (:60-62).
//  * the bounds are the literals -5 and 5 and v_max is 1, whatever the problem says (:10).
//  * a failed move draws rnd2, then 0.7 or 0.3 plus 0.1 * standard_cauchy, clipped to [0.2, 0.9] (:102-107); w is not touched otherwise.
//  * one cost.append per move at most (:110-112); `done` after every move (:114-124): an episode can end in the middle of a pass, the later
//    particles then stay as they are and fes is exact.
//  * NP_ = round((4 - 40) * fes / maxFEs + 40) in double with round-half-even (:151: rint); int(0.2 * NP) in double (:68).
//  * np.random.choice(range(H), p=P) (:54, :56) is cumsum(P), divided by its last entry, then searchsorted(u, side='right').
//  * np.sum over 5 entries is sequential, over 15 numpy's pairwise_sum (mbx_npsum.hpp) (:132-147).
// One deliberate departure: when sum(S_cr) == 0 the reference grows H_cr (:132-134) and dies of IndexError within five generations, nf_cr
// having 5 entries.  Here H_cr stays 5 and P_cr goes back to uniform.  No fixture reaches that branch.
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off).
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"

namespace mbx {

constexpr double kShC1 = 1.49445, kShLb = -5., kShUb = 5., kShVmax = 1.;
constexpr int kShHcr = MBX_SAHL_HCR, kShHls = MBX_SAHL_HLS, kShNsel = MBX_SAHL_NSEL;

// M_cr (:12) without an indexed table (a dynamic index into a local array is scratch memory)
__device__ __forceinline__ double sh_mcr(int k)
{
    return k == 0 ? 0.0001 : k == 1 ? 0.0005 : k == 2 ? 0.001 : k == 3 ? 0.005 : k == 4 ? 0.01 : k == 5 ? 0.05 : k == 6 ? 0.1 : 0.5;
}

// The LDS layout (ShLds, kShNP, sh_lds_doubles, sh_carve) lives in mbx_lds.hpp.

// searchsorted(cdf, u, side='right') over H entries, never past the last one (a tape is caller data)
__device__ __forceinline__ int sh_search(const double* cdf, int H, double u)
{
    int n = 0;
    for (int k = 0; k < H; ++k) n += cdf[k] <= u ? 1 : 0;
    return min(n, H - 1);
}

__device__ __forceinline__ int sh_clamp_row(double v) { return min(max((int)v, 0), kShNP - 1); }

// ------------------------------------------------------------------------------------------------ reset (run_episode :22-47)
__global__ __launch_bounds__(kThreads) void k_sahlpso_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    constexpr int NP = kShNP;
    const int D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const ShLds L = sh_carve(smem, NP, D, false);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_SAHL_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    stage_problem(P, L.eval(L.XR, L.NC));
    for (int e = tid; e < NE; e += kThreads) {
        double up, uv;
        if (tape) { uv = tape[MBX_SAHL_TAPE_VEL(NP, D) + e]; up = tape[MBX_SAHL_TAPE_POS(NP, D) + e]; }
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); up = u53(w.x, w.y); uv = u53(w.z, w.w); }
        const double x = kShLb + (kShUb - kShLb) * up;               // :24
        L.XR[e] = x;
        S[MBX_SAHL_ST_X(NP, D) + e] = x; S[MBX_SAHL_ST_PBPOS(NP, D) + e] = x;
        S[MBX_SAHL_ST_V(NP, D) + e] = -kShVmax + (2 * kShVmax) * uv; // :23
    }
    if (tid < NP && !tape) L.KEY[tid] = rng.draw((uint32_t)tid, MBX_SITE_SH_PERM).x;
    __syncthreads();
    population_costs(P, L.eval(L.XR, L.NC), NP, rng, tape ? tape + MBX_SAHL_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_SH_NOISE_A, MBX_SITE_SH_NOISE_B);
    if (tid < NP) {
        const double c = L.NC[tid];
        int r = 0;
        for (int j = 0; j < NP; ++j) { const double o = L.NC[j]; r += (o < c || (o == c && j < tid)) ? 1 : 0; }
        S[MBX_SAHL_ST_RANK(NP, D) + r] = tid;                        // np.argsort(pBest_cost), once (:68, :153)
        S[MBX_SAHL_ST_FX(NP, D) + tid] = c; S[MBX_SAHL_ST_PBCOST0(NP, D) + tid] = c; S[MBX_SAHL_ST_W(NP, D) + tid] = 0.9;
        S[MBX_SAHL_ST_MOVE_I(NP, D) + tid] = 0.; S[MBX_SAHL_ST_MOVE_CR(NP, D) + tid] = 0.; S[MBX_SAHL_ST_MOVE_LS(NP, D) + tid] = 0.;
        S[MBX_SAHL_ST_MOVE_SUCC(NP, D) + tid] = 0.; S[MBX_SAHL_ST_MOVE_CAUCHY(NP, D) + tid] = 0.;
        // np.random.permutation(remain_index)[:8] (:47)
        if (tape) { if (tid < kShNsel) S[MBX_SAHL_ST_SEL(NP, D) + tid] = sh_clamp_row(tape[MBX_SAHL_TAPE_SEL(NP, D) + tid]); }
        else {
            const uint32_t k = L.KEY[tid];
            int kr = 0;
            for (int j = 0; j < NP; ++j) { const uint32_t o = L.KEY[j]; kr += (o < k || (o == k && j < tid)) ? 1 : 0; }
            if (kr < kShNsel) S[MBX_SAHL_ST_SEL(NP, D) + kr] = tid;
        }
    }
    if (tid < 8) {
        S[MBX_SAHL_ST_PCR(NP, D) + tid] = tid < kShHcr ? 1. / kShHcr : 0.;                // np.ones(H) / H (:40, :43)
        S[MBX_SAHL_ST_NFCR(NP, D) + tid] = 0.; S[MBX_SAHL_ST_NSCR(NP, D) + tid] = 0.;
    }
    if (tid < 16) {
        S[MBX_SAHL_ST_PLS(NP, D) + tid] = tid < kShHls ? 1. / kShHls : 0.;
        S[MBX_SAHL_ST_NFLS(NP, D) + tid] = 0.; S[MBX_SAHL_ST_NSLS(NP, D) + tid] = 0.;
    }
    double gb; int g0;
    block_argmin(L.NC, NP, L.RED, gb, g0);                           // :34-35, first minimum
    if (tid == 0) {
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = g0; sc[MBX_SC_SAHL_NP] = NP; sc[MBX_SC_SAHL_GROW] = g0;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gBest_cost] (:38)
        if (state_out) state_out[b] = (double)NP / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ one pass of `for i in remain_index` (:50-124) and the generation's end (:126-155)
__global__ __launch_bounds__(kThreads) void k_sahlpso_generation(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                                 uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    constexpr int NP0 = kShNP;
    const int D = bp.D, NE = NP0 * D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_SAHL_ST_SCALARS(NP0, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const ShLds L = sh_carve(smem, 1, D, true);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int64_t REC = MBX_SAHL_REC(D);
    const int step = (int)sc[MBX_SC_GEN] + 1;                        // the reference's G of this pass
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(int)sc[MBX_SC_EPISODE]};
    // every scalar is read here, before the first barrier, by every thread; thread 0 writes them back after the last one
    int fes = (int)sc[MBX_SC_FES], log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
    int NP = min(max((int)sc[MBX_SC_SAHL_NP], MBX_SAHL_NP_MIN), NP0), g = sh_clamp_row(sc[MBX_SC_SAHL_GROW]);   // (clamped: mbx_debug_write_state is caller data)
    double gbest = sc[MBX_SC_GBEST];
    const bool stop_rule = !isnan(P.optimum) && bp.early_stop;
    double* cost = sc + MBX_NSCALAR;

    stage_problem(P, L.eval(L.XR, L.NC));
    for (int e = tid; e < NE; e += kThreads) {
        L.X[e] = S[MBX_SAHL_ST_X(NP0, D) + e]; L.V[e] = S[MBX_SAHL_ST_V(NP0, D) + e]; L.PB[e] = S[MBX_SAHL_ST_PBPOS(NP0, D) + e];
    }
    if (tid < NP0) {
        L.FX[tid] = S[MBX_SAHL_ST_FX(NP0, D) + tid]; L.PC0[tid] = S[MBX_SAHL_ST_PBCOST0(NP0, D) + tid]; L.W[tid] = S[MBX_SAHL_ST_W(NP0, D) + tid];
        L.RANK[tid] = sh_clamp_row(S[MBX_SAHL_ST_RANK(NP0, D) + tid]);
        int f = 0;
        for (int j = 0; j < kShNsel; ++j) f |= (int)S[MBX_SAHL_ST_SEL(NP0, D) + j] == tid ? 1 : 0;   // `i in selected_indiv_index` (:59, :75)
        L.SELF[tid] = f;
        L.MI[tid] = 0; L.MCR[tid] = 0; L.MLS[tid] = 0; L.MSUC[tid] = 0; L.MCAU[tid] = 0.;
    }
    if (tid < 16) {
        L.PCR[tid] = tid < 8 ? S[MBX_SAHL_ST_PCR(NP0, D) + tid] : 0.; L.NFCR[tid] = tid < 8 ? S[MBX_SAHL_ST_NFCR(NP0, D) + tid] : 0.;
        L.NSCR[tid] = tid < 8 ? S[MBX_SAHL_ST_NSCR(NP0, D) + tid] : 0.;
        L.PLS[tid] = S[MBX_SAHL_ST_PLS(NP0, D) + tid]; L.NFLS[tid] = S[MBX_SAHL_ST_NFLS(NP0, D) + tid]; L.NSLS[tid] = S[MBX_SAHL_ST_NSLS(NP0, D) + tid];
    }
    if (tid == 0) {                                                  // the two cumulative distributions of this pass (:54, :56): cumsum, then / its last entry
        double c = 0.;
        for (int k = 0; k < kShHcr; ++k) { c = k ? c + S[MBX_SAHL_ST_PCR(NP0, D) + k] : S[MBX_SAHL_ST_PCR(NP0, D)]; L.CDFCR[k] = c; }
        for (int k = 0; k < kShHcr; ++k) L.CDFCR[k] = L.CDFCR[k] / c;
        for (int k = 0; k < kShHls; ++k) { c = k ? c + S[MBX_SAHL_ST_PLS(NP0, D) + k] : S[MBX_SAHL_ST_PLS(NP0, D)]; L.CDFLS[k] = c; }
        for (int k = 0; k < kShHls; ++k) L.CDFLS[k] = L.CDFLS[k] / c;
    }
    __syncthreads();

    const bool adapt = (step % MBX_SAHL_LP) != 0 || step == 1;        // :53
    const int nbp = max(1, (int)(0.2 * (double)NP));                  // :68
    bool done = false;
    int k = 0;
    for (; k < NP && !done; ++k) {
        const int i = NP == NP0 ? k : L.RANK[k];                      // remain_index[k]
        const double* rec = tape ? tape + k * REC : nullptr;
        int cri = 0, lsi = 0;
        if (tid < 64) {                                               // ---- the move (:51-86), wave 0
            double cr = 0.;
            if (adapt) {
                double ucr, uls;
                if (rec) { ucr = rec[MBX_SAHL_REC_UCR]; uls = rec[MBX_SAHL_REC_ULS]; }
                else { const U4 w = rng.draw((uint32_t)k, MBX_SITE_SH_CHOICE); ucr = u53(w.x, w.y); uls = u53(w.z, w.w); }
                cri = sh_search(L.CDFCR, kShHcr, ucr); lsi = sh_search(L.CDFLS, kShHls, uls);
                cr = sh_mcr(cri);
            }
            const bool sel = L.SELF[i] != 0;
            int o;
            if (rec) {
                if (sel) { const int m = sh_clamp_row(rec[MBX_SAHL_REC_M]), n = sh_clamp_row(rec[MBX_SAHL_REC_N]); o = L.FX[m] < L.FX[n] ? m : n; }
                else o = sh_clamp_row(rec[MBX_SAHL_REC_PICK]);
            } else {
                const U4 w = rng.draw((uint32_t)k, MBX_SITE_SH_PICK);
                if (sel) {
                    const int jm = (int)__umulhi(w.x, (uint32_t)NP), jn = (int)__umulhi(w.y, (uint32_t)NP);
                    const int m = NP == NP0 ? jm : L.RANK[jm], n = NP == NP0 ? jn : L.RANK[jn];
                    o = L.FX[m] < L.FX[n] ? m : n;                    // the CURRENT f_X (:62)
                } else o = L.RANK[(int)__umulhi(w.z, (uint32_t)nbp)];
            }
            if (tid < D) {
                const int d = tid, e = i * D + d;
                double cu, r1 = 0., rv;
                if (rec) { cu = rec[MBX_SAHL_REC_CROSS(D) + d]; if (!sel) r1 = rec[MBX_SAHL_REC_RND1(D) + d]; rv = rec[MBX_SAHL_REC_VEL(D) + d]; }
                else {
                    const U4 w = rng.draw((uint32_t)(64 * k + d), MBX_SITE_SH_ELEM), v = rng.draw((uint32_t)(64 * k + d), MBX_SITE_SH_VEL);
                    cu = u53(w.x, w.y); r1 = u53(w.z, w.w); rv = u53(v.x, v.y);
                }
                double pb = L.PB[e];
                if (cu < cr) { pb = L.PB[o * D + d]; L.PB[e] = pb; }  // e[mask] = o[mask]: into the row pBest[i] (:72-74)
                double ex = pb;
                if (!sel) ex = r1 * pb + (1 - r1) * L.X[g * D + d];    // gBest = the row X[g] as it is now (:77)
                const double x = L.X[e];
                double v = L.W[i] * L.V[e] + kShC1 * rv * (ex - x);    // :83
                v = fmin(fmax(v, -kShVmax), kShVmax);                  // :84
                const double nx = fmin(fmax(x + v, kShLb), kShUb);     // :86
                L.V[e] = v; L.X[e] = nx; L.XR[d] = nx;
            }
            if (tid == 0) { L.NFCR[cri] += 1.; L.NFLS[lsi] += 1.; L.MI[k] = i; L.MCR[k] = cri; L.MLS[k] = lsi; }   // :80-81
        }
        __syncthreads();                                              // the row goes to the evaluator
        {
            const RowPost post{&rng, rec ? rec + MBX_SAHL_REC_NOISE : nullptr, MBX_SITE_SH_NOISE_A, MBX_SITE_SH_NOISE_B, 1, rec ? 0 : k};
            eval_rows(P, L.eval(L.XR, L.NC), 1, &post);               // :88-91; its last barrier hands the cost to every thread
        }
        const double f = L.NC[0];
        const bool succ = f < L.PC0[i];                               // :93, against the INITIAL pbest cost
        if (succ && f < gbest) { gbest = f; g = i; }                  // :95-97
        if (tid < 64) {                                               // ---- the move's bookkeeping (:92-108), wave 0
            if (succ && tid < D) L.PB[i * D + tid] = L.X[i * D + tid]; // :94
            if (tid == 0) {
                L.FX[i] = f; L.MSUC[k] = succ ? 1 : 0;
                if (succ) { L.NSCR[cri] += 1.; L.NSLS[lsi] += 1.; }   // :99-100
                else {                                                // :102-107
                    double rnd2, ca;
                    if (rec) { rnd2 = rec[MBX_SAHL_REC_RND2]; ca = rec[MBX_SAHL_REC_CAUCHY]; }
                    else { const U4 w = rng.draw((uint32_t)k, MBX_SITE_SH_FAIL); rnd2 = u53(w.x, w.y); ca = tan(3.141592653589793 * (u53(w.z, w.w) - 0.5)); }
                    const double wn = (rnd2 < 0.5 ? 0.7 : 0.3) + 0.1 * ca;
                    L.W[i] = fmin(fmax(wn, 0.2), 0.9);
                    L.MCAU[k] = ca;
                }
            }
            wave_lds_fence();                                           // the next move of this wave reads f_X, w and the pBest row
        }
        fes += 1;                                                     // :92
        if ((double)fes >= (double)log_index * bp.log_interval) {    // :110-112, once
            log_index += 1;
            if (cost_len <= bp.n_logpoint) { if (tid == 0) curve_put(cost, bp.n_logpoint, cost_len, gbest); cost_len += 1; }
        }
        done = fes >= bp.max_fes || (stop_rule && gbest <= 1e-8);     // :114-117
    }
    if (tid == 0) {
        if (done) {                                                   // :119-124
            if (cost_len >= bp.n_logpoint + 1) curve_put(cost, bp.n_logpoint, cost_len - 1, gbest);
            else curve_put(cost, bp.n_logpoint, cost_len++, gbest);
        } else {
            if (step % MBX_SAHL_LP == 0) {                            // :126-147
                double sum = 0.;
                for (int j = 0; j < kShHcr; ++j) { const double nf = L.NFCR[j]; const double v = nf != 0. ? L.NSCR[j] / nf : 0.; L.RED[j] = v; sum += v; }
                for (int j = 0; j < kShHcr; ++j) L.PCR[j] = sum == 0. ? 1. / kShHcr : L.RED[j] / sum;      // (sum == 0: the departure, see the header)
                for (int j = 0; j < kShHls; ++j) { const double nf = L.NFLS[j]; L.RED[j] = nf != 0. ? L.NSLS[j] / nf : 0.; }
                static_assert(kShHls <= 128, "np_sum_block is numpy's order for n <= 128");
                const double sl = np_sum_block([&](int j) { return L.RED[j]; }, kShHls);
                for (int j = 0; j < kShHls; ++j) L.PLS[j] = sl == 0. ? 1. / kShHls : L.RED[j] / sl;
            }
            const int np_new = (int)rint((double)((int64_t)(4 - NP0) * fes) / (double)bp.max_fes + (double)NP0);    // :151
            if (np_new < NP) NP = max(np_new, MBX_SAHL_NP_MIN);
        }
    }
    __syncthreads();
    // ---- the state block, once per launch
    for (int e = tid; e < NE; e += kThreads) {
        S[MBX_SAHL_ST_X(NP0, D) + e] = L.X[e]; S[MBX_SAHL_ST_V(NP0, D) + e] = L.V[e]; S[MBX_SAHL_ST_PBPOS(NP0, D) + e] = L.PB[e];
    }
    if (tid < NP0) {
        S[MBX_SAHL_ST_FX(NP0, D) + tid] = L.FX[tid]; S[MBX_SAHL_ST_W(NP0, D) + tid] = L.W[tid];
        S[MBX_SAHL_ST_MOVE_I(NP0, D) + tid] = L.MI[tid]; S[MBX_SAHL_ST_MOVE_CR(NP0, D) + tid] = L.MCR[tid]; S[MBX_SAHL_ST_MOVE_LS(NP0, D) + tid] = L.MLS[tid];
        S[MBX_SAHL_ST_MOVE_SUCC(NP0, D) + tid] = L.MSUC[tid]; S[MBX_SAHL_ST_MOVE_CAUCHY(NP0, D) + tid] = L.MCAU[tid];
    }
    if (tid < 8) { S[MBX_SAHL_ST_PCR(NP0, D) + tid] = L.PCR[tid]; S[MBX_SAHL_ST_NFCR(NP0, D) + tid] = L.NFCR[tid]; S[MBX_SAHL_ST_NSCR(NP0, D) + tid] = L.NSCR[tid]; }
    if (tid < 16) { S[MBX_SAHL_ST_PLS(NP0, D) + tid] = L.PLS[tid]; S[MBX_SAHL_ST_NFLS(NP0, D) + tid] = L.NFLS[tid]; S[MBX_SAHL_ST_NSLS(NP0, D) + tid] = L.NSLS[tid]; }
    if (tid == 0) {
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = step; sc[MBX_SC_GBEST_IDX] = g; sc[MBX_SC_SAHL_NP] = NP; sc[MBX_SC_SAHL_GROW] = g;
        sc[MBX_SC_SAHL_MOVES] = k;
        if (state_out) state_out[b] = (double)fes / bp.max_fes;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
