// mbx_madde.hpp — MadDE, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/madde.py:6-284).
//
// DE with three mutation strategies chosen per row with probabilities pm, a success-history memory MF / MCr of H = 10 D entries, an archive
// of replaced parents and a population that shrinks linearly from N0 = 2 D^2 rows to 4 (200 rows at D = 10, 3200 at D = 40).  One __update
// (:197-272) makes and evaluates one trial per live row, NP evaluations.
//
// No agent: mbx_reset is __init_population, every mbx_step (actions = NULL) one __update.  One workgroup of 256 threads per instance,
// dispatched through bp.order; state block and tape: include/mbx_layout.h §13.  The population does not fit the lanes: a thread owns a
// contiguous block of ceil(NP / 256) rows, so that the rank of a row inside its strategy group, or among the improved rows, is a workgroup
// prefix scan over per-thread counts plus a running count.  Population, archive, trial rows and the per-row vectors stay in the state block
// (HBM / L2); LDS holds the evaluator's chunk, the rank -> row lists of the three groups, and, after the evaluations, the archive's
// write arbitration, one compacted vector for the long sums and the (cost, row) pairs of the sort, which share the chunk's memory.
// Trials are evaluated in chunks of md_chunk(D) rows by the block-cooperative evaluator, with the noise draws of the whole update.
// The carve-up and the phases NL_SHADE_LBC and RL-HPSDE have too (chunked evaluation, sorted first population, ranks of the improved rows, archive
// write arbitration, the memory update's sums, replacement and row move) are in mbx_depop.hpp; this file holds MadDE's own draws, mutation,
// crossover, strategy credit and bookkeeping.
//
// Long sums (memory update :147-152, strategy credit :247): the operands are compacted in rank order into LDS and added in numpy's
// pairwise order for a contiguous vector (below 8 elements left to right from 0; up to 128 eight running accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder one by one; above that halves, the left one a multiple of 8 long), md_pairwise.
//
// Archive (:238-244): the parents of the improved rows enter one after another in the reference: append while the archive is short of NA
// rows, else overwrite a random row.  Here, with a = min(NA - rows, improved) appends, the improved row of rank k < a writes row rows + k,
// rank k >= a writes its drawn row, and of several writers of one row the highest rank wins (an atomic maximum in LDS), which is what the
// sequential loop leaves behind.
//
// Sort (:135-139, :258): the reference's argsort is introsort, whose order among equal costs depends on numpy's SIMD dispatch; the kernel
// orders by (cost, row before the sort), numpy's kind='stable' order, with a bitonic network over the pairs in LDS, and moves the rows by
// the permutation into the other population buffer.  It runs at the end of reset and of every update, so the __sort at the start of an
// update is the identity and does not run.
//
// Quirks of the reference kept on purpose:
//   1. the indices the mutations draw are local to the strategy group, but rb is a row of pbest / qbest: `rb == arange(n)` compares a
//      population row with a group rank, and r1 == rb likewise (:32-51, :99-119);
//   2. every rejection loop redraws 25 times at most and then keeps what it has: a one-row group keeps r1 == self; an empty group draws nothing;
//   3. r2 of the first two strategies ranges over the group and then the archive (:47, :77); the third ignores the archive;
//   4. F below 0 is reflected about its location once (2 loc - F, :164) and may stay negative; then min(1, F);
//   5. bounds are repaired by halving towards the bound, the lower one first (:217-218);
//   6. rows with rvs <= 0.01 cross with a random row of the best q share instead of their parent (:222-229); with a non-empty archive
//      that pool is the first int(q (NP + archive rows)) rows of population + archive and reaches into ARCHIVE rows once it exceeds NP;
//   7. the archive is filled against the NA of the update's start and cut to the new NA at its end (:257-261);
//   8. k advances only when some row improved; otherwise MF[k] = MCr[k] = 0.5 (:169-177); a weighted sum not above 1e-6 gives 0.5;
//   9. pm: the mean of an empty group is NaN, `sum > 0` is then false and pm falls back to 1/3 (:248-252); pm is set in __init__ only, so
//      mbx_reset leaves it alone (a new batch starts at 1/3);
//  10. NP = round-half-even(N0 + (4 - N0) FEs / MaxFEs) (:256), FEs overshoots MaxFEs by less than NP and the last NP can be 3;
//  11. gbest is a running minimum; at most one log point per update (:265); the early stop is tested once per update.
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off).
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate_guarded
#include "mbx_depop.hpp"    // the carve-up and the phases shared with NL_SHADE_LBC and RL-HPSDE

namespace mbx {

constexpr int kMdTries = 25;
constexpr double kMdP = 0.18, kMdPqbx = 0.01, kMdM0 = 0.2, kMdNmin = 4.;

// population size after `fes` evaluations (:256): N0 + ((4 - N0) fes) / max_fes, the product exact, rounded half to even
__host__ __device__ inline int md_np_at(int N0, double fes, double max_fes)
{
    const int n = (int)rint((double)N0 + ((kMdNmin - (double)N0) * fes) / max_fes);
    return n < 1 ? 1 : n > N0 ? N0 : n;
}

// ------------------------------------------------------------------------------------------------ reset (__init_population :179-195)
__global__ __launch_bounds__(kThreads) void k_madde_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = (int)MBX_MADDE_H(D);
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const MdLds L = md_carve(smem, N0, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_MADDE_ST_SCALARS(N0, D);
    double* gU = S + MBX_MADDE_ST_U(N0, D);
    double* gNC = S + MBX_MADDE_ST_NCOST(N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(CH, D, L.TC));
    // the rows are drawn chunk by chunk on their way into the evaluator
    auto draw = [&](int g) -> double {
        double u;
        if (tape) u = tape[MBX_MADDE_TAPE_POS(N0, D) + g];
        else { const U4 w = rng.draw((uint32_t)g, MBX_SITE_MD_CROSS); u = u53(w.x, w.y); }
        return gU[g] = u * (ub - lb) + lb;
    };
    md_eval_rows(P, L, N0, N0, D, draw, gNC, rng, tape ? tape + MBX_MADDE_TAPE_NOISE_INIT(N0, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    // sort by (cost, row) and move the rows into buffer 0
    md_init_sorted(L, gU, gNC, S + MBX_MADDE_ST_POP(N0, D), S + MBX_MADDE_ST_COST(N0, D), N0, D);
    for (int t = tid; t < N0; t += kThreads) {
        S[MBX_MADDE_ST_F(N0, D) + t] = 0.;
        S[MBX_MADDE_ST_CR(N0, D) + t] = 0.;
        S[MBX_MADDE_ST_Z(N0, D) + t] = 0.;
        S[MBX_MADDE_ST_C(N0, D) + t] = 0.;
    }
    for (int t = tid; t < H; t += kThreads) { S[MBX_MADDE_ST_MF(N0, D) + t] = kMdM0; S[MBX_MADDE_ST_MCR(N0, D) + t] = kMdM0; }
    if (tid == 0) {
        double* pm = S + MBX_MADDE_ST_PM(N0, D);
        if (pm[0] == 0. && pm[1] == 0. && pm[2] == 0.) pm[0] = pm[1] = pm[2] = 1. / 3.;       // a new batch
        const double gb = L.KEY[0];
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = N0; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_MD_NP] = N0; sc[MBX_SC_MD_ARC] = 0; sc[MBX_SC_MD_NA] = (double)MBX_MADDE_ARC(N0); sc[MBX_SC_MD_K] = 0; sc[MBX_SC_MD_LIVE] = 0;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = (double)N0 / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ generation (__update :197-272)
__global__ __launch_bounds__(kThreads) void k_madde_generation(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                               uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = (int)MBX_MADDE_H(D), A0 = (int)MBX_MADDE_ARC(N0);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_MADDE_ST_SCALARS(N0, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const MdLds L = md_carve(smem, N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int gen = (int)sc[MBX_SC_GEN] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)(int)sc[MBX_SC_EPISODE]};
    const double lb = P.lb, ub = P.ub, fes0 = sc[MBX_SC_FES], mf = (double)bp.max_fes, gbest0 = sc[MBX_SC_GBEST];
    // (clamped: the state block can be caller data, mbx_debug_write_state)
    const int NP = min(max((int)sc[MBX_SC_MD_NP], 1), N0), NA = min(max((int)sc[MBX_SC_MD_NA], 0), A0);
    const int narc = min(max((int)sc[MBX_SC_MD_ARC], 0), A0), k_mem = min(max((int)sc[MBX_SC_MD_K], 0), H - 1);
    const int live = sc[MBX_SC_MD_LIVE] != 0. ? 1 : 0;
    const int log_index0 = (int)sc[MBX_SC_LOG_INDEX], cost_len0 = (int)sc[MBX_SC_COST_LEN];
    const double* pop = S + MBX_MADDE_ST_POP(N0, D) + (int64_t)live * N0 * D;
    double* npop = S + MBX_MADDE_ST_POP(N0, D) + (int64_t)(1 - live) * N0 * D;
    double* gC = S + MBX_MADDE_ST_COST(N0, D);
    double* arc = S + MBX_MADDE_ST_ARC(N0, D);
    double* gMF = S + MBX_MADDE_ST_MF(N0, D);
    double* gMCr = S + MBX_MADDE_ST_MCR(N0, D);
    double* gU = S + MBX_MADDE_ST_U(N0, D);
    double* gNC = S + MBX_MADDE_ST_NCOST(N0, D);
    double* gF = S + MBX_MADDE_ST_F(N0, D);
    double* gCr = S + MBX_MADDE_ST_CR(N0, D);
    double* gpm = S + MBX_MADDE_ST_PM(N0, D);
    const double q = 2 * kMdP - kMdP * fes0 / mf, Fa = 0.5 + 0.5 * fes0 / mf;
    const int NBp = max((int)(kMdP * NP), 2), NBq = max((int)(q * NP), 2);
    const int pool = narc > 0 ? max((int)(q * (NP + narc)), 2) : NBq;
    const int per = (NP + kThreads - 1) / kThreads, row0 = min(tid * per, NP), row1 = min(row0 + per, NP);
    stage_problem(P, L.eval(CH, D, L.TC));
    // ---- F / Cr (:155-165) and the strategy of every row (:203)
    double cdf0 = gpm[0], cdf1 = cdf0 + gpm[1], cdf2 = cdf1 + gpm[2];
    cdf0 /= cdf2; cdf1 /= cdf2; cdf2 /= cdf2;
    int cnt[3] = {0, 0, 0}, base[3], tot[3];
    for (int i = row0; i < row1; ++i) {
        int ind;
        double z, c, um;
        if (tape) {
            ind = min(max((int)tape[MBX_MADDE_TAPE_MEM(N0, D) + i], 0), H - 1);
            z = tape[MBX_MADDE_TAPE_Z(N0, D) + i]; c = tape[MBX_MADDE_TAPE_C(N0, D) + i]; um = tape[MBX_MADDE_TAPE_CHOICE(N0, D) + i];
        } else {
            ind = (int)__umulhi(rng.draw((uint32_t)i, MBX_SITE_MD_PAR).x, (uint32_t)H);
            U4 w = rng.draw((uint32_t)i, MBX_SITE_MD_NORM);
            double z1;
            box_muller(u53(w.x, w.y), u53(w.z, w.w), z, z1);
            w = rng.draw((uint32_t)i, MBX_SITE_MD_CAUCHY);
            c = tan(3.141592653589793 * (u53(w.x, w.y) - 0.5)); um = u53(w.z, w.w);
        }
        const double Cr = fmin(1., fmax(0., gMCr[ind] + 0.1 * z)), loc = gMF[ind];
        double F = c * 0.1 + loc;
        if (F < 0.) F = 2 * loc - F;
        F = fmin(1., F);
        const int mu = min((um >= cdf0) + (um >= cdf1) + (um >= cdf2), 2);
        gF[i] = F; gCr[i] = Cr; L.MU[i] = (uint8_t)mu;
        S[MBX_MADDE_ST_Z(N0, D) + i] = z; S[MBX_MADDE_ST_C(N0, D) + i] = c;
        cnt[mu] += 1;
    }
    md_scan3(L.CNT, cnt, base, tot);
    const int off[3] = {0, tot[0], tot[0] + tot[1]};
    {
        int run[3] = {base[0], base[1], base[2]};
        for (int i = row0; i < row1; ++i) { const int g = L.MU[i]; L.LIST[off[g] + run[g]++] = i; }
    }
    __syncthreads();
    // ---- mutation (:25-126), bound repair (:217-218), crossover (:219-232): trial rows into the state block
    {
        int run[3] = {base[0], base[1], base[2]};
        for (int i = row0; i < row1; ++i) {
            const int g = L.MU[i], n = tot[g], j = run[g]++, lo = off[g];
            const int nb = g == 0 ? NBp : NBq, n2 = g == 2 ? n : n + narc;
            int rb = -1, r1, r2, jr, pick;
            double rvs;
            if (tape) {
                if (g != 1) rb = min(max((int)tape[MBX_MADDE_TAPE_RB(N0, D) + i], 0), nb - 1);
                r1 = min(max((int)tape[MBX_MADDE_TAPE_R1(N0, D) + i], 0), n - 1);
                r2 = min(max((int)tape[MBX_MADDE_TAPE_R2(N0, D) + i], 0), n2 - 1);
                jr = min(max((int)tape[MBX_MADDE_TAPE_JRAND(N0, D) + i], 0), D - 1);
                pick = (int)tape[MBX_MADDE_TAPE_QPICK(N0, D) + i];
                rvs = tape[MBX_MADDE_TAPE_RVS(N0, D) + i];
            } else {
                // the rejection loops: one draw, then at most 25 redraws while the test rejects
                const U4 w = rng.draw((uint32_t)(i * 32), MBX_SITE_MD_IDX);
                if (g != 1) {
                    rb = (int)__umulhi(w.x, (uint32_t)nb);
                    for (int a = 1; a <= kMdTries && rb == j; ++a) rb = (int)__umulhi(rng.draw((uint32_t)(i * 32 + a), MBX_SITE_MD_IDX).x, (uint32_t)nb);
                }
                r1 = (int)__umulhi(w.y, (uint32_t)n);
                for (int a = 1; a <= kMdTries && (r1 == rb || r1 == j); ++a) r1 = (int)__umulhi(rng.draw((uint32_t)(i * 32 + a), MBX_SITE_MD_IDX).y, (uint32_t)n);
                r2 = (int)__umulhi(w.z, (uint32_t)n2);
                for (int a = 1; a <= kMdTries && (r2 == rb || r2 == j || r2 == r1); ++a)
                    r2 = (int)__umulhi(rng.draw((uint32_t)(i * 32 + a), MBX_SITE_MD_IDX).z, (uint32_t)n2);
                const U4 v = rng.draw((uint32_t)i, MBX_SITE_MD_PAR);
                pick = (int)__umulhi(v.y, (uint32_t)pool); jr = (int)__umulhi(v.z, (uint32_t)D); rvs = u32d(v.w);
            }
            pick = min(max(pick, 0), min(pool, NP + narc) - 1);
            const double F = gF[i], Cr = gCr[i], FFa = F * Fa;
            const double* x = pop + (int64_t)i * D;
            const double* xb = pop + (int64_t)max(rb, 0) * D;
            const double* x1 = pop + (int64_t)L.LIST[lo + r1] * D;
            const double* x2 = r2 < n ? pop + (int64_t)L.LIST[lo + r2] * D : arc + (int64_t)(r2 - n) * D;
            const double* par = rvs <= kMdPqbx ? (pick < NP ? pop + (int64_t)pick * D : arc + (int64_t)(pick - NP) * D) : x;
            for (int d = 0; d < D; ++d) {
                double cu;
                if (tape) cu = tape[MBX_MADDE_TAPE_CROSS(N0, D) + (int64_t)i * D + d];
                else { const U4 w = rng.draw((uint32_t)(i * D + d), MBX_SITE_MD_CROSS); cu = u53(w.x, w.y); }
                double v;
                if (g == 0) v = x[d] + F * (xb[d] - x[d]) + F * (x1[d] - x2[d]);
                else if (g == 1) v = x[d] + F * (x1[d] - x2[d]);
                else v = F * x1[d] + FFa * (xb[d] - x2[d]);
                if (v < lb) v = (v + lb) / 2;
                if (v > ub) v = (v + ub) / 2;
                gU[(int64_t)i * D + d] = (cu < Cr || d == jr) ? v : par[d];
            }
        }
    }
    __syncthreads();
    // ---- evaluation of the trials in row chunks
    md_eval_rows(P, L, NP, N0, D, [&](int e) { return gU[e]; }, gNC, rng, tape ? tape + MBX_MADDE_TAPE_NOISE(N0, D) : nullptr, MBX_SITE_MD_NOISE_A,
                 MBX_SITE_MD_NOISE_B);
    // ---- selection (:238): ranks of the improved rows
    int obase, n_opt;
    md_rank_improved(L, gC, gNC, row0, row1, obase, n_opt);
    const int n_app = min(max(NA - narc, 0), n_opt), alen = narc + n_app;
    // ---- archive (:141-145, :239-240)
#ifndef MBX_ABLATE_MD_ARC
    if (alen > 0) {
        auto target = [&](int k) -> int {
            if (tape) return min(max((int)tape[MBX_MADDE_TAPE_ARC(N0, D) + k], 0), alen - 1);
            return (int)__umulhi(rng.draw((uint32_t)k, MBX_SITE_MD_ARC).x, (uint32_t)alen);
        };
        // the parent of an improved row is the row itself: a thread walks its rows with a running rank
        md_archive_write(L, arc, pop, D, narc, n_app, alen, target, [&](auto put) {
            int k = obase;
            for (int i = row0; i < row1; ++i) if (gNC[i] < gC[i]) put(k++, i);
        });
        __syncthreads();
    }
#endif
    // ---- memory (:147-177): weighted Lehmer means over the improved rows, compacted in rank order, numpy's pairwise sums
    double newMF = 0.5, newMCr = 0.5;
#ifndef MBX_ABLATE_MD_SUMS
    if (n_opt > 0) {
        // pass 0: df;  1: w SF;  2: w SF^2;  3: w SCr;  4: w SCr^2
        double sums[5];
        md_weighted_sums(L, gC, gNC, row0, row1, obase, n_opt, [](double c, double nc) { return fmax(0., c - nc); },
                         [&](int pass, double w, int i) { const double s = pass <= 2 ? gF[i] : gCr[i]; return (pass & 1) ? w * s : w * (s * s); }, sums);
        newMF = sums[1] > 0.000001 ? sums[2] / sums[1] : 0.5;
        newMCr = sums[3] > 0.000001 ? sums[4] / sums[3] : 0.5;
    }
#endif
    // ---- strategy credit (:245-252): mean of df / cost over each group
    double cs[3];
    for (int g = 0; g < 3; ++g) {
        int j = base[g];
        for (int i = row0; i < row1; ++i)
            if (L.MU[i] == g) { const double c = gC[i]; L.VEC[j++] = fmax(0., c - gNC[i]) / c; }
        __syncthreads();
#ifndef MBX_ABLATE_MD_SUMS
        if (tid == 0) L.RED[0] = md_pairwise(L.VEC, tot[g]) / (double)tot[g];
#else
        if (tid == 0) L.RED[0] = 1.;
#endif
        __syncthreads();
        cs[g] = L.RED[0];
        __syncthreads();
    }
    double pm0 = 1. / 3., pm1 = 1. / 3., pm2 = 1. / 3.;
    {
        const double s = cs[0] + cs[1] + cs[2];
        if (s > 0.) {
            pm0 = fmax(0.1, fmin(0.9, cs[0] / s)); pm1 = fmax(0.1, fmin(0.9, cs[1] / s)); pm2 = fmax(0.1, fmin(0.9, cs[2] / s));
            const double t = pm0 + pm1 + pm2;
            pm0 /= t; pm1 /= t; pm2 /= t;
        }
    }
    // ---- replacement, LPSR, sort (:254-261): rows into the other buffer in (cost, row) order
    const double fes = fes0 + NP;
    const int NPn = min(md_np_at(N0, fes, mf), NP), NAn = (int)(2.3 * NPn);
    md_replace_sorted(L, gC, gNC, gU, pop, npop, NP, NPn, D);
    // ---- bookkeeping (:263-272)
    if (tid == 0) {
        const double best = L.KEY[0];
        const double gbest = best < gbest0 ? best : gbest0;
        gMF[k_mem] = newMF; gMCr[k_mem] = newMCr;
        gpm[0] = pm0; gpm[1] = pm1; gpm[2] = pm2;
        int log_index = log_index0, cost_len = cost_len0;
        const bool done = log_and_terminate_guarded(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = gen; sc[MBX_SC_GBEST_IDX] = 0;
        sc[MBX_SC_MD_NP] = NPn; sc[MBX_SC_MD_ARC] = min(alen, NAn); sc[MBX_SC_MD_NA] = NAn;
        sc[MBX_SC_MD_K] = n_opt > 0 ? (k_mem + 1) % H : k_mem; sc[MBX_SC_MD_LIVE] = 1 - live;
        if (state_out) state_out[b] = fes / mf;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
