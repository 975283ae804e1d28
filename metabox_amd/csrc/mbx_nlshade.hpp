// mbx_nlshade.hpp — NL_SHADE_LBC, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/nl_shade_lbc.py:11-285).
//
// SHADE-style DE: current-to-pbest mutation with a rank-weighted r2, a success-history memory MF / MCr of H = 20 D entries, an archive of replaced
// parents, a binomial and an exponential crossover side by side, and a population that shrinks non-linearly from N0 = 23 D rows to 4 (230 rows at
// D = 10, 920 at D = 40).  One __update (:163-273) makes and evaluates one trial per live row, NP evaluations.
//
// No agent: mbx_reset is __init_population, every mbx_step (actions = NULL) one __update, mbx_nlshade_run n of them in one launch (the population
// collapses early: more than half of an episode is updates of a handful of rows, where one launch per update is all launch latency).  Step and run
// are one device body (nl_updates).  One workgroup of 256 threads per instance, dispatched through bp.order; state block and tape:
// include/mbx_layout.h §20.  A thread owns a contiguous block of ceil(NP / 256) rows.  Population, archive, trial rows and the memory stay in the
// state block; LDS is the carve-up shared with MadDE (md_carve): the evaluator's chunk, which between evaluations holds the sort keys (Cr, then
// (cost, row)), the cdf of the r2 choice, the archive's write arbitration and the compacted vector of the long sums.  The carve-up, the sort, the
// pairwise sums, the scan and the phases MadDE and RL-HPSDE have too (the reset's chunked evaluation and sorted first population, the archive's
// write arbitration, replacement and row move) are in mbx_depop.hpp; this file holds the algorithm's own draws, mutation, crossovers, memory
// update and bookkeeping, and the update's evaluation loop and ranking, which measured slower through the shared functions.
//
// The reading of the reference, kept on purpose:
//   1. the sort is by (cost, row), numpy's kind='stable' order (the reference's introsort is not reproducible among equal costs); it runs at the end
//      of reset and of every update, so the __sort at the start of an update is the identity and does not run;
//   2. draw order of an update (the Philox route has its own sites, the tape route is fed in this order by the tests): ind_r, the normals of Cr, the
//      Cauchy variates of F, pbs (+ ONE redraw round over [0, NP) for pbs == self), r1 (<= 25 rounds; excludes self and pbs), rvs, the r2 choice
//      (<= 25 rounds; excludes self, pbs, r1), archive indices, jrand, rand(NP, D), L, rvs(NP, D), rand(NP), the noise of the evaluation, one randint
//      per archive overwrite; every rejection loop redraws at most 25 times and keeps what it has;
//   3. Cr = clip(N(MCr[ind], 0.1), 0, 1) is SORTED ascending by value and handed to the rows in cost order (:174); F is not sorted; SCr of the memory
//      update is taken from the sorted Cr;
//   4. F below 0 is reflected once (2 loc - F, :120) and may stay negative; then min(1, F), numpy's minimum (a NaN stays a NaN);
//   5. pb_upper = int(max(2, NP pb)); pb = 0.2 + 0.1 FEs / MaxFEs is set at the end of an update;
//   6. r2 of the population rows is np.random.choice(NP, p = pr), pr = exp(-(i + 1) / NP) / sum: searchsorted(cumsum(pr) / cumsum[-1], u, 'right').
//      The kernel builds the cdf itself (exp per entry, numpy's pairwise sum, a sequential cumsum); the device's exp is not numpy's to the bit, so the
//      fixtures keep only cases whose u lie 1e-9 away from both neighbouring cdf entries;
//   7. pa is reset to 0.5 at the start of every update (:168), so __update_Pa has no effect: pa is NOT carried.  Rows with rvs < 0.5 take x2 from the
//      archive UNLESS the archive holds fewer than 25 rows; then every row uses the population choice.  Archive index: randint(min(rows, NA));
//   8. mutant x + F (xpb - x) + F (x1 - x2) in that expression order; both crossovers are computed for every row, rand(NP) > 0.5 picks the
//      exponential one.  The binomial one uses Crb, not Cr: 0 until FEs + NP > MaxFEs // 2, then the last min(NP, FEs + NP - MaxFEs // 2) rows get
//      2 ((FEs + row) / MaxFEs - 0.5); jrand is always taken.  The exponential one takes the mutant on columns [L, R), R the first column > L whose
//      rvs > Cr (strict), else D: no wrap-around, column L always the mutant's.  Bounds: (u + lb) / 2 below, then (u + ub) / 2 above;
//   9. selection is strict (cost_new < cost_old).  __update_archive(i) is called with the LOOP COUNTER (:244-245): with n improved rows the parents
//      that enter the archive are population rows 0 .. n - 1, the n best, not the improved rows.  Append while the archive is short of NA, then
//      overwrite a randint(rows) row; decided in parallel as MadDE does, the highest rank wins a row;
//  10. df = (old - new) / (old + 1e-9), not clamped; gbest = min(gbest, min(trial costs)) with numpy's min (a NaN trial cost leaves gbest alone);
//  11. NLPSR (:135-147): N = round-half-even(Nmax + (4 - Nmax) (FEs/MaxFEs)^(1 - FEs/MaxFEs)) is a function of (dim, max_fes) alone: the host builds
//      the table (bp.pci) and the kernel indexes it by its update counter, never calling pow for it.  NP only ever shrinks.  A = max(N, 4) cuts the
//      archive and sets NA only when A < archive rows;
//  12. memory (:83-109), with improved rows: MF[k] = sum(w s^pg) / sum(w s^(pg - 1.5)), w = df / sum(df), pg = (MaxFEs - FEs)(p_ini - 1.5) / MaxFEs
//      + 1.5 with p_ini = 3.5 (F) / 1.0 (Cr) and FEs AFTER this update's increment; k advances modulo H.  The sums run in numpy's pairwise order over
//      the operands compacted in rank order.  `sum(df) > 0` false gives 0.5 / 0.9 (k still advances).  A sorted Cr of exactly 0 meets a negative
//      exponent: inf in the denominator, MCr[k] = 0.  Without improved rows MF[k] = 0.5, MCr[k] = 0.9 and k stays.  The device's pow is not libm's
//      to the bit: MF[k] / MCr[k] are the one place the tests compare within a bound;
//  13. at most one log point per update, the early stop (gbest <= 1e-8) tested once per update; the final entry follows MadDE's rule;
//  14. pb (0.4 from __init__) and NA are NOT reset by __init_population: mbx_reset leaves carry[] alone (a new batch starts at 0.4 / N0).
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off).
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate_guarded
#include "mbx_depop.hpp"    // the carve-up and the phases shared with MadDE and RL-HPSDE

namespace mbx {

constexpr int kNlTries = 25, kNlArcMin = 25, kNlNmin = 4;

// searchsorted(cdf, u, side='right') over cdf[0, n), clamped to a row
__device__ __forceinline__ int nl_choice(const double* cdf, int n, double u)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (u < cdf[mid]) hi = mid; else lo = mid + 1; }
    return min(lo, n - 1);
}

// np.min over two runs of costs, a standing before b: NaN if either is, else the first-seen minimum (which decides the sign of a zero).  One step of
// `m = INFINITY; for v: if (isnan(v) || isnan(m)) m = NAN; else if (v < m) m = v;` is m = nl_min_seen(m, v).
__device__ __forceinline__ double nl_min_seen(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : (b < a ? b : a); }
static_assert(kThreads == 4 * 64, "the update folds the minimum over four waves of 64 lanes");

// ------------------------------------------------------------------------------------------------ reset (__init_population :149-160)
__global__ __launch_bounds__(kThreads) void k_nlshade_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = (int)MBX_NLSHADE_H(D);
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const MdLds L = md_carve(smem, N0, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_NLSHADE_ST_SCALARS(N0, D);
    double* gU = S + MBX_NLSHADE_ST_U(N0, D);
    double* gNC = S + MBX_NLSHADE_ST_NCOST(N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(CH, D, L.TC));
    // the rows are drawn chunk by chunk on their way into the evaluator
    auto draw = [&](int g) -> double {
        double u;
        if (tape) u = tape[MBX_NLSHADE_TAPE_POS(N0, D) + g];
        else { const U4 w = rng.draw((uint32_t)g, MBX_SITE_NL_CROSS); u = u53(w.x, w.y); }
        return gU[g] = u * (ub - lb) + lb;
    };
    md_eval_rows(P, L, N0, N0, D, draw, gNC, rng, tape ? tape + MBX_NLSHADE_TAPE_NOISE_INIT(N0, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    // sort by (cost, row) and move the rows into buffer 0
    md_init_sorted(L, gU, gNC, S + MBX_NLSHADE_ST_POP(N0, D), S + MBX_NLSHADE_ST_COST(N0, D), N0, D);
    for (int t = tid; t < N0; t += kThreads) {
        S[MBX_NLSHADE_ST_F(N0, D) + t] = 0.;
        S[MBX_NLSHADE_ST_CR(N0, D) + t] = 0.;
        S[MBX_NLSHADE_ST_Z(N0, D) + t] = 0.;
        S[MBX_NLSHADE_ST_C(N0, D) + t] = 0.;
        S[MBX_NLSHADE_ST_U2(N0, D) + t] = 0.;
        for (int c = 0; c < 4; ++c) S[MBX_NLSHADE_ST_IDX(N0, D) + 4 * t + c] = 0.;
    }
    for (int t = tid; t < H; t += kThreads) { S[MBX_NLSHADE_ST_MF(N0, D) + t] = 0.5; S[MBX_NLSHADE_ST_MCR(N0, D) + t] = 0.9; }
    if (tid == 0) {
        double* carry = S + MBX_NLSHADE_ST_CARRY(N0, D);
        if (carry[0] == 0.) { carry[0] = 0.4; carry[1] = N0; }         // a new batch
        const double gb = L.KEY[0];
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = N0; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_NL_NP] = N0; sc[MBX_SC_NL_ARC] = 0; sc[MBX_SC_NL_K] = 0; sc[MBX_SC_NL_LIVE] = 0;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = (double)N0 / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ update (__update :163-273)
// up to n_updates updates of one instance; a finished instance stays frozen
__device__ __forceinline__ void nl_updates(const BatchParams& bp, int n_updates, double* __restrict__ state_out, double* __restrict__ reward_out,
                                           uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int N0 = bp.NP, D = bp.D, CH = md_chunk(D), H = (int)MBX_NLSHADE_H(D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_NLSHADE_ST_SCALARS(N0, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const MdLds L = md_carve(smem, N0, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const double lb = P.lb, ub = P.ub, mf = (double)bp.max_fes;
    const int half = bp.max_fes / 2, n_sched = (int)bp.pci[0];
    double* gC = S + MBX_NLSHADE_ST_COST(N0, D);
    double* arc = S + MBX_NLSHADE_ST_ARC(N0, D);
    double* gMF = S + MBX_NLSHADE_ST_MF(N0, D);
    double* gMCr = S + MBX_NLSHADE_ST_MCR(N0, D);
    double* gU = S + MBX_NLSHADE_ST_U(N0, D);
    double* gNC = S + MBX_NLSHADE_ST_NCOST(N0, D);
    double* gF = S + MBX_NLSHADE_ST_F(N0, D);
    double* gCr = S + MBX_NLSHADE_ST_CR(N0, D);
    double* gI = S + MBX_NLSHADE_ST_IDX(N0, D);
    double* gZ = S + MBX_NLSHADE_ST_Z(N0, D);
    double* gCv = S + MBX_NLSHADE_ST_C(N0, D);
    double* gU2 = S + MBX_NLSHADE_ST_U2(N0, D);
    double* carry = S + MBX_NLSHADE_ST_CARRY(N0, D);
    double* CDF = L.EV;
    const int episode = (int)sc[MBX_SC_EPISODE];
    stage_problem(P, L.eval(CH, D, L.TC));
    __syncthreads();
    int done = 0;
    for (int it = 0; it < n_updates && !done; ++it) {
        const int gen = (int)sc[MBX_SC_GEN] + 1;
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)episode};
        const double fes0 = sc[MBX_SC_FES], gbest0 = sc[MBX_SC_GBEST], pb = carry[0];
        // (clamped: the state block can be caller data, mbx_debug_write_state)
        const int NP = min(max((int)sc[MBX_SC_NL_NP], 1), N0), NA = min(max((int)carry[1], 0), N0);
        const int narc = min(min(max((int)sc[MBX_SC_NL_ARC], 0), N0), NA), k_mem = min(max((int)sc[MBX_SC_NL_K], 0), H - 1);   // (:166-167)
        const int live = sc[MBX_SC_NL_LIVE] != 0. ? 1 : 0;
        const int log_index0 = (int)sc[MBX_SC_LOG_INDEX], cost_len0 = (int)sc[MBX_SC_COST_LEN];
        const double* pop = S + MBX_NLSHADE_ST_POP(N0, D) + (int64_t)live * N0 * D;
        double* npop = S + MBX_NLSHADE_ST_POP(N0, D) + (int64_t)(1 - live) * N0 * D;
        const int per = (NP + kThreads - 1) / kThreads, row0 = min(tid * per, NP), row1 = min(row0 + per, NP);
        const int pb_upper = min(max((int)fmax(2., (double)NP * pb), 1), NP), npad = md_pad(NP);
        const bool arc_on = narc >= kNlArcMin;
        const int fes0i = (int)fes0, n_crb = fes0i + NP > half ? min(NP, fes0i + NP - half) : 0;
        // ---- choose_F_Cr (:111-121): F per row, Cr sorted ascending by value (:174)
        for (int t = tid; t < npad; t += kThreads) { L.KEY[t] = INFINITY; L.IDX[t] = t; }
        __syncthreads();
        for (int i = row0; i < row1; ++i) {
            int ind;
            double z, c;
            if (tape) {
                ind = (int)tape[MBX_NLSHADE_TAPE_MEM(N0, D) + i]; z = tape[MBX_NLSHADE_TAPE_Z(N0, D) + i]; c = tape[MBX_NLSHADE_TAPE_C(N0, D) + i];
            } else {
                ind = (int)__umulhi(rng.draw((uint32_t)i, MBX_SITE_NL_PAR).x, (uint32_t)H);
                U4 w = rng.draw((uint32_t)i, MBX_SITE_NL_NORM);
                double z1;
                box_muller(u53(w.x, w.y), u53(w.z, w.w), z, z1);
                w = rng.draw((uint32_t)i, MBX_SITE_NL_CAUCHY);
                c = tan(3.141592653589793 * (u53(w.x, w.y) - 0.5));
            }
            ind = min(max(ind, 0), H - 1);
            double Cr = gMCr[ind] + 0.1 * z;
            const double loc = gMF[ind];
            if (Cr < 0.) Cr = 0.;                                    // np.minimum(1, np.maximum(0, .)): a NaN stays
            if (Cr > 1.) Cr = 1.;
            double F = c * 0.1 + loc;
            if (F < 0.) F = 2 * loc - F;
            if (F > 1.) F = 1.;
            gF[i] = F; L.KEY[i] = Cr; gZ[i] = z; gCv[i] = c;
        }
        __syncthreads();
        md_sort(L.KEY, L.IDX, npad);
        for (int t = tid; t < NP; t += kThreads) gCr[t] = L.KEY[t];
        __syncthreads();
        // ---- the cdf of the r2 choice (:179-181, np.random.choice): pr = exp(-(i + 1) / NP), / sum, cumsum, / last
        for (int t = tid; t < NP; t += kThreads) CDF[t] = exp((double)(-(t + 1)) / (double)NP);
        __syncthreads();
        if (tid == 0) L.RED[0] = md_pairwise(CDF, NP);
        __syncthreads();
        { const double s = L.RED[0]; for (int t = tid; t < NP; t += kThreads) CDF[t] = CDF[t] / s; }
        __syncthreads();
        if (tid == 0) { double run = 0.; for (int t = 0; t < NP; ++t) { run += CDF[t]; CDF[t] = run; } L.RED[0] = run; }
        __syncthreads();
        { const double s = L.RED[0]; for (int t = tid; t < NP; t += kThreads) CDF[t] = CDF[t] / s; }
        __syncthreads();
        // ---- mutation (:184-224), the two crossovers (:226-236), bound repair (:239-240): trial rows into the state block
        for (int i = row0; i < row1; ++i) {
            int pbs, r1, r2 = -1, ai = -1, jr, Lc;
            double rvs, u2 = 0., pick;
            if (tape) {
                pbs = (int)tape[MBX_NLSHADE_TAPE_PBS(N0, D) + i]; r1 = (int)tape[MBX_NLSHADE_TAPE_R1(N0, D) + i];
                rvs = tape[MBX_NLSHADE_TAPE_RVS(N0, D) + i]; jr = (int)tape[MBX_NLSHADE_TAPE_JRAND(N0, D) + i];
                Lc = (int)tape[MBX_NLSHADE_TAPE_L(N0, D) + i]; pick = tape[MBX_NLSHADE_TAPE_PICK(N0, D) + i];
            } else {
                const U4 v = rng.draw((uint32_t)i, MBX_SITE_NL_PAR);
                jr = (int)__umulhi(v.y, (uint32_t)D); Lc = (int)__umulhi(v.z, (uint32_t)D); pick = u32d(v.w);
                const U4 cw = rng.draw((uint32_t)i, MBX_SITE_NL_CAUCHY);
                rvs = u53(cw.z, cw.w);
                const U4 w = rng.draw((uint32_t)(i * 32), MBX_SITE_NL_IDX);
                pbs = (int)__umulhi(w.x, (uint32_t)pb_upper);
                if (pbs == i) pbs = (int)__umulhi(rng.draw((uint32_t)(i * 32 + 1), MBX_SITE_NL_IDX).x, (uint32_t)NP);          // one redraw round
                r1 = (int)__umulhi(w.y, (uint32_t)NP);
                for (int a = 1; a <= kNlTries && (r1 == i || r1 == pbs); ++a) r1 = (int)__umulhi(rng.draw((uint32_t)(i * 32 + a), MBX_SITE_NL_IDX).y, (uint32_t)NP);
            }
            pbs = min(max(pbs, 0), NP - 1); r1 = min(max(r1, 0), NP - 1); jr = min(max(jr, 0), D - 1); Lc = min(max(Lc, 0), D - 1);
            const bool from_arc = arc_on && rvs < 0.5;
            if (from_arc) {
                if (tape) ai = (int)tape[MBX_NLSHADE_TAPE_AIDX(N0, D) + i];
                else ai = (int)__umulhi(rng.draw((uint32_t)i, MBX_SITE_NL_ARC).y, (uint32_t)narc);
                ai = min(max(ai, 0), narc - 1);
            } else {
                if (tape) { u2 = tape[MBX_NLSHADE_TAPE_U2(N0, D) + i]; r2 = nl_choice(CDF, NP, u2); }
                else
                    for (int a = 0; a <= kNlTries; ++a) {
                        const U4 w = rng.draw((uint32_t)(i * 32 + a), MBX_SITE_NL_IDX);
                        u2 = u53(w.z, w.w); r2 = nl_choice(CDF, NP, u2);
                        if (!(r2 == i || r2 == pbs || r2 == r1)) break;
                    }
            }
            gI[4 * i] = pbs; gI[4 * i + 1] = r1; gI[4 * i + 2] = r2; gI[4 * i + 3] = ai; gU2[i] = u2;
            const double F = gF[i], Cr = gCr[i];
            const double Crb = i >= NP - n_crb ? 2 * ((double)(fes0i + i) / mf - 0.5) : 0.;
            const bool expo = pick > 0.5;
            const double* x = pop + (int64_t)i * D;
            const double* xb = pop + (int64_t)pbs * D;
            const double* x1 = pop + (int64_t)r1 * D;
            const double* x2 = from_arc ? arc + (int64_t)ai * D : pop + (int64_t)r2 * D;
            bool open = true;                                        // the exponential crossover's window [L, R) is still open at column d
            for (int d = 0; d < D; ++d) {
                double cb, ce;
                if (tape) { cb = tape[MBX_NLSHADE_TAPE_CROSSB(N0, D) + (int64_t)i * D + d]; ce = tape[MBX_NLSHADE_TAPE_CROSSE(N0, D) + (int64_t)i * D + d]; }
                else { const U4 w = rng.draw((uint32_t)(i * D + d), MBX_SITE_NL_CROSS); cb = u53(w.x, w.y); ce = u53(w.z, w.w); }
                const double v = x[d] + F * (xb[d] - x[d]) + F * (x1[d] - x2[d]);
                if (d > Lc && ce > Cr) open = false;
                const bool take = expo ? (d >= Lc && open) : (cb < Crb || d == jr);
                double u = take ? v : x[d];
                if (u < lb) u = (u + lb) / 2;
                if (u > ub) u = (u + ub) / 2;
                gU[(int64_t)i * D + d] = u;
            }
        }
        __syncthreads();
        // ---- evaluation of the trials in row chunks
        // (this loop, the ranking and the sums below are md_eval_rows, md_rank_improved and md_weighted_sums written out: through the shared functions the
        // update measured 1.5 % to 3 % slower, docs/EXPERIMENTS.md "Shared phases of the sorted-DE kernels")
        for (int c0 = 0; c0 < NP; c0 += CH) {
            const int n = min(CH, NP - c0);
            for (int e = tid; e < n * D; e += kThreads) L.EV[e] = gU[(int64_t)c0 * D + e];
            __syncthreads();
            population_costs(P, L.eval(n, D, L.TC), n, rng, tape ? tape + MBX_NLSHADE_TAPE_NOISE(N0, D) : nullptr, MBX_SITE_NL_NOISE_A,
                             MBX_SITE_NL_NOISE_B, c0, N0);
            if (tid < n) gNC[c0 + tid] = L.TC[tid];
            __syncthreads();
        }
        // ---- selection (:243): ranks of the improved rows; np.min of the trial costs
        int ocnt[3] = {0, 0, 0}, obase[3], otot[3];
        double tmin = INFINITY;
        for (int i = row0; i < row1; ++i) {
            const double nc = gNC[i];
            ocnt[0] += nc < gC[i];
            if (isnan(nc) || isnan(tmin)) tmin = NAN; else if (nc < tmin) tmin = nc;
        }
        // (nl_min_seen is associative, so the wave's lanes, and then the four waves, fold in any grouping that keeps thread order; a lane whose partner
        // lies beyond the wave folds with itself; the barriers of the scan stand between RED[4 .. 7] and their reader)
        for (int off = 1; off < 64; off <<= 1) tmin = nl_min_seen(tmin, __shfl_down(tmin, off));
        if ((tid & 63) == 0) L.RED[4 + (tid >> 6)] = tmin;
        md_scan3(L.CNT, ocnt, obase, otot);
        const int n_opt = otot[0], n_app = min(max(NA - narc, 0), n_opt), alen = narc + n_app;
        if (tid == 0) L.RED[1] = nl_min_seen(nl_min_seen(L.RED[4], L.RED[5]), nl_min_seen(L.RED[6], L.RED[7]));
        // ---- archive (:129-133, :244-245): the parent of rank k is population row k
        if (n_opt > 0 && alen > 0) {
            auto target = [&](int k) -> int {
                if (tape) return min(max((int)tape[MBX_NLSHADE_TAPE_ARCW(N0, D) + k], 0), alen - 1);
                return (int)__umulhi(rng.draw((uint32_t)k, MBX_SITE_NL_ARC).x, (uint32_t)alen);
            };
            md_archive_write(L, arc, pop, D, narc, n_app, alen, target, [&](auto put) { for (int k = tid; k < n_opt; k += kThreads) put(k, k); });
        }
        __syncthreads();
        // ---- memory (:83-109): weighted Lehmer-type means over the improved rows, compacted in rank order, numpy's pairwise sums
        const double fes = fes0 + NP;
        const int fesi = fes0i + NP;
        double newMF = 0.5, newMCr = 0.9;
        if (n_opt > 0) {
            const double pgF = (double)(bp.max_fes - fesi) * 2.0 / mf + 1.5, pgCr = (double)(bp.max_fes - fesi) * -0.5 / mf + 1.5;
            // pass 0: df;  1: w SF^pg;  2: w SF^(pg - 1.5);  3: w SCr^pg;  4: w SCr^(pg - 1.5)
            double sums[5] = {0., 0., 0., 0., 0.};
            for (int pass = 0; pass < 5; ++pass) {
                int k = obase[0];
                for (int i = row0; i < row1; ++i) {
                    const double c = gC[i], nc = gNC[i];
                    if (nc < c) {
                        const double df = (c - nc) / (c + 1e-9);
                        double v = df;
                        if (pass > 0) {
                            const double w = df / sums[0], s = pass <= 2 ? gF[i] : gCr[i];
                            const double e = pass == 1 ? pgF : pass == 2 ? pgF - 1.5 : pass == 3 ? pgCr : pgCr - 1.5;
                            v = w * pow(s, e);
                        }
                        L.VEC[k++] = v;
                    }
                }
                __syncthreads();
                if (tid == 0) L.RED[0] = md_pairwise(L.VEC, n_opt);
                __syncthreads();
                sums[pass] = L.RED[0];
                __syncthreads();
                if (pass == 0 && !(sums[0] > 0.)) break;
            }
            if (sums[0] > 0.) { newMF = sums[1] / sums[2]; newMCr = sums[3] / sums[4]; }
        }
        // ---- replacement, NLPSR, sort (:253-262, :135-147): rows into the other buffer in (cost, row) order
        const int Nt = (int)bp.pci[1 + min(max(gen, 0), n_sched)];
        const int NPn = min(max(Nt, 1), NP), A = max(Nt, kNlNmin);
        md_replace_sorted(L, gC, gNC, gU, pop, npop, NP, NPn, D);
        // ---- bookkeeping (:256-273)
        if (tid == 0) {
            const double best = L.RED[1];
            const double gbest = best < gbest0 ? best : gbest0;
            gMF[k_mem] = newMF; gMCr[k_mem] = newMCr;
            int log_index = log_index0, cost_len = cost_len0;
            const bool dn = log_and_terminate_guarded(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
            sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
            sc[MBX_SC_DONE] = dn ? 1. : 0.; sc[MBX_SC_GEN] = gen; sc[MBX_SC_GBEST_IDX] = 0;
            sc[MBX_SC_NL_NP] = NPn; sc[MBX_SC_NL_ARC] = A < alen ? A : alen; sc[MBX_SC_NL_K] = n_opt > 0 ? (k_mem + 1) % H : k_mem;
            sc[MBX_SC_NL_LIVE] = 1 - live;
            carry[0] = 0.2 + 0.1 * (fes / mf);
            if (A < alen) carry[1] = A;
            L.RED[2] = dn ? 1. : 0.;
        }
        __syncthreads();
        done = L.RED[2] != 0.;
        __syncthreads();
    }
    if (tid == 0) {
        if (state_out) state_out[b] = sc[MBX_SC_FES] / mf;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_nlshade_step(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                           uint8_t* __restrict__ done_out)
{
    nl_updates(bp, 1, state_out, reward_out, done_out);
}

__global__ __launch_bounds__(kThreads) void k_nlshade_run(BatchParams bp, int n_updates, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                          uint8_t* __restrict__ done_out)
{
    nl_updates(bp, n_updates, state_out, reward_out, done_out);
}

}  // namespace mbx
