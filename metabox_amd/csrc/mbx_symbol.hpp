// mbx_symbol.hpp — SYMBOL: a population whose update rule is an expression tree handed over per instance and per action, as a resident kernel
// (reference: src/optimizer/symbol_optimizer.py:122-200, src/optimizer/symbol_related/population.py; layout, tokens, tape: include/mbx_layout.h
// section 22).
//
// Every other kernel of this library hard-wires its move.  Here the move is DATA: 63 heap-ordered token slots and a float64 constant per slot.  One
// workgroup owns an instance (through bp.order) and runs the sub-steps of an action -- the index rows of the randx leaves, the rule, the periodic wrap,
// one evaluation of the NP candidate rows, Population.update -- with x, the candidates, pbest_pos, delta_x, the gb / gw / cbest rows, the costs and the
// index rows (bytes) in LDS; after the last sub-step it computes the nine features, the log point, the reward and done.
//
// The rule.  sym_check looks at every slot once (one slot per thread); thread 0 then lists the tree in post-order with the parent / child arithmetic
// of the heap, no stack.  The tree is the same for the whole workgroup, so the walk over that list and the operator dispatch are uniform: each entry
// is read from LDS at a uniform address and handed to the scalar unit (readfirstlane), and the branches on it are scalar branches.  A thread owns the
// elements e = tid, tid + 256, .. of the NP x D block and evaluates the whole list for one element at a time.  The operand stack is at most six deep
// (a path of the tree has six nodes) and is six named registers that SHIFT on push and pop: there is no stack pointer and no indexed private
// array, hence no scratch.  All gathers read the pre-move x: the candidates go to the other position buffer, which was the evaluator's scratch.
//
// The reference's own behaviour, kept on purpose:
//  * the rule is evaluated as its parenthesised infix string is by numpy: (left op right), -(child), float64; next = x + f(..);
//  * one index row per randx occurrence and sub-step, occurrences numbered left to right; `dx` is delta_x = x - pre_x, the quotient population.dx is never read;
//  * the border is 'periodic' (:75): lb + (next - ub) % (ub - lb) with numpy's floored modulo (fmod, plus the divisor where the signs differ; a zero is +0.);
//  * no end test between the sub-steps of an action; one log append per action at most; reward = (pre_gbest - gbest) / init_cost;
//  * pbest strict <; gbest from the first argmin with strict <, else stag_count += 1; gworst = the worst cost ever seen, strict >, first argmax;
//  * reset draws uniform(-ub, ub), not uniform(lb, ub) (population.py:43).
// Arithmetic: float64, no contraction (the build passes -ffp-contract=off).  The feature sums follow include/mbx_layout.h section 22.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"

namespace mbx {

struct SymArgs {
    const int32_t* tokens;      // [B][63], or nullptr: the program comes from `actions`
    const double* consts;       // [B][63]
    const double* actions;      // [B][126] float64: tokens, then constants (mbx_step)
    int n_sub;                  // sub-steps of this launch at most
    int n_action;               // sub-steps of an action
    int resident;               // pbest_pos and delta_x live in LDS (sym_resident)
    int32_t* n_bad;             // [B] or nullptr: 1 where the program was malformed, else 0
};

// numpy's floored float modulo (npy_divmod) for a positive finite divisor
__device__ __forceinline__ double sym_floor_mod(double a, double b)
{
    double m = fmod(a, b);
    if (m != 0.) { if (m < 0.) m += b; }
    else m = 0.;                                                     // copysign(0, b), b > 0
    return m;
}

// One slot per thread: is the program well formed?  Ends with barriers; every thread gets the answer and the number of randx leaves.
__device__ __forceinline__ bool sym_check(const int* TOK, int& n_randx)
{
    const int p = threadIdx.x;
    int bad = 0, rx = 0;
    if (p < MBX_SYM_SLOTS) {
        const int t = TOK[p];
        if (t < -1 || t >= MBX_SYM_NTOK) bad = 1;
        else if (p == 0) bad = !(t >= MBX_SYM_TOK_ADD && t <= MBX_SYM_TOK_NEG);          // an empty root, a leaf at the root
        else if (t != -1) {
            const int q = TOK[(p - 1) >> 1];                                              // under a binary operator, or on the left of the unary one
            bad = !(q == MBX_SYM_TOK_ADD || q == MBX_SYM_TOK_MUL || (q == MBX_SYM_TOK_NEG && (p & 1)));
        }
        if (!bad && t >= MBX_SYM_TOK_ADD && t <= MBX_SYM_TOK_NEG) {                       // an operator has its children
            if (2 * p + 2 >= MBX_SYM_SLOTS) bad = 1;
            else bad = TOK[2 * p + 1] == -1 || (t != MBX_SYM_TOK_NEG && TOK[2 * p + 2] == -1);
        }
        rx = t == MBX_SYM_TOK_RANDX;
    }
    n_randx = __syncthreads_count(rx);
    const int any_bad = __syncthreads_or(bad);
    return !any_bad && n_randx <= MBX_SYM_RANDX_MAX;
}

// Thread 0 lists a checked tree in post-order: PROG[k] = token | argument << 8 (the occurrence number of a randx leaf), PCST[k] = the slot's constant.
// The length goes to PROG[63]: a tree has 63 nodes at most.
__device__ __forceinline__ void sym_list(const int* TOK, const double* CST, int* PROG, double* PCST)
{
    int p = 0, n = 0, rx = 0;
    while (p < 31 && TOK[p] >= 0 && TOK[p] <= MBX_SYM_TOK_NEG) p = 2 * p + 1;             // the first leaf
    for (int guard = 0; guard < MBX_SYM_SLOTS; ++guard) {
        const int t = TOK[p];
        PROG[n] = t == MBX_SYM_TOK_RANDX ? t | (rx++ << 8) : t;
        PCST[n] = CST[p];
        ++n;
        if (p == 0) break;
        const int q = (p - 1) >> 1;
        if ((p & 1) && TOK[q] != MBX_SYM_TOK_NEG) {                                       // a left child of a binary operator: on to the right subtree
            p = p + 1;
            while (p < 31 && TOK[p] >= 0 && TOK[p] <= MBX_SYM_TOK_NEG) p = 2 * p + 1;
        } else p = q;
    }
    PROG[MBX_SYM_SLOTS] = n;
}

// The nine features over the population in `X` (rows) / L.NC (costs); T is free.  All threads call; ends with a barrier; F[0..8] valid for thread 0 only.
__device__ __forceinline__ void sym_features(const SymLds& L, const double* X, int NP, int D, double lb, double ub, double gbest, double gworst, double cbest,
                                             double pre_gbest, double fes, int max_fes, int stag, double* F)
{
    const int tid = threadIdx.x;
    const double den = gworst - gbest + 1e-8, maxd = sqrt((ub - lb) * (ub - lb) * D);
    double* R1 = L.T; double* R2 = L.T + NP; double* R6 = L.T + 2 * NP; double* R7 = L.T + 3 * NP; double* R8 = L.T + 4 * NP;      // T holds 8 NP at least
    if (tid < NP) {
        const double c = L.NC[tid];
        const double* xi = X + tid * D;
        R1[tid] = (c - gbest) / den;
        R7[tid] = (c - cbest) / den;
        R2[tid] = np_sum_block([&](int j) {
            const double* xj = X + j * D;
            double s = 0.;
            for (int d = 0; d < D; ++d) { const double t = xi[d] - xj[d]; s += t * t; }
            return sqrt(s);
        }, NP);
        R6[tid] = sqrt(np_sum_block([&](int d) { const double t = xi[d] - L.CB[d]; return t * t; }, D)) / maxd;
        R8[tid] = sqrt(np_sum_block([&](int d) { const double t = xi[d] - L.GB[d]; return t * t; }, D)) / maxd;
    }
    __syncthreads();
    if (tid < 6) {                                                   // one reduction per lane
        double v;
        if (tid == 5) {                                              // the two standard deviations
            const double mean = np_sum_block([&](int k) { return L.NC[k]; }, NP) / NP;
            const double sd = sqrt(np_sum_block([&](int k) { const double t = L.NC[k] - mean; return t * t; }, NP) / NP);
            const int half = NP / 2;
            const double fmean = np_sum_block([&](int k) { return k < half ? gworst : gbest; }, NP) / NP;
            const double fsd = sqrt(np_sum_block([&](int k) { const double t = (k < half ? gworst : gbest) - fmean; return t * t; }, NP) / NP);
            v = sd / (fsd + 1e-8);
        } else {
            const double* R = tid == 0 ? R1 : tid == 1 ? R2 : tid == 2 ? R6 : tid == 3 ? R7 : R8;
            v = np_sum_block([&](int k) { return R[k]; }, NP);
            v = tid == 1 ? v / ((double)NP * NP) / maxd : v / NP;
        }
        L.RED[8 + tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        F[0] = L.RED[8]; F[1] = L.RED[9]; F[2] = L.RED[13];
        F[3] = ((double)max_fes - fes) / max_fes;
        F[4] = (double)stag / (double)(max_fes / NP);
        F[5] = L.RED[10]; F[6] = L.RED[11]; F[7] = L.RED[12];
        F[8] = gbest < pre_gbest ? 1. : 0.;
    }
}

// MODE 0: reset; 1: one sub-step; 2: up to ar.n_sub sub-steps
template <int MODE>
__device__ __forceinline__ void sym_body(const BatchParams& bp, const SymArgs& ar, double* __restrict__ state_out, double* __restrict__ reward_out,
                                         uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const bool resident = ar.resident != 0;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_SYMBOL_ST_SCALARS(NP, D);
    double* gFEAT = S + MBX_SYMBOL_ST_FEAT(NP, D);
    double* gPB = S + MBX_SYMBOL_ST_PBPOS(NP, D);
    double* gDX = S + MBX_SYMBOL_ST_DX(NP, D);
    if (MODE != 0 && sc[MBX_SC_DONE] != 0.) {                        // a finished instance stays as it is
        if (tid < MBX_SYM_NFEAT && state_out) state_out[(int64_t)b * MBX_SYM_NFEAT + tid] = gFEAT[tid];
        if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; if (ar.n_bad) ar.n_bad[b] = 0; }
        return;
    }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);
    const SymLds L = sym_carve(smem, NP, D, resident);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const double lb = P.lb, ub = P.ub;
    const FastDiv fd(D);

    if (MODE == 0) {                                                 // ---- reset (Population.reset :31-81, init_population :100-107)
        const int episode = (int)sc[MBX_SC_EPISODE] + 1;
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
        stage_problem(P, L.eval(L.A, L.Bf));
        for (int e = tid; e < NE; e += kThreads) {
            double u;
            if (tape) u = tape[MBX_SYMBOL_TAPE_POS(NP, D) + e];
            else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); u = u53(w.x, w.y); }
            const double x = -ub + (ub - (-ub)) * u;
            L.A[e] = x;
            S[MBX_SYMBOL_ST_X(NP, D) + e] = x; gPB[e] = x; gDX[e] = 0.;
        }
        __syncthreads();
        population_costs<0, 0, ConstProblem>(P, L.eval(L.A, L.Bf), NP, rng, tape ? tape + MBX_SYMBOL_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_NOISE1_A,
                                             MBX_SITE_NOISE1_B);
        double gb, gwn; int g0, w0;
        block_argmin(L.NC, NP, L.RED, gb, g0);
        if (tid < NP) { L.T[tid] = -L.NC[tid]; S[MBX_SYMBOL_ST_COST(NP, D) + tid] = L.NC[tid]; S[MBX_SYMBOL_ST_PBEST(NP, D) + tid] = L.NC[tid]; }
        __syncthreads();
        block_argmin(L.T, NP, L.RED, gwn, w0);                       // the first argmax
        const double gw = -gwn;
        if (tid < D) {
            const double g = L.A[g0 * D + tid], w = L.A[w0 * D + tid];
            L.GB[tid] = g; L.CB[tid] = g; L.GW[tid] = w;
            S[MBX_SYMBOL_ST_GBPOS(NP, D) + tid] = g; S[MBX_SYMBOL_ST_CBPOS(NP, D) + tid] = g; S[MBX_SYMBOL_ST_GWPOS(NP, D) + tid] = w;
        }
        __syncthreads();
        double F[MBX_SYM_NFEAT];
        sym_features(L, L.A, NP, D, lb, ub, gb, gw, gb, gb, (double)NP, bp.max_fes, 0, F);
        if (tid == 0) {
            for (int k = 0; k < MBX_NSCALAR; ++k) sc[k] = 0.;
            sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
            sc[MBX_SC_GBEST_IDX] = g0; sc[MBX_SC_SYM_GWORST] = gw; sc[MBX_SC_SYM_CBEST] = gb; sc[MBX_SC_SYM_CBEST_IDX] = g0;
            sc[MBX_SC_SYM_PRE_GBEST] = gb; sc[MBX_SC_SYM_INIT_COST] = gb;
            sc[MBX_NSCALAR] = gb;                                    // cost = [gbest]
            for (int k = 0; k < MBX_SYM_NFEAT; ++k) { gFEAT[k] = F[k]; if (state_out) state_out[(int64_t)b * MBX_SYM_NFEAT + k] = F[k]; }
            gFEAT[MBX_SYM_NFEAT] = 0.;
        }
        return;
    }

    // ---- the program: staged, checked, listed
    if (tid < 64) {
        int t = -1; double c = 0.;
        if (tid < MBX_SYM_SLOTS) {
            if (ar.tokens) { t = ar.tokens[(int64_t)b * MBX_SYM_SLOTS + tid]; c = ar.consts[(int64_t)b * MBX_SYM_SLOTS + tid]; }
            else {
                const double a = ar.actions[(int64_t)b * 2 * MBX_SYM_SLOTS + tid];
                t = (a >= -1. && a < (double)MBX_SYM_NTOK && a == floor(a)) ? (int)a : MBX_SYM_NTOK;       // anything else is an unknown token
                c = ar.actions[(int64_t)b * 2 * MBX_SYM_SLOTS + MBX_SYM_SLOTS + tid];
            }
        }
        L.TOK[tid] = t; L.PCST[tid] = 0.; L.CST[tid] = c;
    }
    __syncthreads();
    int n_randx;
    const bool ok = sym_check(L.TOK, n_randx);
    if (!ok) {                                                       // (uniform) a malformed program: the instance is left untouched
        if (tid < MBX_SYM_NFEAT && state_out) state_out[(int64_t)b * MBX_SYM_NFEAT + tid] = gFEAT[tid];
        if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 0; if (ar.n_bad) ar.n_bad[b] = 1; }
        return;
    }
    if (tid == 0) sym_list(L.TOK, L.CST, L.PROG, L.PCST);

    // every scalar is read here by every thread; thread 0 writes them back after the last barrier
    double gbest = sc[MBX_SC_GBEST], gworst = sc[MBX_SC_SYM_GWORST], cbest = sc[MBX_SC_SYM_CBEST], pre_gbest = sc[MBX_SC_SYM_PRE_GBEST];
    double fes = sc[MBX_SC_FES];
    int gen = (int)sc[MBX_SC_GEN], stag = (int)sc[MBX_SC_SYM_STAG], cb_idx = (int)sc[MBX_SC_SYM_CBEST_IDX], gb_idx = (int)sc[MBX_SC_GBEST_IDX];
    const int n_action = min(max(ar.n_action, 1), MBX_SYM_SUB_MAX);
    int sub = min(max((int)sc[MBX_SC_SYM_SUB], 0), n_action - 1);    // (clamped: mbx_debug_write_state is caller data)
    const uint32_t episode = (uint32_t)(int)sc[MBX_SC_EPISODE];
    uint8_t* gIDX = (uint8_t*)(S + MBX_SYMBOL_ST_IDX(NP, D, bp.n_logpoint));

    double* cur = L.A; double* nxt = L.Bf;                           // x | the candidates; they swap after every sub-step
    stage_problem(P, L.eval(L.A, L.Bf));
    for (int e = tid; e < NE; e += kThreads) {
        cur[e] = S[MBX_SYMBOL_ST_X(NP, D) + e];
        if (resident) { L.PB[e] = gPB[e]; L.DX[e] = gDX[e]; }
    }
    if (tid < NP) { L.PBC[tid] = S[MBX_SYMBOL_ST_PBEST(NP, D) + tid]; L.NC[tid] = S[MBX_SYMBOL_ST_COST(NP, D) + tid]; }
    if (tid < D) { L.GB[tid] = S[MBX_SYMBOL_ST_GBPOS(NP, D) + tid]; L.GW[tid] = S[MBX_SYMBOL_ST_GWPOS(NP, D) + tid]; L.CB[tid] = S[MBX_SYMBOL_ST_CBPOS(NP, D) + tid]; }
    __syncthreads();
    const int n_prog = min(max(L.PROG[MBX_SYM_SLOTS], 1), MBX_SYM_SLOTS);

    const int n = min(MODE == 1 ? 1 : ar.n_sub, n_action - sub);
    for (int it = 0; it < n; ++it) {
        if (sub == 0) pre_gbest = gbest;                             // update() :129
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(gen + 1), episode};
        const double* ts = tape ? tape + MBX_SYMBOL_TAPE_SUB(NP, D, sub) : nullptr;
        // ---- the index rows (:149, :156), one per randx occurrence
        for (int q = tid; q < n_randx * NP; q += kThreads) {
            int r;
            if (ts) r = min(max((int)ts[MBX_SYMBOL_SUB_IDX(NP, D) + q], 0), NP - 1);      // (clamped: a tape is caller data)
            else { const U4 w = rng.draw((uint32_t)q, MBX_SITE_SYM_IDX); r = (int)__umulhi(w.x, (uint32_t)NP); }
            L.IDX[q] = (uint8_t)r;
            gIDX[(int64_t)sub * MBX_SYM_RANDX_MAX * NP + q] = (uint8_t)r;
        }
        __syncthreads();
        // ---- the rule (:161), the wrap (:167), delta_x (population.py:132)
        for (int e = tid; e < NE; e += kThreads) {
            const int i = fd.div(e), d = e - i * D;
            const double x = cur[e];
            double s0 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0., s5 = 0.;
            for (int k = 0; k < n_prog; ++k) {
                const int ins = __builtin_amdgcn_readfirstlane(L.PROG[k]);
                const int t = ins & 255;
                if (t <= MBX_SYM_TOK_MUL) {                          // (left op right): left is the deeper entry
                    s0 = t == MBX_SYM_TOK_ADD ? s1 + s0 : s1 * s0;
                    s1 = s2; s2 = s3; s3 = s4; s4 = s5;
                } else if (t == MBX_SYM_TOK_NEG) s0 = -s0;
                else {
                    double v;
                    switch (t) {
                    case MBX_SYM_TOK_X: v = x; break;
                    case MBX_SYM_TOK_GB: v = L.GB[d]; break;
                    case MBX_SYM_TOK_GW: v = L.GW[d]; break;
                    case MBX_SYM_TOK_DX: v = resident ? L.DX[e] : gDX[e]; break;
                    case MBX_SYM_TOK_PB: v = resident ? L.PB[e] : gPB[e]; break;
                    case MBX_SYM_TOK_RANDX: v = cur[(int)L.IDX[(ins >> 8) * NP + i] * D + d]; break;
                    default: v = L.PCST[k]; break;                   // the two constant tokens
                    }
                    s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
                }
            }
            const double moved = x + s0;
            const double c = lb + sym_floor_mod(moved - ub, ub - lb);
            nxt[e] = c;
            const double dlt = c - x;
            if (resident) L.DX[e] = dlt; else gDX[e] = dlt;
        }
        __syncthreads();
        // ---- the evaluation (population.py:91): cur is dead and serves as the evaluator's scratch
        population_costs<0, 0, ConstProblem>(P, L.eval(nxt, cur), NP, rng, ts ? ts + MBX_SYMBOL_SUB_NOISE(NP, D) : nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B);
        // ---- Population.update (:98-127)
        if (tid < NP) {
            const int impr = L.NC[tid] < L.PBC[tid];
            if (impr) L.PBC[tid] = L.NC[tid];
            L.FLAG[tid] = impr;
            L.T[tid] = -L.NC[tid];
        }
        double cbv, wn; int cbi, wi;
        block_argmin(L.NC, NP, L.RED, cbv, cbi);                      // (its barriers publish FLAG / PBC / T)
        block_argmin(L.T, NP, L.RED, wn, wi);                        // np.argmax: the first index of the largest
        const bool better = cbv < gbest, worse = -wn > gworst;
        if (better) { gbest = cbv; gb_idx = cbi; stag = 0; } else stag += 1;
        if (worse) gworst = -wn;
        cbest = cbv; cb_idx = cbi;
        if (tid < D) {
            const double r = nxt[cbi * D + tid];
            L.CB[tid] = r;
            if (better) L.GB[tid] = r;
            if (worse) L.GW[tid] = nxt[wi * D + tid];
        }
        for (int e = tid; e < NE; e += kThreads) {
            if (L.FLAG[fd.div(e)]) { if (resident) L.PB[e] = nxt[e]; else gPB[e] = nxt[e]; }
        }
        fes += NP; gen += 1; sub += 1;
        { double* t = cur; cur = nxt; nxt = t; }
        __syncthreads();
    }

    // ---- after the last sub-step of the action (:174-200): features, log point, reward, done
    const bool end_of_action = sub >= n_action;
    double F[MBX_SYM_NFEAT];
    if (end_of_action) sym_features(L, cur, NP, D, lb, ub, gbest, gworst, cbest, pre_gbest, fes, bp.max_fes, stag, F);
    // ---- the state block, once per launch
    for (int e = tid; e < NE; e += kThreads) {
        S[MBX_SYMBOL_ST_X(NP, D) + e] = cur[e];
        if (resident) { gPB[e] = L.PB[e]; gDX[e] = L.DX[e]; }
    }
    if (tid < NP) { S[MBX_SYMBOL_ST_PBEST(NP, D) + tid] = L.PBC[tid]; S[MBX_SYMBOL_ST_COST(NP, D) + tid] = L.NC[tid]; }
    if (tid < D) { S[MBX_SYMBOL_ST_GBPOS(NP, D) + tid] = L.GB[tid]; S[MBX_SYMBOL_ST_GWPOS(NP, D) + tid] = L.GW[tid]; S[MBX_SYMBOL_ST_CBPOS(NP, D) + tid] = L.CB[tid]; }
    if (tid == 0) {
        double reward = 0.;
        bool done = false;
        if (end_of_action) {
            int log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
            done = log_and_terminate(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
            reward = (pre_gbest - gbest) / sc[MBX_SC_SYM_INIT_COST];
            sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len; sc[MBX_SC_RETURN] += reward;
            for (int k = 0; k < MBX_SYM_NFEAT; ++k) gFEAT[k] = F[k];
            sub = 0;
        }
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = gen; sc[MBX_SC_GBEST_IDX] = gb_idx;
        sc[MBX_SC_SYM_SUB] = sub; sc[MBX_SC_SYM_GWORST] = gworst; sc[MBX_SC_SYM_CBEST] = cbest; sc[MBX_SC_SYM_CBEST_IDX] = cb_idx;
        sc[MBX_SC_SYM_STAG] = stag; sc[MBX_SC_SYM_PRE_GBEST] = pre_gbest;
        if (state_out) for (int k = 0; k < MBX_SYM_NFEAT; ++k) state_out[(int64_t)b * MBX_SYM_NFEAT + k] = gFEAT[k];
        if (reward_out) reward_out[b] = reward;
        if (done_out) done_out[b] = done ? 1 : 0;
        if (ar.n_bad) ar.n_bad[b] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_symbol_reset(BatchParams bp, SymArgs ar, double* __restrict__ state_out)
{
    sym_body<0>(bp, ar, state_out, nullptr, nullptr);
}

__global__ __launch_bounds__(kThreads) void k_symbol_step(BatchParams bp, SymArgs ar, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                          uint8_t* __restrict__ done_out)
{
    sym_body<1>(bp, ar, state_out, reward_out, done_out);
}

// three waves per SIMD is what the LDS allows at NP = 100, D = 10 (47.9 KB per workgroup); left alone the compiler takes 170 VGPRs for the sub-step loop, which fits two
// (1.84 ms per action of 4096 instances, against 1.61 ms for five one-sub-step launches); capped it takes 144 and still no scratch
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_symbol_run(BatchParams bp, SymArgs ar, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                         uint8_t* __restrict__ done_out)
{
    sym_body<2>(bp, ar, state_out, reward_out, done_out);
}

}  // namespace mbx
