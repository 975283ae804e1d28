// mbx_glpso.hpp — GL-PSO, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/gl_pso.py:5-177).
//
// PSO whose particles are attracted by an "exemplar" each (c1 = 1.49618, w = 0.7298, velocity cap 0.2 (ub - lb)); the exemplars are
// bred every generation by a genetic step over the pbest positions -- crossover (:22-30), mutation (:32-34), an evaluation of the NP
// new exemplars and greedy selection (:36-47) -- and an exemplar that has not improved for more than sg = 7 generations is replaced by
// the winner of a 10-way tournament (:49-66).  Every generation therefore evaluates two populations of NP = 100 rows.
//
// No agent: mbx_reset is init_population, every mbx_step (actions = NULL) one __update.  One workgroup per instance, dispatched
// through bp.order; the state block (include/mbx_layout.h §11) is streamed from HBM once per generation.  pbest_pos and the exemplars
// are staged in the evaluator's Z scratch, which is free between the two evaluations: the crossover gathers pbest_pos[k, d] from it
// and the tournament gathers whole exemplar rows.
//
// Quirks of the reference kept on purpose:
//  * the tournament replaces the exemplar but neither its exemplar_cost nor its counter (:59-66): it fires again every generation
//    until that exemplar wins a selection;
//  * exemplar_stag lives on the optimizer object (:19) and init_population never resets it: mbx_reset leaves the counters alone;
//  * gbest and the cost curve follow the particles only; exemplar costs never enter them (found_best is not observable).
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off); uniform(a, b) = a + (b - a) u.
//
// What is pinned, and by what (tests/glpso_exact.py restates :22-66 and :76-177 on this state block with NP and D at run time; tests/test_glpso_exact.py):
//  * positions, velocities, candidate exemplars and the exemplar rows after selection and tournament: bit for bit, at (NP, D) from (4, 2) to (256, 10), the docking
//    shape included.  No bit-level exception is needed: fmin(fmax(v, lo), hi) is np.clip on every finite input, signed zeros included.  (The two bounces below could
//    be one test, `nx > ub || nx < lb`: a position is never beyond both bounds.)
//  * every cost against the extended-precision evaluators, every `<` decided wherever exact +- allowance decides it;
//  * the rules stated here, each by a planted state: strict `<` for pbest, gbest and the selection (exact ties, c < c); stag > 7 (counters at 6, 7, 8); first on
//    ties in the tournament and in the gbest argmin; the tournament gathering the exemplars after selection and before any replacement of this launch; exemplar_cost
//    and the counter left alone by the tournament; the counters carried over mbx_reset and mbx_batch_rebind; the log test after the first evaluation; mt < 0.01.
// Not pinned: free-running Philox episodes against the reference in distribution, and the normal-noise draws on the Philox route (the host cannot rebuild the
// device's log / cos).  The log-point append below is guarded by the curve's length where the reference's (:160-162) is not: the two part only for a budget with
// log_interval (n_logpoint + 1) <= max_fes, which no test reaches.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"

namespace mbx {

constexpr double kGlW = 0.7298, kGlC1 = 1.49618, kGlPm = 0.01, kGlRho = 0.2;
constexpr int kGlSg = 7, kGlNsel = MBX_GLPSO_NSEL;

// The LDS layout (GpLds, gp_lds_doubles, gp_carve) lives in mbx_lds.hpp.

// __exemplar_update (:61-66) on the staged swarm: Z = pbest_pos, L.PBC = pbest, L.GB = gbest_pos, L.EXC / L.STAG = exemplar_cost and the
// counters.  xb: the exemplar block of the tape (nullptr: Philox).  Writes exemplar / exemplar_cost / stag of the state block (S) and
// ends with a barrier.
template <bool INIT>
__device__ __forceinline__ void gp_exemplar(const DevProblem& P, const GpLds& L, int NP, int D, double* S, const double* xb, const Rng& rng)
{
    const int tid = threadIdx.x, NE = NP * D;
    const double lb = P.lb, ub = P.ub;
    const FastDiv fd(D);
    double* gEX = S + MBX_GLPSO_ST_EX(NP, D);
    // crossover (:22-30) and mutation (:32-34) into X
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e), d = e - i * D;
        int k; double r, mu, mt;
        if (xb) {
            k = min(max((int)xb[MBX_GLPSO_XB_CIDX(NP, D) + e], 0), NP - 1); r = xb[MBX_GLPSO_XB_CU(NP, D) + e];     // (clamped: a tape is caller data)
            mu = xb[MBX_GLPSO_XB_MU(NP, D) + e]; mt = xb[MBX_GLPSO_XB_MTEST(NP, D) + e];
        } else {
            const U4 w = rng.draw((uint32_t)e, MBX_SITE_GL_CROSS);
            k = (int)__umulhi(w.x, (uint32_t)NP); r = u53(w.z, w.w);
            const U4 m = rng.draw((uint32_t)e, MBX_SITE_GL_MUT);
            mu = u53(m.x, m.y); mt = u53(m.z, m.w);
        }
        double ne = L.PBC[k] < L.PBC[i] ? L.Z[k * D + d] : r * L.Z[e] + (1. - r) * L.GB[d];
        if (mt < kGlPm) ne = lb + (ub - lb) * mu;
        L.X[e] = ne;
    }
    __syncthreads();
    // one evaluation of the NP new exemplars (:37); Z / T are the evaluator's again until it returns
    population_costs(P, L.eval(), NP, rng, xb ? xb + MBX_GLPSO_XB_NOISE(NP, D) : nullptr, MBX_SITE_GL_NOISE_A, MBX_SITE_GL_NOISE_B);
    // selection (:38-45): init replaces unconditionally and leaves the counters alone; otherwise strict < , a win zeroes the counter
    int mine = 0;
    if (tid < NP) {
        const double c = L.NC[tid];
        int win = 1;
        if (!INIT) {
            win = c < L.EXC[tid];
            L.STAG[tid] = win ? 0. : L.STAG[tid] + 1.;
            S[MBX_GLPSO_ST_STAG(NP, D) + tid] = L.STAG[tid];
        }
        if (win) { L.EXC[tid] = c; S[MBX_GLPSO_ST_EXCOST(NP, D) + tid] = c; }
        L.FLAG[tid] = win;
        mine = L.STAG[tid] > kGlSg;
    }
    const int n_tour = __syncthreads_count(mine);
    // the exemplars after selection: winners' rows from X, the others' from HBM; staged in Z only when the tournament needs them
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e);
        if (L.FLAG[i]) gEX[e] = L.X[e];
        if (n_tour) L.Z[e] = L.FLAG[i] ? L.X[e] : gEX[e];
    }
    if (!n_tour) { __syncthreads(); return; }
    __syncthreads();
    // tournament (:49-57, 64-66): every row whose counter exceeds sg takes the exemplar with the lowest exemplar_cost among nsel random
    // rows (first on ties, np.argmin); exemplar_cost and the counter stay as they are (reference quirk)
    if (tid < NP) {
        int sel = -1;
        if (L.STAG[tid] > kGlSg) {
            double best = 0.;
            for (int j = 0; j < kGlNsel; ++j) {
                int c;
                if (xb) c = min(max((int)xb[MBX_GLPSO_XB_TOUR(NP, D) + tid * kGlNsel + j], 0), NP - 1);
                else { const U4 w = rng.draw((uint32_t)(tid * kGlNsel + j), MBX_SITE_GL_TOUR); c = (int)__umulhi(w.x, (uint32_t)NP); }
                if (j == 0 || L.EXC[c] < best) { best = L.EXC[c]; sel = c; }
            }
        }
        L.FLAG[tid] = sel;
    }
    __syncthreads();
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e), sel = L.FLAG[i];
        if (sel >= 0) L.X[e] = L.Z[sel * D + (e - i * D)];
    }
    __syncthreads();
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e);
        if (L.FLAG[i] >= 0) gEX[e] = L.X[e];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ reset (init_population :76-107)
__global__ __launch_bounds__(kThreads) void k_glpso_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const GpLds L = gp_carve(smem, NP, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_GLPSO_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub, vmax = kGlRho * (ub - lb);
    stage_problem(P, L.eval());
    for (int e = tid; e < NE; e += kThreads) {
        double up, uv;
        if (tape) { up = tape[MBX_GLPSO_TAPE_POS(NP, D) + e]; uv = tape[MBX_GLPSO_TAPE_VEL(NP, D) + e]; }
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); up = u53(w.x, w.y); uv = u53(w.z, w.w); }
        const double x = lb + (ub - lb) * up;
        L.X[e] = x;
        S[MBX_GLPSO_ST_X(NP, D) + e] = x;
        S[MBX_GLPSO_ST_PBPOS(NP, D) + e] = x;
        S[MBX_GLPSO_ST_V(NP, D) + e] = -vmax + (vmax - (-vmax)) * uv;
    }
    if (tid < NP) L.STAG[tid] = S[MBX_GLPSO_ST_STAG(NP, D) + tid];      // carried over from the previous episode (never reset, :19)
    __syncthreads();
    population_costs(P, L.eval(), NP, rng, tape ? tape + MBX_GLPSO_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    double gb; int g0;
    block_argmin(L.NC, NP, L.RED, gb, g0);
    if (tid < NP) { L.PBC[tid] = L.NC[tid]; S[MBX_GLPSO_ST_PBEST(NP, D) + tid] = L.NC[tid]; }
    if (tid < D) { L.GB[tid] = L.X[g0 * D + tid]; S[MBX_GLPSO_ST_GBPOS(NP, D) + tid] = L.X[g0 * D + tid]; }
    for (int e = tid; e < NE; e += kThreads) L.Z[e] = L.X[e];           // pbest_pos = the swarm
    __syncthreads();
    gp_exemplar<true>(P, L, NP, D, S, tape ? tape + MBX_GLPSO_TAPE_XB_INIT(NP, D) : nullptr, rng);
    if (tid == 0) {
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = 2 * NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = g0;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = (double)(2 * NP) / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ generation (__update :118-177)
__global__ __launch_bounds__(kThreads) void k_glpso_generation(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                               uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_GLPSO_ST_SCALARS(NP, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const GpLds L = gp_carve(smem, NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int gen = (int)sc[MBX_SC_GEN] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)(int)sc[MBX_SC_EPISODE]};
    const double lb = P.lb, ub = P.ub, vmax = kGlRho * (ub - lb);
    double* gX = S + MBX_GLPSO_ST_X(NP, D);
    double* gV = S + MBX_GLPSO_ST_V(NP, D);
    double* gPB = S + MBX_GLPSO_ST_PBPOS(NP, D);
    const double* gEX = S + MBX_GLPSO_ST_EX(NP, D);
    stage_problem(P, L.eval());
    // velocity and position (:121-130)
    for (int e = tid; e < NE; e += kThreads) {
        double r;
        if (tape) r = tape[MBX_GLPSO_TAPE_RAND(NP, D) + e];
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_A); r = u53(w.x, w.y); }
        const double x = gX[e];
        double v = kGlW * gV[e] + kGlC1 * r * (gEX[e] - x);
        v = fmin(fmax(v, -vmax), vmax);
        double nx = x + v;
        if (nx > ub) v = v * -0.5;
        if (nx < lb) v = v * -0.5;
        nx = fmin(fmax(nx, lb), ub);
        gV[e] = v; gX[e] = nx; L.X[e] = nx;
    }
    if (tid < NP) {
        L.PBC[tid] = S[MBX_GLPSO_ST_PBEST(NP, D) + tid];
        L.EXC[tid] = S[MBX_GLPSO_ST_EXCOST(NP, D) + tid];
        L.STAG[tid] = S[MBX_GLPSO_ST_STAG(NP, D) + tid];
    }
    if (tid < D) L.GB[tid] = S[MBX_GLPSO_ST_GBPOS(NP, D) + tid];
    __syncthreads();
    // evaluation of the swarm (:132); Z is the evaluator's scratch until it returns
    population_costs(P, L.eval(), NP, rng, tape ? tape + MBX_GLPSO_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B);
    // pbest (:134, 143-148, strict <) and gbest (:136-138, 149-154: first argmin, strict <)
    if (tid < NP) {
        const int impr = L.NC[tid] < L.PBC[tid];
        if (impr) { L.PBC[tid] = L.NC[tid]; S[MBX_GLPSO_ST_PBEST(NP, D) + tid] = L.NC[tid]; }
        L.FLAG[tid] = impr;
    }
    double cbv; int cb;
    block_argmin(L.NC, NP, L.RED, cbv, cb);                          // (its barriers publish L.FLAG / L.PBC)
    double gbest = sc[MBX_SC_GBEST];
    const bool gb_better = cbv < gbest;
    if (gb_better) gbest = cbv;
    if (gb_better && tid < D) { L.GB[tid] = L.X[cb * D + tid]; S[MBX_GLPSO_ST_GBPOS(NP, D) + tid] = L.X[cb * D + tid]; }
    // pbest_pos staged in Z for the crossover
    const FastDiv fd(D);
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e);
        if (L.FLAG[i]) { L.Z[e] = L.X[e]; gPB[e] = L.X[e]; }
        else L.Z[e] = gPB[e];
    }
    __syncthreads();
    gp_exemplar<false>(P, L, NP, D, S, tape ? tape + MBX_GLPSO_TAPE_XB(NP, D) : nullptr, rng);
    if (tid == 0) {
        // logging between the two evaluations (:160-162), termination after both (:168-176)
        const double fes1 = sc[MBX_SC_FES] + NP, fes = fes1 + NP;
        int log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
        double* cost = sc + MBX_NSCALAR;
        if (fes1 >= (double)log_index * bp.log_interval) { log_index += 1; if (cost_len <= bp.n_logpoint) curve_put(cost, bp.n_logpoint, cost_len++, gbest); }
        bool done = fes >= bp.max_fes;
        if (!isnan(P.optimum) && bp.early_stop) done = done || gbest <= 1e-8;
        if (done) {
            if (cost_len >= bp.n_logpoint + 1) curve_put(cost, bp.n_logpoint, cost_len - 1, gbest);
            else curve_put(cost, bp.n_logpoint, cost_len++, gbest);
        }
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = gen;
        if (gb_better) sc[MBX_SC_GBEST_IDX] = cb;
        if (state_out) state_out[b] = fes / bp.max_fes;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
