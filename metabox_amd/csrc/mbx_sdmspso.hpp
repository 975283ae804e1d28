// mbx_sdmspso.hpp — sDMS-PSO, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/sdms_pso.py:7-243).
//
// Dynamic multi-swarm PSO: NP = 99 particles in 33 sub-swarms of 3 (particle i belongs to sub-swarm i / 3), c1 = c2 = 1.49445, velocity cap
// 0.1 (ub - lb).  In the local phase (while fes < 0.95 maxFEs at the start of a generation) a particle is attracted by its pbest and by its
// sub-swarm's lbest, with one inertia weight per sub-swarm drawn afresh for every update (__get_iwt :128-133): uniform in [0.4, 0.9) until the
// parameter set holds LA = 8 weights and the running generation has counted more than LP = 10 successes, normal(median(parameter_set), 0.1)
// from then on.  A generation is LP = 10 updates; at its end the weight of the sub-swarm with the most successes enters the parameter set (a
// FIFO of 8, :185-191) and every R = 10th generation the swarm is regrouped by a random permutation (:87-96) with lbest found afresh.  In the
// global phase the attractor is gbest and the inertia weight is w, which fell by 0.5 / (maxFEs / NP) per local generation.
//
// No agent: mbx_reset is __reset, every mbx_step (actions = NULL) one __update -- 99 FEs -- and the launch that runs a generation's tenth update
// does the generation's epilogue as well and zeroes success_num for the next one.  The phase is decided where the reference decides it: at a
// generation boundary, from fes < 0.95 * maxFEs in double.  One workgroup per instance, dispatched through bp.order; the state block
// (include/mbx_layout.h §15) is streamed from HBM once per update.  lbest_pos and the per-sub-swarm weights are broadcast from LDS.  The regroup
// is a gather of five arrays by one permutation: the positions and the two cost vectors are gathered out of LDS (the evaluated rows are still
// there), the velocities and the pbest positions are staged through the evaluator's Z scratch one after the other; a thread writes only the
// HBM elements it has read itself.
//
// Quirks of the reference kept on purpose:
//  * no early stop: `done` is evaluated only after the global phase (:232-236), so the episode runs until fes >= maxFEs whatever gbest is and
//    fes overshoots maxFEs; the batch's early_stop flag has no effect on this algorithm;
//  * a generation's ten updates all run, whether or not fes crosses 0.95 maxFEs or maxFEs in between (:218-219);
//  * one cost.append per update at most (:178-180), even when fes has passed several log points;
//  * success counts pbest < lbest_cost against the lbest_cost of BEFORE the update (:120-124), for all three particles of the sub-swarm;
//  * argmin / argmax take the first index on ties (gbest, the sub-swarm's lbest, the arg-max of success_num);
//  * the regroup permutes c_cost too, and leaves gbest alone.
// Not carried: per_no_improve, lbest_no_improve, __regroup_index, __max_cost, __fes_eval (written, never read) and __quasi_Newton (:193-205), which
// runs only in generation 100 and fails there in the reference itself (self.__problem is never assigned): mbx_batch_create rejects a max_fes
// whose local phase reaches that generation.
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off); uniform(a, b) = a + (b - a) u,
// normal(loc, s) = loc + s z, the median of eight values = (a + b) / 2 of the two middle order statistics.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"

namespace mbx {

constexpr double kSdC1 = 1.49445, kSdC2 = 1.49445, kSdRho = 0.1;
constexpr int kSdNS = MBX_SDMS_NS, kSdM = MBX_SDMS_M, kSdLP = MBX_SDMS_LP, kSdLA = MBX_SDMS_LA, kSdR = MBX_SDMS_R;

// generations of the local phase of an episode with this budget (run_episode :209-226 on integers; the comparison is the reference's, in double)
__host__ __device__ inline int sd_local_generations(int max_fes)
{
    int g = 0;
    for (int64_t fes = MBX_SDMS_NP; g < MBX_SDMS_L && (double)fes < 0.95 * (double)max_fes; fes += (int64_t)MBX_SDMS_LP * MBX_SDMS_NP) ++g;
    return g;
}

// The LDS layout (SdLds, sd_lds_doubles, sd_carve) lives in mbx_lds.hpp.

// __random_regroup's permutation (:88) into L.PERM: new row k = old row PERM[k].  tp: the tape's perm slots (nullptr: Philox -- the rank of NP
// keys, the index breaking ties).  Ends with a barrier.
__device__ __forceinline__ void sd_permutation(const SdLds& L, int NP, const double* tp, const Rng& rng)
{
    const int tid = threadIdx.x;
    if (tp) {
        if (tid < NP) L.PERM[tid] = min(max((int)tp[tid], 0), NP - 1);              // (clamped: a tape is caller data)
        __syncthreads();
        return;
    }
    if (tid < NP) L.KEY[tid] = rng.draw((uint32_t)tid, MBX_SITE_SD_PERM).x;
    __syncthreads();
    if (tid < NP) {
        const uint32_t k = L.KEY[tid];
        int r = 0;
        for (int j = 0; j < NP; ++j) { const uint32_t o = L.KEY[j]; r += (o < k || (o == k && j < tid)) ? 1 : 0; }
        L.PERM[tid] = r;
    }
    __syncthreads();
}

// __update_lbest(init = True) (:99-106) on L.PBC, the pbest costs in their new order: lbest_cost / lbest_index per sub-swarm, first minimum.
// The lbest rows come from `pbpos`, the pbest positions in LDS in the order BEFORE the permutation L.PERM.  Ends with a barrier.
__device__ __forceinline__ void sd_lbest_init(const SdLds& L, int NP, int D, double* S, const double* pbpos)
{
    const int tid = threadIdx.x;
    if (tid < kSdNS) {
        double m = L.PBC[tid * kSdM]; int idx = 0;
        for (int j = 1; j < kSdM; ++j) { const double v = L.PBC[tid * kSdM + j]; if (v < m) { m = v; idx = j; } }
        L.LBC[tid] = m; L.LBI[tid] = tid * kSdM + idx;
        S[MBX_SDMS_ST_LBCOST(NP, D) + tid] = m; S[MBX_SDMS_ST_LBIDX(NP, D) + tid] = tid * kSdM + idx;
    }
    __syncthreads();
    const FastDiv fd(D);
    for (int e = tid; e < kSdNS * D; e += kThreads) {
        const int s = fd.div(e);
        S[MBX_SDMS_ST_LBPOS(NP, D) + e] = pbpos[L.PERM[L.LBI[s]] * D + (e - s * D)];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ reset (__reset :68-85, __initilize :45-66)
__global__ __launch_bounds__(kThreads) void k_sdmspso_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const SdLds L = sd_carve(smem, NP, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_SDMS_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub, vmax = kSdRho * (ub - lb);
    const FastDiv fd(D);
    stage_problem(P, L.eval());
    for (int e = tid; e < NE; e += kThreads) {
        double up;
        if (tape) up = tape[MBX_SDMS_TAPE_POS(NP, D) + e];
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); up = u53(w.x, w.y); }
        L.X[e] = lb + (ub - lb) * up;
    }
    __syncthreads();
    population_costs(P, L.eval(), NP, rng, tape ? tape + MBX_SDMS_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_SD_NOISE_A, MBX_SITE_SD_NOISE_B);
    double gb; int g0;
    block_argmin(L.NC, NP, L.RED, gb, g0);
    if (tid < D) S[MBX_SDMS_ST_GBPOS(NP, D) + tid] = L.X[g0 * D + tid];
    // __random_regroup (:80): positions, costs and velocities move together; a velocity is a function of its own uniform, so it is made in place
    sd_permutation(L, NP, tape ? tape + MBX_SDMS_TAPE_PERM_INIT(NP, D) : nullptr, rng);
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e), src = L.PERM[i] * D + (e - i * D);
        double uv;
        if (tape) uv = tape[MBX_SDMS_TAPE_VEL(NP, D) + src];
        else { const U4 w = rng.draw((uint32_t)src, MBX_SITE_ELEM_R); uv = u53(w.z, w.w); }
        const double x = L.X[src];
        S[MBX_SDMS_ST_X(NP, D) + e] = x;
        S[MBX_SDMS_ST_PBPOS(NP, D) + e] = x;
        S[MBX_SDMS_ST_V(NP, D) + e] = -vmax + (vmax - (-vmax)) * uv;
    }
    if (tid < NP) {
        const double c = L.NC[L.PERM[tid]];
        L.PBC[tid] = c;
        S[MBX_SDMS_ST_CCOST(NP, D) + tid] = c; S[MBX_SDMS_ST_PBEST(NP, D) + tid] = c;
    }
    if (tid < kSdNS) {
        S[MBX_SDMS_ST_SUCC(NP, D) + tid] = 0.; S[MBX_SDMS_ST_SUCC_LAST(NP, D) + tid] = 0.;
        S[MBX_SDMS_ST_IWT(NP, D) + tid] = 0.; S[MBX_SDMS_ST_IWT_Z(NP, D) + tid] = 0.;
    }
    if (tid < kSdLA) S[MBX_SDMS_ST_PSET(NP, D) + tid] = 0.;
    __syncthreads();
    sd_lbest_init(L, NP, D, S, L.X);
    if (tid == 0) {
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_SDMS_W] = 0.9;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = (double)NP / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ update (__update :135-183 + run_episode's loop body :211-230)
__global__ __launch_bounds__(kThreads) void k_sdmspso_update(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                             uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_SDMS_ST_SCALARS(NP, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const SdLds L = sd_carve(smem, NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int step = (int)sc[MBX_SC_GEN] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(int)sc[MBX_SC_EPISODE]};
    const double lb = P.lb, ub = P.ub, vmax = kSdRho * (ub - lb);
    const FastDiv fd(D);
    // every scalar is read here, before the first barrier; thread 0 writes them back after the last one
    const double fes0 = sc[MBX_SC_FES];
    double gbest = sc[MBX_SC_GBEST], w = sc[MBX_SC_SDMS_W];
    int mode = (int)sc[MBX_SC_SDMS_MODE], rgen = (int)sc[MBX_SC_SDMS_GEN], npar = min(max((int)sc[MBX_SC_SDMS_NPAR], 0), kSdLA);   // (clamped: mbx_debug_write_state is caller data)
    const int sip = (int)sc[MBX_SC_SDMS_STEP];
    // a generation boundary (:209-217): the phase is decided here and nowhere else; the global phase never returns to the local one
    if (mode == 0 && sip == 0) {
        if (fes0 < 0.95 * (double)bp.max_fes) { rgen += 1; w -= 0.5 / ((double)bp.max_fes / (double)NP); }
        else mode = 1;
    }
    const bool ls = mode == 0;
    double* gX = S + MBX_SDMS_ST_X(NP, D);
    double* gV = S + MBX_SDMS_ST_V(NP, D);
    double* gPB = S + MBX_SDMS_ST_PBPOS(NP, D);
    stage_problem(P, L.eval());
    // __get_iwt (:128-133): one weight per sub-swarm, from the success count and the parameter set as they stand before this update
    int iwt_mode = 2;
    if (ls) {
        double total = 0.;
        for (int s = 0; s < kSdNS; ++s) total += S[MBX_SDMS_ST_SUCC(NP, D) + s];
        iwt_mode = (npar < kSdLA || total <= (double)kSdLP) ? 0 : 1;
    }
    if (tid < kSdNS) {
        L.LBC[tid] = S[MBX_SDMS_ST_LBCOST(NP, D) + tid];
        L.SUC[tid] = S[MBX_SDMS_ST_SUCC(NP, D) + tid];
        L.LBI[tid] = (int)S[MBX_SDMS_ST_LBIDX(NP, D) + tid];
        if (iwt_mode == 0) {
            double u;
            if (tape) u = tape[MBX_SDMS_TAPE_IWT_U(NP, D) + tid];
            else { const U4 r = rng.draw((uint32_t)tid, MBX_SITE_SD_IWT_U); u = u53(r.x, r.y); }
            const double v = 0.5 * u + 0.4;
            L.IWT[tid] = v; S[MBX_SDMS_ST_IWT(NP, D) + tid] = v;
        } else if (iwt_mode == 1) {
            // np.median of the eight entries: the mean of the two middle order statistics
            double a[kSdLA];
            for (int k = 0; k < kSdLA; ++k) a[k] = S[MBX_SDMS_ST_PSET(NP, D) + k];
            for (int k = 1; k < kSdLA; ++k)
                for (int j = k; j > 0; --j) { const double lo = fmin(a[j - 1], a[j]), hi = fmax(a[j - 1], a[j]); a[j - 1] = lo; a[j] = hi; }
            const double med = (a[kSdLA / 2 - 1] + a[kSdLA / 2]) / 2.;
            double z;
            if (tape) z = tape[MBX_SDMS_TAPE_IWT_Z(NP, D) + tid];
            else { const U4 r = rng.draw((uint32_t)tid, MBX_SITE_SD_IWT_Z); z = sqrt(-2.0 * m_log(1.0 - u53(r.x, r.y))) * m_cos(kTwoPi * u53(r.z, r.w)); }
            const double v = med + 0.1 * z;
            L.IWT[tid] = v; S[MBX_SDMS_ST_IWT(NP, D) + tid] = v; S[MBX_SDMS_ST_IWT_Z(NP, D) + tid] = z;
        } else
            L.IWT[tid] = S[MBX_SDMS_ST_IWT(NP, D) + tid];
    }
    if (tid < NP) {
        L.PBC[tid] = S[MBX_SDMS_ST_PBEST(NP, D) + tid];
        if (tape) { L.R1[tid] = tape[MBX_SDMS_TAPE_RAND1(NP, D) + tid]; L.R2[tid] = tape[MBX_SDMS_TAPE_RAND2(NP, D) + tid]; }
        else { const U4 r = rng.draw((uint32_t)tid, MBX_SITE_SD_PART); L.R1[tid] = u53(r.x, r.y); L.R2[tid] = u53(r.z, r.w); }
    }
    // the attractors: lbest rows in the local phase, the gbest row (in row 0's place) in the global one
    if (ls) for (int e = tid; e < kSdNS * D; e += kThreads) L.LBP[e] = S[MBX_SDMS_ST_LBPOS(NP, D) + e];
    if (tid < D) L.GB[tid] = S[MBX_SDMS_ST_GBPOS(NP, D) + tid];
    __syncthreads();
    // velocity and position (:136-150)
    for (int e = tid; e < NE; e += kThreads) {
        const int i = fd.div(e), d = e - i * D, g = i / kSdM;
        const double x = gX[e];
        const double vp = L.R1[i] * (gPB[e] - x);
        double v;
        if (ls) v = L.IWT[g] * gV[e] + kSdC1 * vp + kSdC2 * (L.R2[i] * (L.LBP[g * D + d] - x));
        else v = w * gV[e] + kSdC1 * vp + kSdC2 * (L.R2[i] * (L.GB[d] - x));
        v = fmin(fmax(v, -vmax), vmax);
        const double nx = fmin(fmax(x + v, lb), ub);
        gV[e] = v; gX[e] = nx; L.X[e] = nx;
    }
    __syncthreads();
    // evaluation (:151); Z is the evaluator's scratch until it returns
    population_costs(P, L.eval(), NP, rng, tape ? tape + MBX_SDMS_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_SD_NOISE_A, MBX_SITE_SD_NOISE_B);
    // pbest (:152, 160-165, strict <) and gbest (:153-156, 167-172: first argmin, strict <)
    if (tid < NP) {
        const double c = L.NC[tid];
        const int impr = c < L.PBC[tid];
        if (impr) { L.PBC[tid] = c; S[MBX_SDMS_ST_PBEST(NP, D) + tid] = c; }
        S[MBX_SDMS_ST_CCOST(NP, D) + tid] = c;
        L.FLAG[tid] = impr;
    }
    double cbv; int cb;
    block_argmin(L.NC, NP, L.RED, cbv, cb);                          // (its barriers publish L.FLAG / L.PBC)
    const bool gb_better = cbv < gbest;
    if (gb_better) gbest = cbv;
    if (gb_better && tid < D) S[MBX_SDMS_ST_GBPOS(NP, D) + tid] = L.X[cb * D + tid];
    for (int e = tid; e < NE; e += kThreads) if (L.FLAG[fd.div(e)]) gPB[e] = L.X[e];
    const bool period_end = ls && sip + 1 == kSdLP;
    const bool regroup = period_end && rgen % kSdR == 0;
    if (ls) {
        // __update_lbest (:109-125): success counts against the lbest_cost of before this update, then lbest is replaced by strict <
        if (tid < kSdNS) {
            const double old = L.LBC[tid];
            double m = L.PBC[tid * kSdM]; int idx = 0, succ = m < old;
            for (int j = 1; j < kSdM; ++j) { const double v = L.PBC[tid * kSdM + j]; succ += v < old; if (v < m) { m = v; idx = j; } }
            const double total = L.SUC[tid] + (double)succ;
            L.SUC[tid] = total;
            int won = -1;
            if (m < old) {
                won = tid * kSdM + idx;
                L.LBC[tid] = m; L.LBI[tid] = won;
                S[MBX_SDMS_ST_LBCOST(NP, D) + tid] = m; S[MBX_SDMS_ST_LBIDX(NP, D) + tid] = won;
            }
            L.SWF[tid] = won;
            if (period_end) { S[MBX_SDMS_ST_SUCC_LAST(NP, D) + tid] = total; S[MBX_SDMS_ST_SUCC(NP, D) + tid] = 0.; }   // zeroed for the next generation (:217)
            else S[MBX_SDMS_ST_SUCC(NP, D) + tid] = total;
        }
        __syncthreads();
        // the new lbest rows; a regroup finds every one of them afresh below.  (the row is the particle's pbest position: this update's, still in
        // X, if it improved now -- its HBM copy is being written by other threads -- and the stored one otherwise)
        if (!regroup)
            for (int e = tid; e < kSdNS * D; e += kThreads) {
                const int s = fd.div(e), i = L.SWF[s];
                if (i >= 0) { const int src = i * D + (e - s * D); S[MBX_SDMS_ST_LBPOS(NP, D) + e] = L.FLAG[i] ? L.X[src] : gPB[src]; }
            }
    }
    if (regroup) {
        // __random_regroup (:87-96) + __update_lbest(init = True): five arrays by one permutation
        sd_permutation(L, NP, tape ? tape + MBX_SDMS_TAPE_PERM(NP, D) : nullptr, rng);
        double cc = 0., pb = 0.;
        if (tid < NP) { cc = L.NC[L.PERM[tid]]; pb = L.PBC[L.PERM[tid]]; }
        for (int e = tid; e < NE; e += kThreads) L.Z[e] = gV[e];                                 // the velocities, staged
        __syncthreads();
        if (tid < NP) { L.PBC[tid] = pb; S[MBX_SDMS_ST_CCOST(NP, D) + tid] = cc; S[MBX_SDMS_ST_PBEST(NP, D) + tid] = pb; }
        for (int e = tid; e < NE; e += kThreads) {
            const int i = fd.div(e), src = L.PERM[i] * D + (e - i * D);
            gV[e] = L.Z[src];
        }
        __syncthreads();
        for (int e = tid; e < NE; e += kThreads) L.Z[e] = L.FLAG[fd.div(e)] ? L.X[e] : gPB[e];     // the pbest positions, staged
        __syncthreads();
        for (int e = tid; e < NE; e += kThreads) {
            const int i = fd.div(e), src = L.PERM[i] * D + (e - i * D);
            gPB[e] = L.Z[src]; gX[e] = L.X[src];
        }
        sd_lbest_init(L, NP, D, S, L.Z);
    }
    if (tid == 0) {
        if (period_end) {
            // __update_parameter_set (:185-191): the weight of the sub-swarm with the most successes (first maximum) enters the FIFO
            int am = 0;
            for (int s = 1; s < kSdNS; ++s) if (L.SUC[s] > L.SUC[am]) am = s;
            double* ps = S + MBX_SDMS_ST_PSET(NP, D);
            if (npar < kSdLA) ps[npar++] = L.IWT[am];
            else { for (int k = 0; k + 1 < kSdLA; ++k) ps[k] = ps[k + 1]; ps[kSdLA - 1] = L.IWT[am]; }
        }
        // logging (:178-180, one append per update at most) and termination (:228-241: after a whole generation or a global update only)
        const double fes = fes0 + NP;
        int log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
        double* cost = sc + MBX_NSCALAR;
        if (fes >= (double)log_index * bp.log_interval) { log_index += 1; if (cost_len <= bp.n_logpoint) curve_put(cost, bp.n_logpoint, cost_len++, gbest); }
        const bool done = fes >= bp.max_fes && (!ls || period_end);
        if (done) {
            if (cost_len >= bp.n_logpoint + 1) curve_put(cost, bp.n_logpoint, cost_len - 1, gbest);
            else curve_put(cost, bp.n_logpoint, cost_len++, gbest);
        }
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = step;
        sc[MBX_SC_SDMS_STEP] = ls ? (sip + 1) % kSdLP : 0; sc[MBX_SC_SDMS_MODE] = mode; sc[MBX_SC_SDMS_W] = w; sc[MBX_SC_SDMS_NPAR] = npar;
        sc[MBX_SC_SDMS_IWTMODE] = iwt_mode; sc[MBX_SC_SDMS_GEN] = rgen;
        if (state_out) state_out[b] = fes / bp.max_fes;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
