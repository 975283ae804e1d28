// mbx_nrlpso.hpp — NRLPSO step kernels for gfx950 (reference: src/optimizer/nrlpso_optimizer.py:7-296 and the tabular policy of
// src/agent/nrlpso_agent.py:28-31; layout, quirks and Philox sites: include/mbx_layout.h section 16).
//
// One env step moves ONE particle `pointer` of a swarm of NP (the reference: 100): the cosine similarity cs of its pbest and gbest picks the
// velocity rule of the action, the particle moves, is evaluated, and the reward in {2, 1, 0, -2} combines `f_new < f_old` with
// `ef_new > ef_old`, where ef = (distance[pointer] - d_min) / (d_max - d_min) and distance[i] is the mean distance of particle i to the others
// (cal_ef :110-122).  The reference computes the NP x NP distance matrix from scratch for each ef, twice per step.  Only one row of the population
// moves per step (one or two more when neb_mutation :204-239 replaces rows), so the cached form keeps the symmetric matrix in LDS, rewrites the row
// and the column of every changed particle and RE-SUMS every row mean from LDS in numpy's pairwise order -- the means, d_min and d_max are then
// bit for bit those of a from-scratch update_distance, and the ef_old of a step is what the previous step left unless a mutation came between.
// The recompute form (MBX_F_NRLPSO_RECOMPUTE, or where the matrix does not fit the LDS) does what the reference does.  Matrix rows are NP | 1
// doubles apart: the re-summation walks one row per lane, and ds_read_b64 banks are (address / 4) % 64 over 32 lanes, so an odd stride in doubles
// is conflict-free where a stride of 100 would be 4-way.
// Measured (docs/EXPERIMENTS.md, us per env step, resident, NP = 100): cached 217.5 against recompute 758.5 at D = 10 / 4096 instances, 83.6 against 467.2 at
// D = 30 / 1024 instances, although the cached form's 112-160 KB of LDS hold one workgroup per CU: cached is the default wherever it fits.
//
// One instance per workgroup of 256 threads.  Population and pbest positions stay in LDS for every step of a launch; velocities and the sweep-start
// snapshot are touched one row per step and stay in the state block.  k_nrlpso_step<false> (one step) and <true> (the n_steps loop) are one body.
// Every operation outside the objective is + - * /, sqrt and clip, in numpy's order (np.sum: mbx_npsum.hpp), with -ffp-contract=off.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams, log_and_terminate
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"
#include "mbx_qchoose.hpp"

namespace mbx {

// per-step records of the multi-step kernel (each may be nullptr) and the last action of every instance
struct NrTraj { int32_t* actions; double* state; double* reward; int32_t* last_action; };

// The LDS layout (NrLds, kNrK, nr_stride, nr_lds_doubles, nr_carve) lives in mbx_lds.hpp.

// sqrt(np.sum((a - b) ** 2, -1)) of two rows
static_assert(MBX_NRLPSO_DIM_MAX <= 128 && MBX_NRLPSO_NP_MAX <= 128, "np_sum_block is numpy's order for n <= 128: the D and NP sums of this file rest on nrlpso_check's limits");
__device__ __forceinline__ double nr_dist(const double* a, const double* b, int D)
{
    return sqrt(np_sum_block([&](int d) { const double t = a[d] - b[d]; return t * t; }, D));
}

// row r and column r of the distance matrix from the population in L.POP (lanes j < NP).  No barrier.
__device__ __forceinline__ void nr_dm_row(const NrLds& L, int NP, int D, int r)
{
    const int j = threadIdx.x, S = nr_stride(NP);
    if (j < NP) {
        const double d = nr_dist(L.POP + j * D, L.POP + r * D, D);
        L.DM[r * S + j] = d; L.DM[j * S + r] = d;
    }
}

// update_distance (:114-122): distance[i] = np.sum(matrix[i], -1) / (NP - 1) into L.DIST, d_min / d_max into L.RED[0 / 1].  cached: the matrix
// is in L.DM; otherwise every lane computes its row of distances as it sums them.  All threads call; ends with a barrier.
__device__ __forceinline__ void nr_distances(const NrLds& L, int NP, int D, bool cached)
{
    const int tid = threadIdx.x, S = nr_stride(NP);
    if (tid < NP) {
        double s;
        if (cached) { const double* row = L.DM + tid * S; s = np_sum_block([&](int j) { return row[j]; }, NP); }
        else { const double* x = L.POP + tid * D; s = np_sum_block([&](int j) { return nr_dist(L.POP + j * D, x, D); }, NP); }
        L.DIST[tid] = s / (double)(NP - 1);
    }
    __syncthreads();
    if (tid < 64) {
        double lo = INFINITY, hi = -INFINITY;
        for (int i = tid; i < NP; i += 64) { lo = fmin(lo, L.DIST[i]); hi = fmax(hi, L.DIST[i]); }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off, 64)); hi = fmax(hi, __shfl_xor(hi, off, 64)); }
        if (tid == 0) { L.RED[0] = lo; L.RED[1] = hi; }
    }
    __syncthreads();
}

// argsort of the five distances in L.TMP (:208, :226; insertion sort below 17 elements: stable): first = sort_idx[0], last = sort_idx[-1]
__device__ __forceinline__ void nr_first_last(const double* t, int& first, int& last)
{
    first = 0; last = 0;
    for (int r = 1; r < kNrK; ++r) { if (t[r] < t[first]) first = r; if (!(t[r] < t[last])) last = r; }
}

// ------------------------------------------------------------------------------------------------ reset (init_population :30-59)
__global__ __launch_bounds__(kThreads) void k_nrlpso_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const NrLds L = nr_carve(smem, NP, NP, D, false, false);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_NRLPSO_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(L.X, L.COST));
    for (int e = tid; e < NE; e += kThreads) {
        double u;
        if (tape) u = tape[MBX_NRLPSO_TAPE_POS(NP, D) + e];
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_LDE_ELEM); u = u53(w.x, w.y); }
        const double x = u * (ub - lb) + lb;
        L.X[e] = x;
        S[MBX_NRLPSO_ST_POP(NP, D) + e] = x; S[MBX_NRLPSO_ST_PBPOS(NP, D) + e] = x; S[MBX_NRLPSO_ST_SNAP(NP, D) + e] = x;
        S[MBX_NRLPSO_ST_VEL(NP, D) + e] = 0.;
    }
    __syncthreads();
    population_costs(P, L.eval(L.X, L.COST), NP, rng, tape ? tape + MBX_NRLPSO_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    for (int i = tid; i < NP; i += kThreads) {
        const double f = L.COST[i];
        S[MBX_NRLPSO_ST_COST(NP, D) + i] = f; S[MBX_NRLPSO_ST_PBCOST(NP, D) + i] = f; S[MBX_NRLPSO_ST_STAG(NP, D) + i] = 0.;
        double s0;
        if (tape) s0 = fmin(fmax(tape[MBX_NRLPSO_TAPE_SSTATE(NP, D) + i], 0.), 3.);
        else { const U4 w = rng.draw((uint32_t)i, MBX_SITE_NR_INIT); s0 = (double)__umulhi(w.x, 4u); }
        S[MBX_NRLPSO_ST_SSTATE(NP, D) + i] = s0;
        if (i == 0 && state_out) state_out[b] = s0;                  // the pointer starts at 0 (:31)
    }
    for (int e = tid; e < kNrK * NP + 8; e += kThreads) S[MBX_NRLPSO_ST_PNIDX(NP, D) + e] = 0.;      // both index lists
    if (tid < MBX_NRLPSO_DIAG_SLOTS) S[MBX_NRLPSO_ST_DIAG(NP, D) + tid] = 0.;
    double gb; int g0;
    block_argmin(L.COST, NP, L.RED, gb, g0);
    if (tid < D) S[MBX_NRLPSO_ST_GBPOS(NP, D) + tid] = L.X[g0 * D + tid];
    if (tid == 0) {
        double rw;
        if (tape) rw = tape[MBX_NRLPSO_TAPE_RW(NP, D)];
        else { const U4 w = rng.draw((uint32_t)NP, MBX_SITE_NR_INIT); rw = u53(w.x, w.y); }
        for (int k = 0; k < MBX_NSCALAR; ++k) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = g0; sc[MBX_SC_NRLPSO_G0] = g0; sc[MBX_SC_NRLPSO_ALIAS] = 1.; sc[MBX_SC_NRLPSO_RW] = rw;
        sc[MBX_NSCALAR] = gb;
    }
}

// ------------------------------------------------------------------------------------------------ step (update :241-296)
// MULTI = false: exactly one step (mbx_step, or a one-step rollout); MULTI = true: the n_steps loop.  actions == nullptr: the policy decides.
template <bool MULTI>
__device__ __forceinline__ void nr_steps(const BatchParams& bp, const int32_t* __restrict__ actions, const double* __restrict__ q_table, int n_steps,
                                         int cached_arg, const NrTraj& traj, double* __restrict__ state_out, double* __restrict__ reward_out,
                                         uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, NE = NP * D;
    const bool cached = cached_arg != 0;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_NRLPSO_ST_SCALARS(NP, D);
    if (sc[MBX_SC_DONE] != 0.) {                                     // a finished instance stays frozen: the outputs repeat what its last step left
        if (tid == 0) {
            if (reward_out) reward_out[b] = 0.;
            if (done_out) done_out[b] = 1;
            if (state_out) state_out[b] = S[MBX_NRLPSO_ST_SSTATE(NP, D) + min(max((int)sc[MBX_SC_NRLPSO_POINTER], 0), NP - 1)];
            if (traj.last_action) traj.last_action[b] = (int)S[MBX_NRLPSO_ST_DIAG(NP, D) + MBX_NRLPSO_DIAG_ACTION];
        }
        return;
    }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const NrLds L = nr_carve(smem, 1, NP, D, true, cached);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const double lb = P.lb, ub = P.ub, vmax = -(-0.1 * (ub - lb));       // v_min = -0.1 (ub - lb), v_max = -v_min (:35-36)
    double* gVel = S + MBX_NRLPSO_ST_VEL(NP, D);
    double* gSnap = S + MBX_NRLPSO_ST_SNAP(NP, D);

    stage_problem(P, L.eval(L.X, L.NC));
    for (int e = tid; e < NE; e += kThreads) { L.POP[e] = S[MBX_NRLPSO_ST_POP(NP, D) + e]; L.PB[e] = S[MBX_NRLPSO_ST_PBPOS(NP, D) + e]; }
    for (int i = tid; i < NP; i += kThreads) {
        L.COST[i] = S[MBX_NRLPSO_ST_COST(NP, D) + i]; L.PBCOST[i] = S[MBX_NRLPSO_ST_PBCOST(NP, D) + i];
        L.STAG[i] = S[MBX_NRLPSO_ST_STAG(NP, D) + i]; L.SS[i] = S[MBX_NRLPSO_ST_SSTATE(NP, D) + i];
    }
    for (int e = tid; e < kNrK * NP; e += kThreads) L.PNI[e] = min(max((int)S[MBX_NRLPSO_ST_PNIDX(NP, D) + e], 0), NP - 1);   // an injected block cannot send a read outside
    if (tid < kNrK) L.GNI[tid] = min(max((int)S[MBX_NRLPSO_ST_GNIDX(NP, D) + tid], 0), NP - 1);
    if (tid < D) L.GB[tid] = S[MBX_NRLPSO_ST_GBPOS(NP, D) + tid];
    if (tid < MBX_NSCALAR) L.SC[tid] = sc[tid];
    if (tid < MBX_NRLPSO_DIAG_SLOTS) L.DG[tid] = S[MBX_NRLPSO_ST_DIAG(NP, D) + tid];
    __syncthreads();
    bool stale = true;                                               // L.DIST / d_min / d_max do not describe L.POP
    if (cached) {
        const int S2 = nr_stride(NP);
        for (int e = tid; e < NP * NP; e += kThreads) { const int i = e / NP, j = e - i * NP; L.DM[i * S2 + j] = nr_dist(L.POP + j * D, L.POP + i * D, D); }
        __syncthreads();
    }
    const int episode = (int)L.SC[MBX_SC_EPISODE];
    double reward_sum = 0.;
    int done = 0, last_action = 0;
    for (int it = 0; it < (MULTI ? n_steps : 1) && !done; ++it) {
        const int step = (int)L.SC[MBX_SC_GEN] + 1, p = min(max((int)L.SC[MBX_SC_NRLPSO_POINTER], 0), NP - 1);
        const int g0 = min(max((int)L.SC[MBX_SC_NRLPSO_G0], 0), NP - 1);
        const bool alias = L.SC[MBX_SC_NRLPSO_ALIAS] != 0.;
        const double* gpos = alias ? L.POP + g0 * D : L.GB;          // gbest_pos: the view of a row, or the array of its own
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)episode, true};
        if (tid == 0) {                                              // decision, the scalar draws (:138-139, :128, :132), cal_cs (:124-125)
            int action;
            if (!actions) {
                double u;
                if (tape) u = tape[MBX_NRLPSO_TAPE_CHOICE(NP, D)];
                else { const U4 w = rng.draw(0u, MBX_SITE_POLICY); u = u53(w.x, w.y); }
                action = ql_choose(q_table + 4 * min(max((int)L.SS[p], 0), 3), u);
            } else action = actions[b];
            double r1, r2; int ib, ia;
            if (tape) {
                r1 = tape[MBX_NRLPSO_TAPE_RAND(NP, D)]; r2 = tape[MBX_NRLPSO_TAPE_RAND(NP, D) + 1];
                ib = (int)tape[MBX_NRLPSO_TAPE_IDX(NP, D)]; ia = (int)tape[MBX_NRLPSO_TAPE_IDX(NP, D) + 1];
            } else {
                const U4 w = rng.draw(0u, MBX_SITE_NR_PART), v = rng.draw(1u, MBX_SITE_NR_PART);
                r1 = u53(w.x, w.y); r2 = u53(w.z, w.w); ib = (int)__umulhi(v.x, (uint32_t)kNrK); ia = (int)__umulhi(v.y, (uint32_t)kNrK);
            }
            const double* pb = L.PB + p * D;
            const double num = np_sum_block([&](int d) { return pb[d] * gpos[d]; }, D);
            const double na = sqrt(np_sum_block([&](int d) { return pb[d] * pb[d]; }, D)), nb = sqrt(np_sum_block([&](int d) { return gpos[d] * gpos[d]; }, D));
            L.RED[8] = action; L.RED[9] = r1; L.RED[10] = r2; L.RED[11] = min(max(ib, 0), kNrK - 1); L.RED[12] = min(max(ia, 0), kNrK - 1);
            L.RED[13] = num / (na * nb);
        }
        if (p == 0) {                                                // update_construct_neighborhood (:62-85), cal_w (:88-93)
            for (int e = tid; e < NE; e += kThreads) gSnap[e] = L.POP[e];
            if (tid < NP) {
                const double* x = L.POP + tid * D;
                double bd[kNrK]; int bi[kNrK];
#pragma unroll
                for (int k = 0; k < kNrK; ++k) { bd[k] = INFINITY; bi[k] = 0; }
                for (int j = 0; j < NP; ++j) {
                    const double d = j == tid ? INFINITY : nr_dist(L.PB + j * D, x, D);
                    if (d < bd[kNrK - 1]) {                          // ascending j and strict comparisons: ties go to the lower index
                        bd[kNrK - 1] = d; bi[kNrK - 1] = j;
#pragma unroll
                        for (int k = kNrK - 1; k > 0; --k)
                            if (bd[k] < bd[k - 1]) { const double td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td; const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti; }
                    }
                }
#pragma unroll
                for (int k = 0; k < kNrK; ++k) L.PNI[tid * kNrK + k] = bi[k];
                L.TMP[tid] = nr_dist(gpos, x, D);
            }
            __syncthreads();
            if (tid < NP) {
                const double di = L.TMP[tid];
                int rank = 0;
                for (int j = 0; j < NP; ++j) { const double dj = L.TMP[j]; rank += (dj < di) || (dj == di && j < tid); }
                if (rank < kNrK) L.GNI[rank] = tid;
            }
            if (tid == 0) {
                const double rw = 4 * L.SC[MBX_SC_NRLPSO_RW] * (1 - L.SC[MBX_SC_NRLPSO_RW]), q = L.SC[MBX_SC_FES] / (double)bp.max_fes;
                L.SC[MBX_SC_NRLPSO_RW] = rw;
                L.SC[MBX_SC_NRLPSO_W] = 0.6 - (q * rw * 0.4 + 0.33 * (1. - 0.4) * q);
            }
        }
        __syncthreads();
        // ---- generate_v_vector (:136-194): left to right as numpy evaluates it
        const int action = (int)L.RED[8];
        last_action = action;
        double nv = 0., x = 0.;
        if (tid < D) {
            const int d = tid, e = p * D + d, ib = (int)L.RED[11], ia = (int)L.RED[12];
            const bool neg = L.RED[13] < 0.;
            double r1 = L.RED[9], r2 = L.RED[10];
            x = L.POP[e];
            const double v = gVel[e], w = L.SC[MBX_SC_NRLPSO_W], pbv = L.PB[e], gv = gpos[d];
            const double pbn = gSnap[L.PNI[p * kNrK + ib] * D + d], gbn = gSnap[L.GNI[ia] * D + d];     // get_p_b / get_p_a: rows of the sweep-start copies
            double c1 = 0., c2 = 0., P1 = 0., P2 = 0.;
            bool t1 = false, t2 = false;
            if (action == 0) { c1 = 2.2; c2 = 1.8; if (neg) { P1 = pbv; P2 = gbn; t1 = t2 = true; } else { P1 = pbn; t1 = true; } }
            else if (action == 1) { c1 = 2.1; c2 = 1.8; if (neg) { P1 = pbn; P2 = gv; t1 = t2 = true; } else { P2 = gbn; t2 = true; } }
            else if (action == 2) { c1 = 2.; c2 = 2.; if (neg) { P1 = pbv; P2 = gv; t1 = t2 = true; } else { P2 = gv; t2 = true; } }
            else if (action == 3) {
                c1 = 1.8; c2 = 2.2; P1 = pbn; P2 = gbn; t1 = t2 = true;
                if (tape) { r1 = tape[MBX_NRLPSO_TAPE_R1V(NP, D) + d]; r2 = tape[MBX_NRLPSO_TAPE_R2V(NP, D) + d]; }
                else { const U4 u = rng.draw((uint32_t)d, MBX_SITE_NR_ELEM); r1 = u53(u.x, u.y); r2 = u53(u.z, u.w); }
            }
            nv = v;
            if (t1 || t2) nv = w * v;
            if (t1) nv = nv + (c1 * r1) * (P1 - x);
            if (t2) nv = nv + (c2 * r2) * (P2 - x);
            nv = fmin(fmax(nv, -vmax), vmax);
            gVel[e] = nv;
        }
        // ---- ef_old (:250): what the previous step left, unless it is stale
        if (stale) nr_distances(L, NP, D, cached);
        if (tid == 0) L.RED[14] = (L.DIST[p] - L.RED[0]) / (L.RED[1] - L.RED[0]);
        __syncthreads();
        if (tid < D) {                                               // :252-253
            const double nx = fmin(fmax(x + nv, lb), ub);
            L.POP[p * D + tid] = nx; L.X[tid] = nx;
        }
        __syncthreads();
        // ---- ef_new (:255)
        if (cached) { nr_dm_row(L, NP, D, p); __syncthreads(); }
        nr_distances(L, NP, D, cached);
        stale = !cached;
        if (tid == 0) L.RED[15] = (L.DIST[p] - L.RED[0]) / (L.RED[1] - L.RED[0]);
        {
            const RowPost post{&rng, tape ? tape + MBX_NRLPSO_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_NR_NOISE_A, MBX_SITE_NR_NOISE_B, 3, 0};
            eval_rows(P, L.eval(L.X, L.NC), 1, &post);
        }
        if (tid == 0) {                                              // :256-269
            const double f_new = L.NC[0], f_old = L.COST[p], ef_new = L.RED[15], ef_old = L.RED[14];
            const bool c1 = f_new < f_old, c2 = ef_new > ef_old;
            L.RED[18] = c1 ? (c2 ? 2. : 1.) : (c2 ? 0. : -2.);
            L.COST[p] = f_new;
            const bool improved = f_new < L.PBCOST[p];
            L.STAG[p] = improved ? 0. : L.STAG[p] + 1.;
            L.RED[16] = improved; L.RED[17] = L.STAG[p] >= 2.; L.RED[19] = f_new;
            L.DG[MBX_NRLPSO_DIAG_PMCOST] = 0.; L.DG[MBX_NRLPSO_DIAG_GMCOST] = 0.;
        }
        __syncthreads();
        const bool mutate = L.RED[17] != 0.;
        if (L.RED[16] != 0. && tid < D) L.PB[p * D + tid] = L.POP[p * D + tid];
        __syncthreads();
        if (mutate) {                                                // neb_mutation (:204-239)
            int first, last;
            // pbest neighbourhood
            if (tid < kNrK) L.TMP[tid] = nr_dist(L.PB + p * D, gSnap + L.PNI[p * kNrK + tid] * D, D);
            __syncthreads();
            nr_first_last(L.TMP, first, last);
            if (tid < D) {
                double u;
                if (tape) u = tape[MBX_NRLPSO_TAPE_MUT1(NP, D) + tid];
                else { const U4 w = rng.draw((uint32_t)tid, MBX_SITE_NR_MUT); u = u53(w.x, w.y); }
                L.X[tid] = L.PB[p * D + tid] + u * (gSnap[L.PNI[p * kNrK + first] * D + tid] - gSnap[L.PNI[p * kNrK + last] * D + tid]);
            }
            __syncthreads();
            {
                const RowPost post{&rng, tape ? tape + MBX_NRLPSO_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_NR_NOISE_A, MBX_SITE_NR_NOISE_B, 3, 1};
                eval_rows(P, L.eval(L.X, L.NC), 1, &post);
            }
            {
                const double cost = L.NC[0];
                const bool take = cost < L.PBCOST[p];
                const int q = L.PNI[p * kNrK + last];
                __syncthreads();
                if (tid < D) { if (take) L.PB[p * D + tid] = L.X[tid]; else L.POP[q * D + tid] = L.X[tid]; }
                if (tid == 0) { if (take) L.PBCOST[p] = cost; else L.COST[q] = cost; L.DG[MBX_NRLPSO_DIAG_PMCOST] = cost; }
                __syncthreads();
                if (!take) { stale = true; if (cached) { nr_dm_row(L, NP, D, q); __syncthreads(); } }
            }
            // gbest neighbourhood (gbest_pos may be the row the pbest half has just replaced)
            if (tid < kNrK) L.TMP[tid] = nr_dist(gpos, gSnap + L.GNI[tid] * D, D);
            __syncthreads();
            nr_first_last(L.TMP, first, last);
            if (tid < D) {
                double u;
                if (tape) u = tape[MBX_NRLPSO_TAPE_MUT2(NP, D) + tid];
                else { const U4 w = rng.draw((uint32_t)tid, MBX_SITE_NR_MUT); u = u53(w.z, w.w); }
                L.X[tid] = gpos[tid] + u * (gSnap[L.GNI[first] * D + tid] - gSnap[L.GNI[last] * D + tid]);
            }
            __syncthreads();
            {
                const RowPost post{&rng, tape ? tape + MBX_NRLPSO_TAPE_NOISE(NP, D) : nullptr, MBX_SITE_NR_NOISE_A, MBX_SITE_NR_NOISE_B, 3, 2};
                eval_rows(P, L.eval(L.X, L.NC), 1, &post);
            }
            {
                const double cost = L.NC[0];
                const bool take = cost < L.SC[MBX_SC_GBEST];
                const int q = L.GNI[last];
                __syncthreads();
                if (tid < D) { if (take) L.GB[tid] = L.X[tid]; else L.POP[q * D + tid] = L.X[tid]; }
                if (tid == 0) {
                    if (take) { L.SC[MBX_SC_GBEST] = cost; L.SC[MBX_SC_NRLPSO_ALIAS] = 0.; } else L.COST[q] = cost;
                    L.DG[MBX_NRLPSO_DIAG_GMCOST] = cost;
                }
                __syncthreads();
                if (!take) { stale = true; if (cached) { nr_dm_row(L, NP, D, q); __syncthreads(); } }
            }
        }
        if (tid == 0) {                                              // :274-296
            const double f_new = L.RED[19], reward = L.RED[18];
            double gbest = L.SC[MBX_SC_GBEST];
            if (f_new < gbest) { gbest = f_new; L.SC[MBX_SC_NRLPSO_ALIAS] = 1.; L.SC[MBX_SC_NRLPSO_G0] = p; L.SC[MBX_SC_GBEST_IDX] = p; }
            L.SS[p] = action;
            const int pointer = (p + 1) % NP;
            const double fes = L.SC[MBX_SC_FES] + (mutate ? 3. : 1.);
            int log_index = (int)L.SC[MBX_SC_LOG_INDEX], cost_len = (int)L.SC[MBX_SC_COST_LEN];
            const bool dn = log_and_terminate(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
            L.SC[MBX_SC_GBEST] = gbest; L.SC[MBX_SC_FES] = fes; L.SC[MBX_SC_LOG_INDEX] = log_index; L.SC[MBX_SC_COST_LEN] = cost_len;
            L.SC[MBX_SC_DONE] = dn ? 1. : 0.; L.SC[MBX_SC_RETURN] += reward; L.SC[MBX_SC_GEN] = step; L.SC[MBX_SC_NRLPSO_POINTER] = pointer;
            L.SC[MBX_SC_REINIT] = mutate ? 1. : 0.;
            L.DG[MBX_NRLPSO_DIAG_CS] = L.RED[13]; L.DG[MBX_NRLPSO_DIAG_EF_OLD] = L.RED[14]; L.DG[MBX_NRLPSO_DIAG_EF_NEW] = L.RED[15];
            L.DG[MBX_NRLPSO_DIAG_MUTATED] = mutate ? 1. : 0.; L.DG[MBX_NRLPSO_DIAG_FNEW] = f_new; L.DG[MBX_NRLPSO_DIAG_ACTION] = action;
            const int64_t row = (int64_t)it * bp.B + b;
            if (traj.actions) traj.actions[row] = action;
            if (traj.reward) traj.reward[row] = reward;
            if (traj.state) traj.state[row] = L.SS[pointer];
        }
        __syncthreads();
        reward_sum += L.RED[18];
        done = L.SC[MBX_SC_DONE] != 0.;
    }
    // ---- the state block, once per launch (velocities and the snapshot are already there)
    for (int e = tid; e < NE; e += kThreads) { S[MBX_NRLPSO_ST_POP(NP, D) + e] = L.POP[e]; S[MBX_NRLPSO_ST_PBPOS(NP, D) + e] = L.PB[e]; }
    for (int i = tid; i < NP; i += kThreads) {
        S[MBX_NRLPSO_ST_COST(NP, D) + i] = L.COST[i]; S[MBX_NRLPSO_ST_PBCOST(NP, D) + i] = L.PBCOST[i];
        S[MBX_NRLPSO_ST_STAG(NP, D) + i] = L.STAG[i]; S[MBX_NRLPSO_ST_SSTATE(NP, D) + i] = L.SS[i];
    }
    for (int e = tid; e < kNrK * NP; e += kThreads) S[MBX_NRLPSO_ST_PNIDX(NP, D) + e] = L.PNI[e];
    if (tid < kNrK) S[MBX_NRLPSO_ST_GNIDX(NP, D) + tid] = L.GNI[tid];
    if (tid < D) S[MBX_NRLPSO_ST_GBPOS(NP, D) + tid] = L.SC[MBX_SC_NRLPSO_ALIAS] != 0. ? L.POP[min(max((int)L.SC[MBX_SC_NRLPSO_G0], 0), NP - 1) * D + tid] : L.GB[tid];
    if (tid < MBX_NRLPSO_DIAG_SLOTS) S[MBX_NRLPSO_ST_DIAG(NP, D) + tid] = L.DG[tid];
    if (tid < MBX_NSCALAR) sc[tid] = L.SC[tid];
    if (tid == 0) {
        if (state_out) state_out[b] = L.SS[min(max((int)L.SC[MBX_SC_NRLPSO_POINTER], 0), NP - 1)];
        if (reward_out) reward_out[b] = reward_sum;
        if (done_out) done_out[b] = done ? 1 : 0;
        if (traj.last_action) traj.last_action[b] = last_action;
    }
}

template <bool MULTI>
__global__ __launch_bounds__(kThreads) void k_nrlpso_step(BatchParams bp, const int32_t* __restrict__ actions, const double* __restrict__ q_table, int n_steps,
                                                          int cached, NrTraj traj, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                          uint8_t* __restrict__ done_out)
{
    nr_steps<MULTI>(bp, actions, q_table, n_steps, cached, traj, state_out, reward_out, done_out);
}

}  // namespace mbx
