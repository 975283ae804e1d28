// mbx_jde21.hpp — JDE21, a classic baseline of the test harness, as batched kernels (reference: src/optimizer/jde21.py:6-277).
//
// Self-adaptive DE (jDE) with two populations: a big one of bNP = 160 rows whose trials replace the NEAREST big row (crowding, :46-49) and
// a small one of sNP = 10 rows with ordinary one-to-one selection.  One __update (:83-265) is a big pass of bNP trials followed by
// bNP / 10 small passes of 10 trials, 2 bNP evaluations in all; bNP halves up to three times over the budget (:249-256).
//
// No agent: mbx_reset is __init_population, every mbx_step (actions = NULL) one __update.  One workgroup per instance, dispatched through
// bp.order; state block and tape: include/mbx_layout.h §12.  The big population stays in the state block (HBM / L2); the kernel stages it
// into LDS twice per step (row stride jd_stride(D): padded where D is a multiple of 4, so that lanes reading consecutive rows hit distinct
// banks at D = 10, 12, 30, 40 alike): once as the gather source of the mutation and once, after the evaluations have used the same LDS as their scratch, for the
// crowding search.  All bNP trials stay in LDS (same stride) from the mutation to the selection; they are evaluated in row chunks that fit
// the staging area (three chunks of 54, 53, 53 rows at D = 10, 30, 40), with the noise draws of the whole pass.  The small population lives in LDS
// for the whole step.
//
// Crowding: for every trial i, argmin_j sum_d (pop[j,d] - u[i,d])^2 over the big rows, first index on ties.  A lane owns two trials and
// every eighth pair of candidate rows (a 2 x 2 register tile: four LDS reads per four differences); the eight lanes of a trial pair merge
// with three shuffle steps that carry the index and prefer the lower one.  Each sum follows numpy's pairwise order for a contiguous axis
// (eight running accumulators over blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder one by one; plain
// left-to-right below eight), the square is the product t * t.  -DMBX_ABLATE_CROWD compiles the search out (target = own row; timing only).
//
// Selection (:127-144) is a sequential loop in the reference; here every trial decides in parallel whether it is the one that survives
// that loop: it must be strictly below the incumbent of its target and no other trial of the same target may be lower, or equal and
// earlier.  cbest is the strict running minimum in trial order over the accepted trials, i.e. the lowest surviving trial, earliest first.
//
// Not carried: SF, SCr, df (appended to, never read) and age (a local of __update that restarts at 0, so `age > MaxFEs / 10`, :154,
// cannot fire).  Quirks of the reference kept on purpose:
//   1. __reinitialize (:66) returns rand (ub - lb) + ub: re-seeded rows lie in [ub, 2 ub - lb], outside the box, with cost 1e15;
//   2. the r1 test of the big pass is a product (:173): a draw is redrawn only where r1[i] == i == cbest_id;
//   3. r2 / r3 of the big pass range over bNP + mig rows, mig = 1, 2, 3 by thirds of the budget (:164-169), reaching into the small population;
//   4. every rejection loop redraws 25 times at most and then keeps what it has;
//   5. Cr > 1 becomes 0 (:112); randCr uses CRu_b = 1.1 for the small population too (:103);
//   6. bound repair is Python's float % (:115-116, result takes the divisor's sign): fmod plus the sign fix-up;
//   7. selection in trial order with colliding crowding targets (see above); F / Cr follow the winner;
//   8. gbest = min(cost) is recomputed at the end of each update (:248), the early stop is tested once per update, so fes overshoots;
//   9. the halving window is NP wide while a step advances 2 bNP, so a halving can be missed; it drops the FIRST bNP / 2 rows unsorted and
//      sets cbest_id = argmin(cost) while cbest stays;
//  10. at most one log point per update (:258);
//  11. nReset / sReset / cCopy are counters only (scalars of the state block).
// Arithmetic follows numpy's expression order with no contraction (the build passes -ffp-contract=off).
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"

namespace mbx {

constexpr int kJdTries = 25, kJdParts = 8;
constexpr double kJdTau = 0.1, kJdFinit = 0.5, kJdCrinit = 0.9, kJdFlB = 0.1, kJdFlS = 0.17, kJdFu = 1.1, kJdCrlB = 0.0, kJdCrlS = 0.1, kJdCru = 1.1;
constexpr double kJdEps = 1e-12, kJdMyEps = 0.25, kJdDead = 1e15;

// The LDS layout (JdLds, kJdS, jd_stride, jd_chunk, jd_lds_doubles, jd_carve) lives in mbx_lds.hpp.

// Python's float a % m for m > 0 (:115-116): fmod, then the result takes the divisor's sign
__device__ __forceinline__ double jd_pymod(double a, double m)
{
    double r = fmod(a, m);
    if (r != 0.) { if (r < 0.) r += m; } else r = 0.;
    return r;
}

// __prevecEnakih (:41-43) over cost[lo, lo + n): more than two and more than a quarter of the costs within eps of `best`.  All threads call.
__device__ __forceinline__ bool jd_stuck(const double* cost, int lo, int n, double best)
{
    const int tid = threadIdx.x;
    const int eqs = __syncthreads_count(tid < n && fabs(cost[lo + tid] - best) < kJdEps);
    return eqs > 2 && (double)eqs > n * kJdMyEps;
}

// the big rows [0, n) of the state block into LDS at row stride ps
__device__ __forceinline__ void jd_stage_pop(const double* gP, double* dst, int n, int D, int ps)
{
    const FastDiv fd(D);
    for (int e = threadIdx.x; e < n * D; e += kThreads) {
        const int i = fd.div(e);
        dst[i * ps + (e - i * D)] = gP[e];
    }
}

// One pass of mutation and crossover (:93-120) for n trials, trial rows t0.. of the step (layout §12): F / Cr of the trials into L.TF /
// L.TCR, the trial vectors into `out` at row stride os.  BIG: parents are rows [0, n) (staged in L.EV at stride ps, rows >= bNP from L.SP);
// otherwise the small population in L.SP.  Ends with a barrier.
template <bool BIG>
__device__ __forceinline__ void jd_trials(const DevProblem& P, const JdLds& L, int n, int t0, int bNP, int mig, int cbest_id, int D, int ps,
                                          double* out, int os, const double* tape, int NP, const Rng& rng)
{
    const int tid = threadIdx.x;
    if (tid < n) {
        const int i = BIG ? tid : bNP + tid, t = t0 + tid;
        const int lo = BIG ? 0 : bNP, n1 = BIG ? bNP : kJdS, n23 = BIG ? bNP + mig : kJdS;
        int r1, r2, r3, jr;
        double uF, uCr, vF, vCr;
        if (tape) {       // (clamped: a tape is caller data)
            r1 = min(max((int)tape[MBX_JDE21_TAPE_R1(NP, D) + t], lo), lo + n1 - 1);
            r2 = min(max((int)tape[MBX_JDE21_TAPE_R2(NP, D) + t], lo), lo + n23 - 1);
            r3 = min(max((int)tape[MBX_JDE21_TAPE_R3(NP, D) + t], lo), lo + n23 - 1);
            jr = min(max((int)tape[MBX_JDE21_TAPE_JRAND(NP, D) + t], 0), D - 1);
            uF = tape[MBX_JDE21_TAPE_RANDF(NP, D) + t]; uCr = tape[MBX_JDE21_TAPE_RANDCR(NP, D) + t];
            vF = tape[MBX_JDE21_TAPE_RVSF(NP, D) + t]; vCr = tape[MBX_JDE21_TAPE_RVSCR(NP, D) + t];
        } else {
            // the rejection loops (:171-193, :220-242): one draw, then at most 25 redraws while the test rejects
            U4 w = rng.draw((uint32_t)(t * 32), MBX_SITE_JD_IDX);
            jr = (int)__umulhi(w.w, (uint32_t)D);
            r1 = lo + (int)__umulhi(w.x, (uint32_t)n1);
            for (int a = 1; a <= kJdTries && (BIG ? (r1 == i && r1 == cbest_id) : r1 == i); ++a)
                r1 = lo + (int)__umulhi(rng.draw((uint32_t)(t * 32 + a), MBX_SITE_JD_IDX).x, (uint32_t)n1);
            r2 = lo + (int)__umulhi(w.y, (uint32_t)n23);
            for (int a = 1; a <= kJdTries && (r2 == i || r2 == r1); ++a)
                r2 = lo + (int)__umulhi(rng.draw((uint32_t)(t * 32 + a), MBX_SITE_JD_IDX).y, (uint32_t)n23);
            r3 = lo + (int)__umulhi(w.z, (uint32_t)n23);
            for (int a = 1; a <= kJdTries && (r3 == i || r3 == r1 || r3 == r2); ++a)
                r3 = lo + (int)__umulhi(rng.draw((uint32_t)(t * 32 + a), MBX_SITE_JD_IDX).z, (uint32_t)n23);
            w = rng.draw((uint32_t)t, MBX_SITE_JD_PART);
            uF = u53(w.x, w.y); uCr = u53(w.z, w.w);
            w = rng.draw((uint32_t)t, MBX_SITE_JD_PART2);
            vF = u53(w.x, w.y); vCr = u53(w.z, w.w);
        }
        const double randF = uF * kJdFu + (BIG ? kJdFlB : kJdFlS), randCr = uCr * kJdCru + (BIG ? kJdCrlB : kJdCrlS);
        const double F = vF < kJdTau ? randF : L.FF[i];
        double Cr = vCr < kJdTau ? randCr : L.CR[i];
        if (Cr > 1.) Cr = 0.;
        L.R1[tid] = r1; L.R2[tid] = r2; L.R3[tid] = r3; L.JR[tid] = jr; L.TF[tid] = F; L.TCR[tid] = Cr;
    }
    __syncthreads();
    const double lb = P.lb, ub = P.ub;
    const FastDiv fd(D);
    auto row = [&](int r) -> const double* { return BIG && r < bNP ? L.EV + r * ps : L.SP + (r - bNP) * D; };
    for (int e = tid; e < n * D; e += kThreads) {
        const int k = fd.div(e), d = e - k * D;
        double cu;
        if (tape) cu = tape[MBX_JDE21_TAPE_CROSS(NP, D) + (int64_t)(t0 + k) * D + d];
        else { const U4 w = rng.draw((uint32_t)((t0 + k) * D + d), MBX_SITE_JD_CROSS); cu = u53(w.x, w.y); }
        double v = row(L.R1[k])[d] + L.TF[k] * (row(L.R2[k])[d] - row(L.R3[k])[d]);
        if (v > ub) v = jd_pymod(v - lb, ub - lb) + lb;
        if (v < lb) v = jd_pymod(v - ub, ub - lb) + lb;
        out[k * os + d] = (cu < L.TCR[k] || d == L.JR[k]) ? v : row(BIG ? k : bNP + k)[d];
    }
    __syncthreads();
}

// four squared distances of a 2 x 2 tile (trials ua / ub against candidates pa / pb) in numpy's pairwise summation order
__device__ __forceinline__ void jd_dist4(const double* pa, const double* pb, const double* ua, const double* ub, int D, double (&s)[4])
{
    if (D < 8) {
        s[0] = s[1] = s[2] = s[3] = 0.;
        for (int d = 0; d < D; ++d) {
            const double a = pa[d], b = pb[d], x = ua[d], y = ub[d];
            const double t0 = a - x, t1 = b - x, t2 = a - y, t3 = b - y;
            s[0] += t0 * t0; s[1] += t1 * t1; s[2] += t2 * t2; s[3] += t3 * t3;
        }
        return;
    }
    double r[4][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double a = pa[k], b = pb[k], x = ua[k], y = ub[k];
        const double t0 = a - x, t1 = b - x, t2 = a - y, t3 = b - y;
        r[0][k] = t0 * t0; r[1][k] = t1 * t1; r[2][k] = t2 * t2; r[3][k] = t3 * t3;
    }
    int d = 8;
    for (; d + 8 <= D; d += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double a = pa[d + k], b = pb[d + k], x = ua[d + k], y = ub[d + k];
            const double t0 = a - x, t1 = b - x, t2 = a - y, t3 = b - y;
            r[0][k] += t0 * t0; r[1][k] += t1 * t1; r[2][k] += t2 * t2; r[3][k] += t3 * t3;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = ((r[q][0] + r[q][1]) + (r[q][2] + r[q][3])) + ((r[q][4] + r[q][5]) + (r[q][6] + r[q][7]));
    for (; d < D; ++d) {
        const double a = pa[d], b = pb[d], x = ua[d], y = ub[d];
        const double t0 = a - x, t1 = b - x, t2 = a - y, t3 = b - y;
        s[0] += t0 * t0; s[1] += t1 * t1; s[2] += t2 * t2; s[3] += t3 * t3;
    }
}

// __crowding (:46-49): cid[i] = the big row nearest to trial i (first index on ties).  pop / up: LDS, row stride ps; bNP even.  The
// caller synchronises before and after.
__device__ __forceinline__ void jd_crowding(const double* pop, const double* up, int bNP, int D, int ps, int* cid)
{
    const int tid = threadIdx.x;
#ifdef MBX_ABLATE_CROWD
    if (tid < bNP) cid[tid] = tid;
#else
    const int half = bNP >> 1, nwork = half * kJdParts;
    for (int w0 = 0; w0 < nwork; w0 += kThreads) {
        const int w = w0 + tid, ip = w / kJdParts, p = w % kJdParts;
        double b0 = INFINITY, b1 = INFINITY;
        int j0 = 0x7fffffff, j1 = 0x7fffffff;
        if (w < nwork) {
            const double* ua = up + 2 * ip * ps;
            const double* ub = ua + ps;
            for (int jp = p; jp < half; jp += kJdParts) {
                const double* pa = pop + 2 * jp * ps;
                double s[4];
                jd_dist4(pa, pa + ps, ua, ub, D, s);
                if (s[0] < b0) { b0 = s[0]; j0 = 2 * jp; }
                if (s[1] < b0) { b0 = s[1]; j0 = 2 * jp + 1; }
                if (s[2] < b1) { b1 = s[2]; j1 = 2 * jp; }
                if (s[3] < b1) { b1 = s[3]; j1 = 2 * jp + 1; }
            }
        }
        // the eight lanes of a trial pair (aligned groups: kThreads and the work count are multiples of 8) merge; lower index on ties
#pragma unroll
        for (int off = 1; off < kJdParts; off <<= 1) {
            const double o0 = __shfl_xor(b0, off, 64), o1 = __shfl_xor(b1, off, 64);
            const int i0 = __shfl_xor(j0, off, 64), i1 = __shfl_xor(j1, off, 64);
            if (o0 < b0 || (o0 == b0 && i0 < j0)) { b0 = o0; j0 = i0; }
            if (o1 < b1 || (o1 == b1 && i1 < j1)) { b1 = o1; j1 = i1; }
        }
        if (w < nwork && p == 0) {
            cid[2 * ip] = j0 < bNP ? j0 : 0;          // (every distance inf or NaN: np.argmin answers 0)
            cid[2 * ip + 1] = j1 < bNP ? j1 : 0;
        }
    }
#endif
}

// Selection (:127-144) of n trials with costs L.TC, targets L.CID (rows of L.COST / L.FF / L.CR) and F / Cr in L.TF / L.TCR: the outcome of
// the reference's loop in trial order (header comment).  Leaves L.WIN[i] = 1 for the trials that end up in the population and updates
// cbest / cbest_id (uniform across the workgroup).  COLLIDE = false: the targets are distinct.  Ends with a barrier.
template <bool COLLIDE>
__device__ __forceinline__ void jd_select(const JdLds& L, int n, double& cbest, int& cbest_id)
{
    const int tid = threadIdx.x;
    int win = 0, id = 0;
    double my = 0.;
    if (tid < n) {
        my = L.TC[tid]; id = L.CID[tid];
        win = my < L.COST[id];
        if (COLLIDE && win)
            for (int k = 0; k < n; ++k) {
                const double c = L.TC[k];
                if (k != tid && L.CID[k] == id && (c < my || (c == my && k < tid))) win = 0;
            }
    }
    __syncthreads();
    if (tid < n) {
        L.WIN[tid] = win;
        L.ACC[tid] = win ? my : INFINITY;
        if (win) { L.COST[id] = my; L.FF[id] = L.TF[tid]; L.CR[id] = L.TCR[tid]; }
    }
    __syncthreads();
    double m; int e;
    block_argmin(L.ACC, n, L.RED, m, e);
    if (m < cbest) { cbest = m; cbest_id = L.CID[e]; }
}

// ------------------------------------------------------------------------------------------------ reset (__init_population :68-81)
__global__ __launch_bounds__(kThreads) void k_jde21_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = bp.NP, D = bp.D, CH = jd_chunk(NP, D);
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const JdLds L = jd_carve(smem, NP, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_JDE21_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub;
    stage_problem(P, L.eval(CH, D, L.COST));
    for (int c0 = 0; c0 < NP; c0 += CH) {
        const int n = min(CH, NP - c0);
        for (int e = tid; e < n * D; e += kThreads) {
            const int g = c0 * D + e;
            double u;
            if (tape) u = tape[MBX_JDE21_TAPE_POS(NP, D) + g];
            else { const U4 w = rng.draw((uint32_t)g, MBX_SITE_JD_CROSS); u = u53(w.x, w.y); }
            const double x = u * (ub - lb) + lb;
            L.EV[e] = x;
            S[MBX_JDE21_ST_POP(NP, D) + g] = x;
        }
        __syncthreads();
        population_costs(P, L.eval(n, D, L.COST + c0), n, rng, tape ? tape + MBX_JDE21_TAPE_NOISE_INIT(NP, D) : nullptr, MBX_SITE_NOISE1_A,
                         MBX_SITE_NOISE1_B, c0, NP);
    }
    double gb; int g0;
    block_argmin(L.COST, NP, L.RED, gb, g0);
    if (tid < NP) {
        S[MBX_JDE21_ST_COST(NP, D) + tid] = L.COST[tid];
        S[MBX_JDE21_ST_F(NP, D) + tid] = kJdFinit;
        S[MBX_JDE21_ST_CR(NP, D) + tid] = kJdCrinit;
        S[MBX_JDE21_ST_CROWD(NP, D) + tid] = 0.;
    }
    if (tid == 0) {
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = g0;
        sc[MBX_SC_JD_BNP] = NP - kJdS; sc[MBX_SC_JD_CBEST] = gb; sc[MBX_SC_JD_CBEST_ID] = g0;
        sc[MBX_NSCALAR] = gb;                                        // cost = [gbest]
        if (state_out) state_out[b] = (double)NP / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------ generation (__update :83-265)
// WAVES: the waves per SIMD the register allocation aims at.  3 where the LDS lets three workgroups share a CU (D <= 12: 1914 -> 1526 us per
// step of 4096 instances at D = 10; at 4 the crowding tile spills and the step is slower), 2 otherwise (one workgroup per CU at D = 30 / 40,
// where the tighter register target only costs: 6020 -> 6660 us at D = 30).  jd_waves() is the host's choice.
__host__ __device__ inline int jd_waves(int64_t lds_bytes) { return 3 * lds_bytes <= 160 * 1024 ? 3 : 2; }
template <int WAVES>
__global__ __launch_bounds__(kThreads, WAVES) void k_jde21_generation(BatchParams bp, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                               uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NPmax = bp.NP, D = bp.D, ps = jd_stride(D), CH = jd_chunk(NPmax, D), R = (int)MBX_JDE21_ROWS(NPmax);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_JDE21_ST_SCALARS(NPmax, D);
    if (sc[MBX_SC_DONE] != 0.) { if (tid == 0) { if (reward_out) reward_out[b] = 0.; if (done_out) done_out[b] = 1; } return; }
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const JdLds L = jd_carve(smem, NPmax, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int gen = (int)sc[MBX_SC_GEN] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)(int)sc[MBX_SC_EPISODE]};
    const double lb = P.lb, ub = P.ub, fes0 = sc[MBX_SC_FES];
    // (clamped: the state block can be caller data, mbx_debug_write_state)
    const int bNP = min(max((int)sc[MBX_SC_JD_BNP], 2), NPmax - kJdS) & ~1, NP = bNP + kJdS;
    double cbest = sc[MBX_SC_JD_CBEST];
    int cbest_id = min(max((int)sc[MBX_SC_JD_CBEST_ID], 0), NP - 1);
    int n_reset = (int)sc[MBX_SC_JD_NRESET], s_reset = (int)sc[MBX_SC_JD_SRESET], c_copy = (int)sc[MBX_SC_JD_CCOPY];
    double* gP = S + MBX_JDE21_ST_POP(NPmax, D);
    const FastDiv fd(D);
    stage_problem(P, L.eval(CH, D, L.TC));
    if (tid < NP) {
        L.COST[tid] = S[MBX_JDE21_ST_COST(NPmax, D) + tid];
        L.FF[tid] = S[MBX_JDE21_ST_F(NPmax, D) + tid];
        L.CR[tid] = S[MBX_JDE21_ST_CR(NPmax, D) + tid];
    }
    for (int e = tid; e < kJdS * D; e += kThreads) L.SP[e] = gP[bNP * D + e];
    __syncthreads();
    // big-population reset (:154-162)
    if (jd_stuck(L.COST, 0, bNP, sc[MBX_SC_GBEST])) {
        n_reset += 1;
        for (int e = tid; e < bNP * D; e += kThreads) {
            double u;
            if (tape) u = tape[MBX_JDE21_TAPE_RESEED_B(NPmax, D) + e];
            else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_JD_RESEED); u = u53(w.x, w.y); }
            gP[e] = u * (ub - lb) + ub;
        }
        if (tid < bNP) { L.FF[tid] = kJdFinit; L.CR[tid] = kJdCrinit; L.COST[tid] = kJdDead; }
        __syncthreads();
        block_argmin(L.COST, NP, L.RED, cbest, cbest_id);
    }
    const int mig = fes0 < bp.max_fes / 3. ? 1 : fes0 < 2. * bp.max_fes / 3. ? 2 : 3;
    // ---- big pass: mutation / crossover against the staged population, evaluation in chunks, crowding, selection
    jd_stage_pop(gP, L.EV, bNP, D, ps);
    __syncthreads();
    jd_trials<true>(P, L, bNP, 0, bNP, mig, cbest_id, D, ps, L.UP, ps, tape, NPmax, rng);
    {
        const int nch = (bNP + CH - 1) / CH, per = (bNP + nch - 1) / nch;
        for (int c0 = 0; c0 < bNP; c0 += per) {
            const int n = min(per, bNP - c0);
            for (int e = tid; e < n * D; e += kThreads) {
                const int i = fd.div(e);
                L.EV[e] = L.UP[(c0 + i) * ps + (e - i * D)];
            }
            __syncthreads();
            population_costs(P, L.eval(n, D, L.TC + c0), n, rng, tape ? tape + MBX_JDE21_TAPE_NOISE(NPmax, D) : nullptr, MBX_SITE_JD_NOISE_A,
                             MBX_SITE_JD_NOISE_B, c0, R);
        }
    }
    jd_stage_pop(gP, L.EV, bNP, D, ps);
    __syncthreads();
    jd_crowding(L.EV, L.UP, bNP, D, ps, L.CID);
    __syncthreads();
    jd_select<true>(L, bNP, cbest, cbest_id);
    for (int e = tid; e < bNP * D; e += kThreads) {
        const int i = fd.div(e), d = e - i * D;
        if (L.WIN[i]) gP[L.CID[i] * D + d] = L.UP[i * ps + d];
    }
    if (tid < bNP) S[MBX_JDE21_ST_CROWD(NPmax, D) + tid] = L.CID[tid];
    __syncthreads();
    // ---- small-population reset (:198-210) and the copy of the best big row (:212-216)
    if (cbest_id >= bNP && jd_stuck(L.COST, bNP, kJdS, cbest)) {
        s_reset += 1;
        const double keep = tid < D ? L.SP[(cbest_id - bNP) * D + tid] : 0.;
        __syncthreads();
        for (int e = tid; e < kJdS * D; e += kThreads) {
            double u;
            if (tape) u = tape[MBX_JDE21_TAPE_RESEED_S(NPmax, D) + e];
            else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_JD_RESEED); u = u53(w.z, w.w); }
            L.SP[e] = u * (ub - lb) + ub;
        }
        if (tid < kJdS) { L.FF[bNP + tid] = kJdFinit; L.CR[bNP + tid] = kJdCrinit; L.COST[bNP + tid] = kJdDead; }
        __syncthreads();
        if (tid < D) L.SP[(cbest_id - bNP) * D + tid] = keep;
        if (tid == 0) L.COST[cbest_id] = cbest;
        __syncthreads();
    }
    if (cbest_id < bNP) {
        c_copy += 1;
        if (tid < D) L.SP[tid] = gP[cbest_id * D + tid];
        if (tid == 0) L.COST[bNP] = cbest;
        cbest_id = bNP;
        __syncthreads();
    }
    // ---- small passes (:218-245): 10 trials each, one-to-one selection, the small population stays in LDS
    if (tid < kJdS) L.CID[tid] = bNP + tid;
    for (int p = 0; p < bNP / kJdS; ++p) {
        const int t0 = NPmax - kJdS + p * kJdS;
        jd_trials<false>(P, L, kJdS, t0, bNP, 0, cbest_id, D, ps, L.EV, D, tape, NPmax, rng);
        population_costs(P, L.eval(kJdS, D, L.TC), kJdS, rng, tape ? tape + MBX_JDE21_TAPE_NOISE(NPmax, D) : nullptr, MBX_SITE_JD_NOISE_A,
                         MBX_SITE_JD_NOISE_B, t0, R);
        jd_select<false>(L, kJdS, cbest, cbest_id);
        for (int e = tid; e < kJdS * D; e += kThreads) if (L.WIN[fd.div(e)]) L.SP[e] = L.EV[e];
        __syncthreads();
    }
    // ---- end of the update (:248-265): gbest, halving, state back to HBM, logging, termination
    double gbest; int gi;
    block_argmin(L.COST, NP, L.RED, gbest, gi);
    const double fes = fes0 + bNP + (bNP / kJdS) * kJdS, mf = bp.max_fes;
    const bool halve = (fes - NP <= 0.25 * mf && 0.25 * mf <= fes) || (fes - NP <= 0.5 * mf && 0.5 * mf <= fes) || (fes - NP <= 0.75 * mf && 0.75 * mf <= fes);
    int new_bnp = bNP;
    if (halve) {
        new_bnp = bNP / 2;
        const int h = new_bnp, keep = bNP - h;
        // the surviving big rows move down by h through LDS (source and destination overlap)
        for (int e = tid; e < keep * D; e += kThreads) L.EV[e] = gP[h * D + e];
        double c = 0., f = 0., r = 0.;
        if (tid < NP - h) { c = L.COST[tid + h]; f = L.FF[tid + h]; r = L.CR[tid + h]; }
        __syncthreads();
        for (int e = tid; e < keep * D; e += kThreads) gP[e] = L.EV[e];
        if (tid < NP - h) { L.COST[tid] = c; L.FF[tid] = f; L.CR[tid] = r; }
        __syncthreads();
        double m;
        block_argmin(L.COST, NP - h, L.RED, m, cbest_id);
    }
    for (int e = tid; e < kJdS * D; e += kThreads) gP[new_bnp * D + e] = L.SP[e];
    if (tid < new_bnp + kJdS) {
        S[MBX_JDE21_ST_COST(NPmax, D) + tid] = L.COST[tid];
        S[MBX_JDE21_ST_F(NPmax, D) + tid] = L.FF[tid];
        S[MBX_JDE21_ST_CR(NPmax, D) + tid] = L.CR[tid];
    }
    if (tid == 0) {
        int log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
        const bool done = log_and_terminate_guarded(bp, P, fes, gbest, log_index, cost_len, sc + MBX_NSCALAR);
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_GEN] = gen; sc[MBX_SC_GBEST_IDX] = gi;
        sc[MBX_SC_JD_BNP] = new_bnp; sc[MBX_SC_JD_CBEST] = cbest; sc[MBX_SC_JD_CBEST_ID] = cbest_id;
        sc[MBX_SC_JD_NRESET] = n_reset; sc[MBX_SC_JD_SRESET] = s_reset; sc[MBX_SC_JD_CCOPY] = c_copy;
        if (state_out) state_out[b] = fes / bp.max_fes;
        if (reward_out) reward_out[b] = 0.;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
