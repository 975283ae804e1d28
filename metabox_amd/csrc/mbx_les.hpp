// mbx_les.hpp — LES, a learned evolution strategy, as a resident episode kernel (reference: src/optimizer/les_optimizer.py:18-180; layout, tape and
// Philox sites: include/mbx_layout.h section 18).
//
// A diagonal Gaussian (mu, sigma) over D coordinates is sampled NP = 16 times per generation.  A 68-parameter self-attention module turns the 16
// costs into recombination weights W, a 178-parameter MLP turns three pairs of evolution paths and a timestamp embedding into two learning rates
// per coordinate, and mu / sigma move towards the W-weighted mean / spread of the parents.  The reference's update() is the WHOLE episode in one
// call with no host decision between generations, and meta-training runs one such call per candidate parameter vector: here one workgroup owns
// an instance (through bp.order), keeps parents, costs, mu, sigma, Pc, Ps, the counters and the instance's OWN 246 parameters in LDS, and runs
// n_gens generations per launch.  The narrow phases -- 16 rows, D <= 40 columns -- run on the lanes of wave 0 and hand over inside that wave;
// sampling and the 16-row objective (the evaluator every kernel here shares, eval_rows) use all four waves.  Block barriers per generation: two
// of this file's (the new mu / sigma go to the sampler, the children to the evaluator), one more on a noisy function, plus the evaluator's own.
// gbest, FEs, the log and `done` are recomputed by every thread from the 16 costs, so the loop's exit is uniform without another barrier.
//
// The reference's own behaviour, kept on purpose (line numbers of les_optimizer.py):
//  * costs are problem.eval(x): noise included, the optimum NOT subtracted (:71, :147); `gbest <= 1e-8` (:165) is taken on that value.
//  * shifted_rank = np.argsort(costs) / 16 - 0.5 (:91) is the argsort INDEX (entry r = the row with the r-th smallest cost), not the rank of a row.
//    Equal costs order by (cost, row).
//  * improved = costs < gbest (:93) is always false, gbest already includes the parents; it is computed all the same.
//  * cal_mlp_feature (:102-105): (1 - a) P + a (sum - P) as written, for a in {0.1, 0.5, 0.9}; the NEW paths are the MLP's input and the state.
//  * mu and sigma (:140-143) take 1 - alpha in float32 (the MLP's output is a float32 array) and everything else in float64.
//  * with a skip_step the end rule is REPLACED by step >= skip_step (:167-168): budget and early stop are ignored and FEs runs past maxFEs.
//  * one `if`, not a `while`, for the log point (:170-172); the closing append-or-overwrite (:174-178) uses n_logpoint + 1.
//  * reward = (init_y - gbest) / init_y with init_y the gbest after the first generation of the call (:150-151, :180).
//  * a sigma with a zero entry makes Ps inf / nan exactly as numpy's division does; np.clip's NaN propagation is kept (les_clip).
//  * the log-point append is unguarded, so the cost list can pass n_logpoint + 1 entries (52 at maxFEs = 976); the instance's curve has
//    MBX_LES_CURVE_CAP slots, enough for every episode that runs to its budget.
// One guard the reference does not need: the log-point append (:172) writes only while the curve is shorter than those slots (repeated skip_step
// calls far past the budget would otherwise leave the instance's block).
//
// Arithmetic.  float64 parts follow numpy's expression order with no contraction (the build passes -ffp-contract=off): np.mean / np.std over
// the 16 costs are numpy's pairwise_sum (mbx_npsum.hpp: eight accumulators, then the tree); the reductions over axis 0 of a (16, D) array
// (:103, :105, :141, :143) add row after row, i = 0 .. 15.  float32 parts -- torch's CPU kernels in the reference -- are written as explicit
// fmaf chains, and the summation order of every float32 dot product is:
//  * Linear (Wq, Wk, Wv, ln1, ln2):  acc = bias; acc = fmaf(w[k][j], x[j], acc) for j ascending.
//  * Q K^T:  acc = 0; acc = fmaf(Q[i][k], K[j][k], acc) for k = 0 .. 7; then acc * (1.f / (float)sqrt(8)) (torch's scalar division).
//  * softmax over a row of 16:  m = max; e_j = expf(s_j - m); sum = ((e_0 + e_1) + e_2) + ... left to right; e_j / sum.
//  * attn V:  acc = 0; acc = fmaf(P[i][j], V[j], acc) for j = 0 .. 15; the softmax over the 16 rows as above.
//  * sigmoid(x) = 1 / (1 + expf(-x)).
// The timestamp embedding tanh(t / timestamp - 1) is a float32 table made by the host in extended precision (mbx.hip), one row per generation counter
// up to max_fes / 16 + 64; only a skip_step call that runs further past the budget takes the device's tanh instead.
#pragma once
#include "mbx_device.hpp"
#include "mbx_rlepso.hpp"   // BatchParams
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"

namespace mbx {

constexpr int kLesNTs = MBX_LES_NTS;
constexpr double kLesSigmaRatio = 0.2;
// offsets inside a parameter set (vector2nn order)
constexpr int kLesWq = 0, kLesBq = 24, kLesWk = 32, kLesBk = 56, kLesWv = 64, kLesBv = 67, kLesW1 = 68, kLesB1 = 220, kLesW2 = 228, kLesB2 = 244;

struct LesArgs {
    const float* params;        // [n_sets][246]
    const int32_t* set_of;      // [B] or nullptr = set 0
    int n_sets;
    const float* ts;            // [horizon + 1][13] float32: tanh(t / timestamp - 1)
    int horizon;
    int n_gens;                 // generations of this launch at most
    int skip;                   // 0: budget / early-stop end rule; 1: the skip_step rule
    int step0, skip_total;      // skip route: this launch runs steps step0 .. of a call that ends at step == skip_total
};

// The LDS layout (LesLds, kLesNP, kLesNParam, les_lds_doubles, les_carve) lives in mbx_lds.hpp.

// self.timestamp (:51) without an indexed table (a dynamic index into a local array is scratch memory)
__device__ __forceinline__ int les_stamp(int k)
{
    return k == 0 ? 1 : k == 1 ? 3 : k == 2 ? 10 : k == 3 ? 30 : k == 4 ? 50 : k == 5 ? 100 : k == 6 ? 250 : k == 7 ? 500 : k == 8 ? 750 : k == 9 ? 1000
         : k == 10 ? 1250 : k == 11 ? 1500 : 2000;
}

// np.clip = minimum(maximum(x, lb), ub): a NaN stays a NaN
__device__ __forceinline__ double les_clip(double x, double lb, double ub)
{
    x = x < lb ? lb : x;
    return x > ub ? ub : x;
}

// np.min of two values: a NaN wins (costs of a NaN row, which a zero sigma can make)
__device__ __forceinline__ double les_min(double c, double m) { return (c < m || c != c) ? c : m; }

// softmax over 16 float32 values in LDS, entry i (the header gives the order)
__device__ __forceinline__ float les_softmax16(const float* s, int i)
{
    float m = s[0];
    for (int j = 1; j < kLesNP; ++j) m = fmaxf(m, s[j]);
    float sum = 0.f, mine = 0.f;
    for (int j = 0; j < kLesNP; ++j) { const float e = expf(s[j] - m); sum += e; mine = j == i ? e : mine; }
    return mine / sum;
}

// problem.eval's noise on the 16 raw objective values in L.NC (NoisyProblem.noisy, bbob.py:108-146); the optimum stays in.  Ends with a barrier.
template <class PT>
__device__ __forceinline__ void les_noise(const PT& P, const LesLds& L, const Rng& rng, const double* tape_noise)
{
    if (P.noise_kind == MBX_NOISE_NONE) return;                      // workgroup-uniform
    const int tid = threadIdx.x;
    if (tid < kLesNP) {
        double a, b, c;
        if (tape_noise) { a = tape_noise[tid]; b = tape_noise[kLesNP + tid]; c = tape_noise[2 * kLesNP + tid]; }
        else philox_noise(rng, (uint32_t)tid, MBX_SITE_LES_NOISE_A, MBX_SITE_LES_NOISE_B, P.noise_kind, a, b, c);
        L.NC[tid] = apply_noise(P, L.NC[tid], a, b, c);
    }
    __syncthreads();
}

// z ~ N(0, 1) for the 16 D elements of one sampling into L.ZN: tape, or one Philox draw per element pair
__device__ __forceinline__ void les_normals(const LesLds& L, int NE, const Rng& rng, const double* tape_z)
{
    const int tid = threadIdx.x;
    if (tape_z) { for (int e = tid; e < NE; e += kThreads) L.ZN[e] = tape_z[e]; return; }
    for (int p = tid; 2 * p < NE; p += kThreads) {
        const U4 w = rng.draw((uint32_t)p, MBX_SITE_LES_NORMAL);
        double n0, n1;
        box_muller(u53(w.x, w.y), u53(w.z, w.w), n0, n1);
        L.ZN[2 * p] = n0; L.ZN[2 * p + 1] = n1;
    }
}

// ------------------------------------------------------------------------------------------------ reset (init_population :63-84)
__global__ __launch_bounds__(kThreads) void k_les_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    constexpr int NP = kLesNP;
    const int D = bp.D, NE = NP * D;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const LesLds L = les_carve(smem, D);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_LES_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    stage_problem(P, L.eval());
    if (tid < D) {
        double u;
        if (tape) u = tape[MBX_LES_TAPE_MU(NP, D) + tid];
        else { const U4 w = rng.draw((uint32_t)tid, MBX_SITE_LES_MU); u = u53(w.x, w.y); }
        L.MU[tid] = P.lb + (P.ub - P.lb) * u;                        // :68
        L.SIG[tid] = 1. * P.ub * kLesSigmaRatio;                     // :69
    }
    les_normals(L, NE, rng, tape ? tape + MBX_LES_TAPE_Z0(NP, D) : nullptr);
    __syncthreads();
    const FastDiv fd(D);
    for (int e = tid; e < NE; e += kThreads) {
        const int d = fd.mod(e);
        const double x = les_clip(L.MU[d] + L.SIG[d] * L.ZN[e], P.lb, P.ub);   // :70
        L.XR[e] = x;
        S[MBX_LES_ST_PARENTS(NP, D) + e] = x; S[MBX_LES_ST_Z(NP, D) + e] = L.ZN[e];
    }
    __syncthreads();
    eval_rows(P, L.eval(), NP);                                      // :71
    les_noise(P, L, rng, tape ? tape + MBX_LES_TAPE_NOISE_INIT(NP, D) : nullptr);
    if (tid < NP) { S[MBX_LES_ST_COST(NP, D) + tid] = L.NC[tid]; S[MBX_LES_ST_W(NP, D) + tid] = 0.; }
    if (tid < D) {
        S[MBX_LES_ST_MU(NP, D) + tid] = L.MU[tid]; S[MBX_LES_ST_SIGMA(NP, D) + tid] = L.SIG[tid];
        for (int k = 0; k < 3; ++k) { S[MBX_LES_ST_PC(NP, D) + k * D + tid] = 0.; S[MBX_LES_ST_PS(NP, D) + k * D + tid] = 0.; }
        S[MBX_LES_ST_ALPHA(NP, D) + 2 * tid] = 0.; S[MBX_LES_ST_ALPHA(NP, D) + 2 * tid + 1] = 0.;
    }
    if (tid == 0) {
        double gb = L.NC[0];
        for (int i = 1; i < NP; ++i) gb = les_min(L.NC[i], gb);      // np.min (:75)
        for (int k = 0; k < MBX_NSCALAR; ++k) if (k != MBX_SC_EPISODE) sc[k] = 0.;
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_NSCALAR] = gb;                                        // cost = [min] (:82)
        if (state_out) state_out[b] = gb;
    }
}

// ------------------------------------------------------------------------------------------------ the `while` loop of update (:128-178)
__global__ __launch_bounds__(kThreads) void k_les_run(BatchParams bp, LesArgs ar, double* __restrict__ state_out, double* __restrict__ reward_out,
                                                      uint8_t* __restrict__ done_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    constexpr int NP = kLesNP;
    const int D = bp.D, NE = NP * D;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_LES_ST_SCALARS(NP, D);
    const bool skip = ar.skip != 0;
    // every scalar is read here, before the first barrier, by every thread; thread 0 writes them back after the last one
    double gbest = sc[MBX_SC_GBEST], init_y = sc[skip ? MBX_SC_LES_CALL_INIT_Y : MBX_SC_LES_INIT_Y];
    if (!skip && sc[MBX_SC_DONE] != 0.) {                            // a finished instance stays as it is
        if (tid == 0) {
            if (state_out) state_out[b] = gbest;
            if (reward_out) reward_out[b] = (init_y - gbest) / init_y;
            if (done_out) done_out[b] = 1;
        }
        return;
    }
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const LesLds L = les_carve(smem, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const uint64_t seed = bp.seeds[b];
    const uint32_t episode = (uint32_t)(int)sc[MBX_SC_EPISODE];
    const int curve_cap = (int)MBX_LES_CURVE_CAP(bp.max_fes, bp.log_interval, bp.n_logpoint);
    int fes = (int)sc[MBX_SC_FES], log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN], t = (int)sc[MBX_SC_GEN];
    cost_len = min(max(cost_len, 1), curve_cap);                     // (clamped: mbx_debug_write_state is caller data)
    const bool stop_rule = !isnan(P.optimum) && bp.early_stop;
    const double lb = P.lb, ub = P.ub;
    double* cost = sc + MBX_NSCALAR;
    const int set = ar.set_of ? min(max(ar.set_of[b], 0), ar.n_sets - 1) : 0;     // (clamped: the host has checked the table)

    stage_problem(P, L.eval());
    for (int e = tid; e < NE; e += kThreads) L.XR[e] = S[MBX_LES_ST_PARENTS(NP, D) + e];
    if (tid < NP) L.NC[tid] = S[MBX_LES_ST_COST(NP, D) + tid];
    if (tid < D) {
        L.MU[tid] = S[MBX_LES_ST_MU(NP, D) + tid]; L.SIG[tid] = S[MBX_LES_ST_SIGMA(NP, D) + tid];
        for (int k = 0; k < 3; ++k) { L.PC[k * D + tid] = S[MBX_LES_ST_PC(NP, D) + k * D + tid]; L.PS[k * D + tid] = S[MBX_LES_ST_PS(NP, D) + k * D + tid]; }
    }
    for (int k = tid; k < kLesNParam; k += kThreads) L.PRM[k] = ar.params[(int64_t)set * kLesNParam + k];
    __syncthreads();

    const FastDiv fd(D);
    const float inv_scale = 1.f / (float)2.8284271247461903;         // tensor / np.sqrt(8): torch multiplies by the float32 reciprocal of a scalar divisor
    bool done = false;
    int step = skip ? ar.step0 : 0;
    for (int it = 0; it < ar.n_gens && !done; ++it) {
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(t + 1), episode};
        if (tid < 64) {                                              // ---- the two networks and the D-wide update (:130-143), wave 0
            if (tid < NP) {                                          // cal_attn_feature (:86-95), then Q, K, V of row tid
                static_assert(NP <= 128, "np_sum_block is numpy's order for n <= 128");
                const double mean = np_sum_block([&](int k) { return L.NC[k]; }, NP) / NP;
                const double var = np_sum_block([&](int k) { const double x = L.NC[k] - mean; return x * x; }, NP) / NP;
                const double c = L.NC[tid];
                const double z = (c - mean) / (sqrt(var) + 1e-8);
                int arg = 0;                                         // np.argsort(costs)[tid]: the row whose (cost, row) has rank tid
                for (int i = 0; i < NP; ++i) {
                    const double ci = L.NC[i];
                    int r = 0;
                    for (int j = 0; j < NP; ++j) { const double o = L.NC[j]; r += (o < ci || (o == ci && j < i)) ? 1 : 0; }
                    arg = r == tid ? i : arg;
                }
                const float x0 = (float)z, x1 = (float)((double)arg / NP - 0.5), x2 = c < gbest ? 1.f : 0.f;
                const float* p = L.PRM;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float q = p[kLesBq + k], kk = p[kLesBk + k];
                    q = fmaf(p[kLesWq + 3 * k], x0, q); q = fmaf(p[kLesWq + 3 * k + 1], x1, q); q = fmaf(p[kLesWq + 3 * k + 2], x2, q);
                    kk = fmaf(p[kLesWk + 3 * k], x0, kk); kk = fmaf(p[kLesWk + 3 * k + 1], x1, kk); kk = fmaf(p[kLesWk + 3 * k + 2], x2, kk);
                    L.Q[tid * 8 + k] = q; L.K[tid * 8 + k] = kk;
                }
                float v = p[kLesBv];
                v = fmaf(p[kLesWv], x0, v); v = fmaf(p[kLesWv + 1], x1, v); v = fmaf(p[kLesWv + 2], x2, v);
                L.V[tid] = v;
            }
            wave_lds_fence();
            if (tid < NP) {                                          // softmax(Q K^T / sqrt(8)) V of row tid (:29-30)
                float s[kLesNP];
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc = fmaf(L.Q[tid * 8 + k], L.K[j * 8 + k], acc);
                    s[j] = acc * inv_scale;
                    m = fmaxf(m, s[j]);
                }
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NP; ++j) { s[j] = expf(s[j] - m); sum += s[j]; }
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < NP; ++j) a = fmaf(s[j] / sum, L.V[j], a);
                L.A[tid] = a;
            }
            wave_lds_fence();
            if (tid < NP) L.W[tid] = les_softmax16(L.A, tid);         // softmax over the 16 rows (:30)
            wave_lds_fence();
            if (tid < D) {                                           // cal_mlp_feature (:97-114), LrNet (:38-40), mu and sigma (:140-143)
                const int d = tid;
                const double mu = L.MU[d], sg = L.SIG[d];
                double s1 = 0., s2 = 0., s3 = 0.;
                for (int i = 0; i < NP; ++i) {                       // np.sum(.., axis=0): row after row
                    const double df = L.XR[i * D + d] - mu, w = (double)L.W[i];
                    s1 += df * w; s2 += df / sg * w; s3 += df * df * w;
                }
                float f[19];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double a = k == 0 ? 0.1 : k == 1 ? 0.5 : 0.9;
                    const double pc = L.PC[k * D + d], ps = L.PS[k * D + d];
                    const double npc = (1 - a) * pc + a * (s1 - pc), nps = (1 - a) * ps + a * (s2 - ps);
                    L.PC[k * D + d] = npc; L.PS[k * D + d] = nps;
                    f[k] = (float)npc; f[3 + k] = (float)nps;
                }
                if (t >= 0 && t <= ar.horizon) {
                    const float* ts = ar.ts + (int64_t)t * kLesNTs;
#pragma unroll
                    for (int k = 0; k < kLesNTs; ++k) f[6 + k] = ts[k];
                } else {                                             // past the table (a skip_step call far beyond the budget): the device's tanh
#pragma unroll
                    for (int k = 0; k < kLesNTs; ++k) f[6 + k] = (float)tanh((double)t / (double)les_stamp(k) - 1.);
                }
                const float* p = L.PRM;
                float h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float acc = p[kLesB1 + k];
#pragma unroll
                    for (int j = 0; j < 19; ++j) acc = fmaf(p[kLesW1 + 19 * k + j], f[j], acc);
                    h[k] = acc;
                }
                float al[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    float acc = p[kLesB2 + m];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc = fmaf(p[kLesW2 + 8 * m + k], h[k], acc);
                    al[m] = 1.f / (1.f + expf(-acc));
                }
                L.AL[2 * d] = al[0]; L.AL[2 * d + 1] = al[1];
                L.MU[d] = (double)(1.f - al[0]) * mu + (double)al[0] * s1;
                L.SIG[d] = (double)(1.f - al[1]) * sg + (double)al[1] * sqrt(s3);
            }
        }
        les_normals(L, NE, rng, tape ? tape + MBX_LES_TAPE_Z(NP, D) : nullptr);
        __syncthreads();                                              // mu, sigma and z go to the sampler
        for (int e = tid; e < NE; e += kThreads) L.XR[e] = les_clip(L.MU[fd.mod(e)] + L.SIG[fd.mod(e)] * L.ZN[e], lb, ub);   // :145
        __syncthreads();                                              // the children go to the evaluator
        eval_rows(P, L.eval(), NP);                                   // :147; its last barrier hands the costs to every thread
        les_noise(P, L, rng, tape ? tape + MBX_LES_TAPE_NOISE(NP, D) : nullptr);
        fes += NP;                                                    // :148
        double cmin = L.NC[0];
        for (int i = 1; i < NP; ++i) cmin = les_min(L.NC[i], cmin);
        gbest = les_min(cmin, gbest);                                 // :149
        if (skip ? step == 0 : t == 0) init_y = gbest;                // :150-151
        t += 1;
        done = fes >= bp.max_fes || (stop_rule && gbest <= 1e-8);     // :162-165
        step += 1;
        if (skip) done = step >= ar.skip_total;                       // :167-168
        if ((double)fes >= (double)log_index * bp.log_interval) {    // :170-172, once
            log_index += 1;
            if (cost_len < curve_cap) { if (tid == 0) cost[cost_len] = gbest; cost_len += 1; }
        }
        if (done) {                                                   // :174-178
            if (cost_len >= bp.n_logpoint + 1) { if (tid == 0) cost[cost_len - 1] = gbest; }
            else { if (tid == 0) cost[cost_len] = gbest; cost_len += 1; }
        }
    }
    __syncthreads();
    // ---- the state block, once per launch
    for (int e = tid; e < NE; e += kThreads) { S[MBX_LES_ST_PARENTS(NP, D) + e] = L.XR[e]; S[MBX_LES_ST_Z(NP, D) + e] = L.ZN[e]; }
    if (tid < NP) { S[MBX_LES_ST_COST(NP, D) + tid] = L.NC[tid]; S[MBX_LES_ST_W(NP, D) + tid] = (double)L.W[tid]; }
    if (tid < D) {
        S[MBX_LES_ST_MU(NP, D) + tid] = L.MU[tid]; S[MBX_LES_ST_SIGMA(NP, D) + tid] = L.SIG[tid];
        for (int k = 0; k < 3; ++k) { S[MBX_LES_ST_PC(NP, D) + k * D + tid] = L.PC[k * D + tid]; S[MBX_LES_ST_PS(NP, D) + k * D + tid] = L.PS[k * D + tid]; }
        S[MBX_LES_ST_ALPHA(NP, D) + 2 * tid] = (double)L.AL[2 * tid]; S[MBX_LES_ST_ALPHA(NP, D) + 2 * tid + 1] = (double)L.AL[2 * tid + 1];
    }
    if (tid == 0) {
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len; sc[MBX_SC_GEN] = t;
        sc[skip ? MBX_SC_LES_CALL_INIT_Y : MBX_SC_LES_INIT_Y] = init_y;
        const double reward = (init_y - gbest) / init_y;              // :180
        if (!skip) { sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_RETURN] = reward; }
        if (state_out) state_out[b] = gbest;
        if (reward_out) reward_out[b] = reward;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
}

}  // namespace mbx
