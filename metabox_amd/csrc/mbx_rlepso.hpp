// mbx_rlepso.hpp — fused RLEPSO generation kernels for gfx950.
//
// One workgroup (256 threads = 4 waves) owns one (problem x run) instance.  Per launch it streams the
// instance's state block in from HBM, keeps pbest positions / candidate positions / evaluation scratch
// in LDS, performs one whole RLEPSO_Optimizer.update() (reference: src/optimizer/rlepso_optimizer.py:
// 173-263) including the objective evaluation, and streams the state back out.
//
// Mapping: element e = i*D + d (particle i, dimension d) is owned by thread e % 256; particle-level work
// (pbest/stagnation bookkeeping) is done by thread i; argmin uses wave shuffles.
#pragma once
#include "mbx_device.hpp"
#include "mbx_lds.hpp"

namespace mbx {

struct BatchParams {
    const DevProblem* problems;
    const int32_t* problem_idx;
    const uint64_t* seeds;
    double* state;               // [B][state_stride]
    int64_t state_stride;
    const double* tape;          // nullptr -> Philox
    int64_t tape_stride;
    const int32_t* order;        // launch order: workgroup w owns instance order[w] (most expensive objectives first)
    const double* pci;           // [NP] RLEPSO learning-probability curve pci_i (rlepso_optimizer.py:23-24), computed at batch creation
    int32_t NP, D, max_fes, log_interval, n_logpoint, early_stop, n_group, B;
    int64_t sc_off;              // offset of the scalar block inside an instance's state (per algorithm)
    unsigned long long* clk;     // nullptr, or 2 words {sum of shader cycles (s_memtime), sum of 100 MHz ticks (s_memrealtime)} over the lifetimes of the resident RLEPSO kernel's
                                 // workgroups (mbx_debug_clock_slots; bench.py prices the kernel's vector-issue bound at the clock its own waves saw)
};

// optimizer.cost bookkeeping shared by every update() of the reference (e.g. rlepso_optimizer.py:241-261): append gbest when fes
// reaches the next log point (one append per call at most), decide termination, and on termination overwrite the last entry if the
// curve is already n_logpoint + 1 long, else append.  `cost` is the instance's curve in HBM; returns is_done.
//
// The curve bound (include/mbx.h): the log-point append is unguarded in the reference, so its list can outgrow the n_logpoint + 1 slots of an instance's curve
// (maxFEs = 976, log_interval = 19: 52 entries).  Every curve write goes through curve_put: a write to an index past n_logpoint -- an append or the closing
// overwrite -- is dropped, and cost_len goes on counting, so the slots hold the first n_logpoint + 1 entries of the reference's list and MBX_SC_COST_LEN its length.
__device__ __forceinline__ void curve_put(double* __restrict__ cost, int n_logpoint, int idx, double v)
{
    if (idx <= n_logpoint) cost[idx] = v;
}

template <class PT>
__device__ __forceinline__ bool log_and_terminate(const BatchParams& bp, const PT& P, double fes, double gbest, int& log_index,
                                                  int& cost_len, double* __restrict__ cost)
{
    if (fes >= (double)log_index * bp.log_interval) { log_index += 1; curve_put(cost, bp.n_logpoint, cost_len++, gbest); }
    bool done = fes >= bp.max_fes;
    if (!isnan(P.optimum) && bp.early_stop) done = done || gbest <= 1e-8;
    if (done) {
        if (cost_len >= bp.n_logpoint + 1) curve_put(cost, bp.n_logpoint, cost_len - 1, gbest);
        else curve_put(cost, bp.n_logpoint, cost_len++, gbest);
    }
    return done;
}

// The same bookkeeping as MadDE, NL_SHADE_LBC and JDE21 keep it: the log-point append is guarded, so once the curve holds its n_logpoint + 1
// entries no further log point is appended and cost_len stops counting there.  (RL-HPSDE, which shares its other phases with MadDE and
// NL_SHADE_LBC, uses the unguarded rule above.)
template <class PT>
__device__ __forceinline__ bool log_and_terminate_guarded(const BatchParams& bp, const PT& P, double fes, double gbest, int& log_index,
                                                          int& cost_len, double* __restrict__ cost)
{
    if (fes >= (double)log_index * bp.log_interval) { log_index += 1; if (cost_len <= bp.n_logpoint) curve_put(cost, bp.n_logpoint, cost_len++, gbest); }
    bool done = fes >= bp.max_fes;
    if (!isnan(P.optimum) && bp.early_stop) done = done || gbest <= 1e-8;
    if (done) {
        if (cost_len >= bp.n_logpoint + 1) curve_put(cost, bp.n_logpoint, cost_len - 1, gbest);
        else curve_put(cost, bp.n_logpoint, cost_len++, gbest);
    }
    return done;
}

// The LDS layout (RlLds, rl_z_doubles, rl_lds_doubles, rl_carve) lives in mbx_lds.hpp.

// chunk of the register-resident row in the resident kernel's matvec (matvec_rows_scalar_kc; 0: whole row): at D = 40 the 80 row registers collide
// with the resident velocities / pbest positions
// (config 5, A/B on one box: whole row 2.00 ms, chunks of 20 / 10 / 8: 1.886 / 1.830 / 1.854 ms per generation of 8192 instances in round 2; with the
// fma-chain matvec, round 3: whole row 2.53, chunks of 20 / 10 / 8 / 5 / 4: 1.667 / 1.672 / 1.628 / 1.887 / 1.700 ms -- register allocation, not arithmetic, decides)
#ifndef MBX_RUN_KC40
#define MBX_RUN_KC40 8
#endif
#ifndef MBX_RUN_KC30
#define MBX_RUN_KC30 0
#endif
__host__ __device__ constexpr int rl_run_matvec_chunk(int D) { return D == 40 ? MBX_RUN_KC40 : D == 30 ? MBX_RUN_KC30 : 0; }

// The bbob D = 30 geometry of the reference (NP = 100, rlepso_optimizer.py:9; `--dim 30`): its kernels read the two D x D maps from global memory
// (matvec_rows_scalar) and keep no LDS copy: 90.0 -> 75.6 KB per workgroup, i.e. TWO resident 512-thread workgroups per CU instead of one.
__host__ __device__ constexpr bool rl_maps_in_lds(int NP, int D) { return !(NP == 100 && D == 30); }

// pbest / gbest bookkeeping shared by update() and __reinit() (rlepso_optimizer.py:200-222, 145-168).
// Candidate positions are in L.X, their costs in L.NC.  `stagnation` additionally updates per_no_improve
// against the previous c_cost (:225-233), which only update() does.
__device__ __forceinline__ void rl_commit(const RlLds& L, int NP, int D, bool stagnation, double& gbest, int& gbest_idx,
                                          double* __restrict__ gPB, double* __restrict__ gCC)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < NP; i += MBX_NT) {
        const double nc = L.NC[i];
        if (stagnation) L.PNI[i] = nc < gCC[i] ? 0. : L.PNI[i] + 1;   // c_cost lives in HBM only: thread i is its sole reader/writer
        const int impr = nc < L.PBC[i];
        if (impr) L.PBC[i] = nc;
        L.IMPR[i] = impr;
        gCC[i] = nc;
    }
    double cbv; int cb;
    block_argmin(L.NC, NP, L.RED, cbv, cb);         // contains the barriers that publish IMPR / CC
    const bool better = cbv < gbest;
    if (better) { gbest = cbv; gbest_idx = cb; }
    const int NE = NP * D;
    const FastDiv fd(D);
    for (int e = tid; e < NE; e += MBX_NT) {
        const int i = fd.div(e);
        if (L.IMPR[i]) gPB[e] = L.X[e];                // pbest_position <- new position, straight to HBM
    }
    if (better && tid < D) L.GB[tid] = L.X[cb * D + tid];
    __syncthreads();
}

// Everything the velocity phase needs, bundled so that the per-item routine can be a template on the item width.
struct MoveCtx {
    const RlLds& L; const double* pci; const double* tape; const Rng& rng; double* gPos; double* gVel;
    const int* ORDER; const int* NLESS; const int* RANK; int NP, D, G; double lb, ub, vmax; const FastDiv& fg;
    bool whole_groups;           // NP is a multiple of G and both are compile-time constants: fg.div(i) < G for every particle
};

// Two-headed Gaussian MLP policy (mbx_gauss_mlp in include/mbx.h): RLEPSO's Actor (src/agent/rlepso_agent.py:9-47) and RL-PSO's
// PolicyNetwork (src/agent/rl_pso_agent.py:9-47) share the architecture and differ in the heads.
struct GaussMlp {
    const float* w;              // packed weights
    int32_t in_dim, h1, h2, out_dim;
    float min_sigma, max_sigma;
    int32_t variant;             // MBX_POLICY_RLEPSO / MBX_POLICY_RLPSO
};

__host__ __device__ inline int gauss_mlp_net_floats(int in, int h1, int h2, int A) { return in * h1 + h1 + h1 * h2 + h2 + h2 * A + A; }

// (mu, sigma) from the two nets' raw outputs, float32 like the reference's torch modules
__device__ __forceinline__ void gauss_head(const GaussMlp& net, float am, float as, float& mu, float& sigma)
{
    mu = (tanhf(am) + 1.f) / 2.f;
    if (net.variant == MBX_POLICY_RLPSO) sigma = fminf(fmaxf((tanhf(as) + 1.f) / 2.f, net.min_sigma), net.max_sigma);   // rl_pso_agent.py:27-29
    else sigma = (tanhf(as) + 1.f) / 2.f * (net.max_sigma - net.min_sigma) + net.min_sigma;                               // rlepso_agent.py:25
}

// Normal(mu, sigma).sample() with the instance's Philox stream, then the agent's post-processing:
//   RLEPSO: clamp to [0, 1] (rlepso_agent.py:32);  RL-PSO: samples outside [0, 1) are re-folded as
//   (a + 3 sigma - mu) * (1/6 * sigma) (rl_pso_agent.py:34-35, precedence as written there).
// The policy is float32 and its noise has no counterpart in the reference (torch's global generator), so Box-Muller runs on the
// hardware float32 transcendentals: v_log_f32 (log2) and v_cos_f32 (argument in revolutions, i.e. cos(2 pi u) directly).
__device__ __forceinline__ float sample_action(const Rng& rng, int j, float mu, float sigma, int variant)
{
    const U4 w = rng.draw((uint32_t)j, MBX_SITE_POLICY);
    const float u1 = (float)((w.x >> 8) + 1u) * 5.9604644775390625e-8f;      // (0, 1]
    const float u2 = (float)(w.y >> 8) * 5.9604644775390625e-8f;             // [0, 1)
    const float r = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));     // sqrt(-2 ln u1)
    const float a = mu + sigma * (r * __builtin_amdgcn_cosf(u2));
    if (variant == MBX_POLICY_RLPSO) return fabsf(a - 0.5f) >= 0.5f ? (a + 3.f * sigma - mu) * ((1.f / 6.f) * sigma) : a;
    return fminf(fmaxf(a, 0.f), 1.f);
}

// Per-phase wall-cycle accounting of k_rlepso_step (instrumented builds only: -DMBX_PHASE_TIMING; tools/kbench.py --phases).
#ifdef MBX_PHASE_TIMING
__device__ unsigned long long g_phase_cycles[8192 * 16];         // [block][phase], no atomics: plain accumulation by the owning block
#define MBX_PHASE_BEGIN unsigned long long ph_t = clock64();
#define MBX_PHASE(k) do { if (threadIdx.x == 0) { const unsigned long long t_ = clock64(); g_phase_cycles[(blockIdx.x & 8191) * 16 + (k)] += t_ - ph_t; ph_t = t_; } } while (0)
#else
#define MBX_PHASE_BEGIN
#define MBX_PHASE(k)
#endif

// 256-thread workgroups: 29.8 KB of LDS lets five of them share a CU, so cap the registers at 96 for five waves per SIMD (-5.7 % against
// four; two VGPRs spill).  The 512- / 1024-thread instantiations own their CU and only need the four waves per SIMD a 1024-thread workgroup is.
#ifndef MBX_RL_WAVES
#define MBX_RL_WAVES __attribute__((amdgpu_waves_per_eu(THREADS == 256 ? 5 : 4)))
#endif
#ifndef MBX_FDR_UNROLL
#define MBX_FDR_UNROLL 4
#endif
#ifndef MBX_FDR_UNROLL_D40
#define MBX_FDR_UNROLL_D40 2        // the D = 40 resident kernels (1024 threads; config 5)
#endif
// Unrolled groups per iteration of the scan's main loop in the resident 256-thread kernels (fdr_exact: GR).  The groups of an iteration are loaded and compared one after the
// other -- the register footprint is the one of MBX_FDR_UNROLL candidates -- and read the two LDS streams at constant offsets from ONE pair of address registers, which
// advance once per iteration instead of once per group.  1: one group per iteration and an indexed remainder loop, as every other kernel keeps them (the A/B switch).
#ifndef MBX_FDR_GROUPS
#define MBX_FDR_GROUPS 3
#endif
// The waves of the resident 256-thread kernels run at priority 1 outside the FDR pass and at 0 inside it: vector issue is arbitrated by priority, then age, and five
// workgroups share a CU, so the short dependency-bound phases (policy, ranking, move, objective, commit) of one workgroup are served ahead of the other workgroups' scans,
// which fill whatever is left (docs/EXPERIMENTS.md: -2.3 % / -2.5 % on the headline, no instruction saved).  s_setprio ignores EXEC: all three sit in straight-line code of
// the generation loop that every wave of the workgroup runs.  0: no s_setprio at all (the A/B switch).  The 512- / 1024-thread kernels own their CU and were not measured.
// 2: the same, and level 2 around the phases only wave 0 runs (policy draw, block_argmin's index step, thread 0's logging) and the ones only the waves that hold particles
// run (the ranking's per-particle step, the re-initialisation draw), back to 1 in front of the next barrier: every wave of the workgroup executes each s_setprio (the waves
// without work in the phase go from 2 to 1 a few instructions later, at the barrier they wait at).  Measured and not shipped (docs/EXPERIMENTS.md).
#ifndef MBX_RL_PRIO
#define MBX_RL_PRIO 1
#endif
#ifndef MBX_FDR_OWN_AT
#define MBX_FDR_OWN_AT 64           // flagged items per swarm and generation above which every lane settles its own items instead of one wave per coordinate (fdr_pass)
#endif

// if (lhs < rhs) { ab = a; bb = b; kb = k; } as three EXEC-masked moves (v_cmpx + v_mov_b64 x2 + v_mov_b32) instead of the five
// v_cndmask_b32 the compiler's if-conversion produces: the FDR scan below is VALU-issue bound and this is its innermost statement.
__device__ __forceinline__ void fdr_take(double lhs, double rhs, double& ab, double& bb, int& kb, double a, double b, int k)
{
#ifdef MBX_FDR_BRANCH
    // experiment (tools/fdr_sim/take_stats.py: on real swarms no lane of a wave takes in 50.5 % of the wave-steps): a wave-uniform branch around the masked moves
    if (__builtin_amdgcn_ballot_w64(lhs < rhs) == 0ull) return;
#endif
#ifdef MBX_FDR_SELECT
    if (lhs < rhs) { ab = a; bb = b; kb = k; }
#else
    unsigned long long saved;
    asm("s_mov_b64 %[sv], exec\n\t"
                 "v_cmpx_lt_f64_e32 %[l], %[r]\n\t"
                 "v_mov_b64 %[ab], %[a]\n\t"
                 "v_mov_b64 %[bb], %[b]\n\t"
                 "v_mov_b32 %[kb], %[k]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [ab] "+v"(ab), [bb] "+v"(bb), [kb] "+v"(kb), [sv] "=&s"(saved)
                 : [l] "v"(lhs), [r] "v"(rhs), [a] "v"(a), [b] "v"(b), [k] "s"(k)
                 : "vcc");
#endif
}

// ---- exact resolution of near-ties in the FDR scan (fdr_exact<.., TIE = true>: the DEFAULT of every RLEPSO kernel; TIE = false is the batch option
// MBX_F_FDR_FAST of include/mbx.h) -------------------------------------------------------------------------------------------------
// if (dif < 0) { ab = a; bb = b; kb = k; }: fdr_take on the SIGN of dif = a_j b* - fl(a* b_j) (one fma instead of the second product: same instruction count)
__device__ __forceinline__ void fdr_take_neg(double dif, double& ab, double& bb, int& kb, double a, double b, int k)
{
    unsigned long long saved;
    asm("s_mov_b64 %[sv], exec\n\t"
        "v_cmpx_gt_f64_e32 0, %[d]\n\t"
        "v_mov_b64 %[ab], %[a]\n\t"
        "v_mov_b64 %[bb], %[b]\n\t"
        "v_mov_b32 %[kb], %[k]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [ab] "+v"(ab), [bb] "+v"(bb), [kb] "+v"(kb), [sv] "=&s"(saved)
        : [d] "v"(dif), [a] "v"(a), [b] "v"(b), [k] "s"(k)
        : "vcc");
}
// the two coordinates of a work item in ONE block: both differences are complete before the first compare issues, so neither compare waits on the
// instruction right in front of it
__device__ __forceinline__ void fdr_take_neg2(double dif0, double dif1, double& ab0, double& bb0, int& kb0, double& ab1, double& bb1, int& kb1,
                                              double a, double b0, double b1, int k)
{
    unsigned long long saved;
    asm("s_mov_b64 %[sv], exec\n\t"
        "v_cmpx_gt_f64_e32 0, %[d0]\n\t"
        "v_mov_b64 %[ab0], %[a]\n\t"
        "v_mov_b64 %[bb0], %[b0]\n\t"
        "v_mov_b32 %[kb0], %[k]\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "v_cmpx_gt_f64_e32 0, %[d1]\n\t"
        "v_mov_b64 %[ab1], %[a]\n\t"
        "v_mov_b64 %[bb1], %[b1]\n\t"
        "v_mov_b32 %[kb1], %[k]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [ab0] "+v"(ab0), [bb0] "+v"(bb0), [kb0] "+v"(kb0), [ab1] "+v"(ab1), [bb1] "+v"(bb1), [kb1] "+v"(kb1), [sv] "=&s"(saved)
        : [d0] "v"(dif0), [d1] "v"(dif1), [a] "v"(a), [b0] "v"(b0), [b1] "v"(b1), [k] "s"(k)
        : "vcc");
}
// running minimum of |dif| over the pairs of a scan, kept on the HIGH dwords read as float32 (sign | exponent | 20 mantissa bits of a float64 are monotone in
// the float32 order for finite values): ONE v_min3_f32 covers the two coordinates of a work item
__device__ __forceinline__ float f64_hi_as_f32(double v) { return __int_as_float(__double2hiint(v)); }
__device__ __forceinline__ float fdr_min3_abs(float m, float x, float y)
{
    float r;
    asm("v_min3_f32 %[r], %[m], |%[x]|, |%[y]|" : [r] "=v"(r) : [m] "v"(m), [x] "v"(x), [y] "v"(y));
    return r;
}
// compile-time loop: f(IntC<K>{}) for K = FROM .. TO - 1 (the body sees K as a constant expression, e.g. for an instruction's immediate operand)
template <int K> struct IntC { static constexpr int value = K; };
template <int FROM, int TO, class F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (FROM < TO) { f(IntC<FROM>{}); static_for<FROM + 1, TO>(f); }
}
// old with lane LANE replaced by the wave-uniform value val (v_writelane_b32 with the lane as an immediate)
template <int LANE>
__device__ __forceinline__ int writelane_const(int val, int old)
{
    static_assert(LANE >= 0 && LANE < 64, "a lane of a wave");
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "n"(LANE));
    return old;
}

// Rows of the rank-ordered pbest table that are bitwise copies of the row one rank up -- same cost, same position: particles resting on the same corner of the box (linear
// slope: most of the swarm, for dozens of generations) -- can never be np.argmin's choice (the copy with the lower index precedes them in rank order and ties with them in
// every coordinate), but in the scan each of them is an exact tie with the running best: every item above them would be flagged.  The scan therefore reads their cost as 1e300
// (NCS): a huge positive numerator, never taken, nowhere near a tie.  Called only when equal pbest costs exist in the swarm; thread r owns row r.  The caller synchronises.
// (Measured and dropped: marking single COORDINATES that repeat the one a rank up -- NaN in the table, readers walk up to the value: the walk in the move phase costs every
// batch 7 % and a collapsed linear-slope swarm 2.6x.)
__device__ __forceinline__ void rl_mark_copies(const RlLds& L, int NP, int D, int r)
{
    if (r > 0 && r < NP && L.NC[r] == L.NC[r - 1]) {
        bool same = true;
        for (int d = 0; d < D && same; ++d) same = L.PB[r * D + d] == L.PB[(r - 1) * D + d];
        if (same) L.NCS[r] = 1e300;
    }
}

// A coordinate of an item whose scan met a near-tie (fdr_exact returned true) is settled by its WAVE, lane = candidate: the reference's own rule (rlepso_optimizer.py:
// 100-102: rounded quotients, np.argmin = the first minimal one in PARTICLE order) applied to the scan's winner w and to every candidate that is not CLEARLY worse than w.
//  * dif_k = fma(a_k, b_w, -fl(a_w b_k)) > 2^-49 |a_w b_k| means the exact ratios differ by > 2^-49.2 relative, i.e. the rounded quotient of k is strictly
//    larger than w's: k cannot be the argmin (one pass over the candidates, 64 per step, no division);
//  * candidates bitwise identical to w (same cost, same coordinate: collapsed swarms, coordinates clipped onto a bound) share w's quotient; ranks are (cost, index)-ordered,
//    so the lowest RANK among w and its copies is np.argmin's lowest index -- no division either (the scan's fma may have taken a later copy: its rounding error has a sign);
//  * only if a DIFFERENT candidate is within the band -- a true near-tie, or one clearly better than w, should an earlier near-tie have misled the scan -- the contenders
//    compete with their rounded quotients, lowest particle index among equal ones (ORDER maps ranks to particle indices).
// Exact by construction.  All arguments are wave-uniform, all 64 lanes are active; returns the exemplar's rank (uniform).  Measured on whole episodes of the 24 functions:
// 0.02-0.15 % of the items are flagged, late in an episode up to 0.5 % (Gallagher); every lane redoing its own flagged item would stall the 64 lanes of each wave that holds
// one (6.7 % of the wave-passes at 0.1 %) for a second scan, this form costs the wave ~200 instructions per flagged coordinate.
__device__ __forceinline__ int fdr_settle(const RlLds& L, const int* __restrict__ ORDER, int D, int rk, int d, int nless, int kw, unsigned long long* cnt = nullptr)
{
    const int lane = threadIdx.x & 63;
    const double fi = L.NC[rk];
    const double pp = L.PB[rk * D + d];
    const double aw = L.NC[kw] - fi, bw = fabs(L.PB[kw * D + d] - pp) + 1e-5;
    int first_copy = 0x7fffffff;
    bool others = false;
    for (int k0 = 0; k0 < nless; k0 += 64) {
        const int k = k0 + lane;
        bool band = false, copy = false;
        if (k < nless && k != kw) {
            const double a = L.NC[k] - fi, b = fabs(L.PB[k * D + d] - pp) + 1e-5, pr = aw * b;
            band = __builtin_fma(a, bw, -pr) <= pr * -0x1p-49;      // (pr < 0: the band is 2^-49 |a_w b_k|, the product at hand -- tighter than the scan's flag)
            copy = band && a == aw && b == bw;
        }
        const unsigned long long mc = __builtin_amdgcn_ballot_w64(copy), mo = __builtin_amdgcn_ballot_w64(band && !copy);
        if (mc != 0ull && first_copy == 0x7fffffff) first_copy = k0 + (int)__builtin_ctzll(mc);
        others = others || mo != 0ull;
    }
    int kbest = kw < first_copy ? kw : first_copy;
#ifdef MBX_FDR_COUNT
    if (cnt && lane == 0) atomicAdd(cnt + (others ? 5 : first_copy != 0x7fffffff ? 4 : 6), 1ull);     // experiment: what the flagged coordinates turn out to be
#endif
    if (others) {                                             // wave-uniform, rare: a different candidate within (or below) the band
        double qb = aw / bw;
        int ib = ORDER[kbest];
        for (int k0 = 0; k0 < nless; k0 += 64) {
            const int k = k0 + lane;
            bool cont = false;
            double qk = 0.;
            int ik = 0;
            if (k < nless && k != kw) {
                const double a = L.NC[k] - fi, b = fabs(L.PB[k * D + d] - pp) + 1e-5, pr = aw * b;
                cont = __builtin_fma(a, bw, -pr) <= pr * -0x1p-49 && !(a == aw && b == bw);
                if (cont) { qk = a / b; ik = ORDER[k]; }
            }
            unsigned long long m = __builtin_amdgcn_ballot_w64(cont);
            while (m != 0ull) {
                const int l = (int)__builtin_ctzll(m);
                m &= m - 1ull;
                const double ql = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(qk), l), __builtin_amdgcn_readlane(__double2loint(qk), l));
                const int il = __builtin_amdgcn_readlane(ik, l);
                if (ql < qb || (ql == qb && il < ib)) { qb = ql; ib = il; kbest = k0 + l; }
            }
        }
    }
    return kbest;
}

// ---- FDR exemplar (rlepso_optimizer.py:97-109): argmin_j (pbest_j - pbest_i)/(|p_jd - p_id| + 1e-5), first minimum.
//  * j == i contributes the ratio 0, every particle with a larger pbest a positive one: the minimum is attained
//    among the strictly better particles (negative ratios) if there are any, otherwise it is 0 and np.argmin
//    returns the lowest index with pbest_j == pbest_i.  Only the `nless` better particles are scanned, in
//    ascending-cost order (ORDER / NC), halving the O(NP^2 D) work on average (a wave runs on to the highest rank among its items, see `bound` below).
//  * ratios are compared by cross-multiplication (denominators >= 1e-5 > 0): a_j/b_j < a*/b* <=> a_j b* < a* b_j.
//    The reference compares ROUNDED quotients; the two orders can differ only where two candidates' quotients are within an ulp or two of each other
//    (tests/test_fdr_ties.py: 49 % / 9 % of crafted pairs 0 / 1 ulp apart resolve differently by cross-multiplication alone).
//  * TIE = true (default): every comparison also yields dif = a_j b* - fl(a* b_j); while |dif| > 8 ulp of the products both forms decide alike (a quotient pair
//    that rounds together or apart differs by <= 1 ulp, i.e. |a_j b* - a* b_j| <= 2^-52 |a* b_j|).  The scan keeps min |dif| (high dwords, one v_min3_f32 per
//    two coordinates and candidate) and reports whether it came within 2^-49 x the largest product an item can form, |a_0| x range; the caller then runs
//    fdr_settle on the item.  Bit-exact exemplars on any input whose pbest positions lie inside the box (|p_jd - p_id| <= ub - lb).
//  * TIE = false (MBX_F_FDR_FAST): the cross-multiplied order alone, two products and a compare; identical candidates (same pbest cost and same coordinate)
//    are adjacent in the (cost, index) order, so the strict `<` keeps the lower index like np.argmin.
// Exact float64 scan for W adjacent coordinates d0 .. d0+W-1 of the particle of pbest-rank rk; the exemplar's rank per coordinate goes to kb; returns the near-tie flag.
// The candidates' costs are read from NCS (= NC but for the rows rl_mark_copies took out of the scan).
//  * The loops run to ONE trip count per wave, `bound` (wave-uniform, >= the nless of every lane of the wave, <= NP: fdr_pass passes the highest rank among the
//    wave's items, and nless(rank) <= rank), not to the lane's own nless: counter, loop test and the rank k handed to the takes live on the scalar unit, and the
//    remainder is (bound - 1) mod UN scalar-controlled steps.  (Per-lane trip counts made the loop a divergent one -- a vector compare, a vector counter and EXEC
//    bookkeeping per group, 22 instead of 18 instructions per remainder candidate -- and bought nothing: a lane that is done is masked off while the wave finishes.)
//    A lane that scans past its nless gets the same (ab, bb, kb) and the same flag:
//    - never taken: positions are in (cost, index) order and rows taken out read 1e300, so a candidate at k >= nless has au = NCS[k] - f_i >= 0.  A lane with
//      nless > 0 holds a running best with ab < 0 and bb, b >= 1e-5: dif = fma(au, bb, -fl(ab b)) >= 0, and the strict test 0 > dif fails.  A lane with nless == 0
//      holds ab = a_0 = 0: dif = au bb >= 0 again; its kb stays 0 = nless, the rank of the exemplar when nobody is strictly better.
//    - flag unchanged: a running best has won against candidate 0, so |ab| >= |a_0| bb / b_0 >= |a_0| 1e-5 / range (up to an ulp per comparison), and an extra
//      candidate contributes |dif| >= |ab| b >= |a_0| 1e-10 / range ~ |a_0| 2^-36.5 (range ~ 10) against the threshold |a_0| range 2^-49 ~ |a_0| 2^-45.7: a factor
//      of 2^9 above it (tests/test_fdr_bound.py asserts the margin on real and crafted swarms).  Only a lane with nless == 0 (a_0 = 0: threshold 0, dif = 0 at
//      its cost-ties) has its flag forced to false, which is what its early return used to say.
//    With equal costs the bound overshoots nless by the tied particles only.  No position at or beyond NP is read: the bound is at most a rank.
// UN: candidates per unrolled group (MBX_FDR_UNROLL = 4 everywhere but config 5's resident kernel: 1024 threads, D = 40: 2 / 4 / 8 -> 1.619 / 1.641 / 1.703 ms per
// generation; the headline kernel: 2 / 3 / 4 / 6 / 8 -> 119.9 / 117.1 / 116.5 / 117.5 / 121.6 us; both with per-lane trip counts)
// range: an upper bound of |p_jd - p_id| + 1e-5 (ub - lb + 1e-5), used by the near-tie flag only
// The scan does not read the item's nless: the only thing it decided was `nless > 0` in the flag, and that is a_0 < 0 (NC is in ascending order: somebody is strictly
// better than the item exactly when the best cost is below its own; a NaN cost answers false both ways) -- a compare on a register the scan holds anyway, where
// NLESS[ORDER[rk]] was two dependent LDS reads and their address arithmetic per item.
// GR: groups per iteration of the main loop (MBX_FDR_GROUPS in the resident 256-thread kernels, 1 everywhere else).  With GR > 1 the scan walks two pointers, pc into the
// cost column and pr into the position rows: the main loop covers GR x UN candidates per trip -- group g at pc + g UN and pr + g UN D, constant offsets in the LDS
// instructions -- and advances both once; whole groups that are left (at most GR - 1) go one per trip; the remainder, at most UN - 1 candidates, is straight-line code at
// constant offsets behind scalar tests, with no address arithmetic of its own.  The candidates are visited in the same order, k = 1 .. bound - 1 each exactly once, through
// the same `step`: same exemplars, same flag, and nothing at or beyond `bound` is read (tests/test_gpu_rlepso_trims3.py restates the trip arithmetic).
template <int W, int UN = MBX_FDR_UNROLL, bool TIE = true, int GR = 1>
__device__ __forceinline__ bool fdr_exact(const RlLds& L, int D, int rk, int d0, int bound, int kb[W], double range = 0.)
{
#ifdef MBX_ABLATE_FDR_SCAN
    bound = 1;                                                    // instruction-budget builds: the head and the tail of the scan without its loops
#endif
    const double fi = L.NC[rk];
    double pp[W], ab[W], bb[W];
    const double a0 = L.NC[0] - fi;
#pragma unroll
    for (int q = 0; q < W; ++q) { pp[q] = L.PB[rk * D + d0 + q]; kb[q] = 0; ab[q] = a0; bb[q] = fabs(L.PB[d0 + q] - pp[q]) + 1e-5; }
    const double* col = L.PB + d0;
    if constexpr (TIE) {
    float tiem = __int_as_float(0x7f000000);
    // one candidate against the running best of the W coordinates: the W differences are complete before the first compare issues (fdr_take_neg2)
    auto step = [&](double au, const double (&x)[W], int k) {
        double b[W], difv[W];
#pragma unroll
        for (int q = 0; q < W; ++q) b[q] = fabs(x[q] - pp[q]) + 1e-5;
#pragma unroll
        for (int q = 0; q < W; ++q) difv[q] = ab[q] * b[q];
#pragma unroll
        for (int q = 0; q < W; ++q) difv[q] = __builtin_fma(au, bb[q], -difv[q]);
        if constexpr (W == 2) fdr_take_neg2(difv[0], difv[1], ab[0], bb[0], kb[0], ab[1], bb[1], kb[1], au, b[0], b[1], k);
        else {
#pragma unroll
            for (int q = 0; q < W; ++q) fdr_take_neg(difv[q], ab[q], bb[q], kb[q], au, b[q], k);
        }
        tiem = fdr_min3_abs(tiem, f64_hi_as_f32(difv[0]), f64_hi_as_f32(difv[W - 1]));
    };
    if constexpr (GR > 1) {
    const double* pc = L.NCS + 1;                                 // candidate k's cost
    const double* pr = col + D;                                   // and its row
    // one unrolled group: the LDS reads of its UN candidates are issued before its first comparison
    auto group = [&](const double* c, const double* r, int k) {
        double a[UN], x[UN][W];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            a[u] = c[u];
            // (W == 2: an even coordinate of a row of even D -- one 16-byte read per candidate, as with indices)
            if constexpr (W == 2) { const double2 v = *(const double2*)(r + u * D); x[u][0] = v.x; x[u][1] = v.y; }
            else {
#pragma unroll
                for (int q = 0; q < W; ++q) x[u][q] = r[u * D + q];
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) step(a[u] - fi, x[u], k + u);
    };
    int k = 1;
    for (; k + GR * UN <= bound; k += GR * UN) {
        static_for<0, GR>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            group(pc + g * UN, pr + g * UN * D, k + g * UN);
            __builtin_amdgcn_sched_barrier(0);                    // the next group's reads stay behind this group's comparisons: UN candidates in registers, not GR x UN
        });
        pc += GR * UN; pr += GR * UN * D;
    }
    for (; k + UN <= bound; k += UN) { group(pc, pr, k); pc += UN; pr += UN * D; }
    static_for<0, UN - 1>([&](auto rc) {                          // the remainder: k + r < bound implies k + r - 1 < bound, the tests nest
        constexpr int r = decltype(rc)::value;
        if (k + r < bound) {
            double x[W];
            if constexpr (W == 2) { const double2 v = *(const double2*)(pr + r * D); x[0] = v.x; x[1] = v.y; }
            else {
#pragma unroll
                for (int q = 0; q < W; ++q) x[q] = pr[r * D + q];
            }
            step(pc[r] - fi, x, k + r);
        }
    });
    } else {
    int k = 1;
    for (; k + UN <= bound; k += UN) {
        double a[UN], x[UN][W];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            a[u] = L.NCS[k + u];
#pragma unroll
            for (int q = 0; q < W; ++q) x[u][q] = col[(k + u) * D + q];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) step(a[u] - fi, x[u], k + u);
    }
    for (; k < bound; ++k) {
        double x[W];
#pragma unroll
        for (int q = 0; q < W; ++q) x[q] = col[k * D + q];
        step(L.NCS[k] - fi, x, k);
    }
    }
    const double thr = fabs(a0) * range * 0x1p-49;               // |a* b_j| <= |a_0| x range for every pair of the item
    return a0 < 0. && !(tiem > f64_hi_as_f32(thr) * 1.0000005f);
    } else {
    // unrolled by hand (the compiler does not unroll around the inline assembly of fdr_take); the LDS reads of a group are
    // issued before its first comparison
    int k = 1;
    for (; k + UN <= bound; k += UN) {
        double a[UN], x[UN][W];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            a[u] = L.NCS[k + u];
#pragma unroll
            for (int q = 0; q < W; ++q) x[u][q] = col[(k + u) * D + q];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const double au = a[u] - fi;                      // shared by the W coordinates
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const double b = fabs(x[u][q] - pp[q]) + 1e-5;
                fdr_take(au * bb[q], ab[q] * b, ab[q], bb[q], kb[q], au, b, k + u);
            }
        }
    }
    for (; k < bound; ++k) {
        const double a = L.NCS[k] - fi;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const double b = fabs(col[k * D + q] - pp[q]) + 1e-5;
            fdr_take(a * bb[q], ab[q] * b, ab[q], bb[q], kb[q], a, b, k);
        }
    }
    return false;
    }
}

// The same settlement by the item's OWN lane (both coordinates): what a swarm that has collapsed onto the rounding floor of its costs gets, where most items are flagged and
// one wave per coordinate would take longer than a second pass of everybody (fdr_pass switches at 64 flagged items).
template <int W>
__device__ __noinline__ void fdr_settle_own(const double* __restrict__ NC, const double* __restrict__ PB, const int* __restrict__ ORDER, int D, int rk, int d0, int nless, int* kb)
{
    const double fi = NC[rk];
    double pp[W], aw[W], bw[W];
    int kw[W], first_copy[W];
    bool others[W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        kw[q] = kb[q];
        pp[q] = PB[rk * D + d0 + q];
        aw[q] = NC[kw[q]] - fi;
        bw[q] = fabs(PB[kw[q] * D + d0 + q] - pp[q]) + 1e-5;
        first_copy[q] = 0x7fffffff; others[q] = false;
    }
    for (int k = 0; k < nless; ++k) {                              // pass 1: who is inside the band of the winner?  copies of it, or somebody else?
        const double a = NC[k] - fi;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const double b = fabs(PB[k * D + d0 + q] - pp[q]) + 1e-5, pr = aw[q] * b;
            if (__builtin_fma(a, bw[q], -pr) <= pr * -0x1p-49 && k != kw[q]) {
                if (a == aw[q] && b == bw[q]) { if (first_copy[q] == 0x7fffffff) first_copy[q] = k; }
                else others[q] = true;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < W; ++q) {
        kb[q] = kw[q] < first_copy[q] ? kw[q] : first_copy[q];
        if (others[q]) {                                          // pass 2, rare: rounded quotients, lowest particle index among equal ones
            double qb = aw[q] / bw[q];
            int ib = ORDER[kb[q]];
            for (int k = 0; k < nless; ++k) {
                const double a = NC[k] - fi, b = fabs(PB[k * D + d0 + q] - pp[q]) + 1e-5, pr = aw[q] * b;
                if (__builtin_fma(a, bw[q], -pr) <= pr * -0x1p-49 && k != kw[q] && !(a == aw[q] && b == bw[q])) {
                    const double qk = a / b;
                    const int ik = ORDER[k];
                    if (qk < qb || (qk == qb && ik < ib)) { qb = qk; ib = ik; kb[q] = k; }
                }
            }
        }
    }
}

// The FDR pass of a generation: every (rank, coordinate pair) item of the population -> KB[rank * D + d] = rank of its exemplar.  Items are visited in
// pbest-rank order so that the lanes of a wave own particles of similar rank: the wave scans to ONE trip count, its highest rank (fdr_exact: `bound`), and ~13 ranks
// of NP 100 / D 10 share a wave; the trip count grows with the rank and wave w of
// every resident workgroup shares one SIMD, so odd passes run backwards (boustrophedon): each wave pairs a cheap slice of ranks with an expensive one.
// Items whose scan met a near-tie are appended to the workgroup's list FL (FLN was zeroed before the ranking barrier) and settled after a barrier: up to 64 of them one wave
// per coordinate (fdr_settle), more than that -- a swarm collapsed onto the rounding floor of its costs -- every lane its own (fdr_settle_own: a second pass of everybody is
// then the shorter one).  Ends with the barrier that publishes KB.  Measured and dropped: (a) every lane redoing its own flagged item right away -- 0.1 % of the items stall
// 6.7 % of the wave-passes for a second scan, +10.4 % per generation against +3.5 % of instructions; (b) the flagged lanes' items settled by their own wave right behind
// the pass (readlane + fdr_settle): the serial ~250-instruction chain then sits inside the scan of a wave the other three wait for, +4.8 % in the driver window against
// +3.9 % for the list, +10.6 % against +8.8 % over whole episodes.
//
// The deal (MBX_FDR_DEAL = 1): P = ceil(NI / THREADS) passes hold P THREADS slots, off = P THREADS - NI more than there are items.  In pass p thread tid sits at slot
// s = p THREADS + (p odd ? THREADS - 1 - tid : tid) and owns item s - off; the off slots below zero are idle.  So the 64-item chunks are cut from the TOP of the table
// and the partial chunk is the lowest one, in the first lanes of pass 0: a wave pays for its highest rank, and the chunk that is short of items is then the one that was
// cheapest anyway.  NP 100 / D 10 (500 items, off = 12): bounds 10, 23, 35, 48 | 99, 87, 74, 61, sum 437 -- against 12, 25, 38, 51 | 99, 87, 74, 61 = 447 with the
// partial chunk at the top ranks (MBX_FDR_DEAL = 0: passes filled from item 0, the last one short; the A/B switch) -- and 109 / 110 / 109 / 109 per wave.  A wave all of
// whose slots are idle (NP 100 / D 12: off = 168, waves 0 and 1 of pass 0) skips the scan: its lanes' items are all negative.  Where NI is a multiple of 64 the chunk
// maxima are the same in both deals, and the table is dealt from item 0 as before (fdr_deal_from_top).  Every item is scanned once, through the same `step`, to a bound >= its own rank and <= NP - 1: same exemplars, same flags; only the
// order of FL changes, and each flagged coordinate is settled on its own.
#ifndef MBX_FDR_DEAL
#define MBX_FDR_DEAL 1
#endif
// Which chunk of a pass a wave takes (MBX_FDR_WAVE_DEAL = 1; default 0: chunk w of every pass).  Wave w of every resident workgroup sits on SIMD w, and wave 0 (policy
// draw, block_argmin's index step, logging) and wave 1 (particles 64 .. 99) carry ~330 / ~210 more non-scan vector instructions per generation than waves 2 and 3; a table
// per compile-time geometry (WD of fdr_pass; 0: none) can hand wave 0 a lighter pair of chunks.  WD = 1, NP 100 / D 10 on 256 threads: pass 0 chunks 0, 3, 2, 1 and pass 1
// chunks 1, 3, 2, 0 for waves 0 .. 3, i.e. bounds 10 + 87, 48 + 61, 35 + 74, 23 + 99 = 97 / 109 / 109 / 122 instead of 109 / 110 / 109 / 109: the same eight chunks, so
// the same items, bounds and results.  Measured and not shipped (docs/EXPERIMENTS.md).  -> the first thread of the chunk the wave of first thread w0 takes in `pass`.
#ifndef MBX_FDR_WAVE_DEAL
#define MBX_FDR_WAVE_DEAL 0
#endif
template <int WD>
__device__ __forceinline__ int fdr_deal_chunk(int pass, int w0)
{
    if constexpr (WD == 1) {
        constexpr unsigned tbl[2] = {0x1230u, 0x0231u};           // a nibble per wave
        return (int)((tbl[pass & 1] >> (w0 >> 4)) & 3u) << 6;      // (w0 >> 6) * 4 bits
    } else return w0;
}
// Is the table dealt from the top?  Not where NI is a multiple of 64: every chunk is whole, both deals cut the same chunks and no bound can fall, and there the short pass
// stays the last one -- config 5 (NP 128 / D 40 on 1024 threads, 2560 items, off = 512) measured 1.610 -> 1.691 ms per generation with its eight idle waves in pass 0
// instead of pass 2 (docs/EXPERIMENTS.md).
__device__ __forceinline__ bool fdr_deal_from_top(int NI) { return MBX_FDR_DEAL != 0 && NI % 64 != 0; }
// The item of thread tid (of the wave whose first thread is w0) in pass `pass` (fdr_deal_live: does the slot hold one?), for the scan and for the collapsed-swarm branch
// that settles a lane's own items
template <int THREADS, int WD = 0>
__device__ __forceinline__ int fdr_deal_item(int NI, int pass, int tid, int w0)
{
    if constexpr (WD != 0) tid = fdr_deal_chunk<WD>(pass, w0) + (tid & 63);
    if (fdr_deal_from_top(NI)) {
        const int off = (NI + THREADS - 1) / THREADS * THREADS - NI;
        return pass * THREADS + ((pass & 1) ? THREADS - 1 - tid : tid) - off;
    }
    const int base = pass * THREADS, lim = base + THREADS < NI ? base + THREADS : NI;
    return (pass & 1) ? lim - 1 - tid : base + tid;
}
// Does the slot hold an item?  (From item 0: the parent's own test, on the parent's own expression)
template <int THREADS>
__device__ __forceinline__ bool fdr_deal_live(int NI, int pass, int ps)
{
    if (fdr_deal_from_top(NI)) return pass > 0 || ps >= 0;        // (off < THREADS: the idle slots are all in pass 0; later passes carry no test)
    const int base = pass * THREADS, lim = base + THREADS < NI ? base + THREADS : NI;
    return ps >= base && ps < lim;
}
// The highest item of that wave (scalar; from the top, < 0: the whole wave is idle, and then no slot of it is live)
template <int THREADS, int WD = 0>
__device__ __forceinline__ int fdr_deal_top(int NI, int pass, int w0)
{
    w0 = fdr_deal_chunk<WD>(pass, w0);
    if (fdr_deal_from_top(NI)) {
        const int off = (NI + THREADS - 1) / THREADS * THREADS - NI;
        return pass * THREADS + ((pass & 1) ? THREADS - 1 - w0 : w0 + 63) - off;
    }
    const int base = pass * THREADS, lim = base + THREADS < NI ? base + THREADS : NI;
    return (pass & 1) ? lim - 1 - w0 : (base + w0 + 63 < lim ? base + w0 + 63 : lim - 1);
}

template <int W, int UN, bool TIE, int THREADS, int GR = 1, int WD = 0>
__device__ __forceinline__ void fdr_pass(const RlLds& L, const int* ORDER, const int* NLESS, int NP, int D, int tid, double range, unsigned long long* cnt = nullptr)
{
    const int DW = D / W, NI = NP * DW;
    const FastDiv fw(DW);
    uint32_t mine = 0;                                            // bit p: this thread's item of pass p was flagged
    const int w0 = __builtin_amdgcn_readfirstlane(tid & ~63);     // the wave's first thread, on the scalar unit
    for (int base = 0, pass = 0; base < NI; base += THREADS, ++pass) {
        const int ps = fdr_deal_item<THREADS, WD>(NI, pass, tid, w0);
        if (fdr_deal_live<THREADS>(NI, pass, ps)) {
            const int rk = fw.div(ps), d0 = W * (ps - rk * DW);
            // the scan's trip count, one per wave: the highest rank among the wave's items (consecutive in ps; nless(rank) <= rank), scalar arithmetic from the pass
            // and the wave's place in it (fdr_exact: scanning past a lane's own nless changes nothing)
            const int top = fdr_deal_top<THREADS, WD>(NI, pass, w0);
            int bound = __builtin_amdgcn_readfirstlane(fw.div(top));
#ifdef MBX_FDR_ROUND_BOUND
            // experiment, measured and dropped (docs/EXPERIMENTS.md): the bound rounded up to whole unrolled groups where the table allows it, so that only the waves
            // of the top ranks run the remainder loop.  Exact by the argument in fdr_exact's comment, but a remainder candidate costs 20 vector instructions and a
            // group of UN = 4 costs 74: trading r remainder steps for a whole group ADDS instructions for r < 4.
            { const int up = 1 + (bound - 1 + UN - 1) / UN * UN; bound = bound > 0 && up <= NP ? up : bound; }
#endif
            int kb[W];
            const bool tie = fdr_exact<W, UN, TIE, GR>(L, D, rk, d0, bound, kb, range);
#pragma unroll
            for (int q = 0; q < W; ++q) L.KB[rk * D + d0 + q] = (uint8_t)kb[q];
#ifdef MBX_FDR_COUNT
            if (cnt) { atomicAdd(cnt + 3, 1ull); if (tie) atomicAdd(cnt + 2, 1ull); }       // experiment: how many items does the scan flag? (tools/exp/fdr_flag_rate.py)
#endif
            if (TIE && tie) { L.FL[atomicAdd(L.FLN, 1)] = (uint16_t)ps; mine |= 1u << (pass & 31); }
        }
    }
    __syncthreads();
    if constexpr (TIE) {
        const int n = *L.FLN;                                     // workgroup-uniform
        if (n > 0 && (n <= MBX_FDR_OWN_AT || NI > 32 * THREADS)) {
            for (int c = tid >> 6; c < W * n; c += THREADS / 64) {      // one wave per flagged COORDINATE
                const int ps = L.FL[c / W], rk = fw.div(ps), d = W * (ps - rk * DW) + c % W;
                const int kbest = fdr_settle(L, ORDER, D, rk, d, NLESS[ORDER[rk]], L.KB[rk * D + d], cnt);
                if ((tid & 63) == 0) L.KB[rk * D + d] = (uint8_t)kbest;
            }
            __syncthreads();
        } else if (n > 0) {                                       // a collapsed swarm: every lane settles its own items (passes <= 32: NP x D / W <= 32 x THREADS)
            for (int pass = 0; mine != 0u; ++pass, mine >>= 1) {
                if (!(mine & 1u)) continue;
                const int ps = fdr_deal_item<THREADS, WD>(NI, pass, tid, w0), rk = fw.div(ps), d0 = W * (ps - rk * DW);      // (a flagged pass: the slot held an item)
                int kb[W];
#pragma unroll
                for (int q = 0; q < W; ++q) kb[q] = L.KB[rk * D + d0 + q];
                fdr_settle_own<W>(L.NC, L.PB, ORDER, D, rk, d0, NLESS[ORDER[rk]], kb);
#pragma unroll
                for (int q = 0; q < W; ++q) L.KB[rk * D + d0 + q] = (uint8_t)kb[q];
            }
            __syncthreads();
        }
    }
}

// The arithmetic of the move (rlepso_optimizer.py:179-195) once an item's uniforms and exemplars are known: uf / ucs the FDR weight and the CLPSO uniform of each
// coordinate, xrs the rank of its CLPSO exemplar (the particle's own rank where no tournament was consumed); FDR exemplars from KB.
template <int W, bool RES>
__device__ __forceinline__ void rl_move_apply(const MoveCtx& c, int i, int d0, int rk, const double uf[W], const double ucs[W], const int xrs[W], double cur[W], double vel[W])
{
    const RlLds& L = c.L;
    const int D = c.D, e0 = i * D + d0, es0 = rk * D + d0;
    const double r1 = L.R1[i], r2 = L.R2[i];
    const int g = c.fg.div(i);
    double cw = 0., c1 = 0., c2 = 0., c3 = 0., c4 = 0.;
    // whole_groups (NP a multiple of the group count, known at compile time): every particle has a group, no select on the five coefficients
    if (c.whole_groups || g < c.G) { const double* k = L.COEF + g * 6; cw = k[1]; c1 = k[2]; c2 = k[3]; c3 = k[4]; c4 = k[5]; }
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const int e = e0 + q, d = d0 + q;
        const double pp = L.PB[es0 + q], uc = ucs[q];
        const int xr = xrs[q], kb = L.KB[es0 + q];
        const double ex = L.PB[xr * D + d];                        // CLPSO exemplar (own rank: the particle's own pbest)
        const double v_fdr = uf[q] * (L.PB[kb * D + d] - pp);
        const double v_pbest = r1 * (pp - cur[q]);
        const double v_gbest = r2 * (L.GB[d] - cur[q]);
        const double v_cl = uc * (ex - cur[q]);
        double nv = cw * vel[q] + c1 * v_cl + c2 * v_fdr + c3 * v_gbest + c4 * v_pbest;
        nv = fmin(fmax(nv, -c.vmax), c.vmax);
        double np_ = cur[q] + nv;
        np_ = fmin(fmax(np_, c.lb), c.ub);
        L.X[e] = np_;
        if (RES) { cur[q] = np_; vel[q] = nv; }
        else { c.gPos[e] = np_; c.gVel[e] = nv; }
    }
}

// Velocity / position update of W adjacent coordinates of particle i (rlepso_optimizer.py:179-195); FDR exemplars from KB.
// CLPSO (:76-95): one Philox call carries the uniforms of an element PAIR (site ELEM_A, index e >> 1), another one (site TOURN, same
// index) the two tournament pairs; the latter is only evaluated where a tournament is consumed, i.e. where !(u > pci_i).
// RES: the caller keeps positions / velocities on chip (k_rlepso_run): the new values come back in cur / vel instead of going to HBM.
template <int W, bool RES = false>
__device__ __forceinline__ void rl_move(const MoveCtx& c, int i, int d0, double cur[W], double vel[W])
{
    const RlLds& L = c.L;
    const int NP = c.NP, D = c.D;
    const int rk = c.RANK[i], e0 = i * D + d0;
    // one Philox call carries the four element-wise uniforms of an element PAIR, 32 bits each (site ELEM_A, index e >> 1: words 0 / 2 = CLPSO
    // uniform / FDR weight of the even element, 1 / 3 of the odd one); a two-coordinate work item starts on an even element (D even, d0 even)
    double uf[W];
    U4 wa{0, 0, 0, 0};
    if (c.tape) {
#pragma unroll
        for (int q = 0; q < W; ++q) uf[q] = c.tape[MBX_RLEPSO_TAPE_FDR(NP, D) + e0 + q];
    } else {
        wa = c.rng.draw((uint32_t)e0 >> 1, MBX_SITE_ELEM_A);
        if (W == 2) { uf[0] = u32d(wa.z); uf[W - 1] = u32d(wa.w); }
        else uf[0] = u32d((e0 & 1) ? wa.w : wa.z);
    }
    double ucs[W]; int xrs[W];
    {
        const double pci = c.pci[i];
        bool need = false;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int e = e0 + q;
            if (c.tape) ucs[q] = c.tape[MBX_RLEPSO_TAPE_CLPSO(NP, D) + e];
            else ucs[q] = u32d((W == 2 ? q == 1 : (e & 1)) ? wa.y : wa.x);
            xrs[q] = rk;
            need = need || !(ucs[q] > pci);
        }
        if (need) {
            U4 wt{0, 0, 0, 0};
            if (!c.tape) wt = c.rng.draw((uint32_t)e0 >> 1, MBX_SITE_TOURN);
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const int e = e0 + q;
                if (!(ucs[q] > pci)) {
                    int t1, t2;
                    if (c.tape) { t1 = (int)c.tape[MBX_RLEPSO_TAPE_TOURN(NP, D) + 2 * e]; t2 = (int)c.tape[MBX_RLEPSO_TAPE_TOURN(NP, D) + 2 * e + 1]; }
                    else {
                        const bool odd = W == 2 ? q == 1 : (e & 1);
                        t1 = (int)__umulhi(odd ? wt.z : wt.x, (uint32_t)NP); t2 = (int)__umulhi(odd ? wt.w : wt.y, (uint32_t)NP);
                    }
                    xrs[q] = c.RANK[L.PBC[t2] < L.PBC[t1] ? t2 : t1];   // binary tournament on pbest cost, first candidate wins ties
                }
            }
        }
    }
    rl_move_apply<W, RES>(c, i, d0, rk, uf, ucs, xrs, cur, vel);
}

// ---- the move of the resident kernel with the tournaments COMPACTED per wave (k_rlepso_run, 256-thread geometries; no tape there)
// rl_move runs the MBX_SITE_TOURN Philox call and the two tournament look-ups (about 35 + 30 vector instructions) in every wave-pass in which ONE lane consumes a
// tournament; with pci between 0.05 and 0.5 about 18 % of the items do, so practically every wave-pass pays for them (8 per generation at NP 100 / D 10).  Here a
// wave first draws MBX_SITE_ELEM_A for ALL its items (IT per lane; the four words stay in the lane's registers), the items that consume a tournament append their
// number to the wave's own list (ballot + mbcnt: the position is the count of such lanes below, plus the wave's earlier passes), then the wave deals the listed items
// 64 per step -- TOURN draw, both coordinates' tournaments, the two exemplar ranks written back OVER the list entry -- and every lane picks its entry up again: one
// step per wave instead of IT (23 listed items per wave on average, 128 at most).  Same Philox counters (ELEM_A and TOURN at index it = e0 >> 1), same words, same
// tie rule (the first candidate wins); a coordinate that consumes no tournament ignores the rank computed for it.
//  * The list is the wave's slice of FL (64 IT entries), which the FDR pass has finished with behind its closing barrier and next touches behind the ranking barrier
//    of the following generation: THREADS x IT < NI + THREADS <= 2 NI = NE entries, FL's size, wherever NI >= THREADS (rl_run_listed).
//  * No barrier: writer and readers of an entry are lanes of ONE wave, whose LDS instructions execute in program order; the wavefront fences keep the compiler from
//    reordering them.
#ifndef MBX_RL_LISTED_TOURN
#define MBX_RL_LISTED_TOURN 1       // 0: rl_move per item, as in k_rlepso_step (A/B and instruction-budget builds)
#endif
__host__ __device__ constexpr bool rl_run_listed(int threads, int ni) { return MBX_RL_LISTED_TOURN && threads == 256 && ni >= threads; }

template <int THREADS, int NI, int HD, int IT>
__device__ __forceinline__ void rl_move_listed(const MoveCtx& c, const FastDiv& fh, int tid, double (&vel)[IT][2])
{
    static_assert(NI >= THREADS && NI < 65536, "the wave lists fit FL, an item number fits an entry");
    const RlLds& L = c.L;
    uint16_t* WL = L.FL + (tid >> 6) * (64 * IT);
    U4 wa[IT];
    bool nd[IT][2];
    int pos[IT];
    int n = 0;                                                    // listed items of the wave so far (scalar)
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        // (a lane past the last item draws for the last item and lists nothing: a Philox call costs the wave the same with or without it, and without a branch the
        // need bits stay compare masks on the scalar unit)
        const int it = tid + j * THREADS, itc = it < NI ? it : NI - 1;
        const double pci = c.pci[fh.div(itc)];
        wa[j] = c.rng.draw((uint32_t)itc, MBX_SITE_ELEM_A);
        nd[j][0] = it < NI && !(u32d(wa[j].x) > pci); nd[j][1] = it < NI && !(u32d(wa[j].y) > pci);
        const bool any = nd[j][0] || nd[j][1];
        const unsigned long long m = __builtin_amdgcn_ballot_w64(any);
        pos[j] = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (any) WL[pos[j]] = (uint16_t)it;
        n += __builtin_popcountll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int s = tid & 63; s < n; s += 64) {
        const U4 wt = c.rng.draw((uint32_t)WL[s], MBX_SITE_TOURN);
        const int a1 = (int)__umulhi(wt.x, (uint32_t)c.NP), a2 = (int)__umulhi(wt.y, (uint32_t)c.NP);
        const int b1 = (int)__umulhi(wt.z, (uint32_t)c.NP), b2 = (int)__umulhi(wt.w, (uint32_t)c.NP);
        const int x0 = c.RANK[L.PBC[a2] < L.PBC[a1] ? a2 : a1], x1 = c.RANK[L.PBC[b2] < L.PBC[b1] ? b2 : b1];     // binary tournaments on pbest cost, first candidate wins ties
        WL[s] = (uint16_t)(x0 | x1 << 8);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        const int it = tid + j * THREADS;
        if (it < NI) {
            const int i = fh.div(it), rk = c.RANK[i];
            const uint32_t xw = nd[j][0] || nd[j][1] ? WL[pos[j]] : 0u;
            const double2 c2 = *(const double2*)(L.X + 2 * it);
            double cur[2] = {c2.x, c2.y};
            const double uf[2] = {u32d(wa[j].z), u32d(wa[j].w)}, ucs[2] = {u32d(wa[j].x), u32d(wa[j].y)};
            const int xrs[2] = {nd[j][0] ? (int)(xw & 255u) : rk, nd[j][1] ? (int)(xw >> 8) : rk};
            rl_move_apply<2, true>(c, i, 2 * (it - i * HD), rk, uf, ucs, xrs, cur, vel[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// PBO_Env.reset(): init_population (rlepso_optimizer.py:39-65)
// ------------------------------------------------------------------------------------------------
// THREADS = 256, or 512 when the geometry leaves room for one workgroup per CU only (see rl_block_threads)
template <int THREADS, int NPC = 0, int DC = 0>
__global__ __launch_bounds__(THREADS) void k_rlepso_reset(BatchParams bp, double* __restrict__ state_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = NPC ? NPC : bp.NP, D = DC ? DC : bp.D, NE = NP * D;
    constexpr bool MAPS = rl_maps_in_lds(NPC, DC);
    constexpr int MD = MAPS ? 0 : DC;
    const DevProblem P = bp.problems[bp.problem_idx[b]];
    const RlLds L = rl_carve(smem, NP, D, MAPS);
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_RLEPSO_ST_SCALARS(NP, D);
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;

    const int episode = (int)sc[MBX_SC_EPISODE] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), 0u, (uint32_t)episode};
    const double lb = P.lb, ub = P.ub, vmax = 0.1 * (ub - lb);

    stage_problem<0, MAPS>(P, L.eval());
    for (int e = tid; e < NE; e += MBX_NT) {
        double up, uv;
        if (tape) { up = tape[MBX_RLEPSO_TAPE_REPOS(NP, D) + e]; uv = tape[MBX_RLEPSO_TAPE_REVEL(NP, D) + e]; }
        else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); up = u53(w.x, w.y); uv = u53(w.z, w.w); }
        const double x = lb + (ub - lb) * up;
        L.X[e] = x;
        S[MBX_RLEPSO_ST_POS(NP, D) + e] = x;
        S[MBX_RLEPSO_ST_PBPOS(NP, D) + e] = x;
        S[MBX_RLEPSO_ST_VEL(NP, D) + e] = -vmax + (vmax - (-vmax)) * uv;
    }
    __syncthreads();
    population_costs<0, MD>(P, L.eval(), NP, rng, tape ? tape + MBX_RLEPSO_TAPE_NOISE1(NP, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
    double gb; int gi;
    block_argmin(L.NC, NP, L.RED, gb, gi);
    for (int i = tid; i < NP; i += MBX_NT) {
        const double c = L.NC[i];
        S[MBX_RLEPSO_ST_CCOST(NP, D) + i] = c;
        S[MBX_RLEPSO_ST_PBEST(NP, D) + i] = c;
        S[MBX_RLEPSO_ST_PNI(NP, D) + i] = 0.;
    }
    if (tid < D) S[MBX_RLEPSO_ST_GBPOS(NP, D) + tid] = L.X[gi * D + tid];
    if (tid == 0) {
        sc[MBX_SC_GBEST] = gb; sc[MBX_SC_FES] = NP; sc[MBX_SC_LOG_INDEX] = 1; sc[MBX_SC_COST_LEN] = 1;
        sc[MBX_SC_DONE] = 0; sc[MBX_SC_RETURN] = 0; sc[MBX_SC_GEN] = 0; sc[MBX_SC_EPISODE] = episode;
        sc[MBX_SC_GBEST_IDX] = gi; sc[MBX_SC_REINIT] = 0;
        sc[MBX_NSCALAR] = gb;                                    // cost = [gbest]
        if (state_out) state_out[b] = (double)NP / bp.max_fes;
    }
}

// ------------------------------------------------------------------------------------------------
// PBO_Env.step(action): RLEPSO_Optimizer.update (rlepso_optimizer.py:173-263)
// ------------------------------------------------------------------------------------------------
// Actions come either from `actions` [B, 7G] (PBO_Env.step(action)) or, when `policy_table` is given, are drawn here from
// the actor's (mu, sigma) at the instance's current state (agent.act + env.step in one launch, mbx_rlepso_act_step): row
// fes of the table built by k_gauss_mlp_policy, same Philox draws as mbx_gauss_policy, optionally echoed to actions_out.
// NPC / DC / GC: population, dimension and group count fixed at compile time (0 = taken from the batch).  The reference's own
// geometry (NP = 100 hard-coded in rlepso_optimizer.py:9, n_group = 5, and the D = 10 of its bbob configs) gets an instantiation of
// its own: index arithmetic, the divisions by D and the short D-loops of the evaluator fold into constants (-8 % per generation).
// TIE: the FDR scan flags near-ties and resolves them with the reference's rounded quotients (fdr_exact / fdr_settle): the default; TIE = false is the
// cross-multiplied order alone (MBX_F_FDR_FAST)
template <int THREADS, int NPC = 0, int DC = 0, int GC = 0, bool TIE = true>
__global__ __launch_bounds__(THREADS) MBX_RL_WAVES void k_rlepso_step(BatchParams bp, const float* __restrict__ actions,
                                                          double* __restrict__ state_out, double* __restrict__ reward_out,
                                                          uint8_t* __restrict__ done_out, const float* __restrict__ policy_table,
                                                          int table_rows, float* __restrict__ actions_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = bp.order[blockIdx.x], tid = threadIdx.x;
    const int NP = NPC ? NPC : bp.NP, D = DC ? DC : bp.D, NE = NP * D, G = GC ? GC : bp.n_group;
    double* S = bp.state + (int64_t)b * bp.state_stride;
    double* sc = S + MBX_RLEPSO_ST_SCALARS(NP, D);

    if (sc[MBX_SC_DONE] != 0.) {                                  // finished instances idle (block-uniform exit)
        if (tid == 0) {
            if (state_out) state_out[b] = sc[MBX_SC_FES] / bp.max_fes;
            if (reward_out) reward_out[b] = 0.;
            if (done_out) done_out[b] = 1;
        }
        return;
    }
    MBX_PHASE_BEGIN
    ConstProblem& P = *(ConstProblem*)(bp.problems + bp.problem_idx[b]);   // scalar loads on demand, no SGPR-resident copy
    const RlLds L = rl_carve(smem, NP, D, rl_maps_in_lds(NPC, DC));
    const double* tape = bp.tape ? bp.tape + (int64_t)b * bp.tape_stride : nullptr;
    const float* act = actions + (int64_t)b * (7 * G);

    const int gen = (int)sc[MBX_SC_GEN] + 1;
    const uint64_t seed = bp.seeds[b];
    const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, (uint32_t)(int)sc[MBX_SC_EPISODE], true};
    const double lb = P.lb, ub = P.ub, vmax = 0.1 * (ub - lb);
    double gbest = sc[MBX_SC_GBEST];
    int gbest_idx = (int)sc[MBX_SC_GBEST_IDX];
    const double pre_gbest = gbest;
    double fes = sc[MBX_SC_FES];

    // ---- stage: pbest positions/costs, c_cost, stagnation counters, gbest position, linear maps
    const double* gPB = S + MBX_RLEPSO_ST_PBPOS(NP, D);
    double* gPos = S + MBX_RLEPSO_ST_POS(NP, D);
    double* gVel = S + MBX_RLEPSO_ST_VEL(NP, D);
    float* ACT = (float*)L.R1;                                    // sampled action; R1 is not written before the ranking barrier
    if (policy_table && tid < 7 * G) {
        const int A = 7 * G;
        int row = (int)fes;
        row = row < table_rows ? row : table_rows - 1;
        const float* ms = policy_table + (int64_t)row * 2 * A;
        const float a = sample_action(rng, tid, ms[tid], ms[A + tid], MBX_POLICY_RLEPSO);
        ACT[tid] = a;
        if (actions_out) actions_out[(int64_t)b * A + tid] = a;
    }
    for (int i = tid; i < NP; i += MBX_NT) {
        L.PBC[i] = S[MBX_RLEPSO_ST_PBEST(NP, D) + i];
        L.RANK[i] = 0; L.MASK[i] = 0;
        L.IMPR[i] = i;                                             // ORDER stays a valid index table even if a NaN cost breaks the ranking
        L.PNI[i] = S[MBX_RLEPSO_ST_PNI(NP, D) + i];
    }
    if (tid < D) L.GB[tid] = S[MBX_RLEPSO_ST_GBPOS(NP, D) + tid];
    if (tid == 0) *L.FLN = 0;                                     // list of the FDR scan's near-tie items (fdr_pass): empty before the ranking barrier
    stage_problem<eval_dc(DC), eval_md(DC) == 0>(P, L.eval());
    // __get_coe (:112-132): float32 arithmetic (numpy >= 2 keeps float32 for scalar*python-float), group g
    // reads actions[g*n_group : g*n_group+7]
    auto get_coe = [&](const float* a) {
        const float cm = a[0] * 0.01f;
        const float wv = a[1] * 0.8f + 0.1f;
        float den = a[3] + a[4];
        den = den + a[5]; den = den + a[6]; den = den + 1e-5f;
        float scale = 1.f / den;
        scale = scale * a[2]; scale = scale * 8.f;
        double* c = L.COEF + tid * 6;
        c[0] = (double)cm; c[1] = (double)wv;
        c[2] = (double)(scale * a[3]); c[3] = (double)(scale * a[4]);
        c[4] = (double)(scale * a[5]); c[5] = (double)(scale * a[6]);
    };
    if (!policy_table && tid < G) get_coe(act + tid * G);
    __syncthreads();
    // fused policy: the sampled action became visible with the barrier above; the coefficients are published by the ranking
    // barrier below, before their first use
    if (policy_table && tid < G) get_coe(ACT + tid * G);
    MBX_PHASE(0);                                                 // HBM -> LDS staging
    const int per_group = NP / G;
    const FastDiv fd(D), fg(per_group);
    // ---- rank the particles by (pbest cost, index); all 256 threads take part: thread (i, part) counts, over a slice of j,
    // the particles that are strictly better (nless) and those that are not worse (nle).  rank = nless unless another
    // particle has exactly the same pbest cost (nle - nless > 1: rare), in which case the equal ones are ordered by index.
    int* ORDER = L.IMPR;          // free until the first commit
    int* NLESS = L.MASK;
    int* RANK = L.RANK;           // doubles as the nle accumulator
    {
        const int parts = MBX_NT / NP > 0 ? MBX_NT / NP : 1;
        for (int w = tid; w < parts * NP; w += MBX_NT) {
            const int part = w / NP, i = w - part * NP;
            const int j0 = part * NP / parts, j1 = (part + 1) * NP / parts;
            const double fi = L.PBC[i];
            int nle = 0, nless = 0;
#ifndef MBX_ABLATE_RANK
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const double fj = L.PBC[j];
                nless += fj < fi;
                nle += fj <= fi;
            }
#else
            if (part == 0) { nle = i + 1; nless = i; }
#endif
            atomicAdd(&RANK[i], nle); atomicAdd(&NLESS[i], nless);
        }
    }
    __syncthreads();
    int equal_costs = 0;
    for (int i = tid; i < NP; i += MBX_NT) {                    // per-particle quantities
        const int g = fg.div(i);
        L.CMUT[i] = g < G ? L.COEF[g * 6] * L.PNI[i] : 0.;        // uses per_no_improve BEFORE this step's update (:120)
        if (tape) { L.R1[i] = tape[MBX_RLEPSO_TAPE_RAND1(NP, D) + i]; L.R2[i] = tape[MBX_RLEPSO_TAPE_RAND2(NP, D) + i]; }
        else { const U4 w = rng.draw((uint32_t)i, MBX_SITE_PART); L.R1[i] = u53(w.x, w.y); L.R2[i] = u53(w.z, w.w); }
        const double fi = L.PBC[i];
        int rank = NLESS[i];
        if (RANK[i] - rank > 1) {
            equal_costs = 1;
            for (int j = 0; j < i; ++j) rank += L.PBC[j] == fi;
        }
        RANK[i] = rank;                                            // thread i is the only reader / writer of entry i here
        ORDER[rank] = i; L.NC[rank] = fi; L.NCS[rank] = fi;        // NC: pbest costs in ascending order (free until eval); NCS: the column the FDR scan reads
    }
    equal_costs = __syncthreads_or(equal_costs);
    MBX_PHASE(1);                                                 // ranking + per-particle draws
    // pbest positions are staged in RANK order (row r = particle ORDER[r]): the FDR scan below then walks LDS linearly
    for (int e = tid; e < NE; e += MBX_NT) { const int i = fd.div(e), d = e - i * D; L.PB[RANK[i] * D + d] = gPB[e]; }
    __syncthreads();
    if (equal_costs) {                                            // workgroup-uniform: rows that are copies of the row one rank up leave the FDR scan (rl_mark_copies)
        for (int r = tid; r < NP; r += MBX_NT) rl_mark_copies(L, NP, D, r);
        __syncthreads();
    }
    MBX_PHASE(2);                                                 // pbest rows -> LDS in rank order

    // ---- FDR exemplars -> KB[rank * D + d]  (a pass of its own: the scan's registers are dead before the velocity update starts, which
    // keeps the kernel at 80 VGPRs without scratch; fused into the update it needed 96 and spilled)
#ifndef MBX_ABLATE_FDR
    if ((D & 1) == 0) fdr_pass<2, MBX_FDR_UNROLL, TIE, THREADS>(L, ORDER, NLESS, NP, D, tid, ub - lb + 1e-5);
    else fdr_pass<1, MBX_FDR_UNROLL, TIE, THREADS>(L, ORDER, NLESS, NP, D, tid, ub - lb + 1e-5);
#else
    for (int e = tid; e < NE; e += MBX_NT) L.KB[e] = 0;
    __syncthreads();
#endif

    // ---- velocity / position update (:179-195).  A work item is W adjacent dimensions of one particle (W = 2 when D is even).
    const MoveCtx mc{L, bp.pci, tape, rng, gPos, gVel, ORDER, NLESS, RANK, NP, D, G, lb, ub, vmax, fg, NPC > 0 && GC > 0 && NPC % (GC > 0 ? GC : 1) == 0};
    if ((D & 1) == 0) {
        const int HD = D >> 1, NI = NP * HD;
        const FastDiv fh(HD);
        for (int it = tid; it < NI; it += MBX_NT) {
            const int i = fh.div(it);
            const double2 c2 = *(const double2*)(gPos + 2 * it), v2 = *(const double2*)(gVel + 2 * it);
            double cur[2] = {c2.x, c2.y}, vel[2] = {v2.x, v2.y};
            rl_move<2>(mc, i, 2 * (it - i * HD), cur, vel);
        }
    } else {
        for (int e = tid; e < NE; e += MBX_NT) {
            const int i = fd.div(e);
            double cur[1] = {gPos[e]}, vel[1] = {gVel[e]};
            rl_move<1>(mc, i, e - i * D, cur, vel);
        }
    }
    __syncthreads();
    MBX_PHASE(3);                                                 // move (draws, exemplars, FDR scan, velocity)

    // ---- evaluate, update pbest/gbest and stagnation counters (:198-233)
    population_costs<eval_dc(DC), eval_md(DC)>(P, L.eval(), NP, rng, tape ? tape + MBX_RLEPSO_TAPE_NOISE0(NP, D) : nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B);
    MBX_PHASE(4);                                                 // evaluation
    fes += NP;
    rl_commit(L, NP, D, true, gbest, gbest_idx, S + MBX_RLEPSO_ST_PBPOS(NP, D), S + MBX_RLEPSO_ST_CCOST(NP, D));
    MBX_PHASE(5);                                                 // commit

    // ---- re-initialisation (:238-239, 134-168): P(i) = u < c_mutation_i * 0.01 * per_no_improve_i
    int mine = 0;
    for (int i = tid; i < NP; i += MBX_NT) {
        double u;
        if (tape) u = tape[MBX_RLEPSO_TAPE_REINIT(NP, D) + i];
        else { const U4 w = rng.draw((uint32_t)i, MBX_SITE_REINIT); u = u53(w.x, w.y); }
        const int m = u < L.CMUT[i] * 0.01 * L.PNI[i];
        L.MASK[i] = m;
        mine += m;
    }
    const int n_reinit = __syncthreads_count(mine);               // NP <= 256: at most one particle per thread
    MBX_PHASE(6);                                                 // re-init draw
    if (n_reinit > 0) {
        for (int e = tid; e < NE; e += MBX_NT) {
            const int i = fd.div(e);
            if (L.MASK[i]) {
                double up, uv;
                if (tape) { up = tape[MBX_RLEPSO_TAPE_REPOS(NP, D) + e]; uv = tape[MBX_RLEPSO_TAPE_REVEL(NP, D) + e]; }
                else { const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R); up = u53(w.x, w.y); uv = u53(w.z, w.w); }
                const double x = lb + (ub - lb) * up;
                L.X[e] = x;
                gPos[e] = x;
                gVel[e] = -vmax + (vmax - (-vmax)) * uv;
            }
        }
        __syncthreads();
        // the whole population is re-evaluated but only the re-initialised particles are billed (:141-143)
        population_costs<eval_dc(DC), eval_md(DC)>(P, L.eval(), NP, rng, tape ? tape + MBX_RLEPSO_TAPE_NOISE1(NP, D) : nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
        fes += n_reinit;
        rl_commit(L, NP, D, false, gbest, gbest_idx, S + MBX_RLEPSO_ST_PBPOS(NP, D), S + MBX_RLEPSO_ST_CCOST(NP, D));
    }

    MBX_PHASE(7);                                                 // re-init (move, evaluation, commit)
    // ---- write back what changed
    for (int i = tid; i < NP; i += MBX_NT) {
        S[MBX_RLEPSO_ST_PBEST(NP, D) + i] = L.PBC[i];
        S[MBX_RLEPSO_ST_PNI(NP, D) + i] = L.PNI[i];
    }
    if (gbest < pre_gbest && tid < D) S[MBX_RLEPSO_ST_GBPOS(NP, D) + tid] = L.GB[tid];

    // ---- logging, termination, reward, next state (:241-261)
    if (tid == 0) {
        int log_index = (int)sc[MBX_SC_LOG_INDEX], cost_len = (int)sc[MBX_SC_COST_LEN];
        double* cost = sc + MBX_NSCALAR;
        const bool done = log_and_terminate(bp, P, fes, gbest, log_index, cost_len, cost);
        const double reward = gbest < pre_gbest ? 1. : -1.;
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_RETURN] += reward; sc[MBX_SC_GEN] = gen;
        sc[MBX_SC_GBEST_IDX] = gbest_idx; sc[MBX_SC_REINIT] = n_reinit > 0 ? 1. : 0.;
        if (state_out) state_out[b] = fes / bp.max_fes;
        if (reward_out) reward_out[b] = reward;
        if (done_out) done_out[b] = done ? 1 : 0;
    }
    MBX_PHASE(8);                                                 // write-back, logging
}

// ------------------------------------------------------------------------------------------------
// Agent.rollout_episode's loop (src/agent/rlepso_agent.py:294-303), up to n_gens generations per launch, state ON CHIP in between
// ------------------------------------------------------------------------------------------------
// k_rlepso_step streams an instance's 26.5 KB state block in and out once per generation because a policy outside the kernel needs
// the state between generations.  With the policy inside (actor table, as in mbx_rlepso_act_step) nothing leaves the workgroup between
// two generations, so this kernel loads the block ONCE, runs up to n_gens generations and stores it ONCE: positions stay in LDS (X is
// only read by the evaluator), velocities, pbest positions and c_cost stay in registers of the thread that owns the element / particle,
// the per-particle arrays and the problem constants stay in LDS.  Every generation performs exactly the arithmetic of k_rlepso_step with
// the same Philox counters (gen is part of the counter), so n_gens launches of mbx_rlepso_act_step and one launch of this kernel give
// bit-identical states (tests/test_gpu_rlepso.py).  A workgroup leaves as soon as its instance is done and the hardware dispatcher hands
// its slot to the next workgroup: no lock-step idling, no refill queue needed.
// Compile-time geometry only (even D, NP <= THREADS: particle i's scalars live in thread i); other geometries are stepped by the host
// loop in mbx_rlepso_rollout.
struct RunOut {
    float* traj_actions;         // [n_gens][B][7 G] sampled actions, or nullptr
    double* traj_state;          // [n_gens][B] state after the generation (fes / maxFEs), or nullptr
    double* traj_reward;         // [n_gens][B]
    uint8_t* traj_done;          // [n_gens][B]
    double* state_out;           // [B] state after the last executed generation, or nullptr
    double* reward_out;          // [B] SUM of the rewards of the executed generations, or nullptr
    uint8_t* done_out;           // [B]
};

#ifndef MBX_RUN_WAVES
#define MBX_RUN_WAVES MBX_RL_WAVES
#endif
// The body of k_rlepso_run.  KIND != 0: the instance's function kind, known at compile time -- the evaluator (twice in the body: update and re-initialisation) holds that
// kind's code only.
// ARGS: a callable that returns (a reference to) the kernel's argument block -- the kernel's own parameters, or, out of line, the kernarg segment behind a pointer
// that is re-materialised at every use (each field access a fresh scalar load next to its use: what the compiler does with a kernel's parameters by itself, and
// what it cannot do with values a callee loaded once -- those stay in SGPRs across the whole body or are spilled).
template <int THREADS, int NPC, int DC, int GC, int KIND, int NOISE, bool TIE, class ARGS>
__device__ __forceinline__ void rl_run_body(ARGS ar)
{
    const int n_gens = ar().n_gens;
    static_assert(NPC > 0 && DC > 0 && GC > 0 && (DC & 1) == 0 && NPC <= THREADS, "k_rlepso_run: compile-time geometry, even D, NP <= THREADS");
    constexpr int NP = NPC, D = DC, G = GC, HD = D / 2, NI = NP * HD, IT = (NI + THREADS - 1) / THREADS, A = 7 * G;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = ar().bp.order[blockIdx.x], tid0 = threadIdx.x, tid = tid0;
    double* S = ar().bp.state + (int64_t)b * ar().bp.state_stride;
    double* sc = S + MBX_RLEPSO_ST_SCALARS(NP, D);
    const int64_t B = ar().bp.B;

    if (sc[MBX_SC_DONE] != 0.) {                                  // finished before the launch: what k_rlepso_step reports for it, n_gens times
        const double st = sc[MBX_SC_FES] / ar().bp.max_fes;
        for (int g = tid; g < n_gens; g += THREADS) {
            if (ar().out.traj_state) ar().out.traj_state[g * B + b] = st;
            if (ar().out.traj_reward) ar().out.traj_reward[g * B + b] = 0.;
            if (ar().out.traj_done) ar().out.traj_done[g * B + b] = 1;
        }
        if (tid == 0) {
            if (ar().out.state_out) ar().out.state_out[b] = st;
            if (ar().out.reward_out) ar().out.reward_out[b] = 0.;
            if (ar().out.done_out) ar().out.done_out[b] = 1;
        }
        return;
    }
    // launch clock (diagnostics, off unless a slot pair is attached): s_memtime counters of different XCDs / CUs are offset against each other, so every workgroup
    // measures its OWN lifetime in both time bases and adds the two differences to the launch's sums
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    const bool clocked = ar().bp.clk != nullptr && tid0 == 0;
    if (clocked) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
    ConstProblem& P = *(ConstProblem*)(ar().bp.problems + ar().bp.problem_idx[b]);
    const RlLds L = rl_carve(smem, NP, D, rl_maps_in_lds(NPC, DC));
    int gen = (int)sc[MBX_SC_GEN];
    const uint64_t seed = ar().bp.seeds[b];
    const uint32_t episode = (uint32_t)(int)sc[MBX_SC_EPISODE];
    const double lb = P.lb, ub = P.ub, vmax = 0.1 * (ub - lb);
    double gbest = sc[MBX_SC_GBEST];
    int gbest_idx = (int)sc[MBX_SC_GBEST_IDX];
    // fes, the curve's counters and the return are exact integers (fes <= maxFEs + 2 NP) and the same in every lane: they are carried on the scalar unit
    // (integer adds and compares there instead of float64 ones in all four waves) and become float64 again only where a value is stored
    int fes = __builtin_amdgcn_readfirstlane((int)sc[MBX_SC_FES]);
    int log_index = __builtin_amdgcn_readfirstlane((int)sc[MBX_SC_LOG_INDEX]), cost_len = __builtin_amdgcn_readfirstlane((int)sc[MBX_SC_COST_LEN]);
    double* cost = sc + MBX_NSCALAR;
    int ret = 0;
    int n_reinit = 0;

    // ---- load the state block once: positions -> X (LDS), velocities / pbest positions -> registers of the element's owner
    // (work item it = tid + j THREADS owns the adjacent coordinates 2 it, 2 it + 1 of particle it / HD), c_cost -> register of thread i
    double* gPos = S + MBX_RLEPSO_ST_POS(NP, D);
    double* gVel = S + MBX_RLEPSO_ST_VEL(NP, D);
    double* gPB = S + MBX_RLEPSO_ST_PBPOS(NP, D);
    double vel[IT][2], pbp[IT][2], cc = 0.;
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        const int it = tid + j * THREADS;
        vel[j][0] = vel[j][1] = pbp[j][0] = pbp[j][1] = 0.;
        if (it < NI) {
            const double2 v2 = *(const double2*)(gVel + 2 * it), p2 = *(const double2*)(gPB + 2 * it);
            vel[j][0] = v2.x; vel[j][1] = v2.y; pbp[j][0] = p2.x; pbp[j][1] = p2.y;
            *(double2*)(L.X + 2 * it) = *(const double2*)(gPos + 2 * it);
        }
    }
    if (tid < NP) {
        L.PBC[tid] = S[MBX_RLEPSO_ST_PBEST(NP, D) + tid];
        L.PNI[tid] = S[MBX_RLEPSO_ST_PNI(NP, D) + tid];
        cc = S[MBX_RLEPSO_ST_CCOST(NP, D) + tid];
    }
    if (tid < D) L.GB[tid] = S[MBX_RLEPSO_ST_GBPOS(NP, D) + tid];
    stage_problem<eval_dc(DC), eval_md(DC) == 0, ConstProblem>(P, L.eval());
    constexpr int per_group = NP / G;
    const FastDiv fg(per_group), fh(HD);
    int* ORDER = L.IMPR;          // free until the first commit of a generation
    int* NLESS = L.MASK;
    int* RANK = L.RANK;
    float* ACT = (float*)L.R1;    // sampled action; R1 is not written before the ranking barrier
    int* EQC = (int*)(L.RED + 14);  // equal-cost flag of the ranking (block_argmin uses RED[0..1] only)
    int* RCNT = (int*)(L.RED + 2);  // re-initialisation count of each wave that holds particles (RED[2..9]: up to 16 waves)
    constexpr int PW = (NP + 63) / 64;      // waves that hold particles

    constexpr bool PRIO2 = MBX_RL_PRIO == 2 && THREADS == 256;    // the third priority level (see MBX_RL_PRIO)
    // pbest / gbest bookkeeping of update() and __reinit() (rl_commit with c_cost and the pbest positions in registers)
    auto commit =[&](bool stagnation, int tid) {
        if (tid < NP) {
            const double nc = L.NC[tid];
            if (stagnation) L.PNI[tid] = nc < cc ? 0. : L.PNI[tid] + 1;
            const int impr = nc < L.PBC[tid];
            if (impr) L.PBC[tid] = nc;
            L.IMPR[tid] = impr;
            cc = nc;
        }
        double cbv; int cb;
        if constexpr (PRIO2) { __builtin_amdgcn_s_setprio(2); block_argmin<1>(L.NC, NP, L.RED, cbv, cb); }      // (wave 0's value exchange and index step at level 2)
        else block_argmin(L.NC, NP, L.RED, cbv, cb);    // contains the barriers that publish IMPR
        const bool better = cbv < gbest;
        if (better) { gbest = cbv; gbest_idx = cb; }
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int it = tid + j * THREADS;
            if (it < NI && L.IMPR[fh.div(it)]) { const double2 x2 = *(const double2*)(L.X + 2 * it); pbp[j][0] = x2.x; pbp[j][1] = x2.y; }
        }
        if (better && tid < D) L.GB[tid] = L.X[cb * D + tid];
        if (!stagnation) __syncthreads();                // update()'s commit is followed by the barrier of the re-initialisation count, with nothing shared in between
    };

    bool done = false;
    int g = 0;
    __syncthreads();
    if constexpr (MBX_RL_PRIO && THREADS == 256) __builtin_amdgcn_s_setprio(1);      // (straight-line code every wave of the workgroup runs, like the two calls around the FDR pass)
    for (; g < n_gens && !done; ++g) {
        // the thread index is re-materialised every generation: otherwise the compiler hoists all the index arithmetic of the body out of
        // the loop and spills it (528 B of scratch per thread), which the one-generation kernel never has to carry
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        gen += 1;
        const Rng rng{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)gen, episode, true};
        const double pre_gbest = gbest;
        // ---- agent.act: the action of this generation from row fes of the actor table (same draws as mbx_gauss_policy)
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(2);
        if (tid < A) {
            int row = fes;
            row = row < ar().table_rows ? row : ar().table_rows - 1;
            const float* ms = ar().policy_table + (int64_t)row * 2 * A;
#ifndef MBX_ABLATE_POLICY
            const float a = sample_action(rng, tid, ms[tid], ms[A + tid], MBX_POLICY_RLEPSO);
#else
            const float a = ms[tid];
#endif
            ACT[tid] = a;
            if (ar().out.traj_actions) ar().out.traj_actions[((int64_t)g * B + b) * A + tid] = a;
        }
        if (tid < NP) ORDER[tid] = tid;
        if (tid == 0) { *EQC = 0; *L.FLN = 0; }
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(1);
        __syncthreads();
        if (tid < G) {                                           // __get_coe (:112-132), float32 like k_rlepso_step
            const float* a = ACT + tid * G;
            const float cm = a[0] * 0.01f;
            const float wv = a[1] * 0.8f + 0.1f;
            float den = a[3] + a[4];
            den = den + a[5]; den = den + a[6]; den = den + 1e-5f;
            float scale = 1.f / den;
            scale = scale * a[2]; scale = scale * 8.f;
            double* c = L.COEF + tid * 6;
            c[0] = (double)cm; c[1] = (double)wv;
            c[2] = (double)(scale * a[3]); c[3] = (double)(scale * a[4]);
            c[4] = (double)(scale * a[5]); c[5] = (double)(scale * a[6]);
        }
        // ---- rank the particles by (pbest cost, index).  k_rlepso_step counts, per pair, both `<` and `<=` so that equal costs can be ordered
        // by index; here only the strictly better particles are counted (ONE compare per pair: half the ranking's instructions) and the rank is
        // that count.  Two particles with exactly the same pbest cost then claim the same slot of ORDER: the one that lost the slot sees it
        // (ORDER[rank] != i), raises the workgroup's equal-cost flag, and the workgroup -- uniformly -- redoes the per-particle step with the index
        // tie-break and restages the rows.  Same ranks as k_rlepso_step in every case; the slow path only runs for instances that really hold
        // equal costs (collapsed swarms on F5 / F7 plateaus).
        // The count itself is done ACROSS the lanes: lane l of every wave holds the costs of particles l and l + 64; for each particle i of the wave's share (NP / waves,
        // rounded up) its cost is read once for all lanes (same address: an LDS broadcast), two compares answer all NP pairs, the scalar unit counts the bits of the two
        // masks, and the count is parked in lane k of a result register (v_writelane): 3 vector instructions per particle (the per-lane count it replaced: a compare and
        // an add-with-carry per PAIR, then an atomic), -48 % of the ranking's instructions.  A NaN cost compares false both ways, as in k_rlepso_step.
        {
            static_assert(NP <= 128, "k_rlepso_run: the ranking holds two costs per lane");
            constexpr int WAVES = THREADS / 64, PER = (NP + WAVES - 1) / WAVES;
            const int lane = tid & 63, i0 = (tid >> 6) * PER;
            const double flo = NP >= 64 || lane < NP ? L.PBC[NP >= 64 || lane < NP ? lane : 0] : INFINITY;
            const double fhi = lane + 64 < NP ? L.PBC[lane + 64 < NP ? lane + 64 : 0] : INFINITY;
            int res = 0;
#ifndef MBX_ABLATE_RANK
            static_for<0, PER>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                const double fi = L.PBC[PER * WAVES == NP || i0 + k < NP ? i0 + k : NP - 1];      // (address: the wave's base + a constant)
                const int n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(flo < fi)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(fhi < fi));
                res = writelane_const<k>(n, res);
            });
#else
            res = i0 + lane;
#endif
            if (lane < PER && i0 + lane < NP) NLESS[i0 + lane] = res;
        }
        __syncthreads();
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(2);
        if (tid < NP) {
            const int i = tid, gi = fg.div(i);
            L.CMUT[i] = NP % G == 0 || gi < G ? L.COEF[gi * 6] * L.PNI[i] : 0.;      // (NP a multiple of G: every particle has a group)
            const U4 w = rng.draw((uint32_t)i, MBX_SITE_PART);
            L.R1[i] = u53(w.x, w.y); L.R2[i] = u53(w.z, w.w);
            const int rank = NLESS[i];
            RANK[i] = rank;
            ORDER[rank] = i; L.NC[rank] = L.PBC[i]; L.NCS[rank] = L.PBC[i];
        }
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(1);
        __syncthreads();
        if (tid < NP && ORDER[RANK[tid]] != tid) *EQC = 1;
        // ---- pbest positions -> LDS in rank order, from the owners' registers
        auto stage_pbest = [&](int tid) {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                const int it = tid + j * THREADS;
                if (it < NI) { const int i = fh.div(it), d0 = 2 * (it - i * HD); *(double2*)(L.PB + RANK[i] * D + d0) = double2{pbp[j][0], pbp[j][1]}; }
            }
        };
#ifdef MBX_ABLATE_STAGE
        if (g == 0)
#endif
        stage_pbest(tid);
        __syncthreads();
        if (*EQC) {                                               // workgroup-uniform: equal pbest costs exist, order them by index
            int rank = 0;
            if (tid < NP) {
                const double fi = L.PBC[tid];
                rank = NLESS[tid];
                for (int j = 0; j < tid; ++j) rank += L.PBC[j] == fi;
            }
            __syncthreads();                                      // every thread has read the flag and the fast path's tables
            if (tid < NP) { RANK[tid] = rank; ORDER[rank] = tid; L.NC[rank] = L.PBC[tid]; L.NCS[rank] = L.PBC[tid]; }
            __syncthreads();
            stage_pbest(tid);
            __syncthreads();
            rl_mark_copies(L, NP, D, tid);                        // rows that are copies of the row one rank up leave the FDR scan
            __syncthreads();
        }
        // ---- FDR exemplars -> KB (see k_rlepso_step)
#ifdef MBX_ABLATE_FDR
        for (int e = tid; e < NP * D; e += THREADS) L.KB[e] = 0;
        __syncthreads();
#else
        if constexpr (MBX_RL_PRIO && THREADS == 256) __builtin_amdgcn_s_setprio(0);
        fdr_pass<2, (DC == 40 ? MBX_FDR_UNROLL_D40 : MBX_FDR_UNROLL), TIE, THREADS, (THREADS == 256 ? MBX_FDR_GROUPS : 1), (MBX_FDR_WAVE_DEAL && THREADS == 256 && NPC == 100 && DC == 10 ? 1 : 0)>(L, ORDER, NLESS, NP, D, tid, ub - lb + 1e-5, ar().bp.clk);      // (ends with the barrier that publishes KB)
        if constexpr (MBX_RL_PRIO && THREADS == 256) __builtin_amdgcn_s_setprio(1);
#endif
        // (Measured and dropped, round 3: dealing config 5's half-empty last pass -- 512 items of the highest ranks on 1024 threads -- as single
        // coordinates, one per thread, so that every wave scans: 1.80 -> 1.94 ms per generation; the one-coordinate scan repeats the cost difference
        // and the LDS reads per candidate, which costs more than the idle waves did.)
        // ---- velocity / position update (:179-195): new position -> X, new velocity -> register
        {
            const MoveCtx mc{L, ar().bp.pci, nullptr, rng, nullptr, nullptr, ORDER, NLESS, RANK, NP, D, G, lb, ub, vmax, fg, NP % G == 0};
#ifndef MBX_ABLATE_MOVE
            if constexpr (rl_run_listed(THREADS, NI)) rl_move_listed<THREADS, NI, HD, IT>(mc, fh, tid, vel);
            else {
#pragma unroll
                for (int j = 0; j < IT; ++j) {
                    const int it = tid + j * THREADS;
                    if (it < NI) {
                        const int i = fh.div(it);
                        const double2 c2 = *(const double2*)(L.X + 2 * it);
                        double cur[2] = {c2.x, c2.y};
                        rl_move<2, true>(mc, i, 2 * (it - i * HD), cur, vel[j]);
                    }
                }
            }
#else
            (void)mc;
#endif
        }
        __syncthreads();
        // ---- evaluate, update pbest / gbest and the stagnation counters (:198-233)
        population_costs<eval_dc(DC), eval_md(DC), ConstProblem, rl_run_matvec_chunk(DC), KIND, NOISE>(P, L.eval(), NP, rng, nullptr, MBX_SITE_NOISE0_A, MBX_SITE_NOISE0_B);
        fes += NP;
#ifndef MBX_ABLATE_COMMIT
        commit(true, tid);
#endif
        // ---- re-initialisation (:238-239, 134-168)
        // the count: every wave that holds particles counts its lanes' flags on the scalar unit and publishes the sum; ONE barrier (which is also the one that ends
        // update()'s commit) where __syncthreads_count spends three, a block-size look-up and a cross-lane add in all four waves
        int mine = 0;
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(2);
        if (tid < NP) {
#ifndef MBX_ABLATE_REINIT_DRAW
            const U4 w = rng.draw((uint32_t)tid, MBX_SITE_REINIT);
            const double u = u53(w.x, w.y);
            mine = u < L.CMUT[tid] * 0.01 * L.PNI[tid];
#endif
            L.MASK[tid] = mine;
        }
        {
            const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine != 0));
            if ((tid & 63) == 0 && tid < 64 * PW) RCNT[tid >> 6] = cnt;
            if constexpr (PRIO2) __builtin_amdgcn_s_setprio(1);
            __syncthreads();
            int n = 0;
#pragma unroll
            for (int w = 0; w < PW; ++w) n += RCNT[w];
            n_reinit = __builtin_amdgcn_readfirstlane(n);
        }
        if (n_reinit > 0) {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                const int it = tid + j * THREADS;
                if (it < NI && L.MASK[fh.div(it)]) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int e = 2 * it + q;
                        const U4 w = rng.draw((uint32_t)e, MBX_SITE_ELEM_R);
                        const double up = u53(w.x, w.y), uv = u53(w.z, w.w);
                        L.X[e] = lb + (ub - lb) * up;
                        vel[j][q] = -vmax + (vmax - (-vmax)) * uv;
                    }
                }
            }
            __syncthreads();
            population_costs<eval_dc(DC), eval_md(DC), ConstProblem, rl_run_matvec_chunk(DC), KIND, NOISE>(P, L.eval(), NP, rng, nullptr, MBX_SITE_NOISE1_A, MBX_SITE_NOISE1_B);
            fes += n_reinit;
            commit(false, tid);
        }
        // ---- logging, termination, reward (:241-261): the counters are scalars (see above), the two float64 compares on gbest are made wave-uniform by a ballot;
        // thread 0 writes the curve.  (fes and the log point are integers below 2^31 and 2^62: the integer compare is the reference's float64 one)
#ifndef MBX_ABLATE_LOG
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(2);
        if ((int64_t)fes >= (int64_t)log_index * ar().bp.log_interval) { log_index += 1; if (tid == 0) curve_put(cost, ar().bp.n_logpoint, cost_len, gbest); cost_len += 1; }
        done = fes >= ar().bp.max_fes;
        if (!isnan(P.optimum) && ar().bp.early_stop) done = done || __builtin_amdgcn_ballot_w64(gbest <= 1e-8) != 0ull;
        if (done) {
            if (cost_len >= ar().bp.n_logpoint + 1) { if (tid == 0) curve_put(cost, ar().bp.n_logpoint, cost_len - 1, gbest); }
            else { if (tid == 0) curve_put(cost, ar().bp.n_logpoint, cost_len, gbest); cost_len += 1; }
        }
        const bool improved = __builtin_amdgcn_ballot_w64(gbest < pre_gbest) != 0ull;
        ret += improved ? 1 : -1;
        if (tid == 0) {
            if (ar().out.traj_state) ar().out.traj_state[g * B + b] = (double)fes / ar().bp.max_fes;
            if (ar().out.traj_reward) ar().out.traj_reward[g * B + b] = improved ? 1. : -1.;
            if (ar().out.traj_done) ar().out.traj_done[g * B + b] = done ? 1 : 0;
        }
        if constexpr (PRIO2) __builtin_amdgcn_s_setprio(1);
#endif
    }
    // ---- store the state block once
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        const int it = tid + j * THREADS;
        if (it < NI) {
            *(double2*)(gPos + 2 * it) = *(const double2*)(L.X + 2 * it);
            *(double2*)(gVel + 2 * it) = double2{vel[j][0], vel[j][1]};
            *(double2*)(gPB + 2 * it) = double2{pbp[j][0], pbp[j][1]};
        }
    }
    if (tid < NP) {
        S[MBX_RLEPSO_ST_PBEST(NP, D) + tid] = L.PBC[tid];
        S[MBX_RLEPSO_ST_PNI(NP, D) + tid] = L.PNI[tid];
        S[MBX_RLEPSO_ST_CCOST(NP, D) + tid] = cc;
    }
    if (tid < D) S[MBX_RLEPSO_ST_GBPOS(NP, D) + tid] = L.GB[tid];
    const double st = (double)fes / ar().bp.max_fes;
    for (int t = g + tid; t < n_gens; t += THREADS) {            // generations after the instance finished
        if (ar().out.traj_state) ar().out.traj_state[t * B + b] = st;
        if (ar().out.traj_reward) ar().out.traj_reward[t * B + b] = 0.;
        if (ar().out.traj_done) ar().out.traj_done[t * B + b] = 1;
    }
    if (tid == 0) {
        sc[MBX_SC_GBEST] = gbest; sc[MBX_SC_FES] = fes; sc[MBX_SC_LOG_INDEX] = log_index; sc[MBX_SC_COST_LEN] = cost_len;
        sc[MBX_SC_DONE] = done ? 1. : 0.; sc[MBX_SC_RETURN] += ret; sc[MBX_SC_GEN] = gen;
        sc[MBX_SC_GBEST_IDX] = gbest_idx; sc[MBX_SC_REINIT] = n_reinit > 0 ? 1. : 0.;
        if (ar().out.state_out) ar().out.state_out[b] = st;
        if (ar().out.reward_out) ar().out.reward_out[b] = ret;
        if (ar().out.done_out) ar().out.done_out[b] = done ? 1 : 0;
        if (clocked) {
            atomicAdd(ar().bp.clk, (unsigned long long)__builtin_amdgcn_s_memtime() - clk_c0);
            atomicAdd(ar().bp.clk + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime() - clk_r0);
        }
    }
}

// The kernel's arguments as the kernarg segment lays them out (a callee cannot name the kernel's parameters; it is handed the segment's address)
struct RlRunArgs {
    BatchParams bp;
    const float* policy_table;
    int32_t table_rows, n_gens;
    RunOut out;
};

// rl_run_body out of line, one instantiation per function kind: register-allocated and scheduled without the other kinds' code (a build of the any-kind kernel with every
// kind but one compiled out of the evaluator ran a one-function batch 8-12 % faster: docs/EXPERIMENTS.md).  In a callee s[8:9] is the IMPLICIT argument pointer, so the
// address of the kernel's argument block is an argument; every field access goes through that address (see rl_run_body).
template <int THREADS, int NPC, int DC, int GC, int KIND, int NOISE, bool TIE>
__device__ __noinline__ void rl_run_body_of_kind(uint32_t karg_lo_, uint32_t karg_hi_)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)karg_lo_), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)karg_hi_);
    typedef const RlRunArgs __attribute__((address_space(4))) CArgs;
    auto ar = [&]() -> CArgs& {
        uintptr_t p = (uintptr_t)(((uint64_t)hi << 32) | lo);
        asm volatile("" : "+s"(p));
        return *(CArgs*)p;
    };
    rl_run_body<THREADS, NPC, DC, GC, KIND, NOISE, TIE>(ar);
}

// per-kind bodies for the geometries of configs 1 / 2 (D = 10) and 5 (D = 40): the 24 noise-free BBOB kinds with the noise models compiled out (another
// +2 % on the headline) + the eight kinds of the noisy suite with them (rl_run_kind_ok); the other geometries run the any-kind body inline.  Same-box A/B against the any-kind kernel: D = 10 117.6 -> 113.0 us per generation, D = 40 1.602 -> 1.585 ms.
__host__ __device__ constexpr bool rl_run_per_kind(int DC) { return DC == 10 || DC == 40; }
// a body exists for: the 24 noise-free BBOB kinds; with noise, the eight kinds of the noisy suite (problem/bbob.py: _NOISY)
__host__ __device__ constexpr bool rl_run_kind_ok(int kind, int noise_kind)
{
    return noise_kind == MBX_NOISE_NONE ? (kind >= 1 && kind <= 24)
                                        : (kind == 1 || kind == 7 || kind == 8 || kind == 10 || kind == 14 || kind == 17 || kind == 19 || kind == 21);
}

// TIE: see k_rlepso_step
template <int THREADS, int NPC, int DC, int GC, bool TIE = true>
__global__ __launch_bounds__(THREADS) MBX_RUN_WAVES void k_rlepso_run(BatchParams bp, const float* __restrict__ policy_table, int table_rows,
                                                                     int n_gens, RunOut out)
{
    if constexpr (rl_run_per_kind(DC)) {
        static_assert(sizeof(RlRunArgs) == sizeof(BatchParams) + 8 + 8 + sizeof(RunOut), "RlRunArgs mirrors the kernel's parameter list");
        const uint64_t karg = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
        const uint32_t klo = (uint32_t)karg, khi = (uint32_t)(karg >> 32);
        const DevProblem* pr = bp.problems + bp.problem_idx[bp.order[blockIdx.x]];
        const int kind = __builtin_amdgcn_readfirstlane(pr->kind);
        const bool noisy = __builtin_amdgcn_readfirstlane(pr->noise_kind) != MBX_NOISE_NONE;
#define MBX_RL_KIND(K) case K: rl_run_body_of_kind<THREADS, NPC, DC, GC, K, 0, TIE>(klo, khi); break;
#define MBX_RL_NOISY(K) case K: rl_run_body_of_kind<THREADS, NPC, DC, GC, K, 1, TIE>(klo, khi); break;
        if (noisy) {
            switch (kind) {
            MBX_RL_NOISY(1) MBX_RL_NOISY(7) MBX_RL_NOISY(8) MBX_RL_NOISY(10) MBX_RL_NOISY(14) MBX_RL_NOISY(17) MBX_RL_NOISY(19) MBX_RL_NOISY(21)
            default: rl_run_body_of_kind<THREADS, NPC, DC, GC, 0, -1, TIE>(klo, khi);      // any other (kind, noise model) pair: the any-kind body, out of line like the rest
            }
        } else {
            switch (kind) {
            MBX_RL_KIND(1) MBX_RL_KIND(2) MBX_RL_KIND(3) MBX_RL_KIND(4) MBX_RL_KIND(5) MBX_RL_KIND(6) MBX_RL_KIND(7) MBX_RL_KIND(8)
            MBX_RL_KIND(9) MBX_RL_KIND(10) MBX_RL_KIND(11) MBX_RL_KIND(12) MBX_RL_KIND(13) MBX_RL_KIND(14) MBX_RL_KIND(15) MBX_RL_KIND(16)
            MBX_RL_KIND(17) MBX_RL_KIND(18) MBX_RL_KIND(19) MBX_RL_KIND(20) MBX_RL_KIND(21) MBX_RL_KIND(22) MBX_RL_KIND(23) MBX_RL_KIND(24)
            default: rl_run_body_of_kind<THREADS, NPC, DC, GC, 0, -1, TIE>(klo, khi);
            }
        }
#undef MBX_RL_NOISY
#undef MBX_RL_KIND
    } else {
        typedef const RlRunArgs __attribute__((address_space(4))) CArgs;
        rl_run_body<THREADS, NPC, DC, GC, 0, -1, TIE>([]() -> CArgs& {
            return *(CArgs*)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
        });
    }
}

}  // namespace mbx
