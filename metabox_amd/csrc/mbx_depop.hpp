// mbx_depop.hpp — "DE population in the state block": the device pieces shared by the kernels that keep a cost-sorted, shrinking DE population in
// the state block (MadDE mbx_madde.hpp, NL_SHADE_LBC mbx_nlshade.hpp, RL-HPSDE mbx_rlhpsde.hpp).
//
// The LDS carve-up (MdLds, md_carve), the workgroup prefix scan, numpy's pairwise sum, the bitonic (cost, row) sort, and the phases of a reset and
// of an update that the three algorithms have in common: the chunked evaluation of rows (md_eval_rows), the sorted first population
// (md_init_sorted), the ranks of the improved rows (md_rank_improved), the archive's write arbitration (md_archive_write; RL-HPSDE has no
// archive), the memory update's weighted sums (md_weighted_sums), and the replacement, sort and row move into the other population buffer
// (md_replace_sorted).  The three state layouts differ, so the phases take pointers into the state block and the tape, and callables where the
// algorithms differ; they are templates on the problem type (a DevProblem by value in MadDE, a ConstProblem& in the other two).  What stays
// with each algorithm: its draws, mutation, crossover and bookkeeping; NL_SHADE_LBC's update also keeps its evaluation loop, ranking and sums
// written out, because it measured slower through md_eval_rows / md_rank_improved / md_weighted_sums (docs/EXPERIMENTS.md).
#pragma once
#include "mbx_device.hpp"
#include "mbx_lds.hpp"
#include "mbx_npsum.hpp"    // np_sum_block, np_pairwise: numpy's pairwise summation order

namespace mbx {

// The LDS layout (MdLds, md_chunk, md_pad, md_work_doubles, md_lds_doubles, md_carve) lives in mbx_lds.hpp.

// Exclusive prefix sums over the threads of three per-thread counts (base) and their totals.  All threads call; ends with a barrier.
__device__ __forceinline__ void md_scan3(int* CNT, const int (&c)[3], int (&base)[3], int (&tot)[3])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int g = 0; g < 3; ++g) CNT[g * kThreads + tid] = c[g];
    __syncthreads();
    if (tid < 3) {
        int run = 0;
        for (int t = 0; t < kThreads; ++t) { const int v = CNT[tid * kThreads + t]; CNT[tid * kThreads + t] = run; run += v; }
        CNT[3 * kThreads + tid] = run;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 3; ++g) { base[g] = CNT[g * kThreads + tid]; tot[g] = CNT[3 * kThreads + g]; }
    __syncthreads();
}

// numpy's pairwise sum of a contiguous vector, mbx_npsum.hpp's block and halving: the block out of line (the recursion below names it 64 times) ...
__device__ __noinline__ double md_pw_leaf(const double* a, int n)
{
    return np_sum_block([a](int i) { return a[i]; }, n);
}
// ... and DEPTH levels of halving above it: 128 << DEPTH elements at least (the right half may be the longer one: the depth is chosen with a level to spare)
template <int DEPTH>
__device__ __forceinline__ double md_pw(const double* a, int n)
{
    return np_pairwise<DEPTH>([a](int off, int m) { return md_pw_leaf(a + off, m); }, 0, n);
}
__device__ __forceinline__ double md_pairwise(const double* a, int n) { return md_pw<6>(a, n); }      // n <= 3200

// (cost, row) order of the sort; a NaN cost sorts last, as numpy places it
__device__ __forceinline__ bool md_less(double ka, int ia, double kb, int ib)
{
    const bool an = isnan(ka), bn = isnan(kb);
    if (an || bn) return an == bn ? ia < ib : bn;
    return ka < kb || (ka == kb && ia < ib);
}

// Sort the pairs KEY / IDX [0, npad) (npad a power of two, padded with +inf / rows >= n) ascending by md_less.  All threads call; the
// caller synchronises before, the sort ends with a barrier.
__device__ __forceinline__ void md_sort(double* KEY, int* IDX, int npad)
{
    const int tid = threadIdx.x;
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
#ifndef MBX_ABLATE_MD_SORT
            for (int t = tid; t < (npad >> 1); t += kThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const double ka = KEY[i], kb = KEY[l];
                const int ia = IDX[i], ib = IDX[l];
                if (md_less(kb, ib, ka, ia) == up) { KEY[i] = kb; KEY[l] = ka; IDX[i] = ib; IDX[l] = ia; }
            }
#endif
            __syncthreads();
        }
}

// ------------------------------------------------------------------------------------------------ the shared phases
// Costs of n_rows rows in chunks of md_chunk(D): element e of the rows (row-major) is src(e), the costs go to dst[0, n_rows).  The rows are rows
// 0 .. n_rows - 1 of n_total for the noise draws (tape_noise: [3, n_total] or nullptr; Philox sites site_a / site_b).  The caller has staged
// the problem (stage_problem) and made what src reads visible.  All threads call; ends with a barrier.
template <class PT, class Src>
__device__ __forceinline__ void md_eval_rows(const PT& P, const MdLds& L, int n_rows, int n_total, int D, Src src, double* dst, const Rng& rng,
                                             const double* tape_noise, uint32_t site_a, uint32_t site_b)
{
    const int tid = threadIdx.x, CH = md_chunk(D);
    for (int c0 = 0; c0 < n_rows; c0 += CH) {
        const int n = min(CH, n_rows - c0);
        for (int e = tid; e < n * D; e += kThreads) L.EV[e] = src(c0 * D + e);
        __syncthreads();
        population_costs(P, L.eval(n, D, L.TC), n, rng, tape_noise, site_a, site_b, c0, n_total);
        if (tid < n) dst[c0 + tid] = L.TC[tid];
        __syncthreads();
    }
}

// The tail of a reset: the N0 rows of gU with costs gNC, ordered by (cost, row), into pop; the sorted costs into gC.  They stay in L.KEY, the best
// one in L.KEY[0], until the work area is used again.  All threads call, after a barrier behind the writes of gU / gNC; no barrier at the end.
__device__ __forceinline__ void md_init_sorted(const MdLds& L, const double* gU, const double* gNC, double* pop, double* gC, int N0, int D)
{
    const int tid = threadIdx.x, npad = md_pad(N0);
    for (int t = tid; t < npad; t += kThreads) { L.KEY[t] = t < N0 ? gNC[t] : INFINITY; L.IDX[t] = t; }
    __syncthreads();
    md_sort(L.KEY, L.IDX, npad);
    const FastDiv fd(D);
    for (int e = tid; e < N0 * D; e += kThreads) {
        const int r = fd.div(e);
        pop[e] = gU[min(L.IDX[r], N0 - 1) * D + (e - r * D)];             // (clamped: a NaN cost sorts behind the padding)
    }
    for (int t = tid; t < N0; t += kThreads) gC[t] = L.KEY[t];
}

// Selection is strict (new cost < old cost).  base: the rank, among the improved rows, of this thread's first improved row in [row0, row1);
// n_opt: their number.  All threads call; ends with a barrier.
__device__ __forceinline__ void md_rank_improved(const MdLds& L, const double* gC, const double* gNC, int row0, int row1, int& base, int& n_opt)
{
    int cnt[3] = {0, 0, 0}, b[3], tot[3];
    for (int i = row0; i < row1; ++i) cnt[0] += gNC[i] < gC[i];
    md_scan3(L.CNT, cnt, b, tot);
    base = b[0]; n_opt = tot[0];
}

// The parents of the improved rows enter the archive, decided in parallel: with alen = narc + n_app rows after the n_app appends, the improved row
// of rank k < n_app writes row narc + k, rank k >= n_app overwrites row target(k) in [0, alen), and of several writers of one row the highest rank
// wins (an atomic maximum in L.WIN), which is what the reference's one-after-another loop leaves behind.  ranks(put) calls put(k, parent row) for
// every rank k this thread owns, the same ones at every call.  All threads call, alen > 0; the caller synchronises after.
template <class Target, class Ranks>
__device__ __forceinline__ void md_archive_write(const MdLds& L, double* arc, const double* pop, int D, int narc, int n_app, int alen, Target target,
                                                 Ranks ranks)
{
    for (int t = threadIdx.x; t < alen; t += kThreads) L.WIN[t] = -1;
    __syncthreads();
    ranks([&](int k, int) { if (k >= n_app) atomicMax(&L.WIN[target(k)], k); });
    __syncthreads();
    ranks([&](int k, int i) {
        const int t = k < n_app ? narc + k : target(k);
        if (k < n_app ? L.WIN[t] < 0 : L.WIN[t] == k)
            for (int d = 0; d < D; ++d) arc[(int64_t)t * D + d] = pop[(int64_t)i * D + d];
    });
}

// The sums of a memory update over the n_opt improved rows, each compacted in rank order into L.VEC and added in numpy's pairwise order:
// sums[0] = sum of df(cost, new cost), sums[pass] = sum of term(pass, w, row) with w = df / sums[0] for pass 1 .. NPASS - 1.  All threads call;
// every pass ends with a barrier.  (NL_SHADE_LBC's sums -- another df, pow terms, no later pass unless sums[0] > 0 -- are written out in its kernel.)
template <int NPASS, class Df, class Term>
__device__ __forceinline__ void md_weighted_sums(const MdLds& L, const double* gC, const double* gNC, int row0, int row1, int base, int n_opt, Df df,
                                                 Term term, double (&sums)[NPASS])
{
    for (int pass = 0; pass < NPASS; ++pass) {
        int k = base;
        for (int i = row0; i < row1; ++i) {
            const double c = gC[i], nc = gNC[i];
            if (nc < c) {
                double v = df(c, nc);
                if (pass > 0) v = term(pass, v / sums[0], i);
                L.VEC[k++] = v;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) L.RED[0] = md_pairwise(L.VEC, n_opt);
        __syncthreads();
        sums[pass] = L.RED[0];
        __syncthreads();
    }
}

// Replacement and sort: row t of the NP live rows keeps the better of its cost gC[t] and its trial's gNC[t] (the trial wins only when strictly
// better), the rows are ordered by (cost, row), and the first NPn of them move from pop / gU into npop, their costs into gC.  The sorted costs
// stay in L.KEY.  All threads call, after a barrier behind the last use of the work area; no barrier after the store of gC.
__device__ __forceinline__ void md_replace_sorted(const MdLds& L, double* gC, const double* gNC, const double* gU, const double* pop, double* npop,
                                                  int NP, int NPn, int D)
{
    const int tid = threadIdx.x, npad = md_pad(NP);
    for (int t = tid; t < npad; t += kThreads) {
        double key = INFINITY;
        if (t < NP) { const double c = gC[t], nc = gNC[t]; key = nc < c ? nc : c; }
        L.KEY[t] = key; L.IDX[t] = t;
    }
    __syncthreads();
    md_sort(L.KEY, L.IDX, npad);
#ifndef MBX_ABLATE_MD_SORT
    const FastDiv fd(D);
    for (int e = tid; e < NPn * D; e += kThreads) {
        const int r = fd.div(e), d = e - r * D, p = min(L.IDX[r], NP - 1);      // (clamped: a NaN cost sorts behind the padding)
        npop[e] = gNC[p] < gC[p] ? gU[(int64_t)p * D + d] : pop[(int64_t)p * D + d];
    }
#endif
    __syncthreads();
    for (int t = tid; t < NPn; t += kThreads) gC[t] = L.KEY[t];
}

}  // namespace mbx
