// mbx_npsum.hpp -- numpy's summation order (np.add.reduce over a contiguous axis: pairwise_sum with 8 accumulators), in ONE place for the kernels whose
// results hinge on it: QLPSO's swarm diversity (mbx_qlpso.hpp), DEDQN's and RL-HPSDE's landscape features, NRLPSO's row means, the sums of the sorted-DE
// kernels (md_pairwise, mbx_depop.hpp), SAHLPSO's strategy probabilities and LES's cost statistics.  tests/test_gpu_numpy_order.py runs every routine of
// this file through mbx_debug_reduce against np.add.reduce, bit for bit, at every length it is declared for.
#pragma once

namespace mbx {

// np.add.reduce over n <= 128 contiguous values produced by elem(k): one by one from 0. below 8 values, else 8 accumulators, then the tail (the block of
// numpy's pairwise_sum).  Above 128 values numpy halves first (np_pairwise below): the callers name who keeps n <= 128.
template <class F>
__device__ __forceinline__ double np_sum_block(F elem, int n)
{
    if (n < 8) { double s = 0.; for (int k = 0; k < n; ++k) s += elem(k); return s; }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = elem(k);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += elem(i + k);
    }
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s += elem(i);
    return s;
}

// The halving above 128 elements, DEPTH levels of it: a stretch of more than 128 elements is the sum of its two halves, the left one a multiple of 8 long;
// leaf(off, m) is the block sum of elements off .. off + m - 1, m <= 128.  n2 is rounded down, so the right half may be the longer one by up to 8 + 1 --
// n = 249 .. 255 leave 129 .. 135 elements on the right, which numpy halves again -- and DEPTH has to cover that: a stretch still longer than 128
// elements at depth 0 answers NaN, never a sum in another order.
template <int DEPTH, class Leaf>
__device__ __forceinline__ double np_pairwise(Leaf leaf, int off, int n)
{
    if (n <= 128) return leaf(off, n);
    if constexpr (DEPTH == 0) return NAN;
    else {
        int n2 = n / 2;
        n2 -= n2 % 8;
        return np_pairwise<DEPTH - 1>(leaf, off, n2) + np_pairwise<DEPTH - 1>(leaf, off + n2, n - n2);
    }
}

// np.add.reduce over n <= 256 values produced by elem(k): two levels of halving (the left half is a block; the right one is, or halves into two)
template <class F>
__device__ __forceinline__ double np_sum(F elem, int n)
{
    return np_pairwise<2>([&](int off, int m) { return np_sum_block([&](int k) { return elem(off + k); }, m); }, 0, n);
}

// np_sum_block dealt over eight lanes: lane k of every group of eight keeps the accumulator r[k], and the partial sums meet in np_sum_block's own
// order, so the result is bit-identical with a chain an eighth as long.  EVERY lane of the wave calls (shuffles) and gets the result.  n <= 128.
template <class F>
__device__ __forceinline__ double np_sum_lanes8(F elem, int n)
{
    if (n < 8) { double s = 0.; for (int k = 0; k < n; ++k) s += elem(k); return s; }
    const int k = (int)threadIdx.x & 7, base = (int)threadIdx.x & 56;
    double r = elem(k);
    int i = 8;
    for (; i < n - (n % 8); i += 8) r += elem(i + k);
    double q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = __shfl(r, base + j, 64);
    double s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    for (; i < n; ++i) s += elem(i);
    return s;
}

}  // namespace mbx
