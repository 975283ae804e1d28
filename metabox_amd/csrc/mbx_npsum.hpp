// mbx_npsum.hpp -- numpy's summation order (np.add.reduce over a contiguous axis: pairwise_sum with 8 accumulators), shared by the kernels whose
// results hinge on it: QLPSO's swarm diversity (mbx_qlpso.hpp) and DEDQN's landscape features (mbx_dedqn.hpp).
#pragma once

namespace mbx {

// np.add.reduce over n <= 128 contiguous values produced by elem(k): 8 accumulators, then the tail (numpy's pairwise_sum).
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

// ... and for n <= 256 (one halving step above 128 elements)
template <class F>
__device__ __forceinline__ double np_sum(F elem, int n)
{
    if (n <= 128) return np_sum_block(elem, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum_block(elem, n2) + np_sum_block([&](int k) { return elem(n2 + k); }, n - n2);
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
