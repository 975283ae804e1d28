// mbx_qchoose.hpp -- the choice rule of the tabular agents (QLPSO, NRLPSO), shared by their step kernels (mbx_qlpso.hpp, mbx_nrlpso.hpp).
#pragma once
#include "mbx_device.hpp"

namespace mbx {

// QLPSO_Agent.__get_action (qlpso_agent.py:35-38) and NRLPSO_Agent.__get_action (nrlpso_agent.py:28-31): p = softmax(Q[state]); np.random.choice(4, p = p) with one uniform u:
// index = searchsorted(cumsum(p) / cumsum(p)[-1], u, side = 'right').
__device__ __forceinline__ int ql_choose(const double* __restrict__ q_row, double u)
{
    double e[4], s = 0., cdf[4], c = 0.;
#pragma unroll
    for (int k = 0; k < 4; ++k) { e[k] = m_exp(q_row[k]); s += e[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { c += e[k] / s; cdf[k] = c; }
    int idx = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx += (cdf[k] / cdf[3]) <= u;
    return idx;
}

}  // namespace mbx
