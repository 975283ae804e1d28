"""numpy's summation order, stated plainly, the wrong orders a kernel could have instead, and the vectors that tell them apart.  Not a test module:
tests/test_numpy_order.py (CPU) holds the statement against the installed numpy and proves that the vectors discriminate; tests/test_gpu_numpy_order.py
holds the device routines (csrc/mbx_npsum.hpp, md_pairwise, jd_dist4) against numpy on the same vectors.

The rule (np.add.reduce over a contiguous float64 axis; numpy's pairwise_sum):

    fewer than 8 elements     one by one, starting from 0.
    up to 128 elements        eight accumulators r[k] = a[k] + a[8 + k] + a[16 + k] + ..., combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
                              then the n % 8 elements of the tail one by one
    more than 128 elements    the sum of the left half and the sum of the right half, the left half n // 2 rounded down to a multiple of 8

Every function here takes a matrix [K, n] and sums each of its K rows, all rows in step: `+` between arrays is one IEEE addition per element, and no
reduction of numpy's is called, so the order of the additions is the one written down."""
import functools

import numpy as np

BLOCK = 128


def _block(M):
    """At most 128 elements per row."""
    K, n = M.shape
    if n < 8:
        s = np.zeros(K)
        for k in range(n):
            s = s + M[:, k]
        return s
    r = M[:, :8].copy()
    i = 8
    while i < n - n % 8:
        r = r + M[:, i:i + 8]
        i += 8
    s = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    while i < n:
        s = s + M[:, i]
        i += 1
    return s


def _halved(M, block):
    n = M.shape[1]
    if n <= BLOCK:
        return block(M)
    n2 = n // 2
    n2 -= n2 % 8
    return _halved(M[:, :n2], block) + _halved(M[:, n2:], block)


def numpy_order(M):
    """The rule: the sum of every row of M in numpy's order."""
    return _halved(np.asarray(M, dtype=np.float64), _block)


# ------------------------------------------------------------------------------------------------ the wrong orders
def sequential(M):
    """One by one from 0., at every length."""
    s = np.zeros(M.shape[0])
    for k in range(M.shape[1]):
        s = s + M[:, k]
    return s


def one_halving(M):
    """np_sum as it was: one halving step above 128 elements, both halves handed to the block whatever their length.  numpy's order unless the right half
    is longer than 128 elements, which is n = 249 .. 255."""
    n = M.shape[1]
    assert n <= 256, n
    if n <= BLOCK:
        return _block(M)
    n2 = n // 2
    n2 -= n2 % 8
    return _block(M[:, :n2]) + _block(M[:, n2:])


def binary_tree(M):
    """Halves down to single elements."""
    n = M.shape[1]
    if n == 0:
        return np.zeros(M.shape[0])
    if n == 1:
        return M[:, 0].copy()
    return binary_tree(M[:, :n // 2]) + binary_tree(M[:, n // 2:])


def _block_tail_first(M):
    K, n = M.shape
    if n < 8:
        return _block(M)
    r = M[:, :8].copy()
    i = 8
    while i < n - n % 8:
        r = r + M[:, i:i + 8]
        i += 8
    r[:, :n - i] = r[:, :n - i] + M[:, i:]
    return ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))


def tail_first(M):
    """The tail of a block joins the accumulators before they are combined, not the combined sum after."""
    return _halved(M, _block_tail_first)


# name -> (the order, the lengths at which it is another order than numpy's)
WRONG_ORDERS = {
    'sequential': (sequential, lambda n: n >= 8),
    'one_halving': (one_halving, lambda n: 249 <= n <= 255),
    'binary_tree': (binary_tree, lambda n: n >= 9),
    'tail_first': (tail_first, lambda n: n >= 9 and n % 8 != 0),
}

# ------------------------------------------------------------------------------------------------ the data
N_RANDOM, N_UNIFORM = 12, 4
KINDS = ('random',) * N_RANDOM + ('uniform',) * N_UNIFORM + ('cancellation', 'tenths', 'negative_zeros', 'signed_zeros')
ZERO_KINDS = ('negative_zeros', 'signed_zeros')          # compared with ==: the sign numpy gives a sum of zeros has changed between releases
SEED = 20251


@functools.lru_cache(maxsize=None)
def vectors(n):
    """[len(KINDS), n] float64, C-contiguous, the same at every call: N(0, 1) * exp(U(-8, 8)) rows; U(1, 2) rows (one magnitude: every addition rounds, so a
    tail of one or two elements that joins early still shows, where the wide rows absorb it); a row of small terms with pairs +B, -B (B up to e^40) planted
    at random places; a row of 0.1s; a row of -0.0; a row of zeros of random sign."""
    rs = np.random.RandomState([SEED, n])
    M = np.empty((len(KINDS), n))
    M[:N_RANDOM] = rs.standard_normal((N_RANDOM, n)) * np.exp(rs.uniform(-8, 8, (N_RANDOM, n)))
    M[N_RANDOM:N_RANDOM + N_UNIFORM] = rs.uniform(1, 2, (N_UNIFORM, n))
    c = rs.standard_normal(n)
    where = rs.permutation(n)[:n // 2 * 2].reshape(-1, 2)[:max(n // 4, min(n // 2, 1))]
    big = np.exp(rs.uniform(20, 40, len(where)))
    c[where[:, 0]], c[where[:, 1]] = big, -big
    M[KINDS.index('cancellation')] = c
    M[KINDS.index('tenths')] = 0.1
    M[KINDS.index('negative_zeros')] = -0.0
    M[KINDS.index('signed_zeros')] = np.where(rs.rand(n) < 0.5, -0.0, 0.0)
    M.setflags(write=False)
    return M


def bitwise_rows():
    """Indices of the rows whose sums are compared bit for bit."""
    return np.array([k for k, kind in enumerate(KINDS) if kind not in ZERO_KINDS])


def zero_rows():
    return np.array([k for k, kind in enumerate(KINDS) if kind in ZERO_KINDS])


def lengths_to_256():
    return list(range(0, 257))


@functools.lru_cache(maxsize=None)
def lengths_to_3200():
    """Every length up to 520, the lengths around 1024, 2048 and the upper bound of md_pairwise, and 180 more drawn between them."""
    rs = np.random.RandomState(SEED)
    more = rs.choice(np.arange(521, 3191), 180, replace=False)
    return sorted(set(range(0, 521)) | set(range(1023, 1034)) | set(range(2047, 2058)) | set(range(3191, 3201)) | set(int(v) for v in more))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.view(np.uint64) == want.view(np.uint64)
