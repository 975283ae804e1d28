"""CPU: the plain statement of numpy's summation order (tests/numpy_order.py) against the installed numpy, and the proof that the vectors the device
routines are tested on (tests/test_gpu_numpy_order.py) tell numpy's order from the orders a kernel could have instead.  No GPU, no library."""
import numpy as np
import pytest

import numpy_order as no


def _first_failure(lengths, same):
    """The first length at which same(n) is not all true, or None."""
    for n in lengths:
        ok = same(n)
        if not np.all(ok):
            return n, np.nonzero(~np.asarray(ok))[0].tolist()
    return None


def test_the_statement_is_the_installed_numpy_bit_for_bit():
    """If this fails the installed numpy does not sum in the order the kernels implement, and no kernel is to blame for what the GPU tests then report."""
    rows = no.bitwise_rows()

    def same(n):
        M = no.vectors(n)
        got = no.numpy_order(M)
        want = np.array([np.add.reduce(M[k]) for k in range(len(M))])
        return no.same_bits(got[rows], want[rows])
    lengths = no.lengths_to_3200()
    assert set(range(0, 521)) <= set(lengths) and len([n for n in lengths if n > 520]) >= 200 and max(lengths) == 3200
    assert {*range(1023, 1034), *range(2047, 2058), *range(3191, 3201)} <= set(lengths)
    bad = _first_failure(lengths, same)
    assert bad is None, f'numpy {np.__version__}: np.add.reduce leaves the stated order at length {bad[0]} (rows {bad[1]})'


def test_the_statement_is_numpy_sum_over_the_rows_of_a_matrix():
    """np.sum(M, 1) of a C-contiguous matrix: the other spelling the reference uses (the diversity's np.sum(., 1))."""
    rows = no.bitwise_rows()

    def same(n):
        M = no.vectors(n)
        assert M.flags['C_CONTIGUOUS']
        return no.same_bits(no.numpy_order(M)[rows], np.sum(M, 1)[rows])
    bad = _first_failure(no.lengths_to_3200(), same)
    assert bad is None, f'numpy {np.__version__}: np.sum(M, 1) leaves the stated order at length {bad[0]} (rows {bad[1]})'


@pytest.mark.parametrize('name', sorted(no.WRONG_ORDERS))
def test_the_vectors_tell_numpy_order_from(name):
    """A condition on the recipe, not a measurement: at every length from 9 to 256 at which the named order is another order than numpy's, at least one
    vector gives another double than np.add.reduce.  Where it IS numpy's order (one_halving outside 249 .. 255, tail_first at multiples of 8) it agrees."""
    order, differs_at = no.WRONG_ORDERS[name]
    rows = no.bitwise_rows()
    blind, counts = [], {}
    for n in range(9, 257):
        M = no.vectors(n)
        want = np.array([np.add.reduce(M[k]) for k in rows])
        same = no.same_bits(order(M)[rows], want)
        if differs_at(n):
            counts[n] = int((~same).sum())
            if same.all():
                blind.append(n)
        else:
            assert same.all(), (name, n)
    assert counts, name
    print(f'{name}: differs from np.add.reduce on {min(counts.values())} .. {max(counts.values())} of {len(rows)} vectors per length, {len(counts)} lengths'
          + (f' ({counts})' if len(counts) < 10 else ''))
    assert not blind, (name, 'no vector tells at lengths', blind)


def test_one_halving_is_numpy_order_except_from_249_to_255():
    """np_sum before the fix, restated: where it left numpy's order and on how many of the vectors."""
    rows = no.bitwise_rows()
    off = {}
    for n in range(0, 257):
        M = no.vectors(n)
        d = int((~no.same_bits(no.one_halving(M)[rows], np.sum(M, 1)[rows])).sum())
        if d:
            off[n] = d
    print(f'one_halving differs from numpy at {off} of {len(rows)} vectors per length')
    assert sorted(off) == list(range(249, 256)), off


def test_sums_of_signed_zeros_equal_numpy():
    """Compared with ==; the sign of the sum is printed, not asserted (the sign numpy gives an all-negative-zero sum has changed between releases)."""
    rows = no.zero_rows()
    signs = set()
    for n in no.lengths_to_256():
        M = no.vectors(n)
        got, want = no.numpy_order(M)[rows], np.sum(M, 1)[rows]
        assert np.all(got == want) and np.all(want == 0.), n
        signs |= {(no.KINDS[k], bool(np.signbit(g)), bool(np.signbit(w))) for k, g, w in zip(rows, got, want)}
    print('signed zeros | (kind, sign bit of the statement, sign bit of numpy):', sorted(signs))
