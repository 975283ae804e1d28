"""GPU: the numpy-order sums and the order primitives the step kernels share, each run by itself through mbx_debug_reduce -- the shipped routines of
csrc/mbx_npsum.hpp (np_sum_block, np_sum, np_sum_lanes8), mbx_depop.hpp (md_pairwise, md_sort), mbx_jde21.hpp (jd_dist4) and mbx_device.hpp (block_argmin), not
copies -- against numpy itself: np.add.reduce bit for bit at every length the routine is declared for, np.argmin, np.lexsort.  The vectors are those of
tests/numpy_order.py; tests/test_numpy_order.py shows on the CPU that they tell numpy's order from the wrong ones, and that the installed numpy follows the rule.
Last, QLPSO's diversity word after reset() and after NP + 3 steps at the swarm sizes where np_sum halves twice (249, 255), bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import numpy_order as no
import parity

pytestmark = pytest.mark.gpu

NP_SUM_BLOCK, NP_SUM, MD_PAIRWISE, NP_SUM_LANES8, NP_SUM_LANES8_GROUPS, JD_DIST4, BLOCK_ARGMIN, MD_SORT = range(8)
MBX_E_ARG = -1


def _call(op, cases, out):
    """cases: 1-D float64 arrays; out: a CUDA tensor the op fills.  -> the return code."""
    from metabox_amd import _abi
    lib = _abi.load_lib()
    off = np.concatenate([[0], np.cumsum([len(c) for c in cases])]).astype(np.int32)
    x = np.concatenate([np.asarray(c, dtype=np.float64) for c in cases] + [np.zeros(1)])       # (never an empty buffer)
    xd, od = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    rc = lib.mbx_debug_reduce(op, C.c_void_p(xd.data_ptr()), C.c_void_p(od.data_ptr()), len(cases), C.c_void_p(out.data_ptr()),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _reduce(op, cases, per_case):
    from metabox_amd import _abi
    out = torch.full((len(cases), per_case), float('nan'), dtype=torch.float64, device='cuda')
    _abi.check(_call(op, cases, out))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _want(n):
    """np.add.reduce of every vector of length n."""
    M = no.vectors(n)
    w = np.array([np.add.reduce(M[k]) for k in range(len(M))])
    w.setflags(write=False)
    return w


def _check_sums(what, lengths, got_of_length):
    """got_of_length(n): [n_vectors, ...] -- every trailing entry must be numpy's sum of that vector (bits; == for the rows of zeros)."""
    rows, zeros = no.bitwise_rows(), no.zero_rows()
    for n in lengths:
        got, want = got_of_length(n), _want(n)
        got = got.reshape(len(want), -1)
        bad = ~no.same_bits(got[rows], np.broadcast_to(want[rows, None], got[rows].shape))
        assert not bad.any(), f'{what}: first failing length {n}, vectors {sorted(set(rows[np.nonzero(bad)[0]].tolist()))} ' \
                              f'({[no.KINDS[k] for k in sorted(set(rows[np.nonzero(bad)[0]].tolist()))]}): got {got[rows][bad][:3]}, numpy {want[rows][np.nonzero(bad)[0]][:3]}'
        assert np.all(got[zeros] == want[zeros, None]), f'{what}: zeros, first failing length {n}: {got[zeros]}'


@pytest.mark.parametrize('op,name,lengths', [(NP_SUM_BLOCK, 'np_sum_block', tuple(range(0, 129))), (NP_SUM, 'np_sum', tuple(range(0, 257))),
                                              (MD_PAIRWISE, 'md_pairwise', None)], ids=['np_sum_block', 'np_sum', 'md_pairwise'])
def test_single_thread_sums_are_np_add_reduce_bit_for_bit(op, name, lengths):
    lengths = no.lengths_to_3200() if lengths is None else lengths
    K = len(no.KINDS)
    got = _reduce(op, [no.vectors(n)[k] for n in lengths for k in range(K)], 1).reshape(len(lengths), K)
    at = {n: i for i, n in enumerate(lengths)}
    _check_sums(name, lengths, lambda n: got[at[n]])
    signs = sorted({(no.KINDS[k], bool(np.signbit(got[at[n], k])), bool(np.signbit(_want(n)[k]))) for n in lengths for k in no.zero_rows()})
    print(f'{name}: {len(lengths)} lengths x {K} vectors; zeros (kind, sign bit on the device, sign bit of numpy): {signs}')


def test_np_sum_lanes8_every_lane_holds_numpy_bits():
    """One wave per case, every lane calls: all 64 lanes hold np.add.reduce's bits, at every length 0 .. 128."""
    lengths, K = range(0, 129), len(no.KINDS)
    got = _reduce(NP_SUM_LANES8, [no.vectors(n)[k] for n in lengths for k in range(K)], 64).reshape(len(lengths), K, 64)
    _check_sums('np_sum_lanes8', lengths, lambda n: got[n])


def test_np_sum_lanes8_groups_of_eight_do_not_leak():
    """The header says every group of eight lanes computes for itself: a wave whose eight groups hold eight DIFFERENT vectors (of one length, as the callers' lengths
    are wave-uniform) gives each group numpy's sum of its own vector.  Waves of 8 consecutive vectors, the last wave of a length left partly empty."""
    lengths, K = range(0, 129), len(no.KINDS)
    per = -(-K // 8) * 8                                             # cases per length, padded to whole waves with empty cases
    cases = []
    for n in lengths:
        cases += [no.vectors(n)[k] for k in range(K)] + [np.zeros(0)] * (per - K)
    got = _reduce(NP_SUM_LANES8_GROUPS, cases, 8).reshape(len(lengths), per, 8)
    _check_sums('np_sum_lanes8, eight vectors per wave', lengths, lambda n: got[n, :K])
    assert np.all(got[:, K:] == 0.)                                  # an empty case sums to 0.


def test_jd_dist4_is_numpy_sum_of_squares():
    """The four squared distances of a 2 x 2 tile, D = 2 .. 64, each np.sum((p - u) ** 2) bit for bit; rows that agree in some or all coordinates put exact zeros
    into the sums."""
    rs = np.random.RandomState(5)
    cases, want = [], []
    for D in range(2, 65):
        for rep in range(6):
            pa, pb, ua, ub = (rs.standard_normal(D) * np.exp(rs.uniform(-3, 3, D)) for _ in range(4))
            if rep == 1:                                             # every other coordinate of ua is pa's, a third of ub's are pb's
                ua[::2] = pa[::2]; ub[::3] = pb[::3]
            if rep == 2:                                             # equal rows: two sums are 0.
                ua, ub = pa.copy(), pb.copy()
            if rep == 3:                                             # box-like values, as the kernel sees them
                pa, pb, ua, ub = (rs.uniform(-5, 5, D) for _ in range(4))
            cases.append(np.concatenate([pa, pb, ua, ub]))
            want.append([np.sum((p - u) ** 2) for u in (ua, ub) for p in (pa, pb)])
    got, want = _reduce(JD_DIST4, cases, 4), np.array(want)
    bad = np.nonzero(~(no.same_bits(got, want) | ((want == 0.) & (got == 0.))))
    assert not len(bad[0]), f'jd_dist4: first failing D {2 + bad[0][0] // 6}, case {bad[0][0] % 6}, sum {bad[1][0]}: {got[bad][:3]} != {want[bad][:3]}'
    assert (want == 0.).sum() >= 2 * 63


# ------------------------------------------------------------------------------------------------ block_argmin
ARGMIN_LENGTHS = (1, 2, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


def _documented_argmin(a):
    """block_argmin's comment: a NaN never enters (x < m is false for it); the first index of the minimum of the other entries; 0 when nothing is below +inf."""
    live = ~np.isnan(a) & (a < np.inf)
    return int(np.nonzero(live & (a == a[live].min()))[0][0]) if live.any() else 0


def _argmin_cases(n, rs):
    """(what, vector, has NaN)"""
    out = [(f'random {k}', rs.standard_normal(n) * np.exp(rs.uniform(-4, 4, n)), False) for k in range(3)]
    base = rs.uniform(1, 2, n)
    if n > 65:                                                       # lane l folds entries l, l + 64, ...: the minimum at l + 64 AND at l + 1, for a few l
        for lane in sorted({0, (n - 66) // 2, n - 66}):
            a = base.copy(); a[lane + 64] = a[lane + 1] = 0.5
            out.append((f'minimum at {lane + 64} and {lane + 1}', a, False))
    a = base.copy(); a[0] = a[n - 1] = 0.5
    out.append(('minimum at 0 and n - 1', a, False))
    out.append(('every entry equal', np.full(n, 0.75), False))
    out.append(('every entry +inf', np.full(n, np.inf), False))
    a = base.copy(); a[n - 1] = 0.5
    out.append(('minimum in the last (partial) 64-entry step', a, False))
    if n >= 2:
        for first, second in ((0.0, -0.0), (-0.0, 0.0)):
            i, j = sorted(rs.choice(n, 2, replace=False))
            a = base.copy(); a[i], a[j] = first, second
            out.append((f'{first} at {i} and {second} at {j} tie', a, False))
        for k in range(2):
            a = rs.standard_normal(n); a[rs.choice(n, max(n // 3, 1), replace=False)] = np.nan
            if k:
                a[0] = np.nan
            out.append((f'NaNs {k}', a, True))
        a = np.full(n, np.inf); a[::2] = np.nan
        out.append(('only NaN and +inf', a, True))
    out.append(('every entry NaN', np.full(n, np.nan), True))
    return out


def test_block_argmin_is_np_argmin():
    """The first index of the minimum, np.argmin's, and the value a[index] itself (its bits: -0.0 stays -0.0), with the minimum duplicated across the lanes' strides
    (l + 64 before l + 1), at both ends, everywhere, +-0.0 tied, all +inf (documented answer: 0) and in the last partial step of 64.
    With a NaN present block_argmin is NOT np.argmin, which answers the first NaN's index: by its comment a NaN never enters the comparison, so the answer is the
    first index of the minimum of the non-NaN entries, and 0 if no entry is below +inf.  That documented behaviour is what is asserted for the NaN cases."""
    rs = np.random.RandomState(11)
    what, cases = [], []
    for n in ARGMIN_LENGTHS:
        for w, a, has_nan in _argmin_cases(n, rs):
            what.append((n, w, has_nan)); cases.append(a)
    got = _reduce(BLOCK_ARGMIN, cases, 2)
    for (n, w, has_nan), a, (v, i) in zip(what, cases, got):
        want = _documented_argmin(a)
        if not has_nan:
            assert want == int(np.argmin(a)), (n, w)
        assert i == want, f'block_argmin n = {n}, {w}: index {i}, expected {want}'
        assert no.same_bits(v, a[want]) or (np.isnan(v) and np.isnan(a[want])), f'block_argmin n = {n}, {w}: value {v} is not a[{want}] = {a[want]}'


# ------------------------------------------------------------------------------------------------ md_sort
SORT_LENGTHS = (4, 5, 64, 255, 256, 257, 920, 2049, 3200)


def _pad(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def _sort_cases(n, rs):
    inf = rs.standard_normal(n); inf[rs.choice(n, max(n // 5, 2), replace=False)] = np.inf
    zeros = rs.choice([-0.0, 0.0, -1.0, 1.0], n)
    nans = rs.standard_normal(n); nans[rs.choice(n, min(max(n // 50, 2), n - 1), replace=False)] = np.nan
    nans_ties = rs.choice([0.25, np.inf, np.nan], n, p=[0.6, 0.2, 0.2])
    return [('random', rs.standard_normal(n)), ('three values', rs.choice([0.5, -1.5, 2.0], n)), ('all equal', np.full(n, 3.0)), ('real +inf keys', inf),
            ('all +inf', np.full(n, np.inf)), ('+-0.0', zeros), ('a few NaNs', nans), ('ties, +inf and NaNs', nans_ties)]


def test_md_sort_is_np_lexsort_by_cost_then_row():
    """The stable (cost, row) order of np.lexsort((rows, keys)), NaN last as np.argsort(kind='stable') places it, over keys padded as md_init_sorted pads them (+inf,
    rows >= n, to a power of two).  Real +inf keys stay in front of the padding, in row order; NaN keys sort behind it, which is why the kernels clamp IDX."""
    rs = np.random.RandomState(13)
    what, cases = [], []
    for n in SORT_LENGTHS:
        for w, keys in _sort_cases(n, rs):
            what.append((n, w)); cases.append(keys)
    from metabox_amd import _abi
    out = torch.full((sum(_pad(len(c)) for c in cases),), -1, dtype=torch.int32, device='cuda')
    _abi.check(_call(MD_SORT, cases, out))
    out, o = out.cpu().numpy(), 0
    for (n, w), keys in zip(what, cases):
        P = _pad(n)
        got = out[o:o + P]; o += P
        padded = np.concatenate([keys, np.full(P - n, np.inf)])
        want = np.lexsort((np.arange(P), padded))
        live = np.lexsort((np.arange(n), keys))
        assert np.array_equal(live, np.argsort(keys, kind='stable')), (n, w)
        assert np.array_equal(np.sort(got), np.arange(P)), f'md_sort n = {n}, {w}: not a permutation'
        bad = np.nonzero(got != want)[0]
        assert not len(bad), f'md_sort n = {n}, {w}: first difference at position {bad[0]}: row {got[bad[0]]}, np.lexsort {want[bad[0]]}'
        assert np.array_equal(got[got < n], live), (n, w)
        if not np.isnan(keys).any():
            assert np.array_equal(got[:n], live), (n, w)             # the padding stays behind every real key, +inf included


def test_debug_reduce_refuses_bad_arguments():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    out = torch.zeros(8192, dtype=torch.float64, device='cuda')
    for op, n in ((NP_SUM_BLOCK, 129), (NP_SUM, 257), (MD_PAIRWISE, 3201), (NP_SUM_LANES8, 129), (NP_SUM_LANES8_GROUPS, 129), (JD_DIST4, 6), (JD_DIST4, 4 * 129),
                  (BLOCK_ARGMIN, 0), (BLOCK_ARGMIN, 1 << 20), (MD_SORT, 0), (MD_SORT, 3201), (-1, 4), (8, 4)):
        assert _call(op, [np.zeros(n)], out) == MBX_E_ARG and b'mbx_debug_reduce' in lib.mbx_last_error(), (op, n)
    assert lib.mbx_debug_reduce(NP_SUM, None, None, 1, C.c_void_p(out.data_ptr()), None) == MBX_E_ARG
    assert _call(NP_SUM, [np.ones(256)], out) == 0 and out[0].item() == 256.


# ------------------------------------------------------------------------------------------------ QLPSO, end to end
def _diversity(pop, mean_of=np.mean):
    return mean_of(np.sqrt(np.sum(np.square(pop - np.mean(pop, 0)), 1)))


@pytest.mark.parametrize('NP,D', [(248, 13), (249, 2), (255, 13), (256, 10)])
def test_qlpso_diversity_word_is_numpy_bit_for_bit(NP, D):
    """MBX_SC_QLPSO_DIVERSITY after a Philox reset() (k_qlpso_reset) and after NP + 3 steps (k_qlpso_step) is the reference's expression evaluated by numpy on the
    population of the same state block, bit for bit, for the nine instances of parity.edge_problems.  At NP = 249 and 255 np_sum halves twice; there the test also
    shows that it can tell: np_sum's former order (numpy_order.one_halving) gives another double for at least one of the nine populations."""
    from metabox_amd.suite import Batch, Suite
    ps = parity.edge_problems(D)
    B, nlog = len(ps), 5
    s = Suite(ps)
    b = Batch(s, parity.ALGO['qlpso'], np.arange(B), parity.seeds_for('qlpso', B), NP, 10 * NP, 2 * NP, nlog)
    actions = parity.actions_for('qlpso', NP + 3, B, NP)

    def check(when):
        told = 0
        for k in range(B):
            v = parity.split('qlpso', b.read_state(k), NP, D, nlog)
            pop = v['pop'].reshape(NP, D)
            got, want = v['sc']['diversity'], _diversity(pop)
            assert no.same_bits(got, want), f'QLPSO NP {NP} D {D} instance {k} {when}: diversity {got!r}, numpy {want!r} ({(got - want) / np.spacing(want):+.0f} ulp)'
            told += not no.same_bits(_diversity(pop, lambda d: no.one_halving(d[None])[0] / len(d)), want)
        print(f'QLPSO NP {NP} D {D} {when}: nine diversity words equal numpy; one halving step would differ on {told} of {B}')
        if NP in (249, 255):
            assert told >= 1, (NP, D, when)
    b.reset()
    check('after reset()')
    for g in range(NP + 3):
        b.step(torch.from_numpy(np.ascontiguousarray(actions[g])).cuda())
    check(f'after {NP + 3} steps')
    b.close(); s.close()
