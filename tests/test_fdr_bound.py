"""The FDR scan runs every wave to ONE trip count (csrc/mbx_rlepso.hpp: fdr_exact's `bound`, computed by fdr_pass): a numpy model of the scan, CPU only.

A work item (particle of pbest-rank rk, W adjacent coordinates) needs the candidates at scan positions 1 .. nless(rk) - 1, the particles strictly better than
its own; the kernels let it run on to its wave's bound -- the highest rank among the wave's items -- because the loop counter then lives on the scalar unit.
The claim (comment block of fdr_exact): the extra candidates, positions nless .. bound - 1, all have a cost >= the item's, so they
  * are never taken: the exemplar (ab, bb, kb) is what the item's own range gives;
  * leave the near-tie flag as it was: each contributes |dif| >= |a_0| 1e-10 / range, a factor 1e-10 x 2^49 / range^2 = 562.9 = 2^9.1 (range = 10 + 1e-5) above the
    flag's threshold |a_0| range 2^-49; an item with nless == 0 (threshold 0) has its flag forced to false.
The model restates the scan operation by operation in float64 -- the fused multiply-add from an error-free product (Veltkamp / Dekker), the running minimum on the
high dwords read as float32 like the kernel's v_min3_f32 -- with the kernels' item-to-wave mapping (boustrophedon passes of THREADS items, 64 per wave), and is
run on (a) pbest tables from short oracle rollouts of the 24 bbob functions and (b) crafted swarms (CRAFTED below; tests/test_gpu_fdr_bound.py puts the same swarms
through the kernels).  Asserted for every item: the bound covers the item's own range and stays below NP, no extra candidate is taken, the flag is the same, and the
smallest |dif| of an extra candidate is >= 2^8 thresholds (the bound of the argument is 2^9.1; the observed minimum is printed, and recorded in
docs/EXPERIMENTS.md).
"""
import numpy as np
import pytest

from helpers import problems
from oracle import oracle

LB, UB = -5., 5.
RANGE = UB - LB + 1e-5                                        # what the kernels pass to fdr_pass
NP, D, NLOG, MAXFES, LOGI = 100, 10, 50, 20000, 400


# ------------------------------------------------------------------------------------------------ the kernels' geometry
def wave_bounds(NP_, D_, W, threads):
    """bound[rk, c] of item ps = rk * (D / W) + c, by fdr_pass's own scalar formula: pass p holds items [base, lim), forwards when p is even (thread t: base + t),
    backwards when odd (lim - 1 - t); wave w0 / 64 of the pass scans to the rank of its highest item."""
    DW = D_ // W
    NI = NP_ * DW
    bound = np.full(NI, -1)
    wave_of = np.empty(NI, int)
    for p, base in enumerate(range(0, NI, threads)):
        lim = min(base + threads, NI)
        for tid in range(threads):
            ps = lim - 1 - tid if p & 1 else base + tid
            if not base <= ps < lim:
                continue
            w0 = tid & ~63
            top = lim - 1 - w0 if p & 1 else min(base + w0 + 63, lim - 1)
            bound[ps] = top // DW
            wave_of[ps] = p * (threads // 64) + w0 // 64
    return bound.reshape(NP_, DW), wave_of.reshape(NP_, DW)


@pytest.mark.parametrize('np_,dim,w,threads', [(100, 10, 2, 256), (128, 40, 2, 1024), (100, 30, 2, 512), (100, 12, 2, 256), (100, 40, 2, 1024),
                                               (77, 7, 1, 256), (5, 2, 2, 256), (4, 3, 1, 256), (256, 64, 2, 256), (130, 6, 2, 256)])
def test_the_wave_bound_is_the_highest_rank_of_the_wave_and_below_np(np_, dim, w, threads):
    bound, wave = wave_bounds(np_, dim, w, threads)
    rk = np.arange(np_)[:, None].repeat(dim // w, 1)
    assert (bound >= rk).all() and bound.max() == np_ - 1            # nless(rank) <= rank <= bound <= NP - 1: no position at or beyond NP is read
    for wv in np.unique(wave):
        m = wave == wv
        assert m.sum() <= 64 and (bound[m] == rk[m].max()).all()


# ------------------------------------------------------------------------------------------------ the scan
def _split(a):
    c = 134217729. * a
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """a b + c with one rounding, up to the last bit of a double rounding in s + (t + l): error-free product, error-free sum."""
    h = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    l = ((ah * bh - h) + ah * bl + al * bh) + al * bl
    s = h + c
    z = s - h
    t = (h - (s - z)) + (c - z)
    return s + (t + l)


def hi_f32(v):
    """f64_hi_as_f32: the high dword of a float64 read as a float32."""
    return (np.ascontiguousarray(v, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def rank_tables(f, P):
    """NC, NCS, PB in (cost, index) order, nless per rank (what the kernels stage before the scan, rl_mark_copies included)."""
    order = np.lexsort((np.arange(len(f)), f))
    NC, PB = f[order], P[order]
    nless = np.searchsorted(NC, NC, 'left')
    NCS = NC.copy()
    copy = np.zeros(len(f), bool)
    copy[1:] = (NC[1:] == NC[:-1]) & (PB[1:] == PB[:-1]).all(1)
    NCS[copy] = 1e300
    return order, NC, NCS, PB, nless


def scan_model(f, P, threads=256, W=None):
    """fdr_exact<W, .., TIE = true> for every item, to the wave's bound.  -> dict: kb_own / kb_bound [NP, D] exemplar ranks from the item's own range and from the
    bound's, flag_own / flag_bound [NP, D / W], taken_extra (an extra candidate won a comparison), margin (smallest |dif| of an extra candidate of an item with
    nless > 0, in thresholds of that item; inf when there is no such candidate), extras (their number)."""
    NP_, D_ = P.shape
    W = W or (2 if D_ % 2 == 0 else 1)
    order, NC, NCS, PB, nless = rank_tables(f, P)
    bound, _ = wave_bounds(NP_, D_, W, threads)
    bound = np.repeat(bound, W, axis=1)                            # per coordinate
    nl = nless[:, None].repeat(D_, 1)
    with np.errstate(over='ignore', invalid='ignore'):
        a0 = (NC[0] - NC)[:, None].repeat(D_, 1)
        ab = a0.copy()
        bb = np.abs(PB[0][None, :] - PB) + 1e-5
        kb = np.zeros((NP_, D_), int)
        kb_own = kb.copy()
        tie_own = np.full((NP_, D_), np.float32(np.uint32(0x7f000000).view(np.float32)))
        tie_all = tie_own.copy()
        taken_extra = np.zeros((NP_, D_), bool)
        extra_min = np.full((NP_, D_), np.inf)
        extras = 0
        for k in range(1, int(bound.max())):
            act = k < bound
            own = k < nl
            au = (NCS[k] - NC)[:, None]
            b = np.abs(PB[k][None, :] - PB) + 1e-5
            dif = fma(au, bb, -(ab * b))
            take = act & (0. > dif)
            taken_extra |= take & ~own
            ab = np.where(take, au, ab); bb = np.where(take, b, bb); kb = np.where(take, k, kb)
            kb_own = np.where(take & own, k, kb_own)
            h = np.abs(hi_f32(dif).reshape(NP_, D_))
            tie_own = np.where(own, np.fmin(tie_own, h), tie_own)
            tie_all = np.where(act, np.fmin(tie_all, h), tie_all)
            ext = act & ~own & (nl > 0)
            extras += int(ext.sum())
            extra_min = np.where(ext, np.minimum(extra_min, np.abs(dif)), extra_min)
        thr = np.abs(a0) * RANGE * 2. ** -49
        thr32 = hi_f32(thr).reshape(NP_, D_) * np.float32(1.0000005)
        # the W coordinates of an item share one running minimum and one flag
        grp = lambda x, fn: fn(x.reshape(NP_, D_ // W, W), axis=2)
        flag_own = (nless[:, None] > 0) & ~(grp(tie_own, np.min) > grp(thr32, np.max))
        flag_bound = (nless[:, None] > 0) & ~(grp(tie_all, np.min) > grp(thr32, np.max))
        margin = np.min(np.where(nl > 0, extra_min / np.where(thr > 0, thr, 1.), np.inf))
    return {'kb_own': kb_own, 'kb_bound': kb, 'flag_own': flag_own, 'flag_bound': flag_bound, 'taken_extra': taken_extra, 'margin': float(margin),
            'extras': extras, 'nless': nless, 'order': order}


def check_swarm(f, P, threads=256, tag=''):
    r = scan_model(f, P, threads)
    assert not r['taken_extra'].any(), (tag, 'a candidate at or beyond nless was taken', np.argwhere(r['taken_extra'])[:4])
    assert np.array_equal(r['kb_own'], r['kb_bound']), tag
    assert (r['kb_bound'][r['nless'] == 0] == 0).all(), tag         # nobody strictly better: rank 0, the first of the cost-ties
    assert np.array_equal(r['flag_own'], r['flag_bound']), (tag, 'the near-tie flag changed', np.argwhere(r['flag_own'] != r['flag_bound'])[:4])
    return r


# ------------------------------------------------------------------------------------------------ (b) crafted swarms
def _positions(rs, NP_, D_):
    return rs.uniform(LB, UB, (NP_, D_))


def swarm_all_equal(rs, NP_=NP, D_=D):
    return np.full(NP_, 1000.), _positions(rs, NP_, D_)


def swarm_increasing(rs, NP_=NP, D_=D):
    return 1000. + np.cumsum(rs.uniform(0.1, 3., NP_)), _positions(rs, NP_, D_)        # rank = index: nless(rank) = rank, the bound's worst case


def swarm_two_levels(rs, NP_=NP, D_=D):
    """A third of the swarm ties for the best cost (nless == 0), the rest shares one worse cost: waves hold lanes of both kinds."""
    f = np.where(rs.permutation(NP_) < NP_ // 3, 990., 1000.)
    return f, _positions(rs, NP_, D_)


def swarm_best_duplicated(rs, NP_=NP, D_=D):
    """The best row four times (same cost, same position: rl_mark_copies takes three out of the scan), a few more whole-row copies further up."""
    f = 1000. + rs.uniform(0., 50., NP_)
    P = _positions(rs, NP_, D_)
    idx = rs.choice(NP_, min(10, NP_), replace=False)
    best = idx[0]
    f[best] = 900.
    for j in idx[1:4]:
        f[j], P[j] = f[best], P[best]
    for a, b_ in zip(idx[4::2], idx[5::2]):
        f[b_], P[b_] = f[a], P[a]
    return f, P


def swarm_zero_distance(rs, NP_=NP, D_=D):
    """The argument's worst case, in every coordinate of the items of a `query` row: the best row sits at the far end of the box (b_0 = range), a row barely
    better than the query -- by 1.03e-6 |a_0|, just enough to beat the best one's quotient -- sits 1e-7 from the query's position (bb = 1.01e-5; not AT it, so
    that the velocity it induces tells it from the rows below) and becomes the running best, and rows barely WORSE than the query sit AT the query's position
    (b = 1e-5): the extra candidates with the smallest |dif| the box allows."""
    f = 1000. + rs.uniform(10., 50., NP_)
    P = rs.uniform(-1., 1., (NP_, D_))
    best, near, query = rs.choice(NP_, 3, replace=False)
    worse = [i for i in rs.permutation(NP_) if i not in (best, near, query)][:max(1, min(6, NP_ - 3))]
    f[best] = 0.
    f[query] = 1000.
    f[near] = 1000. - 1000. * 1.03e-6
    P[query] = UB
    P[near] = UB - 1e-7
    P[best] = LB
    for n, j in enumerate(worse):                              # costs right above the query's, the first of them EQUAL to it (au = 0)
        f[j] = 1000. + n * 1e-9
        P[j] = UB
    return f, P


def swarm_wide_costs(rs, NP_=NP, D_=D):
    """Cost gaps over more than 2^40: 1e-6 .. 1e7, a_0 dwarfs most differences."""
    f = 1e-6 * 2. ** (43. * rs.permutation(NP_) / max(NP_ - 1, 1))
    return f, _positions(rs, NP_, D_)


def swarm_ties_beside_long_scans(rs, NP_=NP, D_=D):
    """A fifth of the swarm ties for the best cost and the rest is strictly ordered: the waves that hold the last of the ties (nless == 0) also hold ranks with
    nless = NP / 5 and more; a few whole-row copies among both (rl_mark_copies)."""
    n0 = max(2, NP_ // 5)
    f = np.concatenate([np.full(n0, 500.), 1000. + np.cumsum(rs.uniform(0.1, 3., NP_ - n0))])[rs.permutation(NP_)]
    P = _positions(rs, NP_, D_)
    tied = np.flatnonzero(f == 500.)
    P[tied[1]] = P[tied[0]]
    rest = np.flatnonzero(f != 500.)
    if len(rest) >= 4:
        a, b_, c, d_ = rs.choice(rest, 4, replace=False)
        f[b_], P[b_] = f[a], P[a]
        f[d_], P[d_] = f[c], P[c]
    return f, P


CRAFTED = [swarm_all_equal, swarm_increasing, swarm_two_levels, swarm_best_duplicated, swarm_zero_distance, swarm_wide_costs, swarm_ties_beside_long_scans]


def crafted_swarms(NP_=NP, D_=D, per_kind=3, seed=0):
    rs = np.random.RandomState(seed + 1000 * NP_ + D_)
    return [(mk.__name__, *mk(rs, NP_, D_)) for mk in CRAFTED for _ in range(per_kind)]


# ------------------------------------------------------------------------------------------------ (a) natural swarms
@pytest.fixture(scope='module')
def natural_swarms():
    """pbest tables of the C oracle: the 24 bbob functions x 2 seeds, generations 2 / 5 / 9 / 14 / 20 / 30 of an episode under random actions (288 tables)."""
    cfg = oracle.make_cfg(1, NP, D, MAXFES, LOGI, NLOG)
    rs = np.random.RandomState(5)
    out = []
    for fid in range(1, 25):
        p = problems('bbob', D)[fid]
        for seed in (3, 4):
            o = oracle.RlepsoOracle(p.desc(), p.bias, cfg, seed=100 * fid + seed)
            o.reset()
            for g in range(1, 31):
                o.step(rs.uniform(0., 1., 35).astype(np.float32))
                if g in (2, 5, 9, 14, 20, 30):
                    sp = oracle.split_rlepso_state(o.state(), NP, D, NLOG)
                    out.append((f'F{fid} seed {seed} generation {g}', sp['pbest'].copy(), sp['pbpos'].reshape(NP, D).copy()))
    return out


def test_fma_model_is_a_fused_multiply_add():
    """Against exact rational arithmetic on operands shaped like the scan's (products that nearly cancel included): at most the last bit differs."""
    from fractions import Fraction
    rs = np.random.RandomState(1)
    a = rs.uniform(-50., 50., 400); b = rs.uniform(1e-5, 10., 400)
    c = -(a * b) * np.where(rs.uniform(size=400) < 0.5, 1., 1. + rs.uniform(-1e-9, 1e-9, 400))
    got = fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        assert abs(Fraction(float(g)) - exact) <= abs(exact) * Fraction(1, 2 ** 52), (x, y, z, g)
        assert (g > 0) == (exact > 0) and (g < 0) == (exact < 0)


def test_scanning_to_the_wave_bound_changes_nothing_on_natural_swarms(natural_swarms):
    assert len(natural_swarms) >= 200
    margin, extras = np.inf, 0
    for tag, f, P in natural_swarms:
        r = check_swarm(f, P, 256, tag)
        margin, extras = min(margin, r['margin']), extras + r['extras']
    print(f'{len(natural_swarms)} natural pbest tables, {extras} extra candidates: smallest |dif| = 2^{np.log2(margin):.1f} thresholds')
    assert extras > 100_000 and margin >= 2. ** 8


@pytest.mark.parametrize('np_,dim,threads', [(100, 10, 256), (128, 40, 1024), (77, 7, 256), (5, 2, 256)])
def test_scanning_to_the_wave_bound_changes_nothing_on_crafted_swarms(np_, dim, threads):
    worst = {}
    for name, f, P in crafted_swarms(np_, dim):
        assert (np.abs(P) <= UB).all()
        r = check_swarm(f, P, threads, name)
        worst[name] = min(worst.get(name, np.inf), r['margin'])
        # the model is the reference's rule: where it raises no flag its exemplar is np.argmin of the rounded quotients (rlepso_optimizer.py:98-102)
        fdr = (f[None, :] - f[:, None])[:, :, None] / (np.abs(P[None, :, :] - P[:, None, :]) + 1e-5)
        unflagged = ~np.repeat(r['flag_bound'], dim // r['flag_bound'].shape[1], axis=1)
        assert (r['order'][r['kb_bound']] == np.argmin(fdr, axis=1)[r['order']])[unflagged].all(), name
    print(f'NP {np_} / D {dim}: smallest |dif| of an extra candidate, in thresholds: ' + ', '.join(f'{k[6:]} 2^{np.log2(v):.1f}' for k, v in worst.items()))
    assert min(worst.values()) >= 2. ** 8, worst
    if np_ >= 77:
        # the crafted worst case really is the argument's: within a few per cent of 1e-10 x 2^49 / range^2 = 562.9 thresholds
        assert worst['swarm_zero_distance'] <= 1.05 * 1e-10 * 2. ** 49 / RANGE ** 2, worst
