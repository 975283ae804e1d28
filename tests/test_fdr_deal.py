"""The deal of the FDR pass (csrc/mbx_rlepso.hpp: fdr_deal_item / fdr_deal_top, MBX_FDR_DEAL = 1), restated in numpy.  CPU only.

P = ceil(NI / THREADS) passes hold P THREADS slots, off = P THREADS - NI more than there are items.  In pass p thread tid sits at slot
s = p THREADS + (p odd ? THREADS - 1 - tid : tid) and owns item s - off; a slot whose item is negative is idle.  The 64-item chunks are therefore cut from the top of
the table and the partial chunk is the lowest one.  A wave scans to the rank of its highest item (one scalar: forward p THREADS + w0 + 63 - off, backward
p THREADS + THREADS - 1 - w0 - off); a wave whose highest item is negative has no item at all and skips the scan.

Where NI is a multiple of 64 every chunk is whole, both deals cut the same chunks, and the kernel keeps the parent's deal (config 5 measured slower with its idle waves
in pass 0); the restatement follows it.

Asserted per geometry: every item is dealt exactly once and nothing outside 0 .. NI - 1 is; the wave's scalar is the highest rank among its items and below NP; the
all-idle waves are exactly those with a negative scalar; the sum of the waves' bounds is never above the parent's (tests/test_fdr_bound.py: wave_bounds restates the
parent's deal) and the chunk maxima are the parent's where NI is a multiple of 64.  The scan model of tests/test_fdr_bound.py, fed the new bounds, takes no extra
candidate and changes no flag on the crafted swarms, and gives the exemplars and flags it gives with the parent's bounds.
"""
import numpy as np
import pytest

import test_fdr_bound as fb

GEOMETRIES = [(100, 10, 2, 256), (100, 12, 2, 256), (100, 30, 2, 512), (128, 40, 2, 1024), (77, 7, 1, 256), (5, 2, 2, 256), (4, 2, 2, 256)]


def deal(NP_, D_, W, threads):
    """-> item[P, threads] (< 0: idle slot), top[P, waves] (the wave's scalar: its highest item; dealt from the top, < 0: the wave skips the scan), by the kernel's own
    arithmetic.  Where NI is a multiple of 64 (fdr_deal_from_top is false: no chunk maximum could fall) the kernel keeps the parent's deal, from item 0 with the short
    pass last, and so does this."""
    DW = D_ // W
    NI = NP_ * DW
    P = -(-NI // threads)
    tid = np.arange(threads)
    w0 = np.arange(0, threads, 64)
    if NI % 64 != 0:
        off = P * threads - NI
        item = np.stack([p * threads + (threads - 1 - tid if p & 1 else tid) - off for p in range(P)])
        top = np.stack([p * threads + (threads - 1 - w0 if p & 1 else w0 + 63) - off for p in range(P)])
        return item, top
    item, top = [], []
    for p in range(P):
        base, lim = p * threads, min(p * threads + threads, NI)
        ps = lim - 1 - tid if p & 1 else base + tid
        item.append(np.where((ps >= base) & (ps < lim), ps, -1))
        top.append(lim - 1 - w0 if p & 1 else np.minimum(base + w0 + 63, lim - 1))
    return np.stack(item), np.stack(top)


def new_wave_bounds(NP_, D_, W, threads):
    """The signature of test_fdr_bound.wave_bounds: bound[rk, c] and the wave of item rk * (D / W) + c."""
    DW = D_ // W
    item, top = deal(NP_, D_, W, threads)
    bound = np.full(NP_ * DW, -1)
    wave_of = np.full(NP_ * DW, -1)
    for p in range(item.shape[0]):
        for t in range(threads):
            if item[p, t] >= 0:
                assert bound[item[p, t]] == -1
                bound[item[p, t]] = top[p, t // 64] // DW
                wave_of[item[p, t]] = p * (threads // 64) + t // 64
    return bound.reshape(NP_, DW), wave_of.reshape(NP_, DW)


def wave_sums(bound, wave):
    """{wave id: its bound}"""
    return {int(w): int(b) for w, b in zip(wave.ravel(), bound.ravel())}


@pytest.mark.parametrize('np_,dim,w,threads', GEOMETRIES)
def test_every_item_is_dealt_once_and_the_wave_scalar_is_its_highest_rank(np_, dim, w, threads):
    DW = dim // w
    NI = np_ * DW
    item, top = deal(np_, dim, w, threads)
    P = item.shape[0]
    assert P == -(-NI // threads)
    live = item[item >= 0]
    assert np.array_equal(np.sort(live), np.arange(NI))              # each of 0 .. NI - 1 exactly once, nothing beyond NI - 1
    assert (item < 0).sum() == P * threads - NI and item.min() >= -(P * threads - NI)
    from_top = NI % 64 != 0
    if from_top:
        assert (item[1:] >= 0).all() and (np.diff(item[0]) == 1).all()           # idle slots in pass 0 only, at its low end
        assert P == 1 or np.array_equal(item[1], item[1, 0] - np.arange(threads))      # the boustrophedon: pass 1 runs backwards
    skipped = 0
    for p in range(P):
        for wv in range(threads // 64):
            mine = item[p, 64 * wv:64 * wv + 64]
            if (mine < 0).all():
                assert top[p, wv] < 0 or not from_top                # an all-idle wave skips the scan (from the top: its scalar says so) ...
                skipped += 1
                continue
            assert top[p, wv] >= 0 and top[p, wv] == mine.max()      # ... and no other wave does: the scalar is the wave's highest item
            bound = top[p, wv] // DW
            assert bound == (mine[mine >= 0] // DW).max() and bound <= np_ - 1
    assert skipped == (P * threads - NI) // 64
    # the same through the per-item tables the scan model reads
    bound, wave = new_wave_bounds(np_, dim, w, threads)
    rk = np.arange(np_)[:, None].repeat(DW, 1)
    assert (bound >= rk).all() and bound.max() == np_ - 1
    for wv in np.unique(wave):
        m = wave == wv
        assert m.sum() <= 64 and (bound[m] == rk[m].max()).all()


def test_the_headline_bounds_and_the_parents():
    new = wave_sums(*new_wave_bounds(100, 10, 2, 256))
    assert [new[k] for k in sorted(new)] == [10, 23, 35, 48, 99, 87, 74, 61]
    old = wave_sums(*fb.wave_bounds(100, 10, 2, 256))
    assert [old[k] for k in sorted(old)] == [12, 25, 38, 51, 99, 87, 74, 61] and sum(old.values()) == 447 and sum(new.values()) == 437
    # per wave (= per SIMD): chunk w of each pass
    assert [new[w] + new[4 + w] for w in range(4)] == [109, 110, 109, 109] and [old[w] + old[4 + w] for w in range(4)] == [111, 112, 112, 112]


@pytest.mark.parametrize('np_,dim,w,threads', GEOMETRIES)
def test_the_bound_sum_never_grows_and_stays_where_the_items_fill_whole_waves(np_, dim, w, threads):
    new = wave_sums(*new_wave_bounds(np_, dim, w, threads))
    old = wave_sums(*fb.wave_bounds(np_, dim, w, threads))
    print(f'NP {np_} / D {dim} / {threads} threads: sum of the waves\' bounds {sum(old.values())} -> {sum(new.values())}')
    assert sum(new.values()) <= sum(old.values())
    if (np_ * (dim // w)) % 64 == 0:
        assert sorted(new.values()) == sorted(old.values())
    expected = {(100, 10, 2, 256): (447, 437), (100, 12, 2, 256): (573, 513), (100, 30, 2, 512): (1265, 1209), (128, 40, 2, 1024): (2600, 2600),
                (77, 7, 1, 256): (401, 358)}
    if (np_, dim, w, threads) in expected:
        assert (sum(old.values()), sum(new.values())) == expected[np_, dim, w, threads]


@pytest.mark.parametrize('np_,dim,threads', [(100, 10, 256), (128, 40, 1024), (77, 7, 256), (5, 2, 256)])
def test_the_scan_model_with_the_new_bounds_changes_nothing_on_crafted_swarms(monkeypatch, np_, dim, threads):
    swarms = fb.crafted_swarms(np_, dim)
    before = [fb.scan_model(f, P, threads) for _, f, P in swarms]
    monkeypatch.setattr(fb, 'wave_bounds', new_wave_bounds)
    worst = np.inf
    for (name, f, P), old in zip(swarms, before):
        r = fb.check_swarm(f, P, threads, name)                      # no extra candidate taken, no flag changed against the item's own range
        assert np.array_equal(r['kb_bound'], old['kb_bound']) and np.array_equal(r['flag_bound'], old['flag_bound']), name
        worst = min(worst, r['margin'])
    assert worst >= 2. ** 8, worst                                   # the margin test_fdr_bound.py asks of the parent's bounds
