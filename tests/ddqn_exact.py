"""One env step of DE_DDQN_Optimizer (src/optimizer/de_ddqn_optimizer.py :131-220 update, :76-129 __get_state, operators/mutate.py,
boundary_control.py, crossover.py with Cr = 1) restated in plain numpy over a state block in the kernel's layout (include/mbx_layout.h
MBX_DQ_*, oracle.split_dq_state), and how far a correct float64 kernel may be from it.

The functions are written from the reference's Python, not from the kernel or the C oracle.  Everything after the objective evaluation is
a function of the trial cost `tc`, which is an INPUT (the appended OM_W entry holds it): each word of the next block is then a single IEEE
operation or an integer decision, so the block is compared bit for bit.  What the block stores of the reference's Python objects:

  * X_gbest / X_prebest are numpy VIEWS of population row G0 while GBVIEW / PREVIEW is 1 (init_population :58,:61) and arrays of their own
    afterwards (`X_gbest = trial` :198, `X_prebest = X_gbest` :134).  The GBPOS / PREPOS words are read only where the flag is 0; `resolve`
    gives the position either way and `canon` puts it into the words, so blocks of different writers compare.
  * N_tot / N_succ / OM are deques of gen_max = 10 appended on the left: generation g back sits in ring slot (g - gen) mod 10.  The block
    keeps, of every OM list, its running sum in append order (omsum) and its maximum (ommax): `+=` and a compare per step.
  * MEDLO / MEDHI are the kernel's median cache.  By rule they hold, after a step, the order statistics K - 1 and K (K = NP // 2, 0-based)
    of the cost vector BEFORE selection, both statistic K at odd NP; `dq_step` writes them by that rule (np.sort), so they compare bit for
    bit like every other word.  A writer without the cache (the C oracle) is compared with canon(..., med=False).

Features (`dq_features`), u = 2^-53.  tol = 0 means bit equality (NaN matches NaN): features 0, 3, 4, 5, 12-17 and the trend features
51-66 are the reference's own float64 operation sequence on stored words, which has one possible result.  Reductions are summed in
different orders by numpy, the oracle and the kernel's lanes, so they are compared with the longdouble value inside a bound derived as
TWICE the first-order bound below.  A float64 sum of n terms t_i in ANY order is within n u sum|t_i| of the exact sum (first order;
running-error bound of Higham, Accuracy and Stability, 4.2); every further operation adds u |result| and propagates what it is given:

  * mean (feature 1): e_mean = n u sum|c_i| / n + u |mean|;  f1 = (mean - gbest) / range:  (e_mean + u |mean - gbest|) / |range| + u |f1|.
  * std (feature 2): d_i = c_i - mean carries e_i = e_mean + u |d_i|, its square 2 |d_i| e_i + e_i^2 + u d_i^2 (the second-order term e_i^2
    is kept: it is all there is when the costs are equal and the rounded mean is not one of them); the sum of the n squares adds
    n u sum d_i^2; var = ./n adds u var.  sqrt: |sqrt(v') - sqrt(v)| <= min(e_var /
    sqrt(v), sqrt(e_var)) (the second covers v = 0), + u sqrt(v).  range / 2 is exact; the division adds u |f2|.
  * distances (6-11, 18): each (a_d - b_d)^2 is within 3 u of itself, the D-term sum adds D u: s within (D + 3) u s; sqrt halves that and
    adds u; max_dist = sqrt(sum_D (ub - lb)^2) carries the same ((D + 3) / 2 + 1) u; the division adds u: (D + 6) u |f| in all.
  * credit rates (19-34): G <= 10 quotients N_succ / N_tot, each rounded once (u |q|), then a G-term sum: (G + 1) u sum|q|.
  * credit means (35-50): G-term sum of the omsum words, G u sum|omsum|, divided by the exact integer sum of N_tot (+ u |f|) when that is
    positive, left as it is otherwise (:108).
  * credit maxima (67-82): G u sum|ommax| over the slots with N_succ > 0.
  * window sums (83-98): n u sum|t| over the n window entries of the operator.

range == 0 (all costs equal): the exact features are whatever IEEE division gives (numpy: NaN for 0/0, +-inf for x/0) and must match;
features 1 and 2 are only required to be non-finite (tol = inf), because a mean that differs from the costs by a rounding turns 0/0 into
x/0.

`defect=` plants one deliberate error (tests/test_ddqn_exact.py shows that the comparison rejects each); `tags` names the branches a
step took, ALL_TAGS every branch there is.
"""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GENMAX, W, NFEAT, NSCALAR = 10, 50, 99, 16
SITE_DQ_R = 13
X_GWORST, X_CPRE, X_POINTER, X_GEN, X_STAG, X_OMWLEN, X_G0, X_GBVIEW, X_PREVIEW, X_MEDLO, X_MEDHI = range(11)
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE = range(8)

DEFECTS = {
    1: 'median = upper statistic at even NP',
    2: 'median taken after selection',
    3: 'evict the last entry of the same operator, not the first',
    4: 'worst-trial tie resolved to the last maximum',
    5: 'tc < c_p for selection',
    6: 'stagnation on >',
    7: 'ring slot off by one',
    8: 'prebest cost refreshed each sweep',
    9: 'PREVIEW not following row G0',
    10: 'pointer not wrapping',
    11: 'feature 35 divided when sum N_tot = 0',
    12: 'r4 taken from word y of index 0',
    13: 'generation word = steps - 1',
    14: 'seed high word dropped',
}

ALL_TAGS = frozenset(
    ['already_done', 'sweep_start', 'sweep_inside', 'prebest_rebinds_view', 'prebest_rebinds_copy', 'ring_open_fresh', 'ring_open_overwrite',
     'op0', 'op1', 'op2', 'op3', 'best_is_view', 'best_is_own', 'clip_lo', 'clip_hi', 'clip_none', 'med_even', 'med_odd',
     'ommax_first', 'ommax_raise', 'ommax_keep', 'win_grow', 'win_evict_same', 'win_evict_worst', 'win_evict_worst_tied',
     'stag_gt', 'stag_eq', 'stag_no', 'sel_lt', 'sel_eq', 'sel_no', 'best_lt', 'best_eq', 'best_no', 'gbview_breaks', 'preview_follows',
     'gworst_up', 'gworst_keep', 'ptr_wrap', 'ptr_inc', 'log_point', 'no_log', 'done_budget', 'done_target', 'final_overwrite',
     'final_append', 'running'] + [f'om{m}_{s}' for m in range(4) for s in ('pos', 'nonpos')])

GROUPS = {'mean_std': (1, 2), 'distances': (6, 7, 8, 9, 10, 11, 18), 'credit_rates': tuple(range(19, 35)), 'credit_means': tuple(range(35, 51)),
          'credit_maxima': tuple(range(67, 83)), 'window_sums': tuple(range(83, 99))}
EXACT = (0, 3, 4, 5, 12, 13, 14, 15, 16, 17) + tuple(range(51, 67))


@functools.lru_cache(maxsize=None)
def _lay(NP, D, nlog):
    o, out = 0, {}
    for name, n in (('X', NP * D), ('COST', NP), ('GBPOS', D), ('PREPOS', D), ('R', 8), ('NTOT', 40), ('NSUCC', 160), ('OMSUM', 160),
                    ('OMMAX', 160), ('OMW', 300), ('EXTRA', 16), ('SC', NSCALAR), ('CLOG', nlog + 1)):
        out[name] = o
        o += n
    out['n'] = o
    return namedtuple('Lay', out)(**out)


class Cfg(namedtuple('Cfg', 'NP D nlog max_fes log_interval early_stop lb ub has_optimum')):
    """Geometry, budget and box of one instance; `lay`: the offsets of the block's parts (MBX_DQ_ST_*) and its length n."""

    @property
    def lay(self):
        return _lay(self.NP, self.D, self.nlog)


def parts(S, cfg):
    """Writable views of a block's parts."""
    L, NP, D = cfg.lay, cfg.NP, cfg.D
    return {'X': S[L.X:L.X + NP * D].reshape(NP, D), 'cost': S[L.COST:L.COST + NP], 'gbpos': S[L.GBPOS:L.GBPOS + D], 'prepos': S[L.PREPOS:L.PREPOS + D],
            'r': S[L.R:L.R + 8], 'ntot': S[L.NTOT:L.NTOT + 40].reshape(4, GENMAX), 'nsucc': S[L.NSUCC:L.NSUCC + 160].reshape(16, GENMAX),
            'omsum': S[L.OMSUM:L.OMSUM + 160].reshape(16, GENMAX), 'ommax': S[L.OMMAX:L.OMMAX + 160].reshape(16, GENMAX),
            'omw': S[L.OMW:L.OMW + 300].reshape(W, 6), 'ex': S[L.EXTRA:L.EXTRA + 16], 'sc': S[L.SC:L.SC + NSCALAR], 'clog': S[L.CLOG:L.CLOG + cfg.nlog + 1]}


def slot(g, gen):
    """Ring slot of generation g back (deque index g) when `gen` sweeps have started."""
    return (g - gen) % GENMAX


def resolve(S, cfg):
    """(X_gbest, X_prebest) as the reference sees them: row G0 while the view flag is set, the stored array otherwise."""
    P = parts(S, cfg)
    g0 = int(P['ex'][X_G0])
    return (P['X'][g0] if P['ex'][X_GBVIEW] != 0 else P['gbpos']).copy(), (P['X'][g0] if P['ex'][X_PREVIEW] != 0 else P['prepos']).copy()


def canon(S, cfg, med=True):
    """The block with the words that have no meaning normalised: gbest / prebest positions resolved, cost list beyond its length zeroed
    (med=False: the median cache zeroed as well, for a writer that keeps none)."""
    C = np.array(S, dtype=np.float64, copy=True)
    P = parts(C, cfg)
    gb, pre = resolve(S, cfg)
    P['gbpos'][:] = gb
    P['prepos'][:] = pre
    P['clog'][int(P['sc'][SC_COST_LEN]):] = 0.
    P['omw'][int(P['ex'][X_OMWLEN]):] = 0.
    if not med:
        P['ex'][X_MEDLO] = P['ex'][X_MEDHI] = 0.
    return C


def validate(S, cfg, action=0):
    """Every index the step will use lies inside the layout's ranges (checked on the host before a block is handed to a kernel), and the
    invariants the reference cannot leave hold: X_gbest is a view only while c_gbest is the cost of the row it views; len(cost) ==
    log_index <= n_logpoint before termination."""
    P = parts(S, cfg)
    NP = cfg.NP
    assert S.shape == (cfg.lay.n,) and 0 <= int(action) < 4
    assert np.all(np.isfinite(P['X'])) and np.all(np.isfinite(P['cost']))
    r = P['r'][:5]
    assert np.all(r == np.floor(r)) and np.all((r >= 0) & (r < NP)), r
    ex, sc = P['ex'], P['sc']
    for k, hi in ((X_POINTER, NP), (X_G0, NP), (X_OMWLEN, W + 1), (X_GEN, 1 << 20), (X_STAG, 1 << 30), (X_GBVIEW, 2), (X_PREVIEW, 2)):
        assert ex[k] == np.floor(ex[k]) and 0 <= ex[k] < hi, (k, ex[k])
    n = int(ex[X_OMWLEN])
    ops = P['omw'][:n, 0]
    assert np.all(ops == np.floor(ops)) and np.all((ops >= 0) & (ops < 4))
    assert sc[SC_DONE] in (0., 1.) and sc[SC_FES] == np.floor(sc[SC_FES]) and 0 <= sc[SC_FES] < 2 ** 31
    assert sc[SC_LOG_INDEX] == sc[SC_COST_LEN] and 1 <= sc[SC_LOG_INDEX] <= cfg.nlog or sc[SC_DONE] == 1.
    assert 1 <= sc[SC_COST_LEN] <= cfg.nlog + 1
    assert 0 <= sc[SC_GEN] < 2 ** 31 and 0 <= sc[SC_EPISODE] < 2 ** 31
    if ex[X_GBVIEW] != 0:
        assert sc[SC_GBEST] == P['cost'][int(ex[X_G0])]
    for name in ('ntot', 'nsucc'):
        assert np.all(P[name] == np.floor(P[name])) and np.all(P[name] >= 0)


# ================================================================================================ mutation
def _donor(S, action, cfg):
    P = parts(S, cfg)
    X, r, p = P['X'], P['r'][:5].astype(np.int64), int(P['ex'][X_POINTER])
    best = resolve(S, cfg)[0]
    F = 0.5
    if action == 0:
        return X[r[0]] + F * (X[r[1]] - X[r[2]])                                              # rand_1_single
    if action == 1:
        return X[r[0]] + F * (X[r[1]] - X[r[2]] + X[r[3]] - X[r[4]])                          # rand_2_single
    if action == 2:
        return X[r[0]] + F * (best - X[r[0]] + X[r[1]] - X[r[2]] + X[r[3]] - X[r[4]])         # rand_to_best_2_single
    if action == 3:
        return X[p] + F * (X[r[0]] - X[p] + X[r[1]] - X[r[2]])                                # cur_to_rand_1_single
    raise ValueError('Action error')


def dq_trial(S, action, cfg):
    """The trial vector of update(action): donor in float64 in the reference's association, np.clip to the box; Cr = 1 makes binomial()
    return the donor.  F = 0.5 scales exactly, so a contracted multiply-add gives the same double: bit equality is expected."""
    return np.clip(_donor(S, action, cfg), cfg.lb, cfg.ub)


# ================================================================================================ update()
def dq_step(S, action, tc, r_next, cfg, defect=0):
    """update(action) given the trial's cost `tc` and the five indices `r_next` that the following __get_state draws.
    -> (next block, reward, done, tags)."""
    S = np.array(S, dtype=np.float64, copy=True)
    P = parts(S, cfg)
    NP, ex, sc, cost, X = cfg.NP, P['ex'], P['sc'], P['cost'], P['X']
    tags = set()
    if sc[SC_DONE] != 0:
        return S, 0., True, {'already_done'}
    tc = np.float64(tc)
    p, g0, gen = int(ex[X_POINTER]), int(ex[X_G0]), int(ex[X_GEN])
    gbest, cpre = sc[SC_GBEST], ex[X_CPRE]
    if p == 0:                                                                  # :132-142
        tags.add('sweep_start')
        if ex[X_GBVIEW] != 0:
            ex[X_PREVIEW] = 1.
            tags.add('prebest_rebinds_view')
        else:
            ex[X_PREVIEW] = 0.
            P['prepos'][:] = P['gbpos']
            tags.add('prebest_rebinds_copy')
        if defect == 8:
            cpre = ex[X_CPRE] = gbest
        gen += 1
        s = slot(0, gen)
        tags.add('ring_open_fresh' if gen <= GENMAX else 'ring_open_overwrite')
        if defect == 7:
            s = (s + 1) % GENMAX
        for name in ('ntot', 'nsucc', 'omsum', 'ommax'):
            P[name][:, s] = 0.
    else:
        tags.add('sweep_inside')
    tags.add(f'op{action}')
    tags.add('best_is_view' if ex[X_GBVIEW] != 0 else 'best_is_own')
    v = _donor(S, action, cfg)
    trial = np.clip(v, cfg.lb, cfg.ub)
    lo_hit, hi_hit = bool(np.any(v < cfg.lb)), bool(np.any(v > cfg.ub))
    tags.update(t for t, c in (('clip_lo', lo_hit), ('clip_hi', hi_hit), ('clip_none', not (lo_hit or hi_hit))) if c)
    fes = sc[SC_FES] + 1                                                        # :163
    cpv = cost[p]
    reward = max(cpv - tc, 0)                                                   # :165
    s0 = slot(0, gen)
    P['ntot'][action, s0] += 1                                                  # :167
    srt = np.sort(cost)
    K = NP // 2
    med_hi, med_lo = srt[K], (srt[K] if NP & 1 else srt[K - 1])
    tags.add('med_odd' if NP & 1 else 'med_even')
    median = np.median(cost)                                                    # :172, before selection
    assert median == (med_hi if NP & 1 else (med_lo + med_hi) / 2)
    if defect == 1:
        median = med_hi
    if defect == 2:
        c2 = cost.copy()
        if tc <= cpv:
            c2[p] = tc
        median = np.median(c2)
    om = np.array([cpv - tc, cpre - tc, gbest - tc, median - tc])
    for m in range(4):                                                          # :173-176
        k = action * 4 + m
        if om[m] > 0:
            tags.add(f'om{m}_pos')
            if P['nsucc'][k, s0] == 0:
                P['ommax'][k, s0] = om[m]
                tags.add('ommax_first')
            elif om[m] > P['ommax'][k, s0]:
                P['ommax'][k, s0] = om[m]
                tags.add('ommax_raise')
            else:
                tags.add('ommax_keep')
            P['nsucc'][k, s0] += 1
            P['omsum'][k, s0] += om[m]
        else:
            tags.add(f'om{m}_nonpos')
    n = int(ex[X_OMWLEN])                                                       # :178-187
    win = P['omw']
    if n >= W:
        same = np.nonzero(win[:n, 0].astype(np.int64) == action)[0]
        if len(same):
            d = int(same[-1] if defect == 3 else same[0])
            tags.add('win_evict_same')
        else:
            col = win[:n, 5]
            d = int(np.argmax(col))
            tags.add('win_evict_worst')
            if int((col == col.max()).sum()) > 1:
                tags.add('win_evict_worst_tied')
                if defect == 4:
                    d = n - 1 - int(np.argmax(col[::-1]))
        win[d:n - 1] = win[d + 1:n].copy()
        n -= 1
    else:
        tags.add('win_grow')
    win[n] = [action, om[0], om[1], om[2], om[3], tc]
    n += 1
    stag = ex[X_STAG]
    if (tc > gbest) if defect == 6 else (tc >= gbest):                          # :189
        stag += 1
    tags.add('stag_gt' if tc > gbest else ('stag_eq' if tc == gbest else 'stag_no'))
    if (tc < cpv) if defect == 5 else (tc <= cpv):                              # :192-198
        cost[p] = tc
        X[p] = trial
        if ex[X_PREVIEW] != 0 and p == g0:
            tags.add('preview_follows')
        if tc <= gbest:
            tags.add('best_lt' if tc < gbest else 'best_eq')
            gbest = tc
            P['gbpos'][:] = trial
            if ex[X_GBVIEW] != 0:
                tags.add('gbview_breaks')
            ex[X_GBVIEW] = 0.
        else:
            tags.add('best_no')
    tags.add('sel_lt' if tc < cpv else ('sel_eq' if tc == cpv else 'sel_no'))
    gworst = ex[X_GWORST]
    if tc > gworst:                                                             # :200
        gworst = tc
        tags.add('gworst_up')
    else:
        tags.add('gworst_keep')
    pointer = p + 1 if defect == 10 else (p + 1) % NP                           # :202
    tags.add('ptr_wrap' if p + 1 == NP else 'ptr_inc')
    log_index, cost_len = int(sc[SC_LOG_INDEX]), int(sc[SC_COST_LEN])
    if fes >= log_index * cfg.log_interval:                                     # :204-206
        log_index += 1
        P['clog'][cost_len] = gbest
        cost_len += 1
        tags.add('log_point')
    else:
        tags.add('no_log')
    done = bool(fes >= cfg.max_fes)                                             # :208-211
    if done:
        tags.add('done_budget')
    if cfg.has_optimum and cfg.early_stop and gbest <= 1e-8:
        done = True
        tags.add('done_target')
    if done:                                                                    # :215-219
        if cost_len >= cfg.nlog + 1:
            P['clog'][cost_len - 1] = gbest
            tags.add('final_overwrite')
        else:
            P['clog'][cost_len] = gbest
            cost_len += 1
            tags.add('final_append')
    else:
        tags.add('running')
    P['r'][:5] = r_next
    ex[X_GWORST], ex[X_POINTER], ex[X_GEN], ex[X_STAG], ex[X_OMWLEN] = gworst, pointer, gen, stag, n
    ex[X_MEDLO], ex[X_MEDHI] = med_lo, med_hi
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = gbest, fes, log_index, cost_len, 1. if done else 0.
    sc[SC_RETURN] += reward
    sc[SC_GEN] += 1
    return S, float(reward), done, tags


# ================================================================================================ __get_state()
def dq_features(S, cfg, defect=0, stale_prebest=None):
    """__get_state on a block (after update(), or after init_population) -> (feat [99] longdouble, tol [99]); see the module docstring for
    the rules and the derivation of every bound.  tol: 0 = bit equality, inf = only required to be non-finite."""
    P = parts(S, cfg)
    NP, D, ex, sc, cost, X = cfg.NP, cfg.D, P['ex'], P['sc'], P['cost'], P['X']
    f, tol = np.zeros(NFEAT, dtype=LD), np.zeros(NFEAT)
    pointer, gen = int(ex[X_POINTER]), int(ex[X_GEN])
    gbest, gworst, cpre = sc[SC_GBEST], ex[X_GWORST], ex[X_CPRE]
    r = P['r'][:5].astype(np.int64)
    gbpos, prepos = resolve(S, cfg)
    if defect == 9 and stale_prebest is not None:
        prepos = stale_prebest
    with np.errstate(all='ignore'):
        rng = gworst - gbest
        cp = cost[pointer]
        f[0] = (cp - gbest) / rng
        f[3] = (cfg.max_fes - sc[SC_FES]) / cfg.max_fes
        f[4] = 1.
        f[5] = ex[X_STAG] / cfg.max_fes
        for j in range(5):
            f[12 + j] = (cp - cost[r[j]]) / rng
        f[17] = (cp - cpre) / rng
        # mean / std
        c = cost.astype(LD)
        mean = c.sum() / NP
        e_mean = NP * U * np.abs(c).sum() / NP + U * abs(mean)
        f[1] = (mean - LD(gbest)) / LD(rng)
        d = c - mean
        sd2 = (d * d).sum()
        var = sd2 / NP
        e_sq = sum((2 * abs(t) * (e_mean + U * abs(t)) + (e_mean + U * abs(t)) ** 2 + U * t * t for t in d), LD(0))
        e_var = (e_sq + NP * U * sd2) / NP + U * var
        sv = np.sqrt(var)
        e_sv = (min(e_var / sv, np.sqrt(e_var)) if sv > 0 else np.sqrt(e_var)) + U * sv
        half = LD(rng) / 2
        f[2] = sv / half
        if rng == 0 or not np.isfinite(rng):
            tol[1] = tol[2] = np.inf
        else:
            tol[1] = 2 * float((e_mean + U * abs(mean - LD(gbest))) / abs(LD(rng)) + U * abs(f[1]))
            tol[2] = 2 * float(e_sv / abs(half) + U * abs(f[2]))
        # distances
        span = LD(cfg.ub) - LD(cfg.lb)
        max_dist = np.sqrt(D * span * span)
        xp = X[pointer].astype(LD)
        for k, other in [(6 + j, X[r[j]]) for j in range(5)] + [(11, prepos), (18, gbpos)]:
            dd = xp - other.astype(LD)
            f[k] = np.sqrt((dd * dd).sum()) / max_dist
            tol[k] = 2 * (D + 6) * U * float(f[k])
        # operator credit
        G = min(GENMAX, gen)
        sl = [slot(g, gen) for g in range(G)]
        for op in range(4):
            nt = P['ntot'][op, sl]
            sum_nt = nt.sum()
            for m in range(4):
                q = op * 4 + m
                ns, os_, ox = P['nsucc'][q, sl], P['omsum'][q, sl], P['ommax'][q, sl]
                rate = [LD(ns[g]) / LD(nt[g]) for g in range(G) if nt[g] > 0]
                f[19 + q] = sum(rate, LD(0))
                tol[19 + q] = 2 * (G + 1) * U * float(sum((abs(t) for t in rate), LD(0)))
                b, ab = os_.astype(LD).sum(), float(np.abs(os_).astype(LD).sum())
                if sum_nt > 0 or defect == 11:
                    f[35 + q] = b / LD(sum_nt)
                    tol[35 + q] = 2 * (G * U * ab / float(sum_nt) + U * abs(float(f[35 + q]))) if sum_nt > 0 else 0.
                else:
                    f[35 + q] = b
                    tol[35 + q] = 2 * G * U * ab
                live = ns > 0
                f[67 + q] = ox[live].astype(LD).sum()
                tol[67 + q] = 2 * G * U * float(np.abs(ox[live]).astype(LD).sum())
                if gen >= 2:
                    s0, s1 = slot(0, gen), slot(1, gen)
                    dn = P['ntot'][op, s0] - P['ntot'][op, s1]
                    if dn != 0 and P['nsucc'][q, s0] > 0 and P['nsucc'][q, s1] > 0:
                        f[51 + q] = (P['ommax'][q, s0] - P['ommax'][q, s1]) / (P['ommax'][q, s1] * np.abs(dn))
        # OM_W
        n = min(W, int(ex[X_OMWLEN]))
        cnt, mag = np.zeros(16), np.zeros(16, dtype=LD)
        ops, vals = P['omw'][:n, 0].astype(np.int64), P['omw'][:n, 1:5].astype(LD)
        for op in range(4):
            mine = vals[ops == op]
            f[83 + op * 4:87 + op * 4] = mine.sum(0)
            mag[op * 4:op * 4 + 4] = np.abs(mine).sum(0)
            cnt[op * 4:op * 4 + 4] = len(mine)
        tol[83:99] = 2 * cnt * U * mag.astype(np.float64)
    return f, tol


def judge_features(got, f, tol):
    """-> (list of failing feature indices, {group: worst |got - f| / tol}) for a float64 feature vector `got`."""
    got = np.asarray(got, dtype=np.float64)
    bad, worst = [], {}
    for k in range(NFEAT):
        if tol[k] == 0:
            want = np.float64(f[k])
            if not (got[k].tobytes() == want.tobytes() or (np.isnan(got[k]) and np.isnan(want)) or (got[k] == 0 and want == 0 and k not in EXACT)):
                bad.append(k)
        elif np.isinf(tol[k]):
            if np.isfinite(got[k]):
                bad.append(k)
        elif not abs(LD(got[k]) - f[k]) <= tol[k]:
            bad.append(k)
    for name, idx in GROUPS.items():
        rr = [float(abs(LD(got[k]) - f[k]) / tol[k]) for k in idx if 0 < tol[k] < np.inf]
        worst[name] = max(rr, default=0.)
    return bad, worst


# ================================================================================================ draws
def dq_draws(seed, gen_word, episode, NP, defect=0):
    """The five indices __get_state draws (:85) on the Philox route: site MBX_SITE_DQ_R, counter (index, site, generation word, episode), key
    = the 64-bit seed; index 0 words x..w -> r0..r3, index 1 word x -> r4, each (w * NP) >> 32.  The generation word is 0 in reset and the
    number of update() calls (this one included) in a step."""
    from oracle import oracle
    if defect == 13:
        gen_word -= 1
    if defect == 14:
        seed = int(seed) & 0xFFFFFFFF
    w0 = oracle.philox(int(seed), 0, SITE_DQ_R, int(gen_word), int(episode))
    w1 = oracle.philox(int(seed), 1, SITE_DQ_R, int(gen_word), int(episode))
    words = list(w0) + [w0[1] if defect == 12 else w1[0]]
    return np.array([(int(w) * NP) >> 32 for w in words], dtype=np.float64)


def order_stats(cost):
    """(MEDLO, MEDHI) by rule for a cost vector."""
    srt, K = np.sort(cost), len(cost) // 2
    return (srt[K] if len(cost) & 1 else srt[K - 1]), srt[K]
