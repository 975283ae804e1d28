"""MadDE (src/optimizer/madde.py), a classic baseline of the test harness: the batched HIP kernels (metabox_amd/csrc/mbx_madde.hpp) against
seeded reference episodes (tests/golden/madde_traces*.npz, tools/gen_golden.py madde).

MF, MCr and pm are arithmetic in the cost values, and the kernels' objective values agree with numpy's to helpers.RTOL / ATOL, not to the
bit: one rounding of one cost is amplified until a comparison flips, so a free-running kernel leaves the reference trajectory within tens
of updates and no whole episode can be replayed.  The kernel is pinned one update at a time, from the reference's own state, split at
the evaluation:
  (A) state before + tape -> trial rows u: bit for bit against `restate_trials`;
  (B) u -> ncost: helpers.close against the fixture's trial costs;
  (C) state before + tape + ncost -> state after: bit for bit against `restate_finish` fed the DEVICE's ncost;
and the chain to the reference is closed on the CPU: the restatement (numpy, written from the algorithm's rules, kind='stable' sort) fed
the REFERENCE's recorded ncost reproduces every recorded quantity of every update and every snapshot exactly.

The numpy draws are not stored: MaddeTapeFeeder regenerates them from the seed in the reference's draw order (include/mbx_layout.h §13).
Measured figures are in docs/EXPERIMENTS.md."""
import copy
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

from helpers import GOLDEN, close, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'madde_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
CASES = [str(c) for c in TR['cases']]
ALGO_MADDE, TRIES, NLOG = 15, 25, 50
SITE_NOISE1_A, SITE_NOISE1_B = 7, 8
SITE_PAR, SITE_NORM, SITE_CAUCHY, SITE_IDX, SITE_CROSS, SITE_ARC, SITE_NOISE_A, SITE_NOISE_B = 30, 31, 32, 33, 34, 35, 36, 37
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_GEN, SC_EPISODE, SC_NP, SC_ARC, SC_NA, SC_K, SC_LIVE = 0, 1, 2, 3, 4, 6, 7, 10, 11, 12, 13, 14
P_BEST, P_QBX = 0.18, 0.01


# ------------------------------------------------------------------------------------------------ layout (include/mbx_layout.h §13)
def geom(D):
    n0 = 2 * D * D
    return n0, int(2.3 * n0), 10 * D


def tape_off(D):
    n0 = geom(D)[0]
    names = ('mem', 'z', 'c', 'choice', 'rb', 'r1', 'r2', 'rvs', 'qpick', 'jrand', 'noise')
    o = {k: i * n0 for i, k in enumerate(names)}
    o['arc'], o['cross'] = 13 * n0, 14 * n0
    return o


def tape_stride(D):
    n0 = geom(D)[0]
    return 14 * n0 + n0 * D


def state_off(D, nlog=NLOG):
    n0, a0, h = geom(D)
    o, p = {}, 0
    for k, n in (('pop', 2 * n0 * D), ('cost', n0), ('arc', a0 * D), ('MF', h), ('MCr', h), ('u', n0 * D), ('ncost', n0), ('F', n0), ('Cr', n0), ('z', n0), ('c', n0), ('pm', 4),
                 ('scalars', 16), ('log', nlog + 1)):
        o[k] = p
        p += n
    o['end'] = p
    return o


def to_block(st, D, gen=0, nlog=NLOG):
    """The state block of a restated state (dead areas zero, live buffer 0)."""
    n0, a0, h = geom(D)
    o = state_off(D, nlog)
    b = np.zeros(o['end'])
    n, na = len(st['cost']), len(st['arc'])
    b[o['pop']:o['pop'] + n * D] = st['pop'].ravel()
    b[o['cost']:o['cost'] + n] = st['cost']
    b[o['arc']:o['arc'] + na * D] = st['arc'].ravel()
    b[o['MF']:o['MF'] + h], b[o['MCr']:o['MCr'] + h], b[o['pm']:o['pm'] + 3] = st['MF'], st['MCr'], st['pm']
    sc = b[o['scalars']:o['scalars'] + 16]
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = st['gbest'], st['fes'], st['log_index'], len(st['log']), float(st['done'])
    sc[SC_GEN], sc[SC_EPISODE], sc[SC_NP], sc[SC_ARC], sc[SC_NA], sc[SC_K], sc[SC_LIVE] = gen, 1, n, na, st['NA'], st['k'], 0
    b[o['log']:o['log'] + len(st['log'])] = st['log']
    return b


def from_block(b, D, nlog=NLOG):
    n0, a0, h = geom(D)
    o = state_off(D, nlog)
    sc = b[o['scalars']:o['scalars'] + 16]
    n, na, live = int(sc[SC_NP]), int(sc[SC_ARC]), int(sc[SC_LIVE])
    pop = b[o['pop'] + live * n0 * D:o['pop'] + (live + 1) * n0 * D].reshape(n0, D)
    return {'pop': pop[:n].copy(), 'cost': b[o['cost']:o['cost'] + n].copy(), 'arc': b[o['arc']:o['arc'] + na * D].reshape(na, D).copy(),
            'MF': b[o['MF']:o['MF'] + h].copy(), 'MCr': b[o['MCr']:o['MCr'] + h].copy(), 'pm': b[o['pm']:o['pm'] + 3].copy(), 'k': int(sc[SC_K]),
            'NA': int(sc[SC_NA]), 'fes': int(sc[SC_FES]), 'gbest': sc[SC_GBEST], 'log_index': int(sc[SC_LOG_INDEX]),
            'log': list(b[o['log']:o['log'] + int(sc[SC_COST_LEN])]), 'done': bool(sc[SC_DONE]), 'live': live,
            'u': b[o['u']:o['u'] + n0 * D].reshape(n0, D).copy(), 'ncost': b[o['ncost']:o['ncost'] + n0].copy(),
            'F': b[o['F']:o['F'] + n0].copy(), 'Cr': b[o['Cr']:o['Cr'] + n0].copy(), 'z': b[o['z']:o['z'] + n0].copy(), 'c': b[o['c']:o['c'] + n0].copy(),
            'scalars': sc.copy()}


STATE_KEYS = ('pop', 'cost', 'arc', 'MF', 'MCr', 'pm', 'k', 'NA', 'fes', 'gbest', 'log_index', 'log', 'done')


def same_state(a, b):
    """The first field in which two states differ, or None."""
    for k in STATE_KEYS:
        if not np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)):
            return k
    return None


class Ctx:
    """What an update needs to know about the episode: the box, the budget, whether the problem has an optimum."""

    def __init__(self, D, lb, ub, max_fes, has_opt, early_stop=True, nlog=NLOG):
        self.D, self.lb, self.ub, self.max_fes, self.has_opt, self.early_stop, self.nlog = D, lb, ub, int(max_fes), has_opt, early_stop, nlog
        self.log_interval = self.max_fes // nlog


def q_of(fes, max_fes):
    return 2 * P_BEST - P_BEST * fes / max_fes


def sizes(n, narc, fes, max_fes):
    """Rows of pbest, of the mutation's qbest, and of the pool the qBX rows cross with."""
    q = q_of(fes, max_fes)
    nbq = max(int(q * n), 2)
    return max(int(P_BEST * n), 2), nbq, (max(int(q * (n + narc)), 2) if narc > 0 else nbq)


def strategies(pm, um):
    cdf = np.cumsum(pm)
    cdf /= cdf[-1]
    return np.searchsorted(cdf, um, side='right')


# ------------------------------------------------------------------------------------------------ the reference's draws as tapes
class MaddeTapeFeeder:
    """numpy's legacy stream as MadDE consumes it, laid out as the tape of include/mbx_layout.h §13.  Group sizes follow from the feeder's
    own strategy draw; the population and archive sizes, NA, fes, pm and the number of improved rows are the optimizer's state and come
    from the caller.  All draws go through one RandomState (legacy `normal` keeps a spare Gaussian between calls)."""

    def __init__(self, D, noise_kind, rs):
        self.rs, self.D, self.noise = rs, D, noise_kind
        self.last = {}

    def _noise(self, t, n, total, base):
        r = self.rs
        if self.noise == 1:
            t[base:base + n] = r.randn(n)
        elif self.noise == 2:
            t[base:base + n] = r.rand(n)
            t[base + total:base + total + n] = r.rand(n)
        elif self.noise == 3:
            t[base:base + n] = r.rand(n)
            t[base + total:base + total + n] = r.randn(n)
            t[base + 2 * total:base + 2 * total + n] = r.randn(n)

    def reset_tape(self):
        D = self.D
        n0 = geom(D)[0]
        t = np.zeros(tape_stride(D))
        t[:n0 * D] = self.rs.rand(n0, D).ravel()
        self._noise(t, n0, n0, n0 * D)
        return t

    def _draw(self, n, high, reject):
        """randint(high, size=n), then the bounded redraw: the rejected entries are redrawn together, 25 times at most."""
        if n == 0:
            return np.zeros(0, dtype=int)
        r = self.rs.randint(high, size=n)
        count = 0
        dup = np.where(reject(r))[0]
        while dup.shape[0] > 0 and count < TRIES:
            r[dup] = self.rs.randint(high, size=dup.shape[0])
            dup = np.where(reject(r))[0]
            count += 1
        return r

    def step_tape(self, n, narc, NA, fes, pm, max_fes, n_opt):
        from scipy import stats
        D, rs = self.D, self.rs
        n0, a0, h = geom(D)
        o = tape_off(D)
        t = np.zeros(tape_stride(D))
        nbp, nbq, pool = sizes(n, narc, fes, max_fes)
        t[o['mem']:o['mem'] + n] = rs.randint(0, h, size=n)
        t[o['z']:o['z'] + n] = rs.standard_normal(n)
        t[o['c']:o['c'] + n] = stats.cauchy.rvs(size=n, random_state=rs)
        um = rs.random_sample(n)
        t[o['choice']:o['choice'] + n] = um
        mu = strategies(np.array(pm, dtype=np.float64), um)
        for g in range(3):
            rows = np.where(mu == g)[0]
            m = len(rows)
            me = np.arange(m)
            if g == 0:
                rb = self._draw(m, nbp, lambda r: r == me)
                r1 = self._draw(m, m, lambda r: (r == rb) + (r == me))
                r2 = self._draw(m, m + narc, lambda r: (r == rb) + (r == me) + (r == r1))
            elif g == 1:
                rb = np.zeros(m, dtype=int)
                r1 = self._draw(m, m, lambda r: r == me)
                r2 = self._draw(m, m + narc, lambda r: (r == me) + (r == r1))
            else:
                rb = self._draw(m, nbq, lambda r: r == me)
                r1 = self._draw(m, m, lambda r: (r == rb) + (r == me))
                r2 = self._draw(m, m, lambda r: (r == rb) + (r == me) + (r == r1))
            t[o['rb'] + rows], t[o['r1'] + rows], t[o['r2'] + rows] = rb, r1, r2
        rvs = rs.rand(n)
        t[o['rvs']:o['rvs'] + n] = rvs
        cross = t[o['cross']:o['cross'] + n0 * D].reshape(n0, D)
        qb = np.where(rvs <= P_QBX)[0]
        if len(qb) > 0:
            t[o['qpick'] + qb] = rs.randint(pool, size=len(qb))
            t[o['jrand'] + qb] = rs.randint(D, size=len(qb))
            cross[qb] = rs.rand(len(qb), D)
        rest = np.where(rvs > P_QBX)[0]
        t[o['jrand'] + rest] = rs.randint(D, size=len(rest))
        cross[rest] = rs.rand(len(rest), D)
        self._noise(t, n, n0, o['noise'])
        app = min(max(NA - narc, 0), n_opt)
        for k in range(app, n_opt):
            t[o['arc'] + k] = rs.randint(narc + app)
        self.last = {'groups': [int(np.sum(mu == g)) for g in range(3)], 'qbx': len(qb), 'pool': pool, 'qpick_max': t[o['qpick'] + qb].max() if len(qb) else -1}
        return t


# ------------------------------------------------------------------------------------------------ restatement of reset and of one update
def restate_reset(ctx, t, ncost, pm):
    """__init_population with the draws of tape `t` and the costs `ncost` of the initial rows -> (initial rows, state)."""
    D = ctx.D
    n0 = geom(D)[0]
    u = t[:n0 * D].reshape(n0, D) * (ctx.ub - ctx.lb) + ctx.lb
    order = np.argsort(ncost, kind='stable')
    cost = ncost[order]
    return u, {'pop': u[order], 'cost': cost, 'arc': np.zeros((0, D)), 'MF': np.ones(10 * D) * 0.2, 'MCr': np.ones(10 * D) * 0.2, 'pm': np.array(pm, dtype=np.float64),
               'k': 0, 'NA': int(2.3 * n0), 'fes': n0, 'gbest': cost.min(), 'log_index': 1, 'log': [cost.min()], 'done': False}


def restate_trials(ctx, st, t):
    """The trial rows of one update (no cost is computed on the way, only read) -> (u, {F, Cr, mu})."""
    D, o = ctx.D, tape_off(ctx.D)
    pop, arc = st['pop'], st['arc']
    n, narc = len(pop), len(arc)
    nbp, nbq, pool = sizes(n, narc, st['fes'], ctx.max_fes)
    Fa = 0.5 + 0.5 * st['fes'] / ctx.max_fes
    ind = t[o['mem']:o['mem'] + n].astype(int)
    Cr = np.minimum(1, np.maximum(0, st['MCr'][ind] + 0.1 * t[o['z']:o['z'] + n]))
    loc = st['MF'][ind]
    F = t[o['c']:o['c'] + n] * 0.1 + loc
    neg = F < 0
    F[neg] = 2 * loc[neg] - F[neg]
    F = np.minimum(1, F)
    mu = strategies(st['pm'].copy(), t[o['choice']:o['choice'] + n])
    v = np.zeros((n, D))
    for g in range(3):
        rows = np.where(mu == g)[0]
        if len(rows) == 0:
            continue
        grp, Fs = pop[rows], F[rows][:, None]
        rb, r1, r2 = (t[o[k] + rows].astype(int) for k in ('rb', 'r1', 'r2'))
        x1 = grp[r1]
        x2 = np.concatenate((grp, arc), 0)[r2] if g < 2 else grp[r2]
        if g == 0:
            v[rows] = grp + Fs * (pop[:nbp][rb] - grp) + Fs * (x1 - x2)
        elif g == 1:
            v[rows] = grp + Fs * (x1 - x2)
        else:
            v[rows] = Fs * x1 + Fs * Fa * (pop[:nbq][rb] - x2)
    low = v < ctx.lb
    v[low] = (v[low] + ctx.lb) / 2
    high = v > ctx.ub
    v[high] = (v[high] + ctx.ub) / 2
    parent = pop.copy()
    qb = np.where(t[o['rvs']:o['rvs'] + n] <= P_QBX)[0]
    if len(qb) > 0:
        parent[qb] = np.concatenate((pop, arc), 0)[:pool][t[o['qpick'] + qb].astype(int)]
    cu = t[o['cross']:o['cross'] + n * D].reshape(n, D)
    u = np.where(cu < Cr[:, None], v, parent)
    jr = t[o['jrand']:o['jrand'] + n].astype(int)
    u[np.arange(n), jr] = v[np.arange(n), jr]
    return u, {'F': F, 'Cr': Cr, 'mu': mu}


def _lehmer(df, s):
    w = df / np.sum(df)
    return np.sum(w * (s * s)) / np.sum(w * s) if np.sum(w * s) > 0.000001 else 0.5


def restate_finish(ctx, st, t, aux, u, ncost):
    """Everything downstream of the evaluation as a function of the trial costs it is given -> (state after, what happened)."""
    D, o = ctx.D, tape_off(ctx.D)
    n0 = geom(D)[0]
    pop, cost, F, Cr, mu = st['pop'], st['cost'], aux['F'], aux['Cr'], aux['mu']
    n, narc, k = len(pop), len(st['arc']), st['k']
    optim = np.where(ncost < cost)[0]
    app = min(max(st['NA'] - narc, 0), len(optim))
    arc = np.concatenate((st['arc'], pop[optim[:app]]), 0)
    hit = []
    for j in range(app, len(optim)):                                 # one after another: a later writer of the same row wins
        row = min(max(int(t[o['arc'] + j]), 0), len(arc) - 1)
        arc[row] = pop[optim[j]]
        hit.append(row)
    df = np.maximum(0, cost - ncost)
    MF, MCr = st['MF'].copy(), st['MCr'].copy()
    if len(optim) > 0:
        MF[k], MCr[k] = _lehmer(df[optim], F[optim]), _lehmer(df[optim], Cr[optim])
        k_new = (k + 1) % len(MF)
    else:
        MF[k], MCr[k], k_new = 0.5, 0.5, k
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        credit = np.array([np.mean(df[mu == g] / cost[mu == g]) for g in range(3)])
        if np.sum(credit) > 0:
            pm = np.maximum(0.1, np.minimum(0.9, credit / np.sum(credit)))
            pm /= np.sum(pm)
        else:
            pm = np.ones(3) / 3
    new_pop = pop.copy()
    new_pop[optim] = u[optim]
    new_cost = np.minimum(cost, ncost)
    fes = st['fes'] + n
    n_new = int(np.round(n0 + (4 - n0) * fes / ctx.max_fes))
    NA = int(2.3 * n_new)
    order = np.argsort(new_cost, kind='stable')[:n_new]
    gbest = min(st['gbest'], new_cost[order].min())
    log, log_index = list(st['log']), st['log_index']
    if fes >= log_index * ctx.log_interval:
        log_index += 1
        log.append(gbest)
    done = fes >= ctx.max_fes or (ctx.has_opt and ctx.early_stop and gbest <= 1e-8)
    if done:                                                         # what run_episode does after its loop
        if len(log) >= ctx.nlog + 1:
            log[-1] = gbest
        else:
            log.append(gbest)
    new = {'pop': new_pop[order], 'cost': new_cost[order], 'arc': arc[:NA], 'MF': MF, 'MCr': MCr, 'pm': pm, 'k': k_new, 'NA': NA, 'fes': fes,
           'gbest': gbest, 'log_index': log_index, 'log': log, 'done': bool(done)}
    info = {'n_opt': len(optim), 'n_over': len(optim) - app, 'mem': np.array([MF[k], MCr[k]]), 'hit': hit, 'credit': credit, 'tie': len(np.unique(new_cost)) < n}
    return new, info


# ------------------------------------------------------------------------------------------------ the fixture's episodes
def _problem(suite, dim, fid):
    if suite == 'protein':
        from test_protein import protein
        return protein()[0][fid], 0
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _episodes(case):
    """[(problem, noise kind, fixture key prefix)] in the order the generator ran them on one optimizer object."""
    suite, dim, fid, seed = case.split('/')
    if suite == 'second':
        f1, f2 = fid.split('-')
        return int(dim), int(seed), [(*_problem('bbob', dim, f1), f'{case}/first'), (*_problem('bbob', dim, f2), case)]
    return int(dim), int(seed), [(*_problem(suite, dim, fid), case)]


def _ctx(p, dim, max_fes, protein):
    return Ctx(dim, p.lb, p.ub, max_fes, not protein, nlog=5 if protein else NLOG)         # (the protein suite logs 5 points)


def _ncost_rows(key):
    """The fixture's ragged trial costs: row 0 the initial rows, row g the trials of update g."""
    n = TR[f'{key}/np'].astype(int)
    counts = np.concatenate(([n[0]], n[:-1]))
    edges = np.concatenate(([0], np.cumsum(counts)))
    flat = TR[f'{key}/ncost']
    assert edges[-1] == len(flat), key
    return [flat[edges[g]:edges[g + 1]] for g in range(len(n))]


def host_costs(p, protein, u, t, base, total):
    """The host objective at `u` with the tape's noise draws, minus the optimum where the problem has one."""
    f = oracle.evaluate(p.desc(), u)
    if protein:
        return f
    if p.noise[0] != 0:
        draws = np.stack([t[base + j * total:base + j * total + len(u)] for j in range(3)])
        f = oracle.apply_noise(p.desc(), p.bias, f, draws)
    return f - p.bias


def walk(case, visit=None, check=True):
    """Chain the restatement over the fixture episode(s) of `case` with the feeder's tapes and the REFERENCE's trial costs.  check: every
    recorded quantity and snapshot must be equal, and the host objective at the restated trial rows close to the recorded costs.
    visit(key, ctx, p, g, state before or None, tape, u, aux, reference ncost, state after) is called for the reset (g = 0) and every update."""
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    rs = np.random.RandomState(seed)
    protein = case.startswith('protein')
    n0 = geom(dim)[0]
    for p, nk, key in eps:
        ctx = _ctx(p, dim, max_fes, protein)
        fd = MaddeTapeFeeder(dim, nk, rs)
        rows = _ncost_rows(key)
        G = len(rows) - 1
        snaps = set(int(g) for g in TR[f'{key}/snap_gens'])
        fcr, fcr_at = TR.get(f'{key}/fcr'), 0
        for g in range(G + 1):
            if g == 0:
                t = fd.reset_tape()
                u, new = restate_reset(ctx, t, rows[0], TR[f'{key}/pm0'])
                st, aux, info = None, None, {'n_opt': 0, 'n_over': 0, 'mem': np.array([0.2, 0.2])}
            else:
                t = fd.step_tape(len(st['cost']), len(st['arc']), st['NA'], st['fes'], st['pm'], max_fes, int(TR[f'{key}/n_opt'][g]))
                u, aux = restate_trials(ctx, st, t)
                new, info = restate_finish(ctx, st, t, aux, u, rows[g])
            if check:
                where = (case, key, g)
                assert close(host_costs(p, protein, u, t, n0 * dim if g == 0 else tape_off(dim)['noise'], n0), rows[g]), where
                got = {'fes': new['fes'], 'gbest': new['gbest'], 'np': len(new['cost']), 'narc': len(new['arc']), 'na': new['NA'], 'k': new['k'], 'pm': new['pm'],
                       'mem': info['mem'], 'n_opt': info['n_opt'], 'n_over': info['n_over'], 'cmin': new['cost'].min(), 'csum': np.sum(new['cost'] if g else rows[0])}      # (the reference's rows are still in draw order after its reset)
                for name, v in got.items():
                    assert np.array_equal(np.asarray(v, dtype=np.float64), TR[f'{key}/{name}'][g].astype(np.float64)), (*where, name, v, TR[f'{key}/{name}'][g])
                if g > 0 and fcr is not None:
                    n = len(st['cost'])
                    assert np.array_equal(np.stack([aux['F'], aux['Cr']]), fcr[:, fcr_at:fcr_at + n]), (*where, 'F / Cr')
                    fcr_at += n
                if g in snaps:
                    sp, sc = TR[f'{key}/snap{g}/pop'], TR[f'{key}/snap{g}/cost']
                    if g == 0:                                       # the reference sorts at the start of its first update
                        order = np.argsort(sc, kind='stable')
                        sp, sc = sp[order], sc[order]
                    for name, a, b in (('pop', new['pop'], sp), ('cost', new['cost'], sc), ('arc', new['arc'], TR[f'{key}/snap{g}/arc']),
                                       ('MF', new['MF'], TR[f'{key}/snap{g}/MF']), ('MCr', new['MCr'], TR[f'{key}/snap{g}/MCr'])):
                        assert np.array_equal(a, b), (*where, 'snapshot', name)
            if visit is not None:
                visit(key, ctx, p, g, st, t, u, aux, rows[g], new)
            st = new
        if check:
            assert st['done'] and np.array_equal(st['log'], TR[f'{key}/cost']) and st['fes'] == TR[f'{key}/fes'][-1], (case, key)
    return rs


# ------------------------------------------------------------------------------------------------ CPU
def test_madde_is_exported_and_picked_up_by_the_tester(tmp_path):
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import MadDE
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--test', '--t_optimizer_for_cp', 'MadDE', '--log_dir', str(tmp_path / 'out')])
    t = Tester(cfg)
    assert 'MadDE' in [type(o).__name__ for o in t.t_optimizer_for_cp] and 'MadDE' not in t.skipped and t.skipped == []
    assert isinstance(MadDE(copy.deepcopy(cfg)), MadDE)
    assert all('MadDE' in t.test_results['cost'][str(p)] for p in t.test_set.data)


def test_abi_geometry_of_madde():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_MADDE == ALGO_MADDE
    for D in (10, 12, 30, 40):
        cfg = oracle.make_cfg(ALGO_MADDE, 2 * D * D, D, 2000 * D, 40 * D, NLOG)
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1
        assert lib.mbx_action_dim(C.byref(cfg)) == 0
    for algo in (12, 14):                                            # not assigned
        bad = oracle.make_cfg(algo, 200, 10, 20000, 400, NLOG)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0
    for np_, D in ((100, 10), (170, 10), (201, 10), (200, 12), (2 * 41 * 41, 41), (2 * 64 * 64, 64)):          # np != 2 D^2, dim > 40
        bad = oracle.make_cfg(ALGO_MADDE, np_, D, 20000, 400, NLOG)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0, (np_, D)
    assert state_off(10)['end'] == 3 * 200 * 10 + 6 * 200 + int(2.3 * 200) * 10 + 200 + 4 + 16 + NLOG + 1 and int(2.3 * 200) == 459


@pytest.mark.parametrize('case', CASES)
def test_feeder_consumes_the_reference_stream(case):
    """Over the whole fixture episode(s) the feeder, told the optimizer's state by the fixture, draws exactly what the reference drew: the
    next np.random.rand() after the episode is the one the generator recorded."""
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    rs = np.random.RandomState(seed)
    for p, nk, key in eps:
        fd = MaddeTapeFeeder(dim, nk, rs)
        fd.reset_tape()
        f = {k: TR[f'{key}/{k}'] for k in ('np', 'narc', 'na', 'fes', 'pm', 'n_opt')}
        for g in range(1, len(f['np'])):
            pm = TR[f'{key}/pm0'] if g == 1 else f['pm'][g - 1]
            fd.step_tape(int(f['np'][g - 1]), int(f['narc'][g - 1]), int(f['na'][g - 1]), int(f['fes'][g - 1]), pm, max_fes, int(f['n_opt'][g]))
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case):
    """restate_trials / restate_finish chained from the reset with the feeder's tapes and the fixture's trial costs: every recorded
    quantity of every update and every snapshot equal, no tolerance; the host objective at the restated trial rows is close to the
    recorded costs; F and Cr equal the recorded ones where the fixture holds them; the stream ends where the reference's did."""
    rs = walk(case)
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_records_f_and_cr_for_the_two_shortest_cases():
    keys = [k[:-4] for k in TR if k.endswith('/fcr')]
    assert any(k.startswith('protein') for k in keys) and any(k.startswith('second') for k in keys)
    for k in keys:
        assert TR[f'{k}/fcr'].shape == (2, int(TR[f'{k}/np'][:-1].sum())), k


def test_fixture_covers_the_quirks():
    """The fixture exercises what it is meant to pin (from the recorded arrays and the feeder's own group sizes)."""
    k = 'bbob/10/1/61'
    assert TR[f'{k}/fes'][-1] < TR[f'{k}/max_fes'] and TR[f'{k}/gbest'][-1] <= 1e-8                    # early stop
    k = 'bbob-noisy/10/101/66'
    assert TR[f'{k}/fes'][-1] < TR[f'{k}/max_fes'] and TR[f'{k}/gbest'][-1] <= 1e-8                    # ... on a noisy function
    k = 'bbob/10/15/63'
    assert TR[f'{k}/fes'][-1] == 20001 and TR[f'{k}/np'][-1] == 4 and len(TR[f'{k}/cost']) == 51        # overshoot at the full budget
    assert np.allclose(TR[f'{k}/pm'][-1], [1 / 11, 9 / 11, 1 / 11])                                  # pm clipped
    assert TR['protein/12/1ATN_7/70/np'][-1] == 3 and TR['protein/12/1ATN_7/70/np'][0] == 288
    assert TR['bbob/30/10/69/np'][0] == 1800 and TR['bbob/30/10/69/narc'].max() > 2000
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}
    second = [c for c in CASES if c.startswith('second')]
    assert len(second) == 1 and not np.allclose(TR[f'{second[0]}/pm0'], 1 / 3) and np.array_equal(TR[f'{second[0]}/pm0'], TR[f'{second[0]}/first/pm'][-1])
    seen = {'empty': 0, 'qbx': 0, 'qbx_arc': 0, 'collide': 0}

    def visit(key, ctx, p, g, st, t, u, aux, ncost, new):
        if g > 0:
            n, narc = len(st['cost']), len(st['arc'])
            o = tape_off(ctx.D)
            qb = np.where(t[o['rvs']:o['rvs'] + n] <= P_QBX)[0]
            seen['empty'] += int(min(np.sum(aux['mu'] == j) for j in range(3)) == 0)
            seen['qbx'] += len(qb)
            seen['qbx_arc'] += int(np.sum(t[o['qpick'] + qb] >= n))
            n_opt = int(np.sum(ncost < st['cost']))
            hits = t[o['arc'] + min(max(st['NA'] - narc, 0), n_opt):o['arc'] + n_opt]
            seen['collide'] += int(len(np.unique(hits)) < len(hits))
    for case in ('bbob/10/1/61', 'bbob/10/15/63'):
        walk(case, visit, check=False)
        kk, n_opt, n_over = TR[f'{case}/k'], TR[f'{case}/n_opt'], TR[f'{case}/n_over']
        assert np.any(n_over[1:] > 0) and np.any(n_opt[1:] - n_over[1:] > 0)                          # archive overwrites and appends
        assert np.any(np.diff(kk) != 0) and np.any((np.diff(kk) == 0) & (n_opt[1:] == 0))             # k advances, and stays where nothing improved
        pm = TR[f'{case}/pm'][1:]
        assert np.any(np.all(pm == 1 / 3, axis=1)) and np.any(np.isclose(pm, 1 / 11)) and np.any((pm > 0.12) & (pm < 0.32))   # fallback, clipped, neither
    assert seen['empty'] > 0 and seen['qbx'] > 0 and seen['qbx_arc'] > 0 and seen['collide'] > 0, seen


def test_update_count_follows_from_the_population_schedule():
    from metabox_amd.optimizer import MadDE
    for case in ('bbob/10/15/63', 'bbob/10/22/64', 'bbob/10/24/65', 'bbob/10/7/62', 'bbob/30/10/69', 'protein/12/1ATN_7/70'):
        dim = int(case.split('/')[1])
        assert MadDE.n_updates(dim, int(TR[f'{case}/max_fes'])) == len(TR[f'{case}/fes']) - 1, case
    assert MadDE.n_updates(10, 20000) >= len(TR['bbob/10/1/61/fes']) - 1                              # an early stop takes fewer


# ------------------------------------------------------------------------------------------------ GPU
def _three_way(b, idx, ctx, st, t, u_want, aux, ref_ncost, where, ledger, blk=None):
    """(A) / (B) / (C) for one instance after its step from state `st` with tape `t` (module docstring); the decisions against the
    reference's trial costs go to the ledger."""
    D = ctx.D
    got = from_block(b.read_state(idx) if blk is None else blk, D, ctx.nlog)
    n = len(st['cost'])
    assert np.array_equal(got['u'][:n], u_want), (*where, 'A: trial rows', int(np.sum(got['u'][:n] != u_want)))
    assert np.array_equal(got['F'][:n], aux['F']) and np.array_equal(got['Cr'][:n], aux['Cr']), (*where, 'A: F / Cr')
    dev = got['ncost'][:n]
    if ref_ncost is not None:
        assert close(dev, ref_ncost), (*where, 'B: trial costs', np.abs(dev - ref_ncost).max())
        prove_tie_arrays(st['cost'], ref_ncost, (ref_ncost < st['cost']).astype(np.float64), st['cost'], dev, (dev < st['cost']).astype(np.float64), ledger, 'select', where[0], where[-1])
    want, info = restate_finish(ctx, st, t, aux, got['u'][:n], dev)
    assert got['live'] == 1 and got['scalars'][SC_GEN] == where[-1], where
    bad = same_state(got, want)
    assert bad is None, (*where, 'C: state after', bad, got[bad], want[bad])
    return got, want, info


def _step_states(b, ctx, items, ledger):
    """items: [(where, state before, tape, u, aux, reference ncost)], at most b.B of them, stepped as the instances of one launch."""
    import torch
    tape = torch.zeros(b.B, b.tape_stride, dtype=torch.float64)
    for i, (where, st, t, u, aux, ref) in enumerate(items):
        b.write_state(i, to_block(st, ctx.D, gen=where[-1] - 1, nlog=ctx.nlog))
        tape[i] = torch.from_numpy(t)
    b.set_tape(tape.cuda())
    b.step(None)
    torch.cuda.synchronize()
    return [_three_way(b, i, ctx, st, t, u, aux, ref, where, ledger) for i, (where, st, t, u, aux, ref) in enumerate(items)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_madde_every_update_from_the_reference_state(case):
    """Every update of every fixture episode, one at a time from the restated (= the reference's) state before it, the updates of an
    episode stepped as the instances of one batch: (A) trial rows, F, Cr bit for bit; (B) trial costs close to the reference's; (C) the
    state after bit for bit against the restatement fed the device's costs.  A selection that the device's costs decide differently
    from the reference's must be a proven near tie.  The reset likewise (u = the initial rows)."""
    import torch
    from metabox_amd.suite import Batch, Suite
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    n0 = geom(dim)[0]
    s = Suite([p for p, _, _ in eps])
    per = 128 if dim <= 12 else 16
    pending, ledger, count = {}, [], [0]

    def visit(key, ctx, p, g, st, t, u, aux, ncost, new):
        pending.setdefault(key, (ctx, []))[1].append(((case, key, g), st, t, u, aux, ncost, new))
    walk(case, visit, check=False)
    for k, (p, nk, key) in enumerate(eps):
        ctx, items = pending[key]
        # the reset: a batch of one, the tape's rows and the device's own costs
        where, _, t, u, _, ncost, _ = items[0]
        b1 = Batch(s, ALGO_MADDE, [k], [seed], n0, max_fes, max_fes // ctx.nlog, ctx.nlog)
        assert (b1.state_dim, b1.action_dim, b1.tape_stride) == (1, 0, tape_stride(dim))
        blk = b1.read_state(0)
        blk[state_off(dim, ctx.nlog)['pm']:state_off(dim, ctx.nlog)['pm'] + 3] = TR[f'{key}/pm0']
        b1.write_state(0, blk)
        b1.set_tape(torch.from_numpy(t).cuda().reshape(1, -1))
        st0 = b1.reset()
        torch.cuda.synchronize()
        got = from_block(b1.read_state(0), dim, ctx.nlog)
        assert st0[0, 0].item() == n0 / max_fes
        assert np.array_equal(got['u'], u), (*where, 'A: initial rows')
        assert close(got['ncost'], ncost), (*where, 'B: initial costs', np.abs(got['ncost'] - ncost).max())
        _, want = restate_reset(ctx, t, got['ncost'], TR[f'{key}/pm0'])
        assert got['live'] == 0 and same_state(got, want) is None, (*where, 'C', same_state(got, want))
        b1.close()
        # the updates
        b = Batch(s, ALGO_MADDE, [k] * per, [seed] * per, n0, max_fes, max_fes // ctx.nlog, ctx.nlog)
        b.reset()
        steps = [it[:6] for it in items[1:]]
        for c0 in range(0, len(steps), per):
            _step_states(b, ctx, steps[c0:c0 + per], ledger)
            count[0] += len(steps[c0:c0 + per])
        b.close()
    assert count[0] == sum(len(TR[f'{key}/fes']) - 1 for _, _, key in eps)             # no update skipped
    print(f'{case}: {count[0]} updates, {len(ledger)} with a decision on a proven near tie')
    print_ledger(ledger)


def _crafted(D=10, max_fes=20000, seed=7, fid=1, steps=3, suite='bbob'):
    """A batch of one instance, the restated state after a tape reset and `steps` tape updates (so that the archive holds rows), a feeder
    that continues the stream, and the context."""
    import torch
    from metabox_amd.suite import Batch, Suite
    protein = suite == 'protein'
    p, nk = _problem(suite, D, fid)
    s = Suite([p])
    n0 = geom(D)[0]
    ctx = _ctx(p, D, max_fes, protein)
    b = Batch(s, ALGO_MADDE, [0], [seed], n0, max_fes, max_fes // ctx.nlog, ctx.nlog)
    fd = MaddeTapeFeeder(D, nk, np.random.RandomState(seed))
    b.set_tape(torch.from_numpy(fd.reset_tape()).cuda().reshape(1, -1))
    b.reset()
    for g in range(steps):
        st = from_block(b.read_state(0), D, ctx.nlog)
        b.set_tape(torch.from_numpy(fd.step_tape(len(st['cost']), len(st['arc']), st['NA'], st['fes'], st['pm'], max_fes, len(st['cost']))).cuda().reshape(1, -1))
        b.step(None)
    st = from_block(b.read_state(0), D, ctx.nlog)
    return b, ctx, fd, {k: st[k] for k in STATE_KEYS}


def _tape_for(fd, st, ctx, n_opt=None):
    n = len(st['cost'])
    return fd.step_tape(n, len(st['arc']), st['NA'], st['fes'], st['pm'], ctx.max_fes, n if n_opt is None else n_opt)


def _run_crafted(b, ctx, st, t, gen=9):
    u, aux = restate_trials(ctx, st, t)
    got, want, info = _step_states(b, ctx, [(('crafted', gen), st, t, u, aux, None)], [])[0]
    return got, want, info, aux


@pytest.mark.gpu
def test_hip_madde_equal_costs_sort_in_row_order():
    """Equal costs inside the live rows and across the truncation boundary: the kernel keeps numpy's kind='stable' order."""
    b, ctx, fd, st = _crafted(max_fes=2000, steps=2)
    n = len(st['cost'])
    n_new = int(np.round(200 + (4 - 200) * (st['fes'] + n) / ctx.max_fes))
    st['cost'][:] = np.sort(np.repeat(st['cost'][::4], 4)[:n])          # runs of four equal costs, the boundary falls inside one
    assert n_new % 4 != 0 and n_new < n
    st['gbest'] = st['cost'].min()
    got, want, info, _ = _run_crafted(b, ctx, st, _tape_for(fd, st, ctx))
    assert info['tie'] and len(np.unique(got['cost'])) < len(got['cost'])
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('fill', ['full', 'one short', 'empty'])
def test_hip_madde_archive_fill_levels(fill):
    b, ctx, fd, st = _crafted()
    rs = np.random.RandomState(3)
    rows = {'full': st['NA'], 'one short': st['NA'] - 1, 'empty': 0}[fill]
    st['arc'] = rs.uniform(-5, 5, (rows, 10))
    got, want, info, _ = _run_crafted(b, ctx, st, _tape_for(fd, st, ctx))
    assert info['n_opt'] > 2 and info['n_over'] == {'full': info['n_opt'], 'one short': info['n_opt'] - 1, 'empty': 0}[fill]
    b.close()


@pytest.mark.gpu
def test_hip_madde_colliding_archive_writers_and_the_extremes_of_improvement():
    """Every overwriting row draws archive row 5: the last improved row wins.  Then an update in which nothing improves (k stays, the
    memory slot becomes 0.5) and one in which every row improves."""
    b, ctx, fd, st = _crafted()
    o = tape_off(10)
    st['arc'] = np.random.RandomState(4).uniform(-5, 5, (st['NA'], 10))
    t = _tape_for(fd, st, ctx)
    t[o['arc']:o['arc'] + 200] = 5
    got, want, info, _ = _run_crafted(b, ctx, st, t)
    assert info['n_over'] > 2 and set(info['hit']) == {5}
    worse = copy.deepcopy(st)
    worse['cost'][:] = np.linspace(-1e9, -1e8, len(worse['cost']))        # below every reachable Sphere cost
    worse['gbest'] = -1e9
    got, want, info, _ = _run_crafted(b, ctx, worse, _tape_for(fd, worse, ctx))
    assert info['n_opt'] == 0 and got['k'] == worse['k'] and got['MF'][worse['k']] == 0.5 and got['MCr'][worse['k']] == 0.5
    assert np.array_equal(got['pm'], np.ones(3) / 3)
    better = copy.deepcopy(st)
    better['cost'][:] = np.linspace(1e9, 2e9, len(better['cost']))
    got, want, info, _ = _run_crafted(b, ctx, better, _tape_for(fd, better, ctx))
    assert info['n_opt'] == len(better['cost']) and got['k'] == better['k'] + 1
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(0, 0, 4), (1, 1, 2), (2, 2, 0), (4, 0, 0), (1, 2, 1)])
def test_hip_madde_four_rows_in_every_group_shape(shape):
    """NP = 4 with strategy groups of 0, 1, 2 and 4 rows: a one-row group keeps r1 == self after the bounded redraws."""
    b, ctx, fd, st = _crafted(max_fes=2000, steps=2)
    o = tape_off(10)
    st['pop'], st['cost'] = st['pop'][:4], st['cost'][:4]
    st['arc'], st['NA'], st['fes'], st['pm'] = st['arc'][:9], 9, 1996, np.array([0.2, 0.5, 0.3])     # (the schedule's NP at 1996 and at 2000 FEs is 4)
    cuts = np.cumsum([0.2, 0.5, 0.3]) / np.cumsum([0.2, 0.5, 0.3])[-1]
    um = np.concatenate([np.full(m, [0.1, 0.5, 0.9][g]) for g, m in enumerate(shape)])
    assert list(np.bincount(np.searchsorted(cuts, um, side='right'), minlength=3)) == list(shape)
    # the feeder draws its own strategies: keep its indices only where they are in range for the crafted groups
    t = _tape_for(fd, st, ctx)
    t[o['choice']:o['choice'] + 4] = um
    mu = strategies(st['pm'].copy(), um)
    for g in range(3):
        rows = np.where(mu == g)[0]
        m = len(rows)
        t[o['rb'] + rows] = np.arange(m)[::-1] % 2
        t[o['r1'] + rows] = (np.arange(m) + 1) % max(m, 1)
        t[o['r2'] + rows] = (np.arange(m) + 2) % max(m, 1) if g == 2 else m + np.arange(m)      # an archive row for the first two strategies
    got, want, info, aux = _run_crafted(b, ctx, st, t)
    assert list(np.bincount(aux['mu'], minlength=3)) == list(shape) and len(got['cost']) in (3, 4)
    b.close()


@pytest.mark.gpu
def test_hip_madde_arithmetic_corners():
    """A row whose F is negative before the reflection (and one that stays negative after it), a weighted sum below the 1e-6 threshold,
    and a cost of exactly 0 in a group (the division of the strategy credit)."""
    b, ctx, fd, st = _crafted()
    o = tape_off(10)
    t = _tape_for(fd, st, ctx)
    t[o['c']:o['c'] + 4] = [-3.0, -30.0, -2.5, -1.0]                     # F = 0.2 - 0.3 -> 0.5 ; 0.2 - 3 -> 3.2 -> 1 ; ...
    got, want, info, aux = _run_crafted(b, ctx, st, t)
    assert np.all(aux['F'][:4] > 0) and aux['F'][1] == 1.0
    tiny = copy.deepcopy(st)
    tiny['MF'][:], tiny['MCr'][:] = 1e-9, 0.0                             # F and Cr of every row near 0: sum(w s) <= 1e-6
    t = _tape_for(fd, tiny, ctx)
    t[o['c']:o['c'] + 200], t[o['z']:o['z'] + 200] = 1e-9, -1.0
    tiny['cost'][:] = np.linspace(1e9, 2e9, len(tiny['cost']))
    got, want, info, aux = _run_crafted(b, ctx, tiny, t)
    assert info['n_opt'] > 0 and got['MF'][tiny['k']] == 0.5 and got['MCr'][tiny['k']] == 0.5 and got['k'] == tiny['k'] + 1
    zero = copy.deepcopy(st)
    zero['cost'][0], zero['gbest'] = 0.0, 0.0
    got, want, info, aux = _run_crafted(b, ctx, zero, _tape_for(fd, zero, ctx))
    assert np.isnan(info['credit']).any() and np.array_equal(got['pm'], np.ones(3) / 3)     # 0 / 0 in the best row's group: pm falls back
    b.close()


@pytest.mark.gpu
def test_hip_madde_at_d40_and_on_the_protein_instance():
    """One update at D = 40 with all 3200 rows, and one on the protein instance (no optimum, negative costs allowed)."""
    b, ctx, fd, st = _crafted(D=40, max_fes=80000, steps=0)
    assert len(st['cost']) == 3200 and len(st['arc']) == 0
    _run_crafted(b, ctx, st, _tape_for(fd, st, ctx))
    b.close()
    b, ctx, fd, st = _crafted(D=12, max_fes=1000, steps=2, fid='1ATN_7', suite='protein')
    got, want, info, _ = _run_crafted(b, ctx, st, _tape_for(fd, st, ctx))
    assert not ctx.has_opt and not got['done']
    b.close()


@pytest.mark.gpu
def test_hip_madde_batch_invariance_and_frozen_done_instances():
    """An instance's trajectory does not depend on the batch size, its slot or how the batch is split; done instances are left untouched
    beside live ones."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [1, 5, 8, 15, 20, 24, 103, 117]
    s = Suite([ps[i] for i in ids])
    B, max_fes = len(ids), 3000
    pidx = np.arange(B, dtype=np.int32)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 3
    full = Batch(s, ALGO_MADDE, pidx, seeds, 200, max_fes, max_fes // NLOG, NLOG)
    perm = np.random.RandomState(5).permutation(B)
    parts = [Batch(s, ALGO_MADDE, pidx[perm[:3]], seeds[perm[:3]], 200, max_fes, max_fes // NLOG, NLOG),
             Batch(s, ALGO_MADDE, pidx[perm[3:]], seeds[perm[3:]], 200, max_fes, max_fes // NLOG, NLOG)]
    where = {int(perm[j]): (0, j) if j < 3 else (1, j - 3) for j in range(B)}
    full.reset()
    for pb in parts:
        pb.reset()
    frozen = {}
    from metabox_amd.optimizer import MadDE
    for g in range(1, MadDE.n_updates(10, max_fes) + 3):
        _, _, d = full.step(None)
        for pb in parts:
            pb.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            blk = full.read_state(k)
            pb, j = where[k]
            assert np.array_equal(blk, parts[pb].read_state(j)), (ids[k], g)
            if k in frozen:
                assert np.array_equal(blk, frozen[k]), (ids[k], g)
                assert d[k].item() == 1
            elif from_block(blk, 10)['done']:
                frozen[k] = blk.copy()
    assert len(frozen) == B and len({from_block(v, 10)['scalars'][SC_GEN] for v in frozen.values()}) > 1      # some finished early
    full.close()
    for pb in parts:
        pb.close()


@pytest.mark.gpu
def test_hip_madde_free_running_episodes_match_the_reference_statistically():
    """51 free-running Philox episodes (seeds 1..51) per function through MadDE.run_batch against the 51 recorded reference episodes: a
    two-sided rank-sum test of the final gbest (of the final fes for F1 and F101, which stop early), pvalue > 1e-4 each."""
    from scipy import stats
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import MadDE
    from metabox_amd.suite import Suite
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    assert cfg.maxFEs == 20000
    for suite, fid in (('bbob', 1), ('bbob', 15), ('bbob', 24), ('bbob-noisy', 101)):
        ref = TR[f'finals/{suite}/10/{fid}']
        p = problems(suite, 10)[fid]
        r = MadDE(copy.deepcopy(cfg)).run_batch(Suite([p]), [0] * 51, np.arange(1, 52, dtype=np.uint64))
        n = r['cost_len'].cpu().numpy()
        gbest = np.array([r['cost'][i, n[i] - 1].item() for i in range(51)])
        fes = r['fes'].cpu().numpy().astype(np.float64)
        col = 1 if fid in (1, 101) else 0
        mine = fes if col == 1 else gbest
        pv = stats.ranksums(mine, ref[:, col]).pvalue
        print(f'{suite} F{fid}: median {"fes" if col else "gbest"} {np.median(mine):.6g} against the reference\'s {np.median(ref[:, col]):.6g}, rank-sum p = {pv:.3g}')
        assert pv > 1e-4, (suite, fid, pv)


@pytest.mark.gpu
def test_madde_in_the_tester_and_pm_carry_over(tmp_path):
    """Tester end to end on bbob D = 10 with MadDE in the list; run_episode twice on one object carries pm over, run_batch starts at 1/3."""
    import pickle
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import MadDE
    from metabox_amd.suite import Suite
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--test', '--t_optimizer_for_cp', 'MadDE',
                      '--log_dir', str(tmp_path / 'out')])
    cfg.t_optimizer_for_cp = ['MadDE']
    assert cfg.maxFEs == 20000
    t = Tester(cfg)
    assert t.runs == 51
    t.test()
    with open(t.log_dir + 'test.pkl', 'rb') as f:
        res = pickle.load(f)
    for p in t.test_set.data:
        rows = res['cost'][str(p)]['MadDE']
        assert len(rows) == 51 and all(len(r) == 51 for r in rows), str(p)
        assert all(np.all(np.diff(r) <= 0) for r in rows), str(p)
        assert all(f == 20001 or (f < 20001 and r[-1] <= 1e-8) for f, r in zip(res['fes'][str(p)]['MadDE'], rows)), str(p)
    # the B = 1 view: pm after the first episode is what the second starts with
    ps = problems('bbob', 10)
    c = copy.deepcopy(cfg)
    c.maxFEs, c.log_interval = 3000, 60
    opt = MadDE(c)
    # (most episodes end at 1/3: their last update has an empty strategy group; the seed is fixed, so the search is the same every run)
    np.random.seed(3)
    pms = []
    for _ in range(60):
        opt.run_episode(ps[15])
        pms.append(opt.pm())
        if not np.allclose(pms[-1], 1 / 3):
            break
    assert not np.allclose(pms[-1], 1 / 3), len(pms)
    carried = pms[-1]
    # the next episode binds another suite (a new batch: pm is copied into it), the one after it the same suite again (rebind)
    from metabox_amd import suite as suite_mod
    seen, orig = [], suite_mod.Batch.reset

    def spy(self):
        seen.append(from_block(self.read_state(0), 10)['pm'])
        return orig(self)
    suite_mod.Batch.reset = spy
    try:
        opt.run_episode(ps[3])
        again = opt.pm()
        opt.run_episode(ps[3])
    finally:
        suite_mod.Batch.reset = orig
    assert np.array_equal(seen[0], carried) and np.array_equal(seen[1], again), (seen, carried, again)
    # run_batch: a fresh batch, every instance at 1/3 when its reset runs
    b = MadDE(c).make_batch(Suite([ps[3]]), [0, 0], [1, 2])
    b.reset()
    for k in range(2):
        assert np.array_equal(from_block(b.read_state(k), 10)['pm'], np.ones(3) / 3)
    b.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ Philox route
def _u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0


def _mulhi(w, n):
    return (w * n) >> 32


def philox_indices(seed, gen, episode, mu, narc, nbp, nbq):
    """(rb, r1, r2) of every row under the site map of include/mbx_layout.h §13: one draw, then at most 25 redraws, each index with its
    own attempt counter; local to the row's strategy group as the reference draws them."""
    n = len(mu)
    size = [int(np.sum(mu == g)) for g in range(3)]
    rank = np.zeros(n, dtype=int)
    for g in range(3):
        rank[mu == g] = np.arange(size[g])
    out = np.zeros((n, 3), dtype=int)
    for i in range(n):
        g, m, j = int(mu[i]), size[int(mu[i])], int(rank[i])
        cache = {}

        def word(a, c):
            if a not in cache:
                cache[a] = oracle.philox(seed, i * 32 + a, SITE_IDX, gen, episode)
            return cache[a][c]

        def settle(c, high, reject):
            r, a = _mulhi(word(0, c), high), 1
            while a <= TRIES and reject(r):
                r = _mulhi(word(a, c), high)
                a += 1
            return r
        rb = -1 if g == 1 else settle(0, nbp if g == 0 else nbq, lambda r: r == j)
        r1 = settle(1, m, lambda r: r == rb or r == j)
        r2 = settle(2, m if g == 2 else m + narc, lambda r: r == rb or r == j or r == r1)
        out[i] = (max(rb, 0), r1, r2)
    return out, rank


def philox_tape(seed, gen, episode, ctx, noise_kind, st=None, after=None):
    """The tape that reproduces the Philox stream of (seed, gen, episode): gen 0 the reset, else the update from state `st`.  The two
    transcendental variates z / c and the number of improved rows come from the block the Philox step left (`after`)."""
    D = ctx.D
    n0, a0, h = geom(D)
    o = tape_off(D)
    t = np.zeros(tape_stride(D))

    def ph(idx, site):
        return oracle.philox(seed, idx, site, gen, episode)

    def noise(base, n, sa):
        assert noise_kind in (0, 2), 'only the noise kinds whose draws are exact uniforms are rebuilt here'
        for i in range(n if noise_kind == 2 else 0):
            w = ph(i, sa)
            t[base + i], t[base + n0 + i] = _u53(w[0], w[1]), _u53(w[2], w[3])
    if gen == 0:
        for e in range(n0 * D):
            w = ph(e, SITE_CROSS)
            t[e] = _u53(w[0], w[1])
        noise(n0 * D, n0, SITE_NOISE1_A)
        return t
    n, narc = len(st['cost']), len(st['arc'])
    nbp, nbq, pool = sizes(n, narc, st['fes'], ctx.max_fes)
    for i in range(n):
        w = ph(i, SITE_PAR)
        t[o['mem'] + i], t[o['qpick'] + i], t[o['jrand'] + i], t[o['rvs'] + i] = _mulhi(w[0], h), _mulhi(w[1], pool), _mulhi(w[2], D), w[3] / 2.0 ** 32
        w = ph(i, SITE_CAUCHY)
        t[o['choice'] + i] = _u53(w[2], w[3])
    t[o['z']:o['z'] + n], t[o['c']:o['c'] + n] = after['z'][:n], after['c'][:n]
    mu = strategies(st['pm'].copy(), t[o['choice']:o['choice'] + n])
    idx, _ = philox_indices(seed, gen, episode, mu, narc, nbp, nbq)
    t[o['rb']:o['rb'] + n], t[o['r1']:o['r1'] + n], t[o['r2']:o['r2'] + n] = idx.T
    for e in range(n * D):
        w = ph(e, SITE_CROSS)
        t[o['cross'] + e] = _u53(w[0], w[1])
    n_opt = int(np.sum(after['ncost'][:n] < st['cost']))
    alen = narc + min(max(st['NA'] - narc, 0), n_opt)
    for k in range(n_opt):
        t[o['arc'] + k] = _mulhi(ph(k, SITE_ARC)[0], alen)
    noise(o['noise'], n, SITE_NOISE_A)
    return t


@pytest.mark.gpu
def test_hip_madde_philox_equals_tape():
    """The Philox path and the tape path are the same computation: a tape rebuilt on the host from oracle.philox with the documented site
    map (bounded redraws included; z / c read back from the block, see philox_tape) gives bit-identical state blocks, on a noiseless
    and a uniform-noise problem, while the population shrinks and the archive fills and overflows."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [15, 102]
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    max_fes = 2500
    ctx = Ctx(10, -5.0, 5.0, max_fes, True)
    a = Batch(s, ALGO_MADDE, np.arange(2), seeds, 200, max_fes, max_fes // NLOG, NLOG)
    t = Batch(s, ALGO_MADDE, np.arange(2), seeds, 200, max_fes, max_fes // NLOG, NLOG)
    overwrites = 0
    for g in range(9):
        before = [from_block(a.read_state(k), 10) for k in range(2)]
        if g == 0:
            rows = [philox_tape(int(seeds[k]), 0, int(before[k]['scalars'][SC_EPISODE]) + 1, ctx, ps[ids[k]].noise[0]) for k in range(2)]
            a.reset()
        else:
            a.step(None)
            torch.cuda.synchronize()
            rows = []
            for k in range(2):
                after = from_block(a.read_state(k), 10)
                ep = int(before[k]['scalars'][SC_EPISODE])
                rows.append(philox_tape(int(seeds[k]), g, ep, ctx, ps[ids[k]].noise[0], before[k], after))
                n = len(before[k]['cost'])
                overwrites += max(0, int(np.sum(after['ncost'][:n] < before[k]['cost'])) - max(before[k]['NA'] - len(before[k]['arc']), 0))
        t.set_tape(torch.from_numpy(np.stack(rows)).cuda())
        if g == 0:
            t.reset()
        else:
            t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            sa, st_ = a.read_state(k), t.read_state(k)
            assert np.array_equal(sa, st_), (ids[k], g, int(np.argmax(sa != st_)))
    assert overwrites > 0 and from_block(a.read_state(0), 10)['scalars'][SC_NP] < 200
    a.close(); t.close()


def test_philox_index_draws_are_uniform_under_the_bounded_redraw():
    """The resolved indices of the Philox mode (philox_indices, the host restatement that test_hip_madde_philox_equals_tape proves equal to
    the kernel's draws bit for bit) are uniform over the rows the reference's rejection loops allow."""
    from scipy import stats
    m, narc, nbp = 30, 12, 5
    mu = np.ones(m, dtype=int)                                       # the second strategy: r1 != own rank, r2 none of own rank and r1
    r1s, r2s, js = [], [], []
    for k in range(150):
        idx, rank = philox_indices(1000003 * k + 17, 1 + k % 97, 1, mu, narc, nbp, nbp)
        r1s.append(idx[:, 1]); r2s.append(idx[:, 2]); js.append(rank)
    r1, r2, j = np.concatenate(r1s), np.concatenate(r2s), np.concatenate(js)
    assert r1.min() >= 0 and r1.max() < m and r2.max() < m + narc and not np.any(r1 == j) and not np.any((r2 == j) | (r2 == r1))
    assert stats.chisquare(np.bincount(r1 - (r1 > j), minlength=m - 1)).pvalue > 1e-4
    assert stats.chisquare(np.bincount(r2 - (r2 > j) - (r2 > r1), minlength=m + narc - 2)).pvalue > 1e-4
    # the first strategy: rb over pbest, unequal to the row's own rank where that rank is a pbest row
    mu = np.zeros(m, dtype=int)
    rbs, js = [], []
    for k in range(150):
        idx, rank = philox_indices(7919 * k + 3, 1 + k % 31, 1, mu, narc, nbp, nbp)
        rbs.append(idx[:, 0]); js.append(rank)
    rb, j = np.concatenate(rbs), np.concatenate(js)
    assert rb.min() >= 0 and rb.max() < nbp and not np.any(rb == j)
    assert stats.chisquare(np.bincount(rb[j >= nbp], minlength=nbp)).pvalue > 1e-4
    assert stats.chisquare(np.bincount((rb - (rb > j))[j < nbp], minlength=nbp - 1)).pvalue > 1e-4
