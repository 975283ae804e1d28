"""RL-HPSDE (src/optimizer/rl_hpsde_optimizer.py, src/agent/rl_hpsde_agent.py): the batched HIP kernels (metabox_amd/csrc/mbx_rlhpsde.hpp), their host
classes and the rollout entry point (include/mbx_rlhpsde.h) against seeded reference episodes (tests/golden/rlhpsde_traces*.npz, rlhpsde_policy.npz,
tools/gen_golden.py rlhpsde).

MF / MCr are arithmetic in the cost values (mean_wL weights by cost differences), and the kernels' objective values agree with numpy's to
helpers.RTOL / ATOL, not to the bit: one rounding of one cost leaves the reference trajectory within tens of updates, so no whole episode can be
replayed.  As for MadDE the kernel is pinned one update at a time, from the reference's own state, split at the evaluations:
  (A) state before + tape -> trial rows u, F, Cr, indices: bit for bit against `restate_trials`;
  (B) u -> ncost and walk -> wcost: helpers.close against the fixture's recorded costs;
  (C) state before + tape + ncost + wcost -> state after: bit for bit against `restate_finish` fed the DEVICE's costs;
and the chain to the reference is closed on the CPU: the restatement (numpy, written from the rules in the header of mbx_rlhpsde.hpp, kind='stable'
sort) fed the REFERENCE's recorded trial and walk costs reproduces every recorded quantity of every step and every snapshot exactly.

The numpy draws are not stored: HpTapeFeeder regenerates them from the seed in the reference's call order (include/mbx_layout.h section 19), calling
the same RandomState / scipy methods; the Cauchy and Levy variates are drawn with loc 0 and scale 1, so that loc + 0.1 x is restated exactly.
A search of resets at D = 2 / 3 found state 1 as well as state 0: the D = 3 Bent_Cigar case resets into state 0 and passes through state 1.
Measured figures are in docs/EXPERIMENTS.md."""
import copy
import ctypes as C
import glob
import os

import numpy as np
import pytest

from helpers import GOLDEN, close, problems
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'rlhpsde_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
CASES = [str(c) for c in TR['cases']]
POL = dict(np.load(os.path.join(GOLDEN, 'rlhpsde_policy.npz')))
Q = POL['q_table']
ALGO_RLHPSDE, TRIES, NLOG, WALK, STEPS, MARGIN = 24, 25, 50, 201, 200, 1e-6
SITE_NOISE1_A, SITE_NOISE1_B, SITE_POLICY = 7, 8, 15
SITE_PAR, SITE_NORM, SITE_CAUCHY, SITE_IDX, SITE_CROSS, SITE_NOISE_A, SITE_NOISE_B, SITE_WALK, SITE_WNOISE_A, SITE_WNOISE_B = range(66, 76)
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE, SC_NP, SC_K, SC_LIVE, SC_STATE, SC_ACTION = 0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14
FEAT_R, FEAT_H, FEAT_LEVEL, FEAT_NOPT, FEAT_COUNTS, FEAT_SLOTS = 0, 1, 2, 3, 10, 64
SCALES = [0, 1 / 128, 1 / 64, 1 / 32, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1]
CLASSES = ((-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0))


# ------------------------------------------------------------------------------------------------ layout (include/mbx_layout.h section 19)
def geom(D):
    return 18 * D, max(D // 2, 1)


def tape_off(D):
    n0 = geom(D)[0]
    o = {'zone': 0, 'off': D, 'stepu': 2 * D, 'rd': 202 * D, 'choice': 202 * D + 1, 'wnoise': 202 * D + 2}
    base = 202 * D + 2 + 3 * WALK + 1
    o.update(base=base, pos=base, noise_init=base + n0 * D, mem=base, z=base + n0, x=base + 2 * n0, r=base + 3 * n0, jrand=base + 6 * n0,
             noise=base + 7 * n0, cross=base + 10 * n0)
    return o


def tape_stride(D):
    n0 = geom(D)[0]
    return tape_off(D)['base'] + 10 * n0 + n0 * D


def state_off(D, nlog=NLOG):
    n0, h = geom(D)
    o, p = {}, 0
    for k, n in (('pop', 2 * n0 * D), ('cost', n0), ('MF', h), ('MCr', h), ('u', n0 * D), ('ncost', n0), ('F', n0), ('Cr', n0), ('r', 3 * n0), ('z', n0), ('x', n0),
                 ('walk', WALK * D), ('wcost', WALK), ('feat', FEAT_SLOTS), ('scalars', 16), ('log', nlog + 1)):
        o[k] = p
        p += n
    o['end'] = p
    return o


def to_block(st, D, gen=0, nlog=NLOG):
    """The state block of a restated state (dead areas zero, live buffer 0)."""
    n0, h = geom(D)
    o = state_off(D, nlog)
    b = np.zeros(o['end'])
    n = len(st['cost'])
    b[o['pop']:o['pop'] + n * D] = st['pop'].ravel()
    b[o['cost']:o['cost'] + n] = st['cost']
    b[o['MF']:o['MF'] + h], b[o['MCr']:o['MCr'] + h] = st['MF'], st['MCr']
    sc = b[o['scalars']:o['scalars'] + 16]
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = st['gbest'], st['fes'], st['log_index'], len(st['log']), float(st['done'])
    sc[SC_GEN], sc[SC_EPISODE], sc[SC_NP], sc[SC_K], sc[SC_LIVE], sc[SC_STATE], sc[SC_RETURN] = gen, 1, n, st['k'], 0, st['state'], st.get('ret', 0.)
    b[o['log']:o['log'] + len(st['log'])] = st['log']
    return b


def from_block(b, D, nlog=NLOG):
    n0, h = geom(D)
    o = state_off(D, nlog)
    sc = b[o['scalars']:o['scalars'] + 16]
    n, live = int(sc[SC_NP]), int(sc[SC_LIVE])
    pop = b[o['pop'] + live * n0 * D:o['pop'] + (live + 1) * n0 * D].reshape(n0, D)
    feat = b[o['feat']:o['feat'] + FEAT_SLOTS]
    return {'pop': pop[:n].copy(), 'cost': b[o['cost']:o['cost'] + n].copy(), 'MF': b[o['MF']:o['MF'] + h].copy(), 'MCr': b[o['MCr']:o['MCr'] + h].copy(),
            'k': int(sc[SC_K]), 'fes': int(sc[SC_FES]), 'gbest': sc[SC_GBEST], 'log_index': int(sc[SC_LOG_INDEX]),
            'log': list(b[o['log']:o['log'] + int(sc[SC_COST_LEN])]), 'done': bool(sc[SC_DONE]), 'live': live, 'state': int(sc[SC_STATE]), 'ret': sc[SC_RETURN],
            'u': b[o['u']:o['u'] + n0 * D].reshape(n0, D).copy(), 'ncost': b[o['ncost']:o['ncost'] + n0].copy(),
            'F': b[o['F']:o['F'] + n0].copy(), 'Cr': b[o['Cr']:o['Cr'] + n0].copy(), 'ridx': b[o['r']:o['r'] + 3 * n0].reshape(n0, 3).astype(int),
            'z': b[o['z']:o['z'] + n0].copy(), 'x': b[o['x']:o['x'] + n0].copy(),
            'walk': b[o['walk']:o['walk'] + WALK * D].reshape(WALK, D).copy(), 'wcost': b[o['wcost']:o['wcost'] + WALK].copy(),
            'r': feat[FEAT_R], 'H': feat[FEAT_H], 'n_opt': int(feat[FEAT_NOPT]), 'counts': feat[FEAT_COUNTS:FEAT_COUNTS + 54].reshape(9, 6).astype(int),
            'action': int(sc[SC_ACTION]), 'scalars': sc.copy()}


STATE_KEYS = ('pop', 'cost', 'MF', 'MCr', 'k', 'fes', 'gbest', 'log_index', 'log', 'done', 'state', 'walk', 'r', 'H', 'counts')


def same_state(a, b, keys=STATE_KEYS):
    """The first field in which two states differ, or None."""
    for k in keys:
        if not np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)):
            return k
    return None


class Ctx:
    """What an update needs to know about the episode: the box, the budget, whether the problem has an optimum."""

    def __init__(self, D, lb, ub, max_fes, has_opt, early_stop=True, nlog=NLOG):
        self.D, self.lb, self.ub, self.max_fes, self.has_opt, self.early_stop, self.nlog = D, lb, ub, int(max_fes), has_opt, early_stop, nlog
        self.log_interval = self.max_fes // nlog


def choose(q_row, u):
    """RL_HPSDE_Agent.__get_action with the uniform np.random.choice draws."""
    e = np.exp(q_row)
    cdf = np.cumsum(e / e.sum())
    return int(np.searchsorted(cdf / cdf[-1], u, side='right'))


# ------------------------------------------------------------------------------------------------ the reference's draws as tapes
class HpTapeFeeder:
    """numpy's legacy stream as RL-HPSDE consumes it, laid out as the tape of include/mbx_layout.h section 19.  The population size and the action
    are the optimizer's state and come from the caller.  All draws go through one RandomState (legacy `normal` keeps a spare Gaussian between calls)."""

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

    def _walk(self, t):
        D, rs, o = self.D, self.rs, tape_off(self.D)
        t[o['zone']:o['zone'] + D] = rs.rand(D)
        t[o['off']:o['off'] + D] = rs.rand(D)
        t[o['rd']] = rs.choice(D, 1)[0]
        for s in range(STEPS):
            t[o['stepu'] + s * D:o['stepu'] + (s + 1) * D] = rs.rand(D)
        self._noise(t, WALK, WALK, o['wnoise'])

    def reset_tape(self):
        D, o = self.D, tape_off(self.D)
        n0 = geom(D)[0]
        t = np.zeros(tape_stride(D))
        t[o['pos']:o['pos'] + n0 * D] = self.rs.rand(n0, D).ravel()
        self._noise(t, n0, n0, o['noise_init'])
        self._walk(t)
        return t

    def _random_int(self, n, cols):
        """generate_random_int (mutate.py:12-33): column by column, the repeated entries redrawn together until none is left."""
        rs = self.rs
        r = rs.randint(low=0, high=n, size=(n, cols))
        redraws = [0] * cols
        for col in range(cols):
            while True:
                rep = r[:, col] == np.arange(n)
                for i in range(col):
                    rep |= r[:, col] == r[:, i]
                idx = np.nonzero(rep)[0]
                if idx.size == 0:
                    break
                r[idx, col] = rs.randint(low=0, high=n, size=idx.size)
                redraws[col] += 1
        return r, redraws

    def step_tape(self, n, action, policy):
        from scipy import stats
        D, rs = self.D, self.rs
        n0, h = geom(D)
        o = tape_off(D)
        t = np.zeros(tape_stride(D))
        if policy:
            t[o['choice']] = rs.random_sample(1)[0]
        t[o['mem']:o['mem'] + n] = rs.randint(0, h, size=n)
        t[o['z']:o['z'] + n] = rs.standard_normal(n)
        t[o['x']:o['x'] + n] = (stats.levy if action >> 1 else stats.cauchy).rvs(loc=0, scale=1, size=n, random_state=rs)
        cols = 2 if action & 1 else 3
        r, redraws = self._random_int(n, cols)
        rr = t[o['r']:o['r'] + 3 * n].reshape(n, 3)
        rr[:, :cols] = r
        t[o['jrand']:o['jrand'] + n] = rs.randint(D, size=n)
        t[o['cross']:o['cross'] + n * D] = rs.rand(n, D).ravel()
        self._noise(t, n, n0, o['noise'])
        self._walk(t)
        self.last = {'redraws': redraws}
        return t


# ------------------------------------------------------------------------------------------------ restatement of reset and of one update
def walk_points(ctx, t):
    """__progressive_random_walk with the draws of tape `t` -> [201, D]."""
    D, o = ctx.D, tape_off(ctx.D)
    lb, ub = ctx.lb, ctx.ub
    zone = np.where(t[o['zone']:o['zone'] + D] < 0.5, -1., 1.)
    r = t[o['off']:o['off'] + D] * (ub - lb) / 2
    s = np.zeros((WALK, D))
    s[0] = (ub + lb) / 2 + zone * r
    rd = min(max(int(t[o['rd']]), 0), D - 1)
    s[0][rd] = lb if zone[rd] == -1 else ub
    for k in range(1, WALK):
        s[k] = s[k - 1] + t[o['stepu'] + (k - 1) * D:o['stepu'] + k * D] * (-10) * zone
        cu, cl = s[k] > ub, s[k] < lb
        s[k][cu] = 2 * ub - s[k][cu]
        s[k][cl] = 2 * lb - s[k][cl]
        zone[cu | cl] *= -1
    return s


def landscape(samples, wcost, best):
    """DFDC and DRIE of a walk -> (r, entropy, counts [9, 6], state); where the reference raises the bit is 0."""
    c = wcost[1:]
    dist = np.sqrt(np.add.reduce((samples[1:] - best) * (samples[1:] - best), axis=-1))
    with np.errstate(all='ignore'):
        r = np.mean((c - c.mean()) * (dist - dist.mean())) / (np.sqrt(np.mean((c - c.mean()) * (c - c.mean()))) * np.sqrt(np.mean((dist - dist.mean()) * (dist - dist.mean()))))
    diff = wcost[1:] - wcost[:STEPS]
    e_star = np.max(np.abs(diff))
    counts, hs = np.zeros((9, 6), dtype=int), []
    for lv, scale in enumerate(SCALES):
        sym = (diff < (-scale * e_star)) * (-1) + ((scale * e_star) < diff) * 1
        a, b = sym[:-1], sym[1:]
        counts[lv] = [np.sum((a == x) & (b == y)) for x, y in CLASSES]
        prob = counts[lv] / STEPS
        prob[prob < 1e-15] = 1e-15
        hs.append(-np.sum(prob * np.log(prob) / np.log(6)))
    H = max(hs)
    state = int(0.15 < r <= 1) + 2 * int(0.5 <= H <= 1)
    return r, H, counts, state


def restate_reset(ctx, t, ncost, wcost):
    """init_population with the draws of tape `t`, the costs `ncost` of the initial rows and `wcost` of the walk -> (initial rows, state)."""
    D, o = ctx.D, tape_off(ctx.D)
    n0, h = geom(D)
    u = t[o['pos']:o['pos'] + n0 * D].reshape(n0, D) * (ctx.ub - ctx.lb) + ctx.lb
    order = np.argsort(ncost, kind='stable')
    cost, pop = ncost[order], u[order]
    samples = walk_points(ctx, t)
    r, H, counts, state = landscape(samples, wcost, pop[0])
    return u, {'pop': pop, 'cost': cost, 'MF': np.ones(h) * 0.5, 'MCr': np.ones(h) * 0.5, 'k': 0, 'fes': n0 + WALK, 'gbest': cost[0], 'log_index': 1,
               'log': [cost[0]], 'done': False, 'state': state, 'walk': samples, 'r': r, 'H': H, 'counts': counts, 'ret': 0.}


def restate_trials(ctx, st, t, action):
    """The trial rows of one update (no cost is computed on the way, only read) -> (u, {F, Cr, ridx})."""
    D, o = ctx.D, tape_off(ctx.D)
    pop = st['pop']
    n, h = len(pop), len(st['MF'])
    ind = np.clip(t[o['mem']:o['mem'] + n].astype(int), 0, h - 1)
    Cr = np.minimum(1, np.maximum(0, st['MCr'][ind] + 0.1 * t[o['z']:o['z'] + n]))
    loc = st['MF'][ind]
    F = t[o['x']:o['x'] + n] * 0.1 + loc
    neg = F < 0
    F[neg] = 2 * loc[neg] - F[neg]
    F = np.minimum(1, F)
    ridx = np.clip(t[o['r']:o['r'] + 3 * n].reshape(n, 3).astype(int), 0, n - 1)
    if action & 1:
        ridx[:, 2] = 0
        v = pop + F[:, None] * (pop[0] - pop + pop[ridx[:, 0]] - pop[ridx[:, 1]])
    else:
        v = pop + F[:, None] * (pop[ridx[:, 0]] - pop + pop[ridx[:, 1]] - pop[ridx[:, 2]])
    v = np.clip(v, ctx.lb, ctx.ub)
    cu = t[o['cross']:o['cross'] + n * D].reshape(n, D)
    u = np.where(cu < Cr[:, None], v, pop)
    jr = np.clip(t[o['jrand']:o['jrand'] + n].astype(int), 0, D - 1)
    u[np.arange(n), jr] = v[np.arange(n), jr]
    return u, {'F': F, 'Cr': Cr, 'ridx': ridx}


def _lehmer(df, s):
    w = df / np.sum(df)
    return np.sum(w * (s * s)) / np.sum(w * s) if np.sum(w * s) > 0.000001 else 0.5


def restate_finish(ctx, st, t, aux, u, ncost, wcost):
    """Everything downstream of the trial evaluation as a function of the costs it is given -> (state after, what happened)."""
    D = ctx.D
    n0 = geom(D)[0]
    pop, cost, F, Cr = st['pop'], st['cost'], aux['F'], aux['Cr']
    n, k = len(pop), st['k']
    optim = np.where(ncost < cost)[0]
    df = np.maximum(0, cost - ncost)
    MF, MCr = st['MF'].copy(), st['MCr'].copy()
    if len(optim) > 0:
        MF[k], MCr[k] = _lehmer(df[optim], F[optim]), _lehmer(df[optim], Cr[optim])
        k_new = (k + 1) % len(MF)
    else:
        MF[k], MCr[k], k_new = 0.5, 0.5, k
    new_pop = pop.copy()
    new_pop[optim] = u[optim]
    new_cost = np.minimum(cost, ncost)
    fes = st['fes'] + n
    n_new = min(max(int(n0 + (4 - n0) * fes / ctx.max_fes), 1), n)
    full = np.argsort(new_cost, kind='stable')
    order = full[:n_new]
    gbest = new_cost[order][0]
    log, log_index = list(st['log']), st['log_index']
    if fes >= log_index * ctx.log_interval:
        log_index += 1
        log.append(gbest)
    done = fes >= ctx.max_fes or (ctx.has_opt and ctx.early_stop and gbest <= 1e-8)
    if done:
        if len(log) >= ctx.nlog + 1:
            log[-1] = gbest
        else:
            log.append(gbest)
    reward = len(optim) / n
    samples = walk_points(ctx, t)
    r, H, counts, state = landscape(samples, wcost, new_pop[order][0])
    new = {'pop': new_pop[order], 'cost': new_cost[order], 'MF': MF, 'MCr': MCr, 'k': k_new, 'fes': fes + WALK, 'gbest': gbest, 'log_index': log_index, 'log': log,
           'done': bool(done), 'state': state, 'walk': samples, 'r': r, 'H': H, 'counts': counts, 'ret': st.get('ret', 0.) + reward}
    # equal costs: a tie is harmless where the rows are identical; otherwise the stable order is the one both sides must take
    srt = new_cost[full]
    tie = bool(np.any((srt[1:] == srt[:-1]) & np.any(new_pop[full][1:] != new_pop[full][:-1], axis=1)))
    return new, {'n_opt': len(optim), 'reward': reward, 'tie': tie, 'neg_F': int(np.sum(t[tape_off(D)['x']:tape_off(D)['x'] + n] * 0.1 + st['MF'][np.clip(t[tape_off(D)['mem']:tape_off(D)['mem'] + n].astype(int), 0, len(MF) - 1)] < 0))}


# ------------------------------------------------------------------------------------------------ the fixture's episodes
def _problem(suite, dim, fid):
    if suite == 'protein':
        from test_protein import protein
        return protein()[0][fid], 0
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _case(case):
    suite, dim, fid, seed = case.split('/')
    p, nk = _problem(suite, dim, fid)
    protein = suite == 'protein'
    ctx = Ctx(int(dim), p.lb, p.ub, int(TR[f'{case}/max_fes']), not protein, nlog=5 if protein else NLOG)         # (the protein suite logs 5 points)
    return ctx, p, nk, int(seed), protein


def _ncost_rows(case):
    """The fixture's ragged trial costs: row 0 the initial rows, row g the trials of update g."""
    n = TR[f'{case}/np'].astype(int)
    counts = np.concatenate(([n[0]], n[:-1]))
    edges = np.concatenate(([0], np.cumsum(counts)))
    flat = TR[f'{case}/ncost']
    assert edges[-1] == len(flat), case
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
    """Chain the restatement over the fixture episode of `case` with the feeder's tapes and the REFERENCE's trial and walk costs.  check: every
    recorded quantity and snapshot must be equal, the margins hold, and the host objective at the restated rows is close to the recorded costs.
    visit(ctx, p, g, state before or None, tape, action, u, aux, reference ncost, reference wcost, state after, info) is called for the reset (g = 0)
    and every update."""
    ctx, p, nk, seed, protein = _case(case)
    dim = ctx.D
    rs = np.random.RandomState(seed)
    n0 = geom(dim)[0]
    o = tape_off(dim)
    fd = HpTapeFeeder(dim, nk, rs)
    rows, wc = _ncost_rows(case), TR[f'{case}/wcost']
    policy = bool(TR[f'{case}/policy'])
    G = len(rows) - 1
    snaps = set(int(g) for g in TR[f'{case}/snap_gens'])
    fcr, fcr_at = TR.get(f'{case}/fcr'), 0
    st = None
    for g in range(G + 1):
        where = (case, g)
        if g == 0:
            t, action = fd.reset_tape(), -1
            u, new = restate_reset(ctx, t, rows[0], wc[0])
            aux, info = None, {'n_opt': 0, 'reward': 0., 'tie': False, 'neg_F': 0}
        else:
            action = int(TR[f'{case}/action'][g])
            t = fd.step_tape(len(st['cost']), action, policy)
            if policy and check:
                assert choose(Q[st['state']], t[o['choice']]) == action, (*where, 'the choice rule')
            u, aux = restate_trials(ctx, st, t, action)
            new, info = restate_finish(ctx, st, t, aux, u, rows[g], wc[g])
            info['redraws'] = fd.last['redraws']
        if check:
            assert close(host_costs(p, protein, u, t, o['noise_init'] if g == 0 else o['noise'], n0), rows[g]), where
            assert close(host_costs(p, protein, new['walk'], t, o['wnoise'], WALK), wc[g]), (*where, 'walk costs')
            # (info['tie']: equal costs of DIFFERENT rows were sorted.  The generator kept the case because the reference's order was the stable one there; the
            #  restatement takes the stable order, and every later step's rows, costs and snapshots would differ if the reference had taken another)
            assert abs(new['r'] - 0.15) >= MARGIN and abs(new['H'] - 0.5) >= MARGIN, (*where, 'margins', new['r'], new['H'])
            got = {'fes': new['fes'], 'gbest': new['gbest'], 'np': len(new['cost']), 'k': new['k'], 'MF': new['MF'], 'MCr': new['MCr'], 'state': new['state'],
                   'reward': info['reward'], 'r': new['r'], 'H': new['H'], 'done': new['done']}
            for name, v in got.items():
                assert np.array_equal(np.asarray(v, dtype=np.float64), TR[f'{case}/{name}'][g].astype(np.float64)), (*where, name, v, TR[f'{case}/{name}'][g])
            if g > 0 and fcr is not None:
                n = len(st['cost'])
                assert np.array_equal(np.stack([aux['F'], aux['Cr']]), fcr[:, fcr_at:fcr_at + n]), (*where, 'F / Cr')
                fcr_at += n
            if g in snaps:
                assert np.array_equal(new['pop'], TR[f'{case}/snap{g}/pop']) and np.array_equal(new['cost'], TR[f'{case}/snap{g}/cost']), (*where, 'snapshot')
        if visit is not None:
            visit(ctx, p, g, st, t, action, u, aux, rows[g], wc[g], new, info)
        st = new
    if check:
        assert st['done'] and np.array_equal(st['log'], TR[f'{case}/cost']) and st['fes'] == TR[f'{case}/fes'][-1], case
    return rs


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('case', CASES)
def test_feeder_ends_at_the_recorded_stream_position(case):
    """Over the whole fixture episode the feeder, told the population size and the action by the fixture, draws exactly what the reference drew:
    the next np.random.rand() after the episode is the one the generator recorded."""
    ctx, p, nk, seed, _ = _case(case)
    rs = np.random.RandomState(seed)
    fd = HpTapeFeeder(ctx.D, nk, rs)
    fd.reset_tape()
    n, act = TR[f'{case}/np'], TR[f'{case}/action']
    for g in range(1, len(n)):
        fd.step_tape(int(n[g - 1]), int(act[g]), bool(TR[f'{case}/policy']))
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case):
    """restate_trials / restate_finish chained from the reset with the feeder's tapes and the fixture's trial and walk costs: every recorded quantity
    of every step and every snapshot equal, no tolerance; the host objective at the restated rows is close to the recorded costs; F and Cr equal
    the recorded ones where the fixture holds them; the policy's choice is the recorded action; the stream ends where the reference's did."""
    rs = walk(case)
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_covers_what_it_is_meant_to_pin():
    noisy = {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')}
    assert noisy == {1, 2, 3}                                                                        # every noise kind
    assert sum(c.startswith('bbob/10/') or c.startswith('bbob-noisy/10/') for c in CASES) >= 8 and any(c.startswith('protein/12/') for c in CASES)
    dims = {int(c.split('/')[1]) for c in CASES}
    assert {2, 3, 10, 12} <= dims
    k = [c for c in CASES if c.startswith('bbob/10/5/')][0]                                          # Linear_Slope stops early
    assert TR[f'{k}/fes'][-1] < TR[f'{k}/max_fes'] and TR[f'{k}/gbest'][-1] <= 1e-8 and TR[f'{k}/done'][-1] == 1
    k = [c for c in CASES if c.startswith('bbob/10/15/')][0]                                         # a whole episode at the full budget
    assert TR[f'{k}/max_fes'] == 20000 and TR[f'{k}/fes'][-1] == 20249 and TR[f'{k}/np'][-1] == 3 and len(TR[f'{k}/fes']) - 1 == 70 and len(TR[f'{k}/cost']) == 51
    k = [c for c in CASES if c.startswith('bbob/3/12/')][0]                                          # the reset into state 0, and state 1 later on
    assert TR[f'{k}/state'][0] == 0 and 1 in TR[f'{k}/state']
    assert {int(s) for c in CASES for s in TR[f'{c}/state']} == {0, 1, 2, 3}
    fcr = [c for c in CASES if f'{c}/fcr' in TR]
    assert len(fcr) == 2 and all(TR[f'{c}/fcr'].shape == (2, int(TR[f'{c}/np'][:-1].sum())) for c in fcr)
    seen = {'none_improved': 0, 'neg_F': 0, 'redraw': [0, 0, 0], 'skipped_log': 0, 'acts': set()}

    def visit(ctx, p, g, st, t, action, u, aux, ncost, wcost, new, info):
        if g > 0:
            seen['none_improved'] += info['n_opt'] == 0
            seen['neg_F'] += info['neg_F']
            for c, n in enumerate(info['redraws']):
                seen['redraw'][c] += n
            seen['acts'].add((action, int(np.all(st['MF'] == 0.5))))
            seen['skipped_log'] += int(new['fes'] - st['fes'] > ctx.log_interval)
    for case in CASES:
        walk(case, visit, check=False)
    assert seen['none_improved'] > 0 and seen['neg_F'] > 0 and min(seen['redraw']) > 0 and seen['skipped_log'] > 0, seen
    assert {a for a, fresh in seen['acts'] if fresh} == {0, 1, 2, 3} == {a for a, fresh in seen['acts'] if not fresh}, seen['acts']      # both memories: fresh and updated
    assert all(int(TR[f'{c}/policy']) in (0, 1) for c in CASES) and {int(TR[f'{c}/policy']) for c in CASES} == {0, 1}


def test_update_count_follows_from_the_integer_schedule():
    from metabox_amd.optimizer import RL_HPSDE_Optimizer
    for case in CASES:
        dim, max_fes = int(case.split('/')[1]), int(TR[f'{case}/max_fes'])
        sched = RL_HPSDE_Optimizer.schedule(dim, max_fes)
        fes, n = TR[f'{case}/fes'][1:], TR[f'{case}/np'][1:]
        if TR[f'{case}/gbest'][-1] <= 1e-8 and not case.startswith('protein'):                      # an early stop takes fewer
            sched = sched[:len(fes)]
        assert [f for f, _ in sched] == list(fes) and [m for _, m in sched] == list(n), case
    s = RL_HPSDE_Optimizer.schedule(10, 20000)
    assert len(s) == 70 and s[-1] == (20249, 3)


def test_log_table_is_numpys_log():
    """The kernel takes log(n / 200) from a table of correctly rounded values (extended precision, rounded once); the restatement takes np.log."""
    for n in list(range(1, STEPS)) + [1e-15 * STEPS]:
        x = n / STEPS
        assert np.log(x) == float(np.log(np.longdouble(x))), n


def test_abi_geometry_of_rlhpsde():
    import re
    from metabox_amd import _abi
    lib = _abi.load_lib()
    lib.mbx_last_error.restype = C.c_char_p
    assert _abi.ALGO_RLHPSDE == ALGO_RLHPSDE
    for D in (2, 3, 10, 12, 40):
        cfg = oracle.make_cfg(ALGO_RLHPSDE, 18 * D, D, 20000, 400, NLOG)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1 and lib.mbx_action_dim(C.byref(cfg)) == 1
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
    ok = lambda **kw: lib.mbx_state_dim(C.byref(oracle.make_cfg(ALGO_RLHPSDE, kw.get('np_', 180), kw.get('dim', 10), kw.get('max_fes', 20000), 400, NLOG)))   # noqa: E731
    assert ok() == 1 and ok(max_fes=382) == 1
    for bad in (dict(np_=100), dict(np_=179), dict(np_=18, dim=1), dict(np_=738, dim=41), dict(max_fes=381)):
        assert ok(**bad) < 0 and b'RL-HPSDE' in lib.mbx_last_error(), bad
    for algo in (12, 14, 17, 22, 23):                                # stay unassigned
        assert lib.mbx_state_dim(C.byref(oracle.make_cfg(algo, 180, 10, 20000, 400, NLOG))) < 0
    # the entry point lives in a header of its own: include/mbx_rlhpsde.h declares exactly it, the library exports it, include/mbx.h keeps its 45
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r'\b(mbx_rlhpsde_[a-z_]+)\s*\(', open(os.path.join(root, 'include', 'mbx_rlhpsde.h')).read()))
    assert declared == set(_abi.RLHPSDE_SYMBOLS) == {'mbx_rlhpsde_rollout'} and all(hasattr(lib, n) for n in declared)
    assert not declared & set(_abi.EXPORTED_SYMBOLS) and len(_abi.EXPORTED_SYMBOLS) == 45
    assert 'mbx_rlhpsde' not in open(os.path.join(root, 'include', 'mbx.h')).read().replace('include/mbx_rlhpsde.h', '')
    assert lib.mbx_rlhpsde_rollout(None, None, 1, None, None, None, None, None, None, None, None) < 0 and b'mbx_rlhpsde_rollout' in lib.mbx_last_error()
    assert state_off(10)['end'] == 3 * 180 * 10 + 9 * 180 + 10 + WALK * 11 + 64 + 16 + NLOG + 1


def _agent(max_learning_step=1000, device='cpu'):
    from metabox_amd.agent import RL_HPSDE_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', device, '--max_learning_step', str(max_learning_step)])
    cfg.agent_save_dir = None
    cfg.save_interval = 10 ** 9
    return RL_HPSDE_Agent(cfg), cfg


def test_registered_by_name_and_td_update_is_the_references():
    from metabox_amd import agent, optimizer, tester
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10'])
    opt = tester._lookup(tester._optimizers, 'RL_HPSDE_Optimizer')(cfg)
    assert isinstance(opt, optimizer.RL_HPSDE_Optimizer) and hasattr(opt, 'make_batch')
    assert (cfg.F, cfg.Cr, cfg.NP_max, cfg.NP_min, cfg.Hm, cfg.rw_steps, cfg.step_size) == (0.5, 0.5, 180, 4, 0.5, 200, 10)
    assert tester._lookup(tester._agents, 'RL_HPSDE_Agent') is agent.RL_HPSDE_Agent
    ag, acfg = _agent()
    assert (acfg.n_states, acfg.n_actions, acfg.alpha_max, acfg.alpha_decay, acfg.gamma) == (4, 4, 0.8, False, 0.5)
    assert np.array_equal(ag.load_exported_weights(POL).q_table, Q) and Q.shape == (4, 4)
    # TD(0) on the recorded (s, a, r, s') list of the longest policy case, against the reference's update written out (rl_hpsde_agent.py:45-46)
    k = [c for c in CASES if c.startswith('bbob/10/15/')][0]
    s, a, r = TR[f'{k}/state'], TR[f'{k}/action'], TR[f'{k}/reward']
    ag, _ = _agent()
    q = np.zeros((4, 4))
    for g in range(1, len(s)):
        st, ac, rw, nx = int(s[g - 1]), np.array([int(a[g])]), float(r[g]), int(s[g])
        td = rw + 0.5 * q[nx].max() - q[st][ac]
        q[st][ac] += 0.8 * td
        assert ag.td_update(st, ac, rw, nx) == g
    assert np.array_equal(ag.q_table, q) and ag.learn_steps == len(s) - 1 and np.any(q != 0)


def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


def philox_indices(seed, gen, episode, i, n, cols):
    """The bounded redraw of the Philox route (mbx_rlhpsde.hpp): column by column, one draw and at most TRIES redraws."""
    r = [0, 0, 0]
    for c in range(cols):
        for a in range(TRIES + 1):
            r[c] = (int(oracle.philox(seed, i * 32 + a, SITE_IDX, gen, episode)[c]) * n) >> 32
            if not (r[c] == i or (c > 0 and r[c] == r[0]) or (c > 1 and r[c] == r[1])):
                break
    return r


def test_philox_levy_law_and_bounded_redraw():
    """A host mirror of the Philox Levy draw, x = 1 / s^2 with s the sine half of the Box-Muller pair, has the quartiles of scipy.stats.levy within
    binomial 5 sigma for the sample size used; the bounded index redraw stays uniform over the admissible values at NP = 4 and NP = 7."""
    from scipy import stats
    N = 4000
    x = np.empty(N)
    for i in range(N):
        w = oracle.philox(12345, i, SITE_NORM, 3, 1)
        s = np.sqrt(-2.0 * np.log(1.0 - _u53(int(w[0]), int(w[1])))) * np.sin(2 * np.pi * _u53(int(w[2]), int(w[3])))
        x[i] = 1. / (s * s)
    for q in (0.25, 0.5, 0.75):
        below = np.sum(x < stats.levy.ppf(q))
        assert abs(below - N * q) <= 5 * np.sqrt(N * q * (1 - q)), (q, below)
    for n in (4, 7):
        rows = 600
        counts = np.zeros((3, n, n))
        for i in range(rows):
            r = philox_indices(99, 5, 1, i % n, n, 3) if i < n else philox_indices(99 + i // n, 5, 1, i % n, n, 3)
            assert len({i % n, *r}) == 4, (n, i, r)                     # distinct and not the row itself
            for c in range(3):
                counts[c, i % n, r[c]] += 1
        per = rows / n
        for c in range(3):
            for row in range(n):
                q = 1 / (n - 1)
                assert counts[c, row, row] == 0
                assert np.all(np.abs(np.delete(counts[c, row], row) - per * q) <= 5 * np.sqrt(per * q * (1 - q))), (n, c, row, counts[c, row])


# ------------------------------------------------------------------------------------------------ GPU
def _batch(ps, idx, seeds, D, max_fes, nlog=NLOG, early_stop=True):
    from metabox_amd.suite import Batch, Suite
    return Batch(Suite(ps), ALGO_RLHPSDE, idx, seeds, 18 * D, max_fes, max_fes // nlog, nlog, early_stop=early_stop)


def _three_way(b, idx, ctx, st, t, action, u_want, aux, ref_ncost, ref_wcost, where, want_state=None):
    """(A) / (B) / (C) for one instance after its step from state `st` with tape `t` (module docstring)."""
    D = ctx.D
    got = from_block(b.read_state(idx), D, ctx.nlog)
    n = len(st['cost'])
    assert np.array_equal(got['u'][:n], u_want), (*where, 'A: trial rows', int(np.sum(got['u'][:n] != u_want)))
    assert np.array_equal(got['F'][:n], aux['F']) and np.array_equal(got['Cr'][:n], aux['Cr']), (*where, 'A: F / Cr')
    assert np.array_equal(got['ridx'][:n], aux['ridx']), (*where, 'A: indices')
    dev, wdev = got['ncost'][:n], got['wcost']
    if ref_ncost is not None:
        assert close(dev, ref_ncost), (*where, 'B: trial costs', np.abs(dev - ref_ncost).max())
        assert close(wdev, ref_wcost), (*where, 'B: walk costs', np.abs(wdev - ref_wcost).max())
    want, info = restate_finish(ctx, st, t, aux, got['u'][:n], dev, wdev)
    assert got['live'] == 1 and got['scalars'][SC_GEN] == where[-1] and got['action'] == action and got['n_opt'] == info['n_opt'], where
    bad = same_state(got, want)
    assert bad is None, (*where, 'C: state after', bad, got[bad], want[bad])
    assert got['ret'] == want['ret'] and float(b.reward[idx].item()) == info['reward'] and int(b.state[idx, 0].item()) == want['state'], (*where, 'C: outputs')
    assert bool(b.done[idx].item()) == want['done'], (*where, 'C: done')
    if want_state is not None:
        assert want['state'] == want_state, (*where, 'the state the reference recorded', want['state'], want_state, want['r'], want['H'])
    return got, want, info


def _step_states(b, ctx, items):
    """items: [(where, state before, tape, action, u, aux, reference ncost, reference wcost, recorded state)], at most b.B of them, stepped as the
    instances of one launch."""
    import torch
    tape = torch.zeros(b.B, b.tape_stride, dtype=torch.float64)
    acts = torch.zeros(b.B, dtype=torch.int32)
    for i, (where, st, t, action, u, aux, ref, wref, rec_state) in enumerate(items):
        b.write_state(i, to_block(st, ctx.D, gen=where[-1] - 1, nlog=ctx.nlog))
        tape[i] = torch.from_numpy(t)
        acts[i] = action
    for i in range(len(items), b.B):                                 # idle instances of the launch: frozen
        blk = b.read_state(i)
        blk[state_off(ctx.D, ctx.nlog)['scalars'] + SC_DONE] = 1.
        b.write_state(i, blk)
    b.set_tape(tape.cuda())
    b.step(acts.cuda())
    torch.cuda.synchronize()
    return [_three_way(b, i, ctx, st, t, action, u, aux, ref, wref, where, rec_state) for i, (where, st, t, action, u, aux, ref, wref, rec_state) in enumerate(items)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_rlhpsde_every_update_from_the_reference_state(case):
    """Every update of every fixture episode, one at a time from the restated (= the reference's) state before it, the updates of an episode stepped
    as the instances of one batch: (A) trial rows, F, Cr, indices bit for bit; (B) trial and walk costs close to the reference's; (C) the state after
    bit for bit against the restatement fed the device's costs, and the landscape state the one the reference recorded.  The reset likewise (u = the
    initial rows), the reset into state 0 at D = 3 included.  No mismatch budget, no update skipped."""
    import torch
    ctx, p, nk, seed, protein = _case(case)
    dim, max_fes = ctx.D, ctx.max_fes
    items = []

    def visit(ctx_, p_, g, st, t, action, u, aux, ncost, wcost, new, info):
        items.append(((case, g), st, t, action, u, aux, ncost, wcost, int(TR[f'{case}/state'][g])))
    walk(case, visit, check=False)
    # the reset: a batch of one, the tape's rows and the device's own costs
    where, _, t, _, u, _, ncost, wcost, rec_state = items[0]
    b1 = _batch([p], [0], [seed], dim, max_fes, ctx.nlog)
    assert (b1.state_dim, b1.action_dim, b1.tape_stride) == (1, 1, tape_stride(dim))
    b1.set_tape(torch.from_numpy(t).cuda().reshape(1, -1))
    st0 = b1.reset()
    torch.cuda.synchronize()
    got = from_block(b1.read_state(0), dim, ctx.nlog)
    assert np.array_equal(got['u'], u), (*where, 'A: initial rows')
    assert close(got['ncost'], ncost) and close(got['wcost'], wcost), (*where, 'B: initial and walk costs')
    _, want = restate_reset(ctx, t, got['ncost'], got['wcost'])
    assert got['live'] == 0 and same_state(got, want) is None, (*where, 'C', same_state(got, want))
    assert int(st0[0, 0].item()) == want['state'] == rec_state, (*where, 'state', want['state'], rec_state)
    b1.close()
    # the updates
    steps = items[1:]
    per = min(len(steps), 64)
    b = _batch([p], [0] * per, [seed] * per, dim, max_fes, ctx.nlog)
    b.reset()
    count = 0
    for c0 in range(0, len(steps), per):
        _step_states(b, ctx, steps[c0:c0 + per])
        count += len(steps[c0:c0 + per])
    b.close()
    assert count == len(TR[f'{case}/fes']) - 1                       # no update skipped
    print(f'{case}: reset + {count} updates')


# ------------------------------------------------------------------------------------------------ GPU: crafted states
def _state_of(b, D, nlog):
    st = from_block(b.read_state(0), D, nlog)
    return {k: st[k] for k in ('pop', 'cost', 'MF', 'MCr', 'k', 'fes', 'gbest', 'log_index', 'log', 'done', 'state', 'ret')}


def _crafted(D=10, max_fes=20000, seed=7, fid=1, suite='bbob'):
    """A batch of one instance without the early stop, the restated state after a tape reset, a feeder that continues the stream, and the context."""
    import torch
    protein = suite == 'protein'
    p, nk = _problem(suite, D, fid)
    ctx = Ctx(D, p.lb, p.ub, max_fes, not protein, early_stop=False, nlog=5 if protein else NLOG)
    b = _batch([p], [0], [seed], D, max_fes, ctx.nlog, early_stop=False)
    fd = HpTapeFeeder(D, nk, np.random.RandomState(seed))
    b.set_tape(torch.from_numpy(fd.reset_tape()).cuda().reshape(1, -1))
    b.reset()
    torch.cuda.synchronize()
    return b, ctx, fd, _state_of(b, D, ctx.nlog), p, protein


def _run_crafted(b, ctx, p, protein, st, t, action, gen=9):
    """One update of instance 0 from the crafted state: (A) and (C) against the restatement, (B) against the host objective at the device's rows."""
    import torch
    D = ctx.D
    b.write_state(0, to_block(st, D, gen=gen - 1, nlog=ctx.nlog))
    b.set_tape(torch.from_numpy(t).cuda().reshape(1, -1))
    b.step(torch.tensor([action], dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    u, aux = restate_trials(ctx, st, t, action)
    got, want, info = _three_way(b, 0, ctx, st, t, action, u, aux, None, None, ('crafted', gen))
    n, o = len(st['cost']), tape_off(D)
    assert close(got['ncost'][:n], host_costs(p, protein, got['u'][:n], t, o['noise'], geom(D)[0])), 'B: trial costs against the host objective'
    assert close(got['wcost'], host_costs(p, protein, got['walk'], t, o['wnoise'], WALK)), 'B: walk costs against the host objective'
    return got, want, info, aux


@pytest.mark.gpu
def test_hip_rlhpsde_crafted_states():
    """Equal costs sort in row order; NP = 4 with both mutations; a last step that leaves NP = 3 and whose walk is still billed; a step with no
    improvement; a weighted sum not above 1e-6; F reflected and still negative -- one update each against the restatement."""
    b, ctx, fd, st, p, protein = _crafted()
    D, o = ctx.D, tape_off(ctx.D)
    # equal costs of different rows, below every trial cost: they keep their order
    s = copy.deepcopy(st)
    s['cost'][:3] = -1e300
    got, want, info, _ = _run_crafted(b, ctx, p, protein, s, fd.step_tape(len(s['cost']), 0, False), 0)
    assert np.array_equal(got['pop'][:3], s['pop'][:3]) and np.all(got['cost'][:3] == -1e300) and not np.array_equal(s['pop'][0], s['pop'][1])
    # ... and among the rows in the middle of the order
    s = copy.deepcopy(st)
    s['cost'][:] = -np.arange(len(s['cost']), 0, -1, dtype=np.float64) - 1e6
    s['cost'][40:44] = s['cost'][40]
    got, want, info, _ = _run_crafted(b, ctx, p, protein, s, fd.step_tape(len(s['cost']), 3, False), 3)
    assert info['n_opt'] == 0 and len(got['pop']) < len(s['pop']) and np.array_equal(got['pop'], s['pop'][:len(got['pop'])]) and got['k'] == s['k'] and got['MF'][s['k']] == 0.5 and got['MCr'][s['k']] == 0.5   # no improvement
    assert float(b.reward[0].item()) == 0.
    # NP = 4, both mutations; then the last step, which leaves NP = 3 and still bills its walk
    for action in (0, 1, 2, 3):
        s = copy.deepcopy(st)
        s.update(pop=st['pop'][:4].copy(), cost=st['cost'][:4].copy(), fes=19000)
        got, want, info, aux = _run_crafted(b, ctx, p, protein, s, fd.step_tape(4, action, False), action)
        assert len(got['cost']) == 4 and not got['done'] and got['fes'] == 19000 + 4 + WALK
        assert all(len({i, *aux['ridx'][i][:2 if action & 1 else 3]}) == (3 if action & 1 else 4) for i in range(4))
    s.update(fes=ctx.max_fes - 2)
    got, want, info, _ = _run_crafted(b, ctx, p, protein, s, fd.step_tape(4, 1, False), 1)
    assert len(got['cost']) == 3 and got['done'] and got['fes'] == ctx.max_fes + 2 + WALK and bool(b.done[0].item())
    # every row improves with Cr = 0: sum(w Cr) = 0 <= 1e-6 gives MCr[k] = 0.5, MF[k] is a Lehmer mean, k advances
    s = copy.deepcopy(st)
    s['cost'][:] = 1e300
    t = fd.step_tape(len(s['cost']), 0, False)
    t[o['z']:o['z'] + len(s['cost'])] = -100.
    got, want, info, aux = _run_crafted(b, ctx, p, protein, s, t, 0)
    assert info['n_opt'] == len(s['cost']) and np.all(aux['Cr'] == 0) and got['MCr'][0] == 0.5 and got['MF'][0] != 0.5 and got['k'] == 1
    assert float(b.reward[0].item()) == 1.
    # F reflected and still negative: a negative location
    s = copy.deepcopy(st)
    s['MF'][:] = -0.3
    t = fd.step_tape(len(s['cost']), 1, False)
    t[o['x']:o['x'] + len(s['cost'])] = -1.
    got, want, info, aux = _run_crafted(b, ctx, p, protein, s, t, 1)
    assert np.all(aux['F'] < 0) and np.all(aux['F'] == 2 * -0.3 - (-1. * 0.1 + -0.3))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('suite,D,fid', [('bbob', 40, 15), ('protein', 12, '1ATN_7'), ('bbob-noisy', 10, 128)])
def test_hip_rlhpsde_one_update_at_other_geometries(suite, D, fid):
    """D = 40 (720 rows, three per thread), the protein instance and a noisy function: the reset and one update per action against the restatement."""
    b, ctx, fd, st, p, protein = _crafted(D=D, max_fes=1500 if suite == 'protein' else 2000 * D, seed=11, fid=fid, suite=suite)
    for action in (0, 3):
        got, want, info, _ = _run_crafted(b, ctx, p, protein, st, fd.step_tape(len(st['cost']), action, False), action, gen=1)
    b.close()


# ------------------------------------------------------------------------------------------------ GPU: routes
def _routes(D, n, fids, max_fes, suite='bbob'):
    import torch
    ps = [problems(suite, D)[f] for f in fids]
    B = len(ps)
    idx, seeds = np.arange(B), np.arange(B, dtype=np.uint64) * 7 + 3
    q = torch.from_numpy(Q).cuda()
    one = _batch(ps, idx, seeds, D, max_fes)
    one.reset()
    acts, states, rewards = [], [], []
    for g in range(n):
        s, r, d, a, traj = one.rlhpsde_rollout(q, 1, trajectory=True)
        acts.append(traj['actions'][0].clone()); states.append(s[:, 0].clone()); rewards.append(r.clone())
    torch.cuda.synchronize()
    blocks, res = [one.read_state(i) for i in range(B)], one.results()
    ret = torch.zeros_like(rewards[0])
    for r_ in rewards:                                               # the kernel's own order: one after another from zero
        ret = ret + r_

    def same(b, who):
        torch.cuda.synchronize()
        for i in range(B):
            assert np.array_equal(b.read_state(i), blocks[i]), (who, i)
        r2 = b.results()
        for k in res:
            assert torch.equal(r2[k], res[k]), (who, k)
        assert torch.equal(b.state, one.state) and torch.equal(b.done, one.done), who
    multi = _batch(ps, idx, seeds, D, max_fes)
    multi.reset()
    s, r, d, a, traj = multi.rlhpsde_rollout(q, n, trajectory=True)
    same(multi, 'one n-step rollout')
    alive = torch.stack(acts) >= 0
    assert torch.equal(traj['actions'], torch.stack(acts)) and torch.equal(traj['state'][alive], torch.stack(states)[alive]) and torch.equal(r, ret)
    multi.close()
    st = _batch(ps, idx, seeds, D, max_fes)
    st.reset()
    for g in range(n):
        st.step(torch.where(acts[g] < 0, torch.zeros_like(acts[g]), acts[g]).contiguous())
    same(st, 'mbx_step')
    st.close()
    return one, ps, idx, seeds, q, blocks


@pytest.mark.gpu
def test_hip_rlhpsde_routes_are_bit_identical():
    """n one-step rollouts == one n-step rollout == mbx_step fed the recorded actions: state blocks, states, rewards and curves, at D = 10 (n = 5) and at
    D = 2 (n = 12, the population shrinks inside the launch); then the D = 2 batch runs to the end and stays frozen; an instance alone equals the same
    instance in a batch of 7 mixed functions."""
    import torch
    one, ps, idx, seeds, q, blocks = _routes(10, 5, (1, 8, 15, 21), 20000)
    # batch invariance: instance 2 alone, and in a batch of 7 mixed functions
    alone = _batch([ps[2]], [0], [seeds[2]], 10, 20000)
    alone.reset()
    alone.rlhpsde_rollout(q, 5)
    torch.cuda.synchronize()
    assert np.array_equal(alone.read_state(0), blocks[2])
    alone.close()
    seven = [problems('bbob', 10)[f] for f in (3, 5, 15, 7, 22, 24, 12)]
    mixed = _batch(seven, np.arange(7), [11, 12, int(seeds[2]), 14, 15, 16, 17], 10, 20000)
    mixed.reset()
    mixed.rlhpsde_rollout(q, 5)
    torch.cuda.synchronize()
    assert np.array_equal(mixed.read_state(2), blocks[2])
    mixed.close(); one.close()
    one, ps, idx, seeds, q, blocks = _routes(2, 12, (3, 15, 24), 3000)
    nps = [from_block(b_, 2)['cost'].shape[0] for b_ in blocks]
    assert max(nps) < 36, nps                                         # the population shrank inside the launch
    for _ in range(4):
        one.rlhpsde_rollout(q, 8)
    torch.cuda.synchronize()
    assert bool(one.done.all())
    frozen = [one.read_state(i) for i in range(3)]
    state = one.state.clone()
    _, r, d, _ = one.rlhpsde_rollout(q, 3)
    assert bool(d.all()) and bool((r == 0).all()) and torch.equal(one.state, state)
    _, r, d = one.step(torch.zeros(3, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert bool(d.all()) and bool((r == 0).all()) and torch.equal(one.state, state) and all(np.array_equal(one.read_state(i), frozen[i]) for i in range(3))
    for i in range(3):                                                # the integer schedule: fes, steps and the final NP
        got = from_block(frozen[i], 2)
        from metabox_amd.optimizer import RL_HPSDE_Optimizer
        sched = RL_HPSDE_Optimizer.schedule(2, 3000)
        assert got['fes'] == sched[-1][0] and int(got['scalars'][SC_GEN]) == len(sched) and len(got['cost']) == sched[-1][1], (i, got['fes'], sched[-1])
    one.close()


EP0 = 0          # the Philox episode word of a fresh batch's first reset (the counter starts at -1)


def philox_walk(t, seed, gen, episode, D):
    o = tape_off(D)
    for d in range(D):
        w = oracle.philox(seed, d, SITE_WALK, gen, episode)
        t[o['zone'] + d], t[o['off'] + d] = _u53(int(w[0]), int(w[1])), _u53(int(w[2]), int(w[3]))
    for k in range(STEPS * D):
        w = oracle.philox(seed, D + k, SITE_WALK, gen, episode)
        t[o['stepu'] + k] = _u53(int(w[0]), int(w[1]))
    t[o['rd']] = (int(oracle.philox(seed, WALK * D, SITE_WALK, gen, episode)[0]) * D) >> 32


@pytest.mark.gpu
def test_hip_rlhpsde_philox_route_equals_the_rebuilt_tape():
    """A batch stepped from Philox and one stepped from tapes rebuilt on the host with oracle.philox and the documented sites leave the same blocks.  The
    standard normal behind Cr and the Cauchy / Levy variate behind F go through the device's log, cos, sin and tan: the tape takes them from the state
    block of the Philox run, and the host mirror must agree with them to 1e-12 relative."""
    import torch
    D, seed, steps = 3, 77, 4
    n0, h = geom(D)
    o = tape_off(D)
    p = problems('bbob', D)[12]
    a, b = _batch([p], [0], [seed], D, 3000), _batch([p], [0], [seed], D, 3000)
    q = torch.from_numpy(np.array([[0., 1., 2., 3.], [3., 2., 1., 0.], [0., 0., 0., 0.], [1., 0., 1., 0.]])).cuda()
    t = np.zeros(tape_stride(D))
    for e in range(n0 * D):
        w = oracle.philox(seed, e, SITE_CROSS, 0, EP0)
        t[o['pos'] + e] = _u53(int(w[0]), int(w[1]))
    philox_walk(t, seed, 0, EP0, D)
    b.set_tape(torch.from_numpy(t[None]).cuda())
    a.reset(); b.reset()
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and np.array_equal(a.read_state(0), b.read_state(0))
    seen = set()
    for g in range(1, steps + 1):
        before = from_block(a.read_state(0), D)
        n = len(before['cost'])
        _, _, _, act = a.rlhpsde_rollout(q, 1)
        torch.cuda.synchronize()
        after = from_block(a.read_state(0), D)
        action = int(act[0].item())
        seen.add(action)
        t = np.zeros(tape_stride(D))
        w = oracle.philox(seed, 0, SITE_POLICY, g, EP0)
        t[o['choice']] = _u53(int(w[0]), int(w[1]))
        assert choose(q.cpu().numpy()[before['state']], t[o['choice']]) == action
        for i in range(n):
            w = oracle.philox(seed, i, SITE_PAR, g, EP0)
            t[o['mem'] + i], t[o['jrand'] + i] = (int(w[0]) * h) >> 32, (int(w[1]) * D) >> 32
            t[o['r'] + 3 * i:o['r'] + 3 * i + 3] = philox_indices(seed, g, EP0, i, n, 2 if action & 1 else 3)
            w = oracle.philox(seed, i, SITE_NORM, g, EP0)
            rad, ang = np.sqrt(-2.0 * np.log(1.0 - _u53(int(w[0]), int(w[1])))), 2 * np.pi * _u53(int(w[2]), int(w[3]))
            z, sn = rad * np.cos(ang), rad * np.sin(ang)
            if action >> 1:
                x = 1. / (sn * sn)
            else:
                w = oracle.philox(seed, i, SITE_CAUCHY, g, EP0)
                x = np.tan(np.pi * (_u53(int(w[0]), int(w[1])) - 0.5))
            assert abs(z - after['z'][i]) <= 1e-12 * max(1., abs(z)) and abs(x - after['x'][i]) <= 1e-9 * abs(x), (g, i, z, after['z'][i], x, after['x'][i])
            for d in range(D):
                w = oracle.philox(seed, i * D + d, SITE_CROSS, g, EP0)
                t[o['cross'] + i * D + d] = _u53(int(w[0]), int(w[1]))
        t[o['z']:o['z'] + n], t[o['x']:o['x'] + n] = after['z'][:n], after['x'][:n]
        philox_walk(t, seed, g, EP0, D)
        b.set_tape(torch.from_numpy(t[None]).cuda())
        b.rlhpsde_rollout(q, 1)
        torch.cuda.synchronize()
        assert np.array_equal(a.read_state(0), b.read_state(0)) and torch.equal(a.state, b.state), g
    assert len(seen) >= 2, seen
    a.close(); b.close()


@pytest.mark.gpu
def test_hip_rlhpsde_refuses_a_rollout_without_a_table():
    from metabox_amd import _abi
    p = problems('bbob', 10)[1]
    b = _batch([p], [0], [1], 10, 20000)
    b.reset()
    rc = b.lib.mbx_rlhpsde_rollout(b._h, None, 1, None, None, None, None, None, None, None, None)
    assert rc < 0 and b'Q-table' in b.lib.mbx_last_error()
    with pytest.raises(_abi.MbxError):
        _abi.check(b.lib.mbx_rlhpsde_rollout(b._h, None, 1, None, None, None, None, None, None, None, None))
    b.close()


# ------------------------------------------------------------------------------------------------ GPU: whole episodes
def mann_whitney_p(x, y):
    from scipy import stats
    return float(stats.mannwhitneyu(x, y, alternative='two-sided').pvalue)


@pytest.mark.gpu
def test_hip_rlhpsde_free_running_episodes_match_the_reference_in_distribution():
    """Whole episodes of rollout_batch with the shipped Q-table on three functions, as many runs as the fixture holds of the reference (32 each): a
    two-sided Mann-Whitney test on the final costs must not reject at p = 0.001, and every episode's fes, step count and final NP are the integer
    schedule's.  (The numpy restatement of this file, run free under seeds other than the reference's with the host objective, passes the same test on the CPU:
    docs/EXPERIMENTS.md.)"""
    from metabox_amd.config import get_config
    from metabox_amd.environment import BatchedPBO_Env
    from metabox_amd.optimizer import RL_HPSDE_Optimizer
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    cfg.agent_save_dir = None
    agent, _ = _agent(device='cuda')
    agent.load_exported_weights(POL)
    fids = (8, 15, 21)
    runs = len(TR['finals/bbob/10/8'])
    assert runs >= 32
    pb = [problems('bbob', 10)[f] for f in fids]
    env = BatchedPBO_Env(pb, RL_HPSDE_Optimizer(copy.deepcopy(cfg)), np.repeat(np.arange(3), runs), np.arange(3 * runs, dtype=np.uint64) + 1000)
    out = agent.rollout_batch(env)
    sched = RL_HPSDE_Optimizer.schedule(10, 20000)
    assert bool((out['fes'] == sched[-1][0]).all()) and bool((out['steps'] == len(sched)).all()) and bool((out['cost_len'] == 51).all())
    nps = [int(env.batch.read_state(i)[state_off(10)['scalars'] + SC_NP]) for i in range(3 * runs)]
    assert set(nps) == {sched[-1][1]}
    final = out['cost'][:, -1].cpu().numpy()
    env.close()
    for k, f in enumerate(fids):
        ref = TR[f'finals/bbob/10/{f}']
        assert np.all(ref[:, 1] == sched[-1][0]) and np.all(ref[:, 2] == len(sched)) and np.all(ref[:, 3] == sched[-1][1])
        pv = mann_whitney_p(final[k * runs:(k + 1) * runs], ref[:, 0])
        print(f'F{f}: median {np.median(final[k * runs:(k + 1) * runs]):.4g} against the reference\'s {np.median(ref[:, 0]):.4g}, p = {pv:.3g}')
        assert pv >= 0.001, (f, pv)


@pytest.mark.gpu
def test_rlhpsde_in_the_harness(tmp_path):
    """RL_HPSDE_Agent.rollout_batch through the Tester, which writes a test.pkl with the pair's rows; the B = 1 protocol view steps an episode to done
    with the reference's fes."""
    import pickle
    from metabox_amd.agent.utils import save_class
    from metabox_amd.config import get_config
    from metabox_amd.environment import PBO_Env
    from metabox_amd.optimizer import RL_HPSDE_Optimizer
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    cfg.agent_save_dir = None
    agent, _ = _agent(device='cuda')
    agent.load_exported_weights(POL)
    np.random.seed(4)
    info = agent.to('cuda').rollout_episode(PBO_Env(problems('bbob', 10)[15], RL_HPSDE_Optimizer(copy.deepcopy(cfg))))
    assert info['fes'] == 20249 and len(info['cost']) == 51 and info['cost'][0] >= info['cost'][-1] and 0 < info['return'] <= 70
    load_dir = str(tmp_path / 'models') + '/'
    save_class(load_dir, 'RL_HPSDE_Agent', agent)
    tcfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--log_dir', str(tmp_path / 'out'), '--agent_load_dir', load_dir, '--test_runs', '2',
                       '--test', '--agent_for_cp', 'RL_HPSDE_Agent', '--l_optimizer_for_cp', 'RL_HPSDE_Optimizer'])
    tcfg.maxFEs, tcfg.log_interval = 4000, 80
    t = Tester(tcfg)
    assert t.skipped == []
    res = t.test()
    for prob, rows in res['cost'].items():
        assert len(rows['RL_HPSDE_Agent']) == 2 and all(len(r) == 51 and r[0] >= r[-1] for r in rows['RL_HPSDE_Agent']), prob
        assert all(v <= 4000 + 180 + WALK for v in res['fes'][prob]['RL_HPSDE_Agent']), prob
    pkls = glob.glob(os.path.join(str(tmp_path / 'out'), '**', 'test.pkl'), recursive=True)
    assert len(pkls) == 1
    with open(pkls[0], 'rb') as f:
        saved = pickle.load(f)
    assert all('RL_HPSDE_Agent' in saved['cost'][prob] for prob in res['cost'])
    learner, lcfg = _agent(3, 'cuda')
    np.random.seed(2)
    done, info = learner.train_episode(PBO_Env(problems('bbob', 10)[16], RL_HPSDE_Optimizer(copy.deepcopy(cfg))))
    assert done and info['learn_steps'] == 3 and np.any(learner.q_table != 0)
