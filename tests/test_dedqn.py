"""DEDQN (src/optimizer/dedqn_optimizer.py, src/agent/dedqn_agent.py): the HIP kernels of metabox_amd/csrc/mbx_dedqn.hpp against seeded
reference episodes (tests/golden/dedqn_traces*.npz, dedqn_policy.npz, dedqn_train.npz; tools/gen_golden.py dedqn).

The chain to the reference is closed on the CPU: a numpy restatement of one update() and of the four landscape features, fed the
REFERENCE's recorded trial costs and samples_cost and a walk regenerated from the seed, reproduces every recorded state, reward and
snapshot bit for bit (no tolerance), and the feeder ends every episode at the stream position the generator recorded.
On the GPU the kernels replay the same episodes from the same tapes with the recorded actions.  Their objective values agree with
numpy's to helpers.RTOL / ATOL, not to the bit, so
  - everything that is a decision (selection, survival, reward, fes, done, pointer, curve length, nop, the ruggedness transition counts)
    must be exact -- the generator asserted margins that make the feature decisions safe; a selection that differs must be a proven
    near tie (helpers.prove_tie_arrays), after which that episode is a different, equally valid trajectory and is not compared further;
  - the kernel's arithmetic is isolated by feeding the restatement the KERNEL's own samples_cost (read back from the state block):
    fdc / acf / rie may then differ from an extended-precision evaluation of the same expressions by at most 4x the float64
    restatement's own error plus 4 ulp of the result;
  - against the reference's recorded states fdc / acf must be inside helpers' cost tolerance propagated through the expressions'
    own first derivatives (`_sensitivity`), and the kernel's own rie and nop equal to the recorded ones, bit for bit (the kernel takes the
    logarithm of a frequency n / NP from a table of correctly rounded values, which numpy's log matches at NP = 100: `entropies_cr`).
What the fixture does NOT pin against the reference: a noisy function redraws every cost at every step, so no 99-step noisy episode meets
the generator's ruggedness margins at every step; the three noisy cases run a budget of 2000 FEs (9 steps each).  Beyond those steps noisy
behaviour is covered kernel against kernel only (the route-equivalence test on a mixed bbob + bbob-noisy suite, and the crafted noisy state).
The numpy draws are not stored: DedqnTapeFeeder regenerates them in the reference's draw order (include/mbx_layout.h §14).
Measured figures are in docs/EXPERIMENTS.md."""
import copy
import ctypes as C
import functools
import glob
import os
import pickle

import numpy as np
import pytest

from helpers import ATOL, GOLDEN, RTOL, close, load, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'dedqn_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
CASES = [str(c) for c in TR['cases']]
POL = load('dedqn_policy.npz')
TRAIN = load('dedqn_train.npz')
ALGO_DEDQN, NP0, F, CR = 16, 100, 0.5, 0.5
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE, SC_POINTER, SC_G0, SC_ALIAS = 0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12
FEAT_LEVEL, FEAT_COUNTS, FEAT_UCOST, FEAT_Q, FEAT_SLOTS = 4, 5, 11, 12, 16
SITE_LDE_ELEM, SITE_DQ_JRAND, SITE_DD_R, SITE_DD_WALK = 12, 14, 38, 39


# ------------------------------------------------------------------------------------------------ layout (include/mbx_layout.h §14)
def state_off(NP, D, nlog):
    o, p = {}, 0
    for k, n in (('pop', NP * D), ('cost', NP), ('surv', NP), ('scost', NP), ('gpos', D), ('feat', FEAT_SLOTS), ('scalars', 16), ('log', nlog + 1)):
        o[k] = p
        p += n
    o['end'] = p
    return o


def tape_stride(NP, D):
    return 2 * NP * D + 6 * NP + 8


def step_off(NP, D):
    return {'r': 0, 'jrand': 4, 'noise': 5, 'cross': 8, 'walk': 8 + D, 'nfeat': 8 + D + NP * D}


def reset_off(NP, D):
    return {'pos': 0, 'noise': NP * D, 'walk': NP * D + 3 * NP, 'nfeat': 2 * NP * D + 3 * NP}


class Ctx:
    def __init__(self, NP, D, lb, ub, max_fes, has_opt, nlog=50, early_stop=True):
        self.NP, self.D, self.lb, self.ub, self.max_fes, self.has_opt, self.nlog, self.early_stop = NP, D, lb, ub, int(max_fes), has_opt, nlog, early_stop
        self.log_interval = self.max_fes // nlog


def to_block(st, ctx, gen=0, episode=1):
    o = state_off(ctx.NP, ctx.D, ctx.nlog)
    b = np.zeros(o['end'])
    b[o['pop']:o['cost']] = st['pop'].ravel()
    b[o['cost']:o['surv']], b[o['surv']:o['scost']], b[o['scost']:o['gpos']] = st['cost'], st['surv'], st['scost']
    b[o['gpos']:o['feat']] = st['pop'][st['g0']] if st['alias'] else st['gpos']
    b[o['feat']:o['feat'] + 4] = st['feat']
    sc = b[o['scalars']:o['log']]
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE], sc[SC_GEN], sc[SC_EPISODE] = st['gbest'], st['fes'], st['log_index'], len(st['log']), float(st['done']), gen, episode
    sc[SC_POINTER], sc[SC_G0], sc[SC_ALIAS] = st['pointer'], st['g0'], float(st['alias'])
    b[o['log']:o['log'] + len(st['log'])] = st['log']
    return b


def from_block(b, ctx):
    NP, D = ctx.NP, ctx.D
    o = state_off(NP, D, ctx.nlog)
    sc = b[o['scalars']:o['log']]
    feat = b[o['feat']:o['scalars']]
    return {'pop': b[o['pop']:o['cost']].reshape(NP, D).copy(), 'cost': b[o['cost']:o['surv']].copy(), 'surv': b[o['surv']:o['scost']].copy(),
            'scost': b[o['scost']:o['gpos']].copy(), 'gpos': b[o['gpos']:o['feat']].copy(), 'feat': feat[:4].copy(), 'level': int(feat[FEAT_LEVEL]),
            'counts': feat[FEAT_COUNTS:FEAT_COUNTS + 6].astype(int), 'ucost': feat[FEAT_UCOST], 'q': feat[FEAT_Q:FEAT_Q + 3].copy(),
            'gbest': sc[SC_GBEST], 'fes': int(sc[SC_FES]), 'log_index': int(sc[SC_LOG_INDEX]), 'log': list(b[o['log']:o['log'] + int(sc[SC_COST_LEN])]),
            'done': bool(sc[SC_DONE]), 'pointer': int(sc[SC_POINTER]), 'g0': int(sc[SC_G0]), 'alias': bool(sc[SC_ALIAS]), 'gen': int(sc[SC_GEN]),
            'ret': sc[SC_RETURN]}


STATE_KEYS = ('pop', 'cost', 'surv', 'gpos', 'gbest', 'fes', 'log_index', 'log', 'done', 'pointer', 'alias')


def same_state(a, b):
    """The first field in which two states differ, or None (gpos: the position gbest names, through the view or not)."""
    for k in STATE_KEYS:
        x, y = ((s['pop'][s['g0']] if s['alias'] else s['gpos']) for s in (a, b)) if k == 'gpos' else (a[k], b[k])
        if not np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)):
            return k
    return None


# ------------------------------------------------------------------------------------------------ the reference's draws as tapes
class DedqnTapeFeeder:
    """numpy's legacy stream as DEDQN consumes it: init_population (:145-156) and update (:159-206) with __cal_feature's walk and
    evaluation behind each.  All draws go through one RandomState (legacy `randn` keeps a spare Gaussian between calls)."""

    def __init__(self, NP, D, noise_kind, rs):
        self.NP, self.D, self.noise, self.rs = NP, D, noise_kind, rs
        self.attempts = 0

    def _noise(self, t, n, base):
        r = self.rs
        if self.noise == 1:
            t[base:base + n] = r.randn(n)
        elif self.noise == 2:
            t[base:base + n] = r.rand(n)
            t[base + n:base + 2 * n] = r.rand(n)
        elif self.noise == 3:
            t[base:base + n] = r.rand(n)
            t[base + n:base + 2 * n] = r.randn(n)
            t[base + 2 * n:base + 3 * n] = r.randn(n)

    def reset_tape(self):
        NP, D = self.NP, self.D
        o = reset_off(NP, D)
        t = np.zeros(tape_stride(NP, D))
        t[:NP * D] = self.rs.rand(NP, D).ravel()
        self._noise(t, NP, o['noise'])
        t[o['walk']:o['walk'] + NP * D] = self.rs.rand(NP, D).ravel()       # rand(dim), NP times
        self._noise(t, NP, o['nfeat'])
        return t

    def step_tape(self, action, pointer):
        NP, D = self.NP, self.D
        o = step_off(NP, D)
        t = np.zeros(tape_stride(NP, D))
        cols = 3 if action in (0, 1) else 4
        r = self.rs.randint(low=0, high=NP, size=cols)
        self.attempts = 1
        while pointer in r:
            r = self.rs.randint(low=0, high=NP, size=cols)
            self.attempts += 1
        t[:cols] = r
        t[o['jrand']] = self.rs.randint(D, size=1)[0]
        t[o['cross']:o['cross'] + D] = self.rs.rand(1, D)[0]
        self._noise(t, 1, o['noise'])
        t[o['walk']:o['walk'] + NP * D] = self.rs.rand(NP, D).ravel()
        self._noise(t, NP, o['nfeat'])
        return t


# ------------------------------------------------------------------------------------------------ restatement: features, reset, one update
def walk_of(pop, wu):
    """random_walk_sampling (:79-89) with the uniforms wu [NP, D]."""
    w = np.empty_like(wu)
    w[0] = wu[0]
    for i in range(1, len(wu)):
        w[i] = (w[i - 1] + wu[i]) % 1
    pmin, pmax = np.min(pop, axis=0), np.max(pop, axis=0)
    return pmin + (pmax - pmin) * w


def transition_counts(diff, star, T=np.float64):
    """[9, 6] transition counts of the symbol strings of cal_rie (:22-47)."""
    out = np.zeros((9, 6), dtype=int)
    for k in range(9):
        eps = star / T(2 ** k) if k < 8 else T(0)
        s = np.where(diff < -eps, -1, np.where(diff > eps, 1, 0))
        a, b = s[:-1], s[1:]
        five = [(a == -1) & (b == 0), (a == -1) & (b == 1), (a == 0) & (b == 1), (a == 0) & (b == -1), (a == 1) & (b == -1)]
        out[k, :5] = [int(x.sum()) for x in five]
        out[k, 5] = len(a) - out[k, :5].sum()
    return out


def features(samples, f):
    """cal_fdc / cal_rie / cal_acf / cal_nop (:8-76) in numpy's own arithmetic; nop orders by (distance, index).
    -> (state [4], the nine entropies, [9, 6] counts, distances)."""
    n = len(f)
    best = np.argmin(f)
    dist = np.linalg.norm(samples - samples[best], axis=-1)
    cfd = np.mean((f - np.mean(f)) * (dist - np.mean(dist)))
    fdc = cfd / (np.var(dist) * np.var(f) + 1e-6)
    diff = f[1:] - f[:-1]
    star = max(0., diff.max())
    counts = transition_counts(diff, star)
    hs = []
    for k in range(9):
        freq = counts[k].astype(np.float64)
        freq[freq == 0] = n
        freq /= n
        hs.append(-np.sum(freq * np.log(freq) / np.log(6)))
    avg = np.mean(f)
    a = np.sum((f - avg) ** 2) + 1e-6
    acf = 0
    for v in (f[:-1] - avg) * (f[1:] - avg):
        acf += v
    acf /= a
    fs = f[np.lexsort((np.arange(n), dist))]
    nop = int(np.sum(fs[1:] < fs[:-1])) / n
    return np.array([fdc, max(hs), acf, nop]), np.array(hs), counts, dist


def entropies_cr(counts, n):
    """The nine entropies of cal_rie from the transition counts with a CORRECTLY ROUNDED log of the frequencies (np.longdouble's log, then one
    rounding to double; 200-bit arithmetic agrees on all 8250 arguments n / NP, NP <= 128): what the kernel evaluates.  numpy's own log is
    correctly rounded on every argument n / 100, so at NP = 100 this is the reference's value to the bit; it is not at 16 arguments of other NP."""
    hs = []
    for k in range(9):
        freq = counts[k].astype(np.float64)
        freq[freq == 0] = n
        freq /= n
        hs.append(-np.sum(freq * np.log(freq.astype(np.longdouble)).astype(np.float64) / np.log(6)))
    return np.array(hs)


def features_wide(samples, f):
    """The same expressions in np.longdouble on the same float64 inputs -> (fdc, the nine entropies, acf)."""
    L = np.longdouble
    s, f = samples.astype(L), f.astype(L)
    n = len(f)
    d = np.sqrt(np.sum((s - s[np.argmin(f)]) ** 2, axis=-1))
    cf, cd = f - np.sum(f) / n, d - np.sum(d) / n
    fdc = (np.sum(cf * cd) / n) / ((np.sum(cd * cd) / n) * (np.sum(cf * cf) / n) + L(1e-6))
    diff = f[1:] - f[:-1]
    counts = transition_counts(diff, max(L(0), diff.max()), L)
    hs = []
    for k in range(9):
        freq = counts[k].astype(L)
        freq[freq == 0] = n
        freq /= n
        hs.append(-np.sum(freq * np.log(freq) / np.log(L(6))))
    acf = np.sum(cf[:-1] * cf[1:]) / (np.sum(cf * cf) + L(1e-6))
    return fdc, np.array(hs), acf


def _sensitivity(f, dist):
    """First derivatives of fdc and acf with respect to the costs (the distances depend on the costs only through argmin, which the
    generator's margin fixes).  With c = f - mean(f), e = dist - mean(dist), N = mean(c e), Den = var(dist) var(f) + 1e-6:
      d fdc / d f_j = e_j / (n Den) - N var(dist) 2 c_j / (n Den^2)
    and with A = sum_i c_i c_{i+1}, S = sum c^2:
      d A / d f_j = c_{j-1} + c_{j+1} - (1/n) sum_i (c_i + c_{i+1}),  d acf / d f_j = dA_j / (S + 1e-6) - A 2 c_j / (S + 1e-6)^2.
    A cost perturbation inside helpers.close, |delta_j| <= ATOL + RTOL |f_j|, moves a feature by at most sum_j |d / d f_j| delta_j to first
    order; the tests allow twice that plus 16 ulp."""
    n = len(f)
    c, e = f - f.mean(), dist - dist.mean()
    vd, N = np.mean(e * e), np.mean(c * e)
    den = vd * np.mean(c * c) + 1e-6
    g_fdc = e / (n * den) - N * vd * 2 * c / (n * den * den)
    A, S = np.sum(c[:-1] * c[1:]), np.sum(c * c) + 1e-6
    nb = np.zeros(n)
    nb[1:] += c[:-1]
    nb[:-1] += c[1:]
    g_acf = (nb - np.sum(c[:-1] + c[1:]) / n) / S - A * 2 * c / (S * S)
    tol = ATOL + RTOL * np.abs(f)
    return np.sum(np.abs(g_fdc) * tol), np.sum(np.abs(g_acf) * tol)


def _finish(ctx, st):
    """Logging and termination after the features (:190-204)."""
    if st['fes'] >= st['log_index'] * ctx.log_interval:
        st['log_index'] += 1
        st['log'].append(st['gbest'])
    st['done'] = bool(st['fes'] >= ctx.max_fes or (ctx.has_opt and ctx.early_stop and st['cost'].min() <= 1e-8))
    if st['done']:
        if len(st['log']) >= ctx.nlog + 1:
            st['log'][-1] = st['gbest']
        else:
            st['log'].append(st['gbest'])


def restate_reset(ctx, t, cost, scost, pointer=0):
    """init_population with the draws of tape `t`, the initial costs and the samples_cost it is given."""
    NP, D = ctx.NP, ctx.D
    o = reset_off(NP, D)
    pop = t[:NP * D].reshape(NP, D) * (ctx.ub - ctx.lb) + ctx.lb
    g0 = int(np.argmin(cost))
    ft = features(walk_of(pop, t[o['walk']:o['walk'] + NP * D].reshape(NP, D)), scost)
    feat = ft[0]
    return {'rie_cr': entropies_cr(ft[2], NP).max(), 'pop': pop, 'cost': np.array(cost, dtype=np.float64), 'surv': np.ones(NP), 'scost': np.array(scost), 'g0': g0, 'alias': True, 'gpos': pop[g0].copy(),
            'gbest': cost[g0], 'fes': 2 * NP, 'log_index': 1, 'log': [cost[g0]], 'done': False, 'pointer': pointer, 'feat': feat}


def restate_trial(ctx, st, action, t):
    """Mutation (left to right as written), np.clip, binomial crossover -> the trial row."""
    D, o = ctx.D, step_off(ctx.NP, ctx.D)
    x, p = st['pop'], st['pointer']
    r = t[:4].astype(int)
    best = x[st['g0']] if st['alias'] else st['gpos']
    if action == 0:
        v = x[r[0]] + F * (x[r[1]] - x[r[2]])
    elif action == 1:
        v = x[p] + F * (x[r[0]] - x[p] + x[r[1]] - x[r[2]])
    else:
        v = best + F * (x[r[0]] - x[r[1]] + x[r[2]] - x[r[3]])
    v = np.clip(v, ctx.lb, ctx.ub)
    u = np.where(t[o['cross']:o['cross'] + D] < CR, v, x[p])
    u[int(t[o['jrand']])] = v[int(t[o['jrand']])]
    return u


def restate_finish(ctx, st, t, u, ucost, scost):
    """Everything downstream of the two evaluations as a function of the costs it is given -> (state after, reward, selected)."""
    NP, D, o = ctx.NP, ctx.D, step_off(ctx.NP, ctx.D)
    new = {k: (v.copy() if isinstance(v, np.ndarray) else copy.copy(v)) for k, v in st.items()}
    p = st['pointer']
    sel = bool(ucost <= st['cost'][p])
    if sel:
        new['pop'][p], new['cost'][p], new['surv'][p] = u, ucost, 1
        if ucost < st['gbest']:
            new['gpos'], new['gbest'], new['alias'] = u.copy(), ucost, False
    else:
        new['surv'][p] += 1
    new['fes'] = st['fes'] + 2 * NP
    new['scost'] = np.array(scost)
    ft = features(walk_of(new['pop'], t[o['walk']:o['walk'] + NP * D].reshape(NP, D)), new['scost'])
    new['feat'], new['rie_cr'] = ft[0], entropies_cr(ft[2], NP).max()
    _finish(ctx, new)
    acc = 0
    for i in range(NP):
        if i == p:
            if new['surv'][i] == 1:
                acc += 1
        else:
            acc += 1 / new['surv'][i]
    new['pointer'] = (p + 1) % NP
    return new, acc / NP, sel


# ------------------------------------------------------------------------------------------------ the fixture's episodes
def _problem(suite, dim, fid):
    if suite == 'protein':
        from test_protein import protein
        return protein()[0][fid], 0
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _setup(case):
    suite, dim, fid, seed = case.split('/')
    p, nk = _problem(suite, dim, fid)
    protein = suite == 'protein'
    ctx = Ctx(NP0, int(dim), p.lb, p.ub, int(TR[f'{case}/max_fes']), not protein, nlog=5 if protein else 50)
    keys = [(case, int(seed))] + ([(f'{case}/second', int(seed) + 1)] if f'{case}/second/actions' in TR else [])
    return p, nk, protein, ctx, keys


def host_cost(p, protein, u, draws):
    f = oracle.evaluate(p.desc(), np.atleast_2d(u))
    if protein:
        return f
    if p.noise[0] != 0:
        f = oracle.apply_noise(p.desc(), p.bias, f, draws)
    return f - p.bias


@functools.lru_cache(maxsize=None)
def chain(case):
    """The restatement chained over the fixture episode(s) of `case` with the feeder's tapes and the REFERENCE's recorded costs ->
    {key: [(tape, action, trial row, state after, reward)]}, entry 0 the reset; and the feeder's RandomState after each episode."""
    p, nk, protein, ctx, keys = _setup(case)
    out, ends = {}, {}
    for key, seed in keys:
        rs = np.random.RandomState(seed)
        fd = DedqnTapeFeeder(ctx.NP, ctx.D, nk, rs)
        t = fd.reset_tape()
        st = restate_reset(ctx, t, TR[f'{key}/snap0/cost'], TR[f'{key}/scost'][0], pointer=int(TR[f'{key}/pointer0']))
        rows = [(t, None, None, st, None)]
        for g, a in enumerate(TR[f'{key}/actions']):
            t = fd.step_tape(int(a), st['pointer'])
            u = restate_trial(ctx, st, int(a), t)
            st, reward, _ = restate_finish(ctx, st, t, u, TR[f'{key}/ucost'][g], TR[f'{key}/scost'][g + 1])
            st['attempts'] = fd.attempts
            rows.append((t, int(a), u, st, reward))
        out[key], ends[key] = rows, rs.rand()
    return out, ends


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case):
    """Fed the reference's recorded trial costs and samples_cost and the walk regenerated from the seed, the restatement reproduces every
    recorded state, reward, done, gbest, fes and snapshot bit for bit; the host objective at the restated trial rows is close to the
    recorded trial costs; the feeder ends each episode at the stream position the generator recorded."""
    p, nk, protein, ctx, keys = _setup(case)
    rows_of, ends = chain(case)
    for key, _ in keys:
        rows = rows_of[key]
        G = len(TR[f'{key}/actions'])
        assert len(rows) == G + 1
        snaps = set(int(s) for s in TR[f'{key}/snap_steps'])
        for g, (t, a, u, st, reward) in enumerate(rows):
            where = (key, g)
            assert np.array_equal(st['feat'], TR[f'{key}/states'][g]), (*where, st['feat'], TR[f'{key}/states'][g])
            assert st['rie_cr'] == TR[f'{key}/states'][g][1], (*where, 'rie with a correctly rounded log', st['rie_cr'], TR[f'{key}/states'][g][1])
            assert st['gbest'] == TR[f'{key}/gbest'][g] and st['fes'] == TR[f'{key}/fes'][g], where
            if g > 0:
                assert reward == TR[f'{key}/reward'][g - 1] and st['done'] == TR[f'{key}/done'][g - 1], where
                assert close(host_cost(p, protein, u, t[step_off(ctx.NP, ctx.D)['noise']:][:3].reshape(3, 1)), TR[f'{key}/ucost'][g - 1]), where
            if g in snaps:
                for name, mine in (('pop', st['pop']), ('cost', st['cost']), ('survival', st['surv'])):
                    assert np.array_equal(mine, TR[f'{key}/snap{g}/{name}']), (*where, 'snapshot', name)
        st = rows[-1][3]
        assert st['done'] and np.array_equal(st['log'], TR[f'{key}/cost']) and st['pointer'] == TR[f'{key}/pointer'], key
        assert np.array_equal(st['pop'][st['g0']] if st['alias'] else st['gpos'], TR[f'{key}/gbest_pos']), key
        assert ends[key] == float(TR[f'{key}/next_rand']), key


def test_fixture_covers_the_quirks():
    """What the fixture is meant to pin, from the recorded arrays."""
    k = next(c for c in CASES if c.startswith('bbob/10/1/'))
    assert len(TR[f'{k}/actions']) == 99 and TR[f'{k}/fes'][-1] == 20000 and len(TR[f'{k}/cost']) == 51 and TR[f'{k}/fes'][0] == 200      # accounting
    assert set(TR[f'{k}/actions']) == {2}                                                                # the purely greedy case
    for c in CASES:
        if c.startswith('bbob/10/') and int(TR[f'{c}/max_fes']) == 20000:
            assert len(TR[f'{c}/actions']) == 99 and len(TR[f'{c}/cost']) == 51, c
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}    # one per noise model
    k = next(c for c in CASES if c.startswith('bbob/30/'))
    assert int(TR[f'{k}/max_fes']) // 50 < 200 and len(TR[f'{k}/cost']) == len(TR[f'{k}/actions']) + 2 < 51   # one append per step, then the final one
    k = next(c for c in CASES if c.startswith('protein'))
    assert len(TR[f'{k}/actions']) == 4 and TR[f'{k}/fes'][-1] == 1000
    k = next(c for c in CASES if f'{c}/second/actions' in TR)
    assert TR[f'{k}/second/pointer0'] == TR[f'{k}/pointer'] != 0 and np.all(TR[f'{k}/second/snap0/survival'] == 1)   # the pointer carries over, survival does not
    assert any(len(set(TR[f'{c}/actions'])) == 3 for c in CASES)
    seen = {'redraw': 0, 'reject': 0, 'alias_kept': 0, 'alias_dropped': 0}
    for c in CASES:
        rows_of, _ = chain(c)
        for key, rows in rows_of.items():
            for (t, a, u, st, r), (_, _, _, prev, _) in zip(rows[1:], rows[:-1]):
                seen['redraw'] += st['attempts'] > 1
                seen['reject'] += st['surv'][prev['pointer']] > 1
            seen['alias_kept' if rows[-1][3]['alias'] else 'alias_dropped'] += 1
    assert seen['redraw'] > 0 and seen['reject'] > 0 and seen['alias_dropped'] > 0, seen


def test_abi_geometry_of_dedqn():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_DEDQN == ALGO_DEDQN
    for np_, D in ((100, 10), (100, 12), (100, 30), (4, 2), (128, 40)):
        cfg = oracle.make_cfg(ALGO_DEDQN, np_, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(cfg)) == 4 and lib.mbx_action_dim(C.byref(cfg)) == 1
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(np_, D)
        assert max(step_off(np_, D)['nfeat'], reset_off(np_, D)['nfeat']) + 3 * np_ <= tape_stride(np_, D)
    for np_, D in ((3, 10), (129, 10), (256, 10), (100, 41), (100, 64)):                     # np outside [4, 128], dim > 40
        bad = oracle.make_cfg(ALGO_DEDQN, np_, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_action_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0, (np_, D)
    for algo in (12, 14, 17):                                                                 # not assigned
        bad = oracle.make_cfg(algo, 100, 10, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0
    assert state_off(100, 10, 50)['end'] == 1000 + 300 + 10 + 16 + 16 + 51


class _Npz(dict):
    @property
    def files(self):
        return list(self)


def _agent(max_learning_step=10, device='cpu'):
    import torch
    from metabox_amd.agent import DEDQN_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', device, '--max_learning_step', str(max_learning_step)])
    cfg.agent_save_dir = None
    cfg.save_interval = 10 ** 9
    return DEDQN_Agent(cfg), cfg, torch


@pytest.mark.parametrize('detach', [False, True])
def test_training_update_matches_the_reference_only_with_the_attached_target(detach):
    """One reference DQN update (dedqn_train.npz): learn_from_batch reproduces the gradients and the weights after the AdamW step; the same
    update with the TD target detached does NOT -- the fixture pins the reference's non-detached target."""
    agent, cfg, torch = _agent()
    agent.load_exported_weights(_Npz({k[len('init/'):]: TRAIN[k] for k in TRAIN.files if k.startswith('init/net/')}))
    obs, act, rew, nxt, dn = (torch.as_tensor(TRAIN[f'batch/{k}']) for k in ('obs', 'act', 'rew', 'nxt', 'done'))
    with torch.enable_grad():
        agent.learn_from_batch(obs, act, rew, nxt, dn, detach_target=detach)
    grads = {k: p.grad.detach().numpy() for k, p in agent.q_net.named_parameters()}
    post = {k: v.detach().numpy() for k, v in agent.q_net.state_dict().items()}
    ok_g = all(np.allclose(grads[k], TRAIN[f'grad/net/{k}'], rtol=1e-5, atol=1e-8) for k in grads)
    ok_p = all(np.allclose(post[k], TRAIN[f'post/net/{k}'], rtol=1e-6, atol=1e-9) for k in post)
    if detach:
        worst = max(np.abs(grads[k] - TRAIN[f'grad/net/{k}']).max() / (np.abs(TRAIN[f'grad/net/{k}']).max() + 1e-30) for k in grads)
        assert not ok_g and worst > 1e-2, worst
    else:
        assert ok_g and ok_p


def test_agent_acts_like_the_shipped_network():
    """The torch module with the exported weights reproduces the 64 recorded (state -> Q, argmax) pairs; packed_weights has the documented layout."""
    agent, cfg, torch = _agent()
    agent.load_exported_weights(POL)
    with torch.no_grad():
        q = agent.q_net(torch.as_tensor(POL['io/x'], dtype=torch.float32)).numpy()
    assert np.abs(q - POL['io/q']).max() <= 1e-5 and np.array_equal(q.argmax(1), POL['io/argmax'])
    assert np.array_equal(agent.greedy_batch(torch.as_tensor(POL['io/x'])).numpy(), POL['io/argmax'])
    w = agent.packed_weights().numpy()
    assert w.shape == (193,) and np.array_equal(w[:40].reshape(4, 10), POL['net/net.layer0-linear.weight'].T) and np.array_equal(w[190:], POL['net/net.layer2-linear.bias'])
    assert cfg.gamma == 0.8 and cfg.memory_size == 100 and cfg.warm_up_size == 64 and cfg.epsilon == 0.1 and cfg.lr == 1e-4


def test_registered_by_name():
    from metabox_amd import agent, optimizer
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10'])
    opt = optimizer.DEDQN_Optimizer(cfg)
    assert (cfg.NP, cfg.F, cfg.Cr, cfg.rwsteps) == (100, 0.5, 0.5, 100) and hasattr(agent, 'DEDQN_Agent') and hasattr(opt, 'make_batch')


# ------------------------------------------------------------------------------------------------ GPU: tape replay of the fixture
def _ulps(x, ref):
    return float(abs(np.longdouble(x) - np.longdouble(ref)) / np.spacing(abs(np.float64(ref)) if ref != 0 else 1e-300))


def check_features(got, tape_walk, where, worst):
    """Kernel arithmetic isolated: the restatement fed the kernel's own samples_cost and the same walk.  nop and the winning level's
    transition counts exact; rie equal to the evaluation with a correctly rounded log (entropies_cr); fdc / rie / acf within 4x the float64
    restatement's own error (against np.longdouble) + 4 ulp."""
    NP, D = got['pop'].shape
    samples = walk_of(got['pop'], tape_walk.reshape(NP, D))
    mine, hs, counts, dist = features(samples, got['scost'])
    wf, whs, wa = features_wide(samples, got['scost'])
    assert got['feat'][3] == mine[3], (*where, 'nop', got['feat'][3], mine[3])
    assert got['feat'][1] == entropies_cr(counts, NP).max(), (*where, 'rie against the correctly rounded evaluation', got['feat'][1], entropies_cr(counts, NP).max())
    assert np.array_equal(got['counts'], counts[got['level']]), (*where, 'transition counts', got['level'], got['counts'], counts[got['level']])
    for name, k, wide, m in (('fdc', 0, wf, mine[0]), ('rie', 1, whs.max(), mine[1]), ('acf', 2, wa, mine[2])):
        bound = 4 * abs(np.longdouble(m) - wide) + 4 * np.spacing(abs(np.float64(wide)))
        err = abs(np.longdouble(got['feat'][k]) - wide)
        assert err <= bound, (*where, name, got['feat'][k], m, float(err), float(bound))
        worst[name] = max(worst.get(name, 0.), _ulps(got['feat'][k], np.float64(wide)))
        worst[name + '/numpy'] = max(worst.get(name + '/numpy', 0.), _ulps(m, np.float64(wide)))
    return mine, dist


@functools.lru_cache(maxsize=None)
def replay(case):
    """Every fixture episode of `case` through mbx_reset / k_dedqn_step with the feeder's tapes and the recorded actions ->
    {key: [(state row, reward, done, state block as a dict)]}, entry 0 the reset."""
    import torch
    from metabox_amd.suite import Batch, Suite
    p, nk, protein, ctx, keys = _setup(case)
    rows_of, _ = chain(case)
    s = Suite([p])
    b = Batch(s, ALGO_DEDQN, [0], [int(keys[0][1])], ctx.NP, ctx.max_fes, ctx.log_interval, ctx.nlog)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (4, 1, tape_stride(ctx.NP, ctx.D))
    dev_tape = torch.empty(1, b.tape_stride, dtype=torch.float64, device='cuda')
    out = {}
    for key, _ in keys:                                              # the second episode runs on the same batch: the pointer carries over
        rec = []
        for g, (t, a, u, st, reward) in enumerate(rows_of[key]):
            dev_tape.copy_(torch.from_numpy(t[None]))
            b.set_tape(dev_tape)
            if g == 0:
                state = b.reset()
                torch.cuda.synchronize()
                rec.append((state[0].cpu().numpy().copy(), None, None, from_block(b.read_state(0), ctx)))
            else:
                state, r, d = b.step(torch.tensor([a], dtype=torch.int32, device='cuda'))
                torch.cuda.synchronize()
                rec.append((state[0].cpu().numpy().copy(), float(r[0].item()), bool(d[0].item()), from_block(b.read_state(0), ctx)))
        res = b.results()
        out[key] = (rec, {k: v.cpu().numpy() for k, v in res.items()})
    b.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_dedqn_tape_replay_matches_the_reference(case):
    """fes, done, pointer, curve length, the survival counters at the snapshots and the reward sequence exact; gbest / cost curve /
    snapshots / trial costs within helpers.close; nop and rie equal to the recorded ones, fdc / acf inside the cost tolerance
    propagated through their derivatives.  The first differing selection, if any, must be a proven near tie; no mismatch budget."""
    p, nk, protein, ctx, keys = _setup(case)
    rows_of, _ = chain(case)
    got_of = replay(case)
    ledger = []
    for key, _ in keys:
        rec, res = got_of[key]
        snaps = set(int(s) for s in TR[f'{key}/snap_steps'])
        diverged = False
        for g, ((t, a, u, st, reward), (state, r, d, got)) in enumerate(zip(rows_of[key], rec)):
            where = (key, g)
            if g > 0:
                prev_ref, prev_dev = rows_of[key][g - 1][3], rec[g - 1][3]
                pp = prev_ref['pointer']
                assert close(got['ucost'], TR[f'{key}/ucost'][g - 1]), (*where, 'trial cost', got['ucost'], TR[f'{key}/ucost'][g - 1])
                ref_sel, dev_sel = float(TR[f'{key}/ucost'][g - 1] <= prev_ref['cost'][pp]), float(got['surv'][pp] == 1)
                if not prove_tie_arrays(prev_ref['cost'][pp:pp + 1], TR[f'{key}/ucost'][g - 1:g], [ref_sel], prev_dev['cost'][pp:pp + 1], [got['ucost']], [dev_sel],
                                        ledger, 'select', key, g):
                    diverged = True
                    break
                assert r == TR[f'{key}/reward'][g - 1] and d == TR[f'{key}/done'][g - 1] and got['done'] == d, (*where, 'reward / done', r, TR[f'{key}/reward'][g - 1])
            assert got['fes'] == TR[f'{key}/fes'][g] and got['pointer'] == (int(TR[f'{key}/pointer0']) + g) % ctx.NP and got['gen'] == g, where
            assert close(got['gbest'], TR[f'{key}/gbest'][g]) and close(got['scost'], TR[f'{key}/scost'][g]), where
            assert np.array_equal(got['surv'], st['surv']) and got['alias'] == st['alias'], (*where, 'survival / alias')
            assert np.array_equal(state, got['feat']), where
            # against the reference's recorded state
            ref_state = TR[f'{key}/states'][g]
            o = (reset_off if g == 0 else step_off)(ctx.NP, ctx.D)
            samples = walk_of(got['pop'], t[o['walk']:o['walk'] + ctx.NP * ctx.D].reshape(ctx.NP, ctx.D))
            mine, _, _, dist = features(samples, got['scost'])
            assert got['feat'][3] == ref_state[3], (*where, 'nop', got['feat'][3], ref_state[3])
            assert got['feat'][1] == ref_state[1], (*where, 'rie', got['feat'][1], ref_state[1])
            s_fdc, s_acf = _sensitivity(TR[f'{key}/scost'][g], dist)
            for name, k, sens in (('fdc', 0, s_fdc), ('acf', 2, s_acf)):
                bound = 2 * sens + 16 * np.spacing(abs(ref_state[k]))
                assert abs(got['feat'][k] - ref_state[k]) <= bound, (*where, name, got['feat'][k], ref_state[k], bound)
            if g in snaps:
                assert close(got['pop'], TR[f'{key}/snap{g}/pop']) and close(got['cost'], TR[f'{key}/snap{g}/cost']), (*where, 'snapshot')
                assert np.array_equal(got['surv'], TR[f'{key}/snap{g}/survival']), (*where, 'snapshot survival')
        if not diverged:
            ref_cost = TR[f'{key}/cost']
            assert int(res['cost_len'][0]) == len(ref_cost) and close(res['cost'][0, :len(ref_cost)], ref_cost), key
            assert res['fes'][0] == TR[f'{key}/fes'][-1] and int(res['steps'][0]) == len(TR[f'{key}/actions']), key
            assert res['return'][0] == pytest.approx(float(np.sum(TR[f'{key}/reward'])), rel=1e-13), key
            assert close(rec[-1][3]['gpos'], TR[f'{key}/gbest_pos']), key
    print(f'{case}: {sum(len(got_of[k][0]) - 1 for k, _ in keys)} steps, {len(ledger)} selection(s) on a proven near tie')
    print_ledger(ledger)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_dedqn_features_are_the_restatement_of_the_kernels_own_costs(case):
    """At every step of the tape replay the restatement, fed the kernel's own samples_cost (state block) and the same walk, gives the
    kernel's four features: nop and the transition counts exactly, fdc / rie / acf within the derived bound (see check_features)."""
    p, nk, protein, ctx, keys = _setup(case)
    rows_of, _ = chain(case)
    got_of = replay(case)
    worst = {}
    for key, _ in keys:
        for g, ((t, a, u, st, reward), (state, r, d, got)) in enumerate(zip(rows_of[key], got_of[key][0])):
            o = (reset_off if g == 0 else step_off)(ctx.NP, ctx.D)
            check_features(got, t[o['walk']:o['walk'] + ctx.NP * ctx.D], (key, g), worst)
    print(f'{case}: largest error in ulp of the extended-precision value, kernel / numpy restatement: ' +
          ', '.join(f'{n} {worst[n]:.2f} / {worst[n + "/numpy"]:.2f}' for n in ('fdc', 'rie', 'acf')))


# ------------------------------------------------------------------------------------------------ GPU: crafted states against the restatement
def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


def philox_step_tape(seed, step, episode, NP, D, action, pointer):
    """The tape that holds what the Philox route of k_dedqn_step draws on a noise-free function (include/mbx_layout.h §14) -> (tape, attempts)."""
    o = step_off(NP, D)
    t = np.zeros(tape_stride(NP, D))
    cols = 3 if action in (0, 1) else 4
    for attempt in range(1024):
        w = oracle.philox(seed, attempt, SITE_DD_R, step, episode)
        r = [(x * NP) >> 32 for x in w]
        if pointer not in r[:cols]:
            break
    t[:4] = r
    t[o['jrand']] = (oracle.philox(seed, 0, SITE_DQ_JRAND, step, episode)[0] * D) >> 32
    for d in range(D):
        w = oracle.philox(seed, d, SITE_LDE_ELEM, step, episode)
        t[o['cross'] + d] = _u53(w[0], w[1])
    for e in range(NP * D):
        w = oracle.philox(seed, e, SITE_DD_WALK, step, episode)
        t[o['walk'] + e] = _u53(w[0], w[1])
    return t, attempt + 1


def _crafted_batch(NP, D, fid=15, suite='bbob', seed=11, max_fes=None, B=1):
    from metabox_amd.suite import Batch, Suite
    p, nk = _problem(suite, D, fid)
    max_fes = max_fes or 40 * NP
    ctx = Ctx(NP, D, p.lb, p.ub, max_fes, True, nlog=10)
    s = Suite([p])
    b = Batch(s, ALGO_DEDQN, [0] * B, [seed + 3 * i for i in range(B)], NP, max_fes, ctx.log_interval, 10)
    return b, ctx, p, nk


def _state_of(got, ctx):
    return {k: got[k] for k in ('pop', 'cost', 'surv', 'scost', 'gpos', 'gbest', 'fes', 'log_index', 'log', 'done', 'pointer', 'g0', 'alias', 'feat')}


def _step_and_check(b, ctx, st, action, t, worst, where, idx=0, use_tape=True, gen=3):
    """Write `st`, step with `action` (tape `t`, or Philox when use_tape is False: `t` then holds what Philox draws), and compare the
    state block with the restatement fed the device's own costs: bit for bit, features as in check_features."""
    import torch
    b.write_state(idx, to_block(st, ctx, gen=gen))
    tape = torch.zeros(b.B, b.tape_stride, dtype=torch.float64)
    tape[idx] = torch.from_numpy(t)
    b.set_tape(tape.cuda() if use_tape else None)
    acts = torch.zeros(b.B, dtype=torch.int32)
    acts[idx] = action
    state, r, d = b.step(acts.cuda())
    torch.cuda.synchronize()
    got = from_block(b.read_state(idx), ctx)
    u = restate_trial(ctx, st, action, t)
    want, reward, sel = restate_finish(ctx, st, t, u, got['ucost'], got['scost'])
    if sel:
        assert np.array_equal(got['pop'][st['pointer']], u), (*where, 'trial row')
    bad = same_state(got, want)
    assert bad is None, (*where, 'state after', bad, got[bad], want[bad])
    assert r[idx].item() == reward and bool(d[idx].item()) == want['done'] and got['gen'] == gen + 1, (*where, 'reward / done', r[idx].item(), reward)
    o = step_off(ctx.NP, ctx.D)
    check_features(got, t[o['walk']:o['walk'] + ctx.NP * ctx.D], where, worst)
    assert np.array_equal(state[idx].cpu().numpy(), got['feat'])
    return got, want, sel


@pytest.mark.gpu
@pytest.mark.parametrize('D', [2, 10, 12, 40])
def test_hip_dedqn_small_shapes_against_the_restatement(D):
    """np in {4, 7, 8, 9, 64, 65, 100, 128} (the pairwise-sum block edges and the wave boundary) at this dimension: a Philox reset, then one
    taped step per action value from the state the reset left, each against the restatement fed the device's own costs."""
    import torch
    worst = {}
    for NP in (4, 7, 8, 9, 64, 65, 100, 128):
        b, ctx, p, nk = _crafted_batch(NP, D)
        state = b.reset()
        torch.cuda.synchronize()
        got = from_block(b.read_state(0), ctx)
        assert got['fes'] == 2 * NP and got['alias'] and got['g0'] == int(np.argmin(got['cost'])) and np.all(got['surv'] == 1) and np.array_equal(state[0].cpu().numpy(), got['feat'])
        assert close(got['cost'], host_cost(p, False, got['pop'], None)) and close(got['scost'], got['cost'])
        st = _state_of(got, ctx)
        fd = DedqnTapeFeeder(NP, D, nk, np.random.RandomState(100 * NP + D))
        for action in (0, 1, 2):
            st['pointer'] = (NP - 1) if action == 2 else action          # the last row wraps the pointer
            t = fd.step_tape(action, st['pointer'])
            got, want, _ = _step_and_check(b, ctx, st, action, t, worst, (NP, D, action))
            assert got['pointer'] == (st['pointer'] + 1) % NP
        b.close()
    print(f'D = {D}: largest feature error in ulp, kernel / numpy: ' + ', '.join(f'{n} {worst[n]:.2f} / {worst[n + "/numpy"]:.2f}' for n in ('fdc', 'rie', 'acf')))


@pytest.mark.gpu
def test_hip_dedqn_out_of_range_actions_take_the_last_operator_and_the_view_raises():
    """Like k_dq_step, the kernel sends every action outside 0 / 1 down its last branch (best_2); the B = 1 view raises like the reference."""
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.environment import PBO_Env
    from metabox_amd.optimizer import DEDQN_Optimizer
    b, ctx, p, nk = _crafted_batch(100, 10)
    b.reset()
    torch.cuda.synchronize()
    st = _state_of(from_block(b.read_state(0), ctx), ctx)
    fd = DedqnTapeFeeder(100, 10, nk, np.random.RandomState(8))
    for action in (3, -1, 7):
        _step_and_check(b, ctx, st, action, fd.step_tape(2, st['pointer']), {}, ('action', action))
    b.close()
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    env = PBO_Env(problems('bbob', 10)[1], DEDQN_Optimizer(cfg))
    env.reset()
    with pytest.raises(ValueError):
        env.step(3)


@pytest.mark.gpu
def test_hip_dedqn_equal_walk_distances_and_flat_fitness():
    """A collapsed population (pmin == pmax in every coordinate): every walk point is the same point, all distances are 0 and nop follows
    the index order.  On a noise-free function the costs are equal as well: epsilon_star = 0 and every transition is 'else' at every level.
    On a noisy one the costs differ while the distances tie."""
    import torch
    for suite, fid in (('bbob', 15), ('bbob-noisy', 101)):
        b, ctx, p, nk = _crafted_batch(100, 10, fid=fid, suite=suite)
        fd = DedqnTapeFeeder(100, 10, nk, np.random.RandomState(21))
        b.set_tape(torch.from_numpy(fd.reset_tape()[None]).cuda())
        b.reset()
        torch.cuda.synchronize()
        st = _state_of(from_block(b.read_state(0), ctx), ctx)
        st['pop'] = np.tile(st['pop'][3], (100, 1))
        st['cost'] = np.full(100, st['cost'][3])
        st['g0'], st['gbest'], st['log'] = 0, st['cost'][0], [st['cost'][0]]
        t = fd.step_tape(0, st['pointer'])
        got, want, sel = _step_and_check(b, ctx, st, 0, t, {}, (suite, 'collapsed'))
        samples = walk_of(got['pop'], t[step_off(100, 10)['walk']:][:1000].reshape(100, 10))
        assert np.all(samples == samples[0])
        if nk == 0:
            assert np.all(got['scost'] == got['scost'][0]) and got['feat'][3] == 0 and abs(got['feat'][0]) < 1e-9 and abs(got['feat'][2]) < 1e-9    # (the pairwise mean of equal values is not exact)
            assert list(got['counts']) == [0, 0, 0, 0, 0, 98] and got['level'] == 0
        else:
            assert len(np.unique(got['scost'])) > 50 and got['feat'][3] == np.sum(got['scost'][1:] < got['scost'][:-1]) / 100
        b.close()


@pytest.mark.gpu
def test_hip_dedqn_aliased_gbest_follows_its_row_on_an_exact_tie():
    """While gbest is the view of row g0, a trial for that row with EXACTLY its cost overwrites the row and gbest's position moves with it
    (and best_2 then mutates from the new position); a strict improvement ends the aliasing."""
    import torch
    b, ctx, p, nk = _crafted_batch(100, 10, fid=8)
    b.reset()
    torch.cuda.synchronize()
    st = _state_of(from_block(b.read_state(0), ctx), ctx)
    g0 = st['g0']
    st['pointer'] = g0
    o = step_off(100, 10)
    t = DedqnTapeFeeder(100, 10, nk, np.random.RandomState(5)).step_tape(0, g0)
    q = (g0 + 7) % 100
    t[:4] = [q, q, q, 0]                                               # rand_1 with r1 == r2: the trial is row q itself
    t[o['cross']:o['cross'] + 10] = 0.25
    got, _, sel = _step_and_check(b, ctx, st, 0, t, {}, ('alias', 'probe'))
    assert not sel and np.array_equal(restate_trial(ctx, st, 0, t), st['pop'][q])
    tie = copy.deepcopy(st)
    tie['cost'] = np.maximum(st['cost'], got['ucost']) + 1.        # row g0 costs exactly what the trial will cost, the others more
    tie['cost'][g0] = got['ucost']
    tie['gbest'], tie['log'] = got['ucost'], [got['ucost']]
    got, want, sel = _step_and_check(b, ctx, tie, 0, t, {}, ('alias', 'tie'))
    assert sel and got['alias'] and got['g0'] == g0 and np.array_equal(got['gpos'], st['pop'][q]) and not np.array_equal(got['gpos'], st['pop'][g0])
    nxt = _state_of(got, ctx)
    t2 = DedqnTapeFeeder(100, 10, nk, np.random.RandomState(6)).step_tape(2, nxt['pointer'])
    _step_and_check(b, ctx, nxt, 2, t2, {}, ('alias', 'best_2 from the moved view'))
    strict = copy.deepcopy(tie)
    strict['cost'][g0] = strict['gbest'] = np.nextafter(got['ucost'], np.inf)
    strict['log'] = [strict['gbest']]
    got, want, sel = _step_and_check(b, ctx, strict, 0, t, {}, ('alias', 'strict'))
    assert sel and not got['alias'] and np.array_equal(got['gpos'], st['pop'][q])
    b.close()


@pytest.mark.gpu
def test_hip_dedqn_philox_route_and_the_redraw_on_a_collision():
    """The Philox route draws what include/mbx_layout.h §14 says: a step from Philox equals the step from the tape rebuilt on the host from the
    same counters, for a seed whose first draw of r hits the pointer (attempt index in the counter) and for one whose first draw is kept."""
    import torch
    seen = set()
    for seed in range(1, 400):
        t, attempts = philox_step_tape(seed, 1, 1, 100, 10, 2, 0)
        kind = 'collision' if attempts > 1 else 'clean'
        if kind in seen:
            continue
        seen.add(kind)
        from metabox_amd.suite import Batch, Suite
        p, nk = _problem('bbob', 10, 15)
        ctx = Ctx(100, 10, p.lb, p.ub, 4000, True, nlog=10)
        b = Batch(Suite([p]), ALGO_DEDQN, [0], [seed], 100, 4000, 400, 10)
        b.reset()
        torch.cuda.synchronize()
        st = _state_of(from_block(b.read_state(0), ctx), ctx)
        assert st['pointer'] == 0
        _step_and_check(b, ctx, st, 2, t, {}, ('philox', kind, seed), use_tape=False, gen=0)
        b.close()
        if len(seen) == 2:
            break
    assert seen == {'collision', 'clean'}


@pytest.mark.gpu
def test_dedqn_optimizer_carries_its_pointer_to_another_problem():
    """The reference's pointer lives on the optimizer object (:118) and init_population never resets it: after 3 steps on one problem the
    B = 1 view starts the next PROBLEM at row 3 (a new batch, the pointer written into its state block), with fresh survival counters."""
    from metabox_amd.config import get_config
    from metabox_amd.environment import PBO_Env
    from metabox_amd.optimizer import DEDQN_Optimizer
    from metabox_amd.suite import Suite
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    ps = [problems('bbob', 10)[f] for f in (1, 15)]
    Suite(ps)
    np.random.seed(9)
    opt = DEDQN_Optimizer(cfg)
    env = PBO_Env(ps[0], opt)
    env.reset()
    for a in (0, 1, 2):
        env.step(a)
    first = opt._DEDQN_Optimizer__batch
    assert int(first.read_public(0)[SC_POINTER]) == 3
    env2 = PBO_Env(ps[1], opt)
    s0 = env2.reset()
    second = opt._DEDQN_Optimizer__batch
    ctx = Ctx(100, 10, ps[1].lb, ps[1].ub, cfg.maxFEs, True)
    got = from_block(second.read_state(0), ctx)
    assert second is not first and got['pointer'] == 3 and got['fes'] == 200 and np.all(got['surv'] == 1) and np.array_equal(s0, got['feat'])
    _, _, done = env2.step(2)
    got = from_block(second.read_state(0), ctx)
    assert got['pointer'] == 4 and got['surv'][3] in (1, 2) and np.all(np.delete(got['surv'], 3) == 1) and not done and opt.fes == 400


# ------------------------------------------------------------------------------------------------ GPU: kernel routes, policy, harness
@pytest.mark.gpu
def test_hip_dedqn_resident_rollout_is_bit_identical_to_single_steps():
    """k_dedqn_run with n_steps = 97 then 2 == 99 one-step resident launches == k_dedqn_step fed the recorded actions: state blocks,
    results and returns, in Philox mode on a mixed bbob + bbob-noisy suite."""
    import torch
    from metabox_amd.suite import Batch, Suite
    agent, cfg, _ = _agent()
    agent.load_exported_weights(POL)
    w = agent.packed_weights().cuda()
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [1, 5, 8, 15, 21, 24, 101, 102, 103, 117]
    s = Suite([ps[i] for i in ids])
    B = len(ids)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 5
    mk = lambda: Batch(s, ALGO_DEDQN, np.arange(B), seeds, 100, 20000, 400, 50)          # noqa: E731
    ba, bb, bc = mk(), mk(), mk()
    for x in (ba, bb, bc):
        x.reset()
    ret = torch.zeros(B, dtype=torch.float64, device='cuda')
    trajs = []
    for n in (97, 2):
        _, r, _, _, traj = ba.dedqn_rollout(w, n, trajectory=True)
        ret += r
        trajs.append(traj)
    acts = torch.cat([t['actions'] for t in trajs])
    states = torch.cat([t['state'] for t in trajs])
    rewards = torch.cat([t['reward'] for t in trajs])
    for g in range(99):
        _, r1, _, a1 = bb.dedqn_rollout(w, 1)
        live = acts[g] >= 0
        assert torch.equal(a1[live], acts[g][live]), g
        st, r2, d2 = bc.step(torch.where(live, acts[g], torch.zeros_like(acts[g])).contiguous())
        assert torch.equal(r1, r2) and torch.equal(r2[live], rewards[g][live]) and torch.equal(st[live], states[g][live]), g
    ra, rb, rc = ba.results(), bb.results(), bc.results()
    for key in ra:
        assert torch.equal(ra[key], rb[key]) and torch.equal(ra[key], rc[key]), key
    assert torch.equal(ba.state, bb.state) and torch.equal(ba.state, bc.state)
    assert torch.allclose(ret, ra['return'], rtol=1e-13, atol=0)      # (the two launches' sums, added: another association of the same 99 rewards)
    o = state_off(100, 10, 50)
    for k in range(B):
        x, y, z = ba.read_state(k), bb.read_state(k), bc.read_state(k)
        assert np.array_equal(x, y), ids[k]
        z[o['feat'] + FEAT_Q:o['feat'] + FEAT_Q + 3] = x[o['feat'] + FEAT_Q:o['feat'] + FEAT_Q + 3]      # (mbx_step records no Q values)
        assert np.array_equal(x, z), ids[k]
    assert bool((ra['fes'] <= 20000).all()) and int(ra['steps'].max()) == 99 and int(ra['fes'].max()) == 20000
    for x in (ba, bb, bc):
        x.close()


@pytest.mark.gpu
def test_hip_dedqn_in_kernel_network_reproduces_the_reference_pairs():
    """The Q-network inside k_dedqn_run on the 64 recorded states: Q within 1e-5 of the reference's, same argmax, and in agreement with
    the torch module.  The states are written into the state blocks of a 64-instance batch; one one-step launch decides for all."""
    import torch
    from metabox_amd.suite import Batch, Suite
    agent, cfg, _ = _agent()
    agent.load_exported_weights(POL)
    p = problems('bbob', 10)[1]
    ctx = Ctx(100, 10, p.lb, p.ub, 20000, True)
    b = Batch(Suite([p]), ALGO_DEDQN, [0] * 64, np.arange(64, dtype=np.uint64) + 1, 100, 20000, 400, 50)
    b.reset()
    torch.cuda.synchronize()
    o = state_off(100, 10, 50)
    for k in range(64):
        blk = b.read_state(k)
        blk[o['feat']:o['feat'] + 4] = POL['io/x'][k]
        b.write_state(k, blk)
    _, _, _, acts = b.dedqn_rollout(agent.packed_weights().cuda(), 1)
    torch.cuda.synchronize()
    q = np.stack([from_block(b.read_state(k), ctx)['q'] for k in range(64)])
    with torch.no_grad():
        qt = agent.q_net(torch.as_tensor(POL['io/x'], dtype=torch.float32)).numpy()
    print('in-kernel Q against the reference / the torch module: max |dQ| =', np.abs(q - POL['io/q']).max(), np.abs(q - qt).max())
    assert np.abs(q - POL['io/q']).max() <= 1e-5 and np.abs(q - qt).max() <= 1e-5
    assert np.array_equal(acts.cpu().numpy(), POL['io/argmax']) and np.array_equal(q.argmax(1), POL['io/argmax'])
    b.close()


@pytest.mark.gpu
def test_dedqn_in_the_harness(tmp_path):
    """rollout_batch on 64 instances (both policies), rollout_episode through PBO_Env with the pointer carried to the next episode, a
    Tester run naming DEDQN_Agent in agent_for_cp, and train_batch / train_episode changing the weights."""
    import torch
    from metabox_amd.agent import DEDQN_Agent
    from metabox_amd.agent.utils import save_class
    from metabox_amd.config import get_config
    from metabox_amd.environment import BatchedPBO_Env, PBO_Env
    from metabox_amd.optimizer import DEDQN_Optimizer
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    cfg.agent_save_dir = None
    agent = DEDQN_Agent(copy.deepcopy(cfg)).load_exported_weights(POL)
    pb = [problems('bbob', 10)[f] for f in (1, 16)]
    for policy in ('hip', 'torch'):
        env = BatchedPBO_Env(pb, DEDQN_Optimizer(copy.deepcopy(cfg)), np.arange(64) % 2, np.arange(64, dtype=np.uint64) + 5)
        out = agent.rollout_batch(env, policy=policy)
        assert bool((out['fes'] == 20000).all()) and int(out['steps'].max()) == 99 and bool((out['cost_len'] == 51).all()), policy
        assert bool((out['cost'][:, 1:] <= out['cost'][:, :-1]).all()) and bool((out['return'] > 0).all()), policy
        env.close()
    short = copy.deepcopy(cfg)
    short.maxFEs, short.log_interval = 3000, 60
    np.random.seed(4)
    opt = DEDQN_Optimizer(short)
    env = PBO_Env(pb[0], opt)
    info = agent.to('cuda').rollout_episode(env)
    assert info['fes'] == 3000 and len(info['cost']) == 15 + 1 and info['return'] > 0        # 14 steps: one log point each (log_interval 60 < 200), then the final one
    env.reset()
    assert int(opt._DEDQN_Optimizer__batch.read_public(0)[SC_POINTER]) == 14                 # same optimizer object: the pointer carried over
    # Tester, by name
    load_dir = str(tmp_path / 'models') + '/'
    save_class(load_dir, 'DEDQN_Agent', agent)
    tcfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--log_dir', str(tmp_path / 'out'), '--agent_load_dir', load_dir,
                       '--test_runs', '2', '--test', '--agent_for_cp', 'DEDQN_Agent', '--l_optimizer_for_cp', 'DEDQN_Optimizer'])
    res = Tester(tcfg).test()
    for prob, rows in res['cost'].items():
        assert len(rows['DEDQN_Agent']) == 2 and all(len(r) == 51 and r[0] >= r[-1] for r in rows['DEDQN_Agent']), prob
        assert all(v <= 20000 for v in res['fes'][prob]['DEDQN_Agent']), prob
    # training
    tr = copy.deepcopy(cfg)
    tr.max_learning_step, tr.save_interval, tr.maxFEs, tr.log_interval = 1000, 10 ** 9, 20000, 400
    learner = DEDQN_Agent(tr)
    before = [q.detach().clone() for q in learner.q_net.parameters()]
    env = BatchedPBO_Env(pb, DEDQN_Optimizer(copy.deepcopy(tr)), np.arange(32) % 2, np.arange(32, dtype=np.uint64) + 9)
    with torch.enable_grad():
        exceed, info = learner.train_batch(env, max_updates=2)
    assert info['learn_steps'] == 2 and not exceed and np.isfinite(info['return'])
    assert any(not torch.equal(a.cpu(), c.detach().cpu()) for a, c in zip(before, learner.q_net.parameters()))
    env.close()
    one = DEDQN_Agent(copy.deepcopy(tr))
    one._DEDQN_Agent__max_learning_step = 3
    np.random.seed(2)
    with torch.enable_grad():
        done, info = one.to('cuda').train_episode(PBO_Env(pb[1], DEDQN_Optimizer(copy.deepcopy(tr))))
    assert done and info['learn_steps'] == 3
    pickle.loads(pickle.dumps(learner))
