"""SYMBOL in numpy, in the kernel's order (metabox_amd/csrc/mbx_symbol.hpp; layouts: include/mbx_layout.h section 22).

The restatement of one sub-step, of the end of an action and of the nine features that tests/test_symbol.py holds against the reference's recorded traces
(fed the reference's costs: bit for bit) and against the kernel (fed the kernel's costs: bit for bit, the features included, because every sum below
is taken in the order the kernel takes it).  A population is a plain dict ``pop``; ``pack`` / ``unpack`` map it to the kernel's state block.
"""
import numpy as np

SLOTS, NTOK, RANDX_MAX, SUB_MAX, NFEAT, NSCALAR = 63, 11, 32, 8, 9, 16
ADD, MUL, NEG, CM1, C0, X, GB, GW, DX, RANDX, PB = range(11)
VOCAB = ('+', '*', '-', 'C-1', 'C0', 'x', 'gb', 'gw', 'dx', 'randx', 'pb')
SC = dict(gbest=0, fes=1, log_index=2, cost_len=3, done=4, ret=5, gen=6, episode=7, gbest_idx=8, sub=9, gworst=10, cbest=11, cbest_idx=12, stag=13,
          pre_gbest=14, init_cost=15)


# ------------------------------------------------------------------------------------------------ the rule
def well_formed(tok):
    """The kernel's sym_check: a root operator, every node under a binary operator or on the left of the unary one, every operator with its children
    (hence above slot 31), known tokens only, 32 randx at most."""
    tok = np.asarray(tok)
    if tok.shape != (SLOTS,) or np.any(tok < -1) or np.any(tok >= NTOK) or not (ADD <= tok[0] <= NEG):
        return False
    for p in range(SLOTS):
        t = tok[p]
        if p > 0 and t != -1:
            q = tok[(p - 1) // 2]
            if not (q in (ADD, MUL) or (q == NEG and p % 2 == 1)):
                return False
        if ADD <= t <= NEG:
            if 2 * p + 2 >= SLOTS or tok[2 * p + 1] == -1 or (t != NEG and tok[2 * p + 2] == -1):
                return False
    return int(np.sum(tok == RANDX)) <= RANDX_MAX


def post_order(tok, p=0):
    """Slots of the tree in post-order (for a unary node: the left child, then the node)."""
    t = tok[p]
    if t in (ADD, MUL):
        return post_order(tok, 2 * p + 1) + post_order(tok, 2 * p + 2) + [p]
    if t == NEG:
        return post_order(tok, 2 * p + 1) + [p]
    return [p]


def infix(tok, cst, p=0):
    """The reference's string (prefix_to_infix): (left op right), -(child), a constant as repr of its float64 value."""
    t = tok[p]
    if t in (ADD, MUL):
        return '(' + infix(tok, cst, 2 * p + 1) + VOCAB[t] + infix(tok, cst, 2 * p + 2) + ')'
    if t == NEG:
        return '-(' + infix(tok, cst, 2 * p + 1) + ')'
    return repr(float(cst[p])) if t in (CM1, C0) else VOCAB[t]


def rule(tok, cst, x, gb, gw, dx, pb, idx):
    """f(x, gb, gw, dx, randx.., pb) as numpy evaluates the parenthesised string; idx [k, NP]: the index row of the k-th randx leaf from the left."""
    occ = {p: k for k, p in enumerate(p for p in post_order(tok) if tok[p] == RANDX)}

    def val(p):
        t = tok[p]
        if t == ADD:
            return val(2 * p + 1) + val(2 * p + 2)
        if t == MUL:
            return val(2 * p + 1) * val(2 * p + 2)
        if t == NEG:
            return -val(2 * p + 1)
        if t in (CM1, C0):
            return np.float64(cst[p])
        if t == RANDX:
            return x[np.asarray(idx[occ[p]], dtype=np.int64)]
        return {X: x, GB: gb[None, :], GW: gw[None, :], DX: dx, PB: pb}[t]
    return val(0)


def n_randx(tok):
    return int(np.sum(np.asarray(tok) == RANDX))


# ------------------------------------------------------------------------------------------------ a sub-step and the end of an action
def candidates(pop, tok, cst, idx, lb, ub):
    """next = x + f(..), then the periodic wrap lb + (next - ub) % (ub - lb) (numpy's floored modulo)."""
    x = pop['x']
    nxt = x + rule(tok, cst, x, pop['gb'], pop['gw'], pop['dx'], pop['pb'], idx)
    with np.errstate(invalid='ignore'):
        return np.broadcast_to(lb + (nxt - ub) % (ub - lb), x.shape).copy()


def apply_costs(pop, cand, cost):
    """Population.update (population.py:84-132, filter_survive=False) given the candidates' costs."""
    NP = cand.shape[0]
    if pop['sub'] == 0:
        pop['pre_gbest'] = pop['gbest']
    filt = cost < pop['pbc']
    cbi = int(np.argmin(cost))
    cbv = cost[cbi]
    pop['dx'] = cand - pop['x']
    pop['x'] = cand
    pop['cost'] = cost.copy()
    pop['pb'] = np.where(filt[:, None], cand, pop['pb'])
    pop['pbc'] = np.where(filt, cost, pop['pbc'])
    if cbv < pop['gbest']:
        pop['gbest'], pop['gb'], pop['gbest_idx'], pop['stag'] = cbv, cand[cbi].copy(), cbi, 0
    else:
        pop['stag'] += 1
    pop['cbest'], pop['cb'], pop['cbest_idx'] = cbv, cand[cbi].copy(), cbi
    wi = int(np.argmax(cost))
    if cost[wi] > pop['gworst']:
        pop['gworst'], pop['gw'] = cost[wi], cand[wi].copy()
    pop['fes'] += NP
    pop['gen'] += 1
    pop['sub'] += 1


def _sum(v):
    return np.add.reduce(np.ascontiguousarray(v, dtype=np.float64))          # numpy's pairwise block: the device's np_sum_block (n <= 128)


def _std(v):
    n = len(v)
    d = v - _sum(v) / n
    return np.sqrt(_sum(d * d) / n)


def features(pop, lb, ub, max_fes):
    """feature_encoding (population.py:175-209) with every sum in the kernel's order (include/mbx_layout.h section 22)."""
    x, c = pop['x'], pop['cost']
    NP, D = x.shape
    den = pop['gworst'] - pop['gbest'] + 1e-8
    maxd = np.sqrt((ub - lb) * (ub - lb) * D)
    s = np.zeros((NP, NP))
    for d in range(D):
        t = x[:, None, d] - x[None, :, d]
        s = s + t * t
    s = np.sqrt(s)
    rows = np.array([_sum(s[i]) for i in range(NP)])

    def dist_to(p):
        t = x - p[None, :]
        return np.array([np.sqrt(_sum(t[i] * t[i])) / maxd for i in range(NP)])
    fit = np.where(np.arange(NP) < NP // 2, pop['gworst'], pop['gbest'])
    return np.array([_sum((c - pop['gbest']) / den) / NP,
                     _sum(rows) / (float(NP) * NP) / maxd,
                     _std(c) / (_std(fit) + 1e-8),
                     (float(max_fes) - pop['fes']) / max_fes,
                     float(pop['stag']) / float(max_fes // NP),
                     _sum(dist_to(pop['cb'])) / NP,
                     _sum((c - pop['cbest']) / den) / NP,
                     _sum(dist_to(pop['gb'])) / NP,
                     1. if pop['gbest'] < pop['pre_gbest'] else 0.])


def end_action(pop, max_fes, log_interval, n_logpoint, stop_rule):
    """symbol_optimizer.py:174-197: the log point, the reward, done and the closing entry of the curve.  -> (reward, done)"""
    if pop['fes'] >= pop['log_index'] * log_interval:
        pop['log_index'] += 1
        pop['curve'].append(pop['gbest'])
    reward = (pop['pre_gbest'] - pop['gbest']) / pop['init_cost']
    done = pop['fes'] >= max_fes or (stop_rule and pop['gbest'] <= 1e-8)
    if done:
        if len(pop['curve']) >= n_logpoint + 1:
            pop['curve'][-1] = pop['gbest']
        else:
            pop['curve'].append(pop['gbest'])
    pop['ret'] += reward
    pop['done'] = bool(done)
    pop['sub'] = 0
    return reward, bool(done)


def initial(x0, cost):
    """Population.reset given the initial positions' costs."""
    g, w = int(np.argmin(cost)), int(np.argmax(cost))
    return dict(x=x0.copy(), pb=x0.copy(), dx=np.zeros_like(x0), cost=cost.copy(), pbc=cost.copy(), gb=x0[g].copy(), gw=x0[w].copy(), cb=x0[g].copy(),
                gbest=cost[g], gworst=cost[w], cbest=cost[g], cbest_idx=g, gbest_idx=g, stag=0, fes=float(len(cost)), gen=0, sub=0, pre_gbest=cost[g],
                init_cost=cost[g], log_index=1, curve=[cost[g]], ret=0., done=False)


# ------------------------------------------------------------------------------------------------ the kernel's state block and tape
def offsets(NP, D, nlog):
    o, off = {}, 0
    for name, n in (('x', NP * D), ('pb', NP * D), ('dx', NP * D), ('cost', NP), ('pbc', NP), ('gb', D), ('gw', D), ('cb', D), ('feat', 10), ('sc', NSCALAR),
                    ('curve', nlog + 1), ('idx', SUB_MAX * RANDX_MAX * NP // 8 + 1)):
        o[name] = (off, n)
        off += n
    o['total'] = off
    return o


def unpack(block, NP, D, nlog):
    o = offsets(NP, D, nlog)
    g = lambda k: block[o[k][0]:o[k][0] + o[k][1]].copy()
    sc = g('sc')
    pop = dict(x=g('x').reshape(NP, D), pb=g('pb').reshape(NP, D), dx=g('dx').reshape(NP, D), cost=g('cost'), pbc=g('pbc'), gb=g('gb'), gw=g('gw'), cb=g('cb'),
               feat=g('feat')[:NFEAT], curve=list(g('curve')[:min(int(sc[SC['cost_len']]), nlog + 1)]), done=bool(sc[SC['done']]), episode=int(sc[SC['episode']]))
    for k in ('gbest', 'gworst', 'cbest', 'pre_gbest', 'init_cost', 'fes', 'ret'):
        pop[k] = sc[SC[k]]
    for k in ('cbest_idx', 'gbest_idx', 'stag', 'gen', 'sub', 'log_index', 'cost_len'):
        pop[k] = int(sc[SC[k]])
    pop['idx'] = np.ascontiguousarray(block[o['idx'][0]:o['idx'][0] + SUB_MAX * RANDX_MAX * NP // 8]).view(np.uint8).reshape(SUB_MAX, RANDX_MAX, NP).copy()
    return pop


def pack(pop, NP, D, nlog, block):
    """Write `pop` over a state block read from the kernel (the episode counter and the index bytes are kept)."""
    o = offsets(NP, D, nlog)
    out = np.array(block, dtype=np.float64)
    for k in ('x', 'pb', 'dx', 'cost', 'pbc', 'gb', 'gw', 'cb'):
        out[o[k][0]:o[k][0] + o[k][1]] = np.asarray(pop[k], dtype=np.float64).ravel()
    sc = out[o['sc'][0]:o['sc'][0] + NSCALAR]
    for k in ('gbest', 'gworst', 'cbest', 'pre_gbest', 'init_cost', 'fes', 'ret', 'cbest_idx', 'gbest_idx', 'stag', 'gen', 'sub', 'log_index'):
        sc[SC[k]] = float(pop[k])
    sc[SC['cost_len']] = len(pop['curve'])
    sc[SC['done']] = float(pop['done'])
    n = min(len(pop['curve']), nlog + 1)
    out[o['curve'][0]:o['curve'][0] + n] = pop['curve'][:n]
    if 'feat' in pop:
        out[o['feat'][0]:o['feat'][0] + NFEAT] = pop['feat']
    return out


def tape_stride(NP, D):
    return NP * D + 3 * NP + SUB_MAX * (RANDX_MAX + 3) * NP


def make_tape(NP, D, pos_u=None, noise_init=None, subs=()):
    """subs: per sub-step (idx [k, NP] or None, noise [3, NP] or None)."""
    t = np.zeros(tape_stride(NP, D))
    if pos_u is not None:
        t[:NP * D] = np.asarray(pos_u).ravel()
    if noise_init is not None:
        t[NP * D:NP * D + 3 * NP] = np.asarray(noise_init).ravel()
    for s, (idx, noise) in enumerate(subs):
        base = NP * D + 3 * NP + s * (RANDX_MAX + 3) * NP
        if idx is not None and len(idx):
            idx = np.asarray(idx, dtype=np.float64)
            t[base:base + idx.size] = idx.ravel()
        if noise is not None:
            t[base + RANDX_MAX * NP:base + (RANDX_MAX + 3) * NP] = np.asarray(noise).ravel()
    return t
