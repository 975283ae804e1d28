"""GL-PSO (src/optimizer/gl_pso.py:22-66, 76-177) restated on the state block of include/mbx_layout.h §11, and the judge of one launch.  Not a test module.

The restatement takes NP and D at run time and follows numpy's expression order, so positions, velocities and candidate exemplars are BIT FOR BIT what the
reference computes from the same draws (the kernels are built with -ffp-contract=off):

    uniform(a, b)        a + (b - a) u
    velocity             w V + (c1 r) (ex - x); np.clip to +-vmax, vmax = 0.2 (ub - lb)
    position             x + v; v *= -0.5 where x + v > ub, then where x + v < lb (two np.where, in this order); np.clip to [lb, ub]
    crossover            pbest_position[k, d] where pbest[k] < pbest[i], else r pb + (1 - r) gb
    mutation             lb + (ub - lb) mu where mt < 0.01

No bit-level exception had to be stated: fmin(fmax(v, lo), hi) and np.clip agree on every finite input, signed zeros included (lo < 0 < hi for the velocity, and
the position bounds are not zero).  One equivalence is worth a line: a position cannot lie beyond both bounds, so the two `where` bounces never both fire and folding
them into one `where(a | b)` is the same function (DEFECTS['bounce_merged'] below is kept to show that, and 'bounce_after_clip' is the merge that does go wrong).

Costs are NOT restated: `judge` takes them from the block after the launch and holds them against the extended-precision evaluators (bbob_exact / protein_exact):
a stored cost must lie within the allowance of the exact cost of the restated row, a decision (`<`) is *decided* when exact +- allowance lies on one side of
the other operand and *undecided* (counted, never excused silently) otherwise.  Everything downstream of the costs -- gbest, the tournament, the counters, the
curve -- is exact on the kernel's own numbers.

The stand-in "kernel" of the CPU tests is the restatement itself with float64 costs; every entry of DEFECTS is one deliberate slip in it.

The curve: the reference appends at a log point without looking at the list's length (:160-162), only the closing entry does (:172-176); the restatement follows
that, with the library's rule that a write past slot n_logpoint is dropped while the length goes on counting (include/mbx.h).  The kernel guards the append
instead; the two differ only for budgets with log_interval (n_logpoint + 1) <= max_fes, which no test here uses (docs/EXPERIMENTS.md)."""
import numpy as np

import bbob_exact as be
import protein_exact as pe
from oracle import oracle

W, C1, PM, RHO, SG, NSEL = 0.7298, 1.49618, 0.01, 0.2, 7, 10
NSC = 16
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE, SC_GBEST_IDX = range(9)

# name -> what the slip is.  tests/test_glpso_exact.py shows that `judge` rejects each on the planted states (and names the state).
DEFECTS = {
    'pb_le': 'pbest improves on <=', 'gb_le': 'gbest improves on <=', 'sel_le': 'exemplar selection wins on <=',
    'stag_ge': 'tournament fires at stag >= 7', 'tour_last': 'tournament takes the last of equal costs',
    'tour_live': 'tournament gathers rows already replaced in the same launch', 'tour_cost': 'tournament copies the winner\'s exemplar_cost',
    'tour_zero': 'tournament zeroes the counter', 'reset_zero_stag': 'reset zeroes the counters', 'reset_lt': 'reset selects with <',
    'cross_current': 'crossover reads current_position for pbest_position', 'cross_reversed': 'crossover filter reversed',
    'cross_le': 'crossover filter on <=', 'mut_le': 'mutation on mt <= 0.01', 'bounce_after_clip': 'the bounces folded into the clip: tested on the clipped position',
    'bounce_ge': 'bounce on >= ub / <= lb', 'log_2np': 'log test at fes + 2 NP', 'gb_excost': 'gbest fed by exemplar costs',
    'gb_last': 'gbest argmin takes the last of equal costs', 'row_last': 'row index e / D one short at the last element',
}
EQUIVALENT = {'bounce_merged': 'the two bounces in one where(a | b): the same function, a position is never beyond both bounds'}


# ------------------------------------------------------------------------------------------------ layout
def tape_stride(NP, D):
    return 6 * NP * D + 6 * NP + NSEL * NP


def state_doubles(NP, D, nlog):
    return 4 * NP * D + 3 * NP + D + NSC + nlog + 1


def split_state(st, D, nlog=50, NP=100):
    """Views into one state block (writing through them writes the block)."""
    NE = NP * D
    o = 4 * NE + 3 * NP + D
    return {'X': st[:NE], 'V': st[NE:2 * NE], 'pbpos': st[2 * NE:3 * NE], 'pbest': st[3 * NE:3 * NE + NP],
            'exemplar': st[3 * NE + NP:4 * NE + NP], 'excost': st[4 * NE + NP:4 * NE + 2 * NP], 'stag': st[4 * NE + 2 * NP:4 * NE + 3 * NP],
            'gbpos': st[4 * NE + 3 * NP:o], 'scalars': st[o:o + NSC], 'cost': st[o + NSC:o + NSC + 1 + nlog]}


def split_tape(tape, NP, D, reset):
    """-> dict of the draws of one launch: pos / vel (reset) or rand (generation), noise [3, NP], and the exemplar block cidx, cu, mu, mt, xnoise [3, NP],
    tour [NP, NSEL]."""
    NE = NP * D
    t = np.asarray(tape, dtype=np.float64)
    out, o = {}, 0
    for name in (('pos', 'vel') if reset else ('rand',)):
        out[name] = t[o:o + NE].reshape(NP, D); o += NE
    out['noise'] = t[o:o + 3 * NP].reshape(3, NP); o += 3 * NP
    for name in ('cidx', 'cu', 'mu', 'mt'):
        out[name] = t[o:o + NE].reshape(NP, D); o += NE
    out['xnoise'] = t[o:o + 3 * NP].reshape(3, NP); o += 3 * NP
    out['tour'] = t[o:o + NP * NSEL].reshape(NP, NSEL)
    return out


def noise_rows(rs, NP, kind):
    """The three noise rows of one evaluation for noise model `kind`, drawn as the reference draws them."""
    rows = np.zeros((3, NP))
    if kind == 1:
        rows[0] = rs.randn(NP)
    elif kind == 2:
        rows[0], rows[1] = rs.rand(NP), rs.rand(NP)
    elif kind == 3:
        rows[0], rows[1], rows[2] = rs.rand(NP), rs.randn(NP), rs.randn(NP)
    return rows.ravel()


def random_tape(rs, NP, D, kind, reset):
    """A full tape of one launch from `rs`: uniforms, indices in range, noise rows of the instance's kind, tournament indices."""
    NE = NP * D
    head = [rs.rand(NE), rs.rand(NE)] if reset else [rs.rand(NE)]
    parts = head + [noise_rows(rs, NP, kind), rs.randint(0, NP, NE).astype(np.float64), rs.rand(NE), rs.rand(NE), rs.rand(NE), noise_rows(rs, NP, kind),
                    rs.randint(0, NP, NP * NSEL).astype(np.float64)]
    out = np.zeros(tape_stride(NP, D))
    t = np.concatenate(parts)
    out[:len(t)] = t
    return out


class Cfg:
    """One instance's problem and budget.  protein: the docking instance (no optimum, no noise, costs from the oracle's energy)."""

    def __init__(self, problem, NP, max_fes, log_interval, n_logpoint, early_stop=True, protein=False):
        self.problem, self.NP, self.D = problem, int(NP), int(problem.dim)
        self.max_fes, self.log_interval, self.n_logpoint, self.early_stop = int(max_fes), int(log_interval), int(n_logpoint), bool(early_stop)
        self.protein = protein
        self.lb, self.ub = float(problem.lb), float(problem.ub)
        self.noise_kind = 0 if protein else int(problem.noise[0])
        self.has_optimum = not protein

    def with_problem(self, problem, protein=False):
        return Cfg(problem, self.NP, self.max_fes, self.log_interval, self.n_logpoint, self.early_stop, protein)


def reference_costs(cfg):
    """The reference's float64 objective (oracle.evaluate / apply_noise, pinned to the reference by tests/test_oracle_bbob.py) minus the optimum."""
    p = cfg.problem

    def costs(X, rows):
        f = oracle.evaluate(p.desc(), X)
        if cfg.protein:
            return f
        if cfg.noise_kind:
            f = oracle.apply_noise(p.desc(), p.bias, f, rows)
        return f - p.bias
    return costs


def float64_costs(cfg):
    """The stand-in kernel's costs: bbob_exact.float64_eval (the oracle's energy for the docking instance)."""
    p = cfg.problem

    def costs(X, rows):
        if cfg.protein:
            return oracle.evaluate(p.desc(), X)
        return np.asarray(be.float64_eval(p, X, rows if cfg.noise_kind else None), dtype=np.float64)
    return costs


def allowance(cfg, X, rows):
    """-> (allow [m], n_ambiguous [m], exact [m] longdouble) of the rows of X with the tape's noise rows."""
    if cfg.protein:
        return pe.allowance(cfg.problem, X, with_energy=True)
    return be.allowance(cfg.problem, X, rows if cfg.noise_kind else None)


# ------------------------------------------------------------------------------------------------ the pieces (shared by the restatement and the judge)
def _idx(a, NP):
    """(int) of a tape double, clamped: a tape is caller data."""
    return np.clip(np.trunc(a), 0, NP - 1).astype(np.int64)


def _rows_of(NP, D, defect):
    """Row of every element; DEFECTS['row_last'] is a division that is one short at the last element."""
    r = np.repeat(np.arange(NP), D).reshape(NP, D)
    if defect == 'row_last':
        r[-1, -1] = NP - 2
    return r


def _by_row(flag, NP, D, defect):
    return np.asarray(flag)[_rows_of(NP, D, defect)]


def move(X, V, EX, r, cfg, defect=None):
    """:121-129 -> (new position, new velocity, events)."""
    lb, ub = cfg.lb, cfg.ub
    vmax = RHO * (ub - lb)
    raw = W * V + C1 * r * (EX - X)
    v = np.clip(raw, -vmax, vmax)
    nx = X + v
    if defect == 'bounce_after_clip':
        t = np.clip(nx, lb, ub)
        hi, lo = t > ub, t < lb
    elif defect == 'bounce_ge':
        hi, lo = nx >= ub, nx <= lb
    else:
        hi, lo = nx > ub, nx < lb
    if defect == 'bounce_merged':
        v = np.where(hi | lo, v * -0.5, v)
    else:
        v = np.where(hi, v * -0.5, v)
        v = np.where(lo, v * -0.5, v)
    ev = {'bounce_ub': bool(hi.any()), 'bounce_lb': bool(lo.any()), 'vclamp': bool((np.abs(raw) > vmax).any())}
    return np.clip(nx, lb, ub), v, ev


def candidates(pbest, pbpos, gbpos, t, cfg, defect=None, X=None):
    """:22-34 on the values AFTER the pbest / gbest update -> (new exemplars [NP, D], mutated mask)."""
    NP, D = cfg.NP, cfg.D
    k = _idx(t['cidx'], NP)
    src = X if defect == 'cross_current' else pbpos
    mine = pbest[_rows_of(NP, D, defect)]
    filt = pbest[k] > mine if defect == 'cross_reversed' else pbest[k] <= mine if defect == 'cross_le' else pbest[k] < mine
    r = t['cu']
    uni = r * src + (1 - r) * gbpos[None, :]
    ne = np.where(filt, src[k, np.arange(D)[None, :]], uni)
    mut = t['mt'] <= PM if defect == 'mut_le' else t['mt'] < PM
    return np.where(mut, cfg.lb + (cfg.ub - cfg.lb) * t['mu'], ne), mut


def tournament(post, excost, stag, tour, cfg, defect=None):
    """:49-57, 64-66 on the exemplars after selection -> (exemplars, rows that fired, their chosen rows)."""
    NP = cfg.NP
    fired = np.nonzero(stag >= SG if defect == 'stag_ge' else stag > SG)[0]
    final, chosen = post.copy(), []
    for i in fired:
        idx = _idx(tour[i], NP)
        c = excost[idx]
        j = len(c) - 1 - int(np.argmin(c[::-1])) if defect == 'tour_last' else int(np.argmin(c))
        chosen.append(int(idx[j]))
        final[i] = (final if defect == 'tour_live' else post)[idx[j]]
    return final, fired, np.array(chosen, dtype=np.int64)


def bookkeep(sc, curve, gbest, cfg, defect=None):
    """:160-162 with fes after the FIRST evaluation, :168-176 after both.  Writes the scalars and the curve in place."""
    NP, nlog = cfg.NP, cfg.n_logpoint
    fes1 = sc[SC_FES] + NP
    fes = fes1 + NP
    log_index, cost_len = int(sc[SC_LOG_INDEX]), int(sc[SC_COST_LEN])

    def put(i, v):
        if i <= nlog:
            curve[i] = v
    if (fes if defect == 'log_2np' else fes1) >= log_index * cfg.log_interval:
        log_index += 1
        put(cost_len, gbest); cost_len += 1
    done = fes >= cfg.max_fes
    if cfg.has_optimum and cfg.early_stop:
        done = done or gbest <= 1e-8
    if done:
        if cost_len >= nlog + 1:
            put(cost_len - 1, gbest)
        else:
            put(cost_len, gbest); cost_len += 1
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = gbest, fes, log_index, cost_len, 1. if done else 0.
    sc[SC_GEN] += 1


def _argmin(c, last=False):
    return len(c) - 1 - int(np.argmin(c[::-1])) if last else int(np.argmin(c))


def _exemplar_update(s, t, cfg, costs, init, defect, X):
    """__exemplar_update (:59-66) on the split block `s`, in place."""
    NP, D = cfg.NP, cfg.D
    cand, _ = candidates(s['pbest'].copy(), s['pbpos'].reshape(NP, D).copy(), s['gbpos'].copy(), t, cfg, defect, X)
    c = costs(cand, t['xnoise'])
    if init and defect != 'reset_lt':
        win = np.ones(NP, dtype=bool)
    else:
        win = c <= s['excost'] if defect == 'sel_le' else c < s['excost']
    if not init:
        s['stag'][:] = np.where(win, 0., s['stag'] + 1)
    elif defect == 'reset_zero_stag':
        s['stag'][:] = 0.
    s['excost'][:] = np.where(win, c, s['excost'])
    post = np.where(_by_row(win, NP, D, defect), cand, s['exemplar'].reshape(NP, D))
    final, fired, chosen = tournament(post, s['excost'].copy(), s['stag'].copy(), t['tour'], cfg, defect)
    if defect == 'tour_cost':
        s['excost'][fired] = s['excost'].copy()[chosen]
    if defect == 'tour_zero':
        s['stag'][fired] = 0.
    s['exemplar'][:] = final.ravel()


def restate_reset(block_before, tape, cfg, costs=None, defect=None):
    """init_population (:76-107) -> the block after mbx_reset."""
    costs = costs or float64_costs(cfg)
    NP, D = cfg.NP, cfg.D
    b = np.array(block_before, dtype=np.float64)
    s = split_state(b, D, cfg.n_logpoint, NP)
    t = split_tape(tape, NP, D, True)
    lb, ub = cfg.lb, cfg.ub
    vmax = RHO * (ub - lb)
    X = lb + (ub - lb) * t['pos']
    s['X'][:] = X.ravel(); s['pbpos'][:] = X.ravel()
    s['V'][:] = (-vmax + (vmax - (-vmax)) * t['vel']).ravel()
    c = costs(X, t['noise'])
    g0 = _argmin(c, defect == 'gb_last')
    s['pbest'][:] = c
    s['gbpos'][:] = X[g0]
    _exemplar_update(s, t, cfg, costs, True, defect, X)
    gb = c[g0]
    if defect == 'gb_excost':
        gb = min(gb, s['excost'].min())
    episode = s['scalars'][SC_EPISODE] + 1
    s['scalars'][:] = 0.
    sc = s['scalars']
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_EPISODE], sc[SC_GBEST_IDX] = gb, 2 * NP, 1, 1, episode, g0
    s['cost'][0] = gb
    return b


def restate_generation(block_before, tape, cfg, costs=None, defect=None):
    """__update (:118-177) -> the block after mbx_step.  A finished instance is left alone."""
    costs = costs or float64_costs(cfg)
    NP, D = cfg.NP, cfg.D
    b = np.array(block_before, dtype=np.float64)
    s = split_state(b, D, cfg.n_logpoint, NP)
    if s['scalars'][SC_DONE] != 0.:
        return b
    t = split_tape(tape, NP, D, False)
    X, V, _ = move(s['X'].reshape(NP, D), s['V'].reshape(NP, D), s['exemplar'].reshape(NP, D), t['rand'], cfg, defect)
    s['X'][:] = X.ravel(); s['V'][:] = V.ravel()
    c = costs(X, t['noise'])
    impr = c <= s['pbest'] if defect == 'pb_le' else c < s['pbest']
    s['pbest'][:] = np.where(impr, c, s['pbest'])
    s['pbpos'][:] = np.where(_by_row(impr, NP, D, defect), X, s['pbpos'].reshape(NP, D)).ravel()
    cb = _argmin(c, defect == 'gb_last')
    gbest = s['scalars'][SC_GBEST]
    if c[cb] <= gbest if defect == 'gb_le' else c[cb] < gbest:
        gbest = c[cb]
        s['gbpos'][:] = X[cb]
        s['scalars'][SC_GBEST_IDX] = cb
    _exemplar_update(s, t, cfg, costs, False, defect, X)
    if defect == 'gb_excost':
        gbest = min(gbest, s['excost'].min())
    bookkeep(s['scalars'], s['cost'], gbest, cfg, defect)
    return b


def outputs(block_after, cfg):
    """(state_out, reward_out, done_out) of the launch that left `block_after` (state_out is fes / max_fes; a frozen instance's is not rewritten)."""
    sc = split_state(block_after, cfg.D, cfg.n_logpoint, cfg.NP)['scalars']
    return sc[SC_FES] / cfg.max_fes, 0., int(sc[SC_DONE] != 0.)


# ------------------------------------------------------------------------------------------------ the judge
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class Rejected(AssertionError):
    pass


def _need(ok, *what):
    if not ok:
        raise Rejected(what)


class Report(dict):
    """decisions / undecided (list of (kind, row)) / self_ties (an undecided candidate that is the row's exemplar, its pbest_position or gbest_position to 4 ulp: see _judge_exemplars) / worst cost error over allowance / ambiguous rows / events seen."""

    def __init__(self):
        super().__init__(decisions=0, undecided=[], self_ties=0, worst=0., ambiguous=0, events=set())

    def merge(self, o):
        self['decisions'] += o['decisions']; self['undecided'] += o['undecided']; self['ambiguous'] += o['ambiguous']; self['self_ties'] += o['self_ties']
        self['worst'] = max(self['worst'], o['worst']); self['events'] |= o['events']
        return self


def _cost_check(rep, kind, got, rows, allow, exact):
    """Stored costs `got[rows]` against exact +- allow."""
    if len(rows) == 0:
        return
    err = np.abs(np.asarray(got[rows], dtype=be.LD) - exact[rows]).astype(np.float64)
    ratio = err / allow[rows]
    bad = ~(ratio <= 1.)
    _need(not bad.any(), kind, 'cost outside the allowance', [(int(rows[j]), float(got[rows[j]]), float(exact[rows[j]]), float(allow[rows[j]])) for j in np.nonzero(bad)[0][:4]])
    rep['worst'] = max(rep['worst'], float(ratio.max()))


def _decisions(rep, kind, took, other, allow, exact, known):
    """`took[i]`: the kernel decided cost_i < other_i.  Must be so when exact + allow < other, must not when exact - allow >= other; `known` rows
    ({row: decision}) are planted exact ties whose outcome follows from the evaluator being a function of the row."""
    lo = (exact - allow.astype(be.LD)).astype(np.float64)
    hi = (exact + allow.astype(be.LD)).astype(np.float64)
    hi = np.where(hi.astype(be.LD) < exact + allow.astype(be.LD), np.nextafter(hi, np.inf), hi)       # rounded outwards
    lo = np.where(lo.astype(be.LD) > exact - allow.astype(be.LD), np.nextafter(lo, -np.inf), lo)
    must, mustnt = hi < other, lo >= other
    for i in range(len(took)):
        rep['decisions'] += 1
        if i in known:
            _need(bool(took[i]) == bool(known[i]), kind, 'planted tie decided the wrong way', i)
        elif must[i]:
            _need(took[i], kind, 'decided improvement not taken', i, float(exact[i]), float(allow[i]), float(other[i]))
        elif mustnt[i]:
            _need(not took[i], kind, 'decided loss taken', i, float(exact[i]), float(allow[i]), float(other[i]))
        else:
            rep['undecided'].append((kind, i))


def _judge_exemplars(rep, b0, b1, t, cfg, init, known):
    NP, D = cfg.NP, cfg.D
    cand, mut = candidates(b1['pbest'], b1['pbpos'].reshape(NP, D), b1['gbpos'], t, cfg)
    if mut.any():
        rep['events'].add('mutation')
    allow, amb, exact = allowance(cfg, cand, t['xnoise'])
    rep['ambiguous'] += int((amb > 0).sum())
    ex0, ex1 = b0['exemplar'].reshape(NP, D), b1['exemplar'].reshape(NP, D)
    if init:
        won = np.ones(NP, dtype=bool)
        _need(same(b1['stag'], b0['stag']), 'reset', 'the counters moved', np.flatnonzero(b1['stag'] != b0['stag'])[:4])
    else:
        won = b1['stag'] == 0.
        lost = b1['stag'] == b0['stag'] + 1
        _need(bool(np.all(won | lost)), 'selection', 'a counter is neither 0 nor +1', np.flatnonzero(~(won | lost))[:4])
        w = np.nonzero(won)[0]
        _need(bool(np.all(b1['excost'][w] < b0['excost'][w])), 'selection', 'a win that is not strictly lower (or a counter zeroed without one)',
              w[~(b1['excost'][w] < b0['excost'][w])][:4])
        lz = np.nonzero(~won)[0]
        _need(same(b1['excost'][lz], b0['excost'][lz]), 'selection', 'exemplar_cost of a losing row moved', lz[_bits(b1['excost'][lz]) != _bits(b0['excost'][lz])][:4])
        n0 = len(rep['undecided'])
        _decisions(rep, 'selection', won, b0['excost'], allow, exact, known.get('sel', {}))
        # a candidate that IS a point this row has bred before, up to the roundings of r x + (1 - r) x: the holder of gbest breeds its own pbest_position
        # every generation, and in a small swarm whole candidates are copies of gbest_position.  Its exemplar_cost is then the cost of (nearly) the same
        # point -- also after a tournament has replaced the exemplar itself, which keeps the cost -- and the selection compares two evaluations of one point, a
        # few ulp of cost apart, which no evaluator model decides.  Such rows, when undecided, are counted apart (Report['self_ties']); nothing else is excused.
        def at(P):
            return (np.abs(cand - P) <= 4 * np.spacing(np.abs(P))).all(axis=1)
        near = at(ex0) | at(b1['pbpos'].reshape(NP, D)) | at(np.broadcast_to(b1['gbpos'], (NP, D)))
        mine = [u for u in rep['undecided'][n0:] if near[u[1]]]
        rep['undecided'][n0:] = [u for u in rep['undecided'][n0:] if not near[u[1]]]
        rep['self_ties'] += len(mine)
    _cost_check(rep, 'exemplar_cost', b1['excost'], np.nonzero(won)[0], allow, exact)
    post = np.where(won[:, None], cand, ex0)
    final, fired, chosen = tournament(post, b1['excost'], b1['stag'], t['tour'], cfg)
    if len(fired):
        rep['events'].add('tournament')
    bad = np.nonzero((_bits(final) != _bits(ex1)).any(axis=1))[0]
    _need(bad.size == 0, 'exemplar', 'rows differ from selection + tournament on the kernel\'s own costs', bad[:6], 'fired', fired[:8], 'chosen', chosen[:8])


def _judge_scalars(b0, b1, cfg, reset):
    sc0, sc1 = b0['scalars'], b1['scalars']
    want, curve = sc0.copy(), b0['cost'].copy()
    if reset:
        want[:] = 0.
        want[SC_FES], want[SC_LOG_INDEX], want[SC_COST_LEN], want[SC_EPISODE] = 2 * cfg.NP, 1, 1, sc0[SC_EPISODE] + 1
        want[SC_GBEST], want[SC_GBEST_IDX] = sc1[SC_GBEST], sc1[SC_GBEST_IDX]            # (judged by the caller)
        curve[0] = sc1[SC_GBEST]
    else:
        want[SC_GBEST_IDX] = sc1[SC_GBEST_IDX]
        bookkeep(want, curve, sc1[SC_GBEST], cfg)
    names = ('gbest', 'fes', 'log_index', 'cost_len', 'done', 'return', 'gen', 'episode', 'gbest_idx')
    bad = np.nonzero(_bits(want) != _bits(sc1))[0]
    _need(bad.size == 0, 'scalars', [(names[k] if k < len(names) else int(k), float(sc1[k]), float(want[k])) for k in bad])
    n = min(int(want[SC_COST_LEN]), cfg.n_logpoint + 1)              # the slots past the list are reported padded with its last value (mbx_debug_read_state)
    _need(same(curve[:n], b1['cost'][:n]), 'curve', b1['cost'].tolist(), curve.tolist())


def _judge_outs(outs, b1, cfg, frozen=False):
    if outs is None:
        return
    st, rw, dn = outs
    want = outputs(b1, cfg)
    _need(rw == 0. and int(dn) == want[2], 'outputs', 'reward / done', float(rw), int(dn), want)
    if not frozen:
        _need(st == want[0], 'outputs', 'state', float(st), want[0])


def judge(block_before, tape, block_after, cfg, reset=False, outs=None, known=None):
    """One launch of the kernel (or of a stand-in): `block_after` must follow from `block_before` and `tape`.  Raises Rejected; -> Report.
    outs: (state_out, reward_out, done_out) of the instance, when the caller has them.  known: {'pbest': {row: bool}, 'sel': {row: bool}}, the planted exact ties."""
    known = known or {}
    NP, D = cfg.NP, cfg.D
    n = state_doubles(NP, D, cfg.n_logpoint)
    blk0, blk1 = np.array(block_before, dtype=np.float64), np.array(block_after, dtype=np.float64)
    _need(same(blk0[n:], blk1[n:]), 'padding', 'words past the block moved')
    b0, b1 = split_state(blk0, D, cfg.n_logpoint, NP), split_state(blk1, D, cfg.n_logpoint, NP)
    rep = Report()
    if not reset and b0['scalars'][SC_DONE] != 0.:
        _need(same(blk0, blk1), 'frozen', 'a finished instance moved', np.flatnonzero(_bits(blk0) != _bits(blk1))[:8])
        _judge_outs(outs, blk1, cfg, frozen=True)
        rep['events'].add('frozen')
        return rep
    t = split_tape(tape, NP, D, reset)
    lb, ub = cfg.lb, cfg.ub
    X1, V1 = b1['X'].reshape(NP, D), b1['V'].reshape(NP, D)
    if reset:
        vmax = RHO * (ub - lb)
        X, V = lb + (ub - lb) * t['pos'], -vmax + (vmax - (-vmax)) * t['vel']
    else:
        X, V, ev = move(b0['X'].reshape(NP, D), b0['V'].reshape(NP, D), b0['exemplar'].reshape(NP, D), t['rand'], cfg)
        rep['events'] |= {k for k, v in ev.items() if v}
    _need(same(X, X1), 'X', 'positions differ from the restatement', np.argwhere(_bits(X) != _bits(X1))[:4].tolist())
    _need(same(V, V1), 'V', 'velocities differ from the restatement', np.argwhere(_bits(V) != _bits(V1))[:4].tolist())
    allow, amb, exact = allowance(cfg, X, t['noise'])
    rep['ambiguous'] += int((amb > 0).sum())
    pb0, pb1 = b0['pbest'], b1['pbest']
    pp0, pp1 = b0['pbpos'].reshape(NP, D), b1['pbpos'].reshape(NP, D)
    sc0, sc1 = b0['scalars'], b1['scalars']
    if reset:
        impr = np.ones(NP, dtype=bool)
        gb0 = np.inf
    else:
        impr = _bits(pb1) != _bits(pb0)
        _need(bool(np.all(pb1[impr] < pb0[impr])), 'pbest', 'moved without a strict improvement', np.flatnonzero(impr)[~(pb1[impr] < pb0[impr])][:4])
        _decisions(rep, 'pbest', impr, pb0, allow, exact, known.get('pbest', {}))
        gb0 = sc0[SC_GBEST]
        _need(bool(np.all(pb0 >= gb0)), 'precondition', 'a pbest below gbest in the block before: the gbest rule below needs pbest >= gbest')
    rows = np.nonzero(impr)[0]
    _cost_check(rep, 'pbest', pb1, rows, allow, exact)
    _need(same(pp1[impr], X[impr]), 'pbest_position', 'an improved row is not the new position', rows[(_bits(pp1[impr]) != _bits(X[impr])).any(axis=1)][:4])
    _need(same(pp1[~impr], pp0[~impr]), 'pbest_position', 'an unimproved row moved', np.flatnonzero(~impr)[(_bits(pp1[~impr]) != _bits(pp0[~impr])).any(axis=1)][:4])
    # gbest: exact on the kernel's own numbers (an unimproved particle's cost is >= its pbest >= gbest)
    m = pb1[rows].min() if len(rows) else np.inf
    if m < gb0:
        g = int(rows[int(np.argmin(pb1[rows]))])
        _need(_bits(sc1[SC_GBEST]) == _bits(m) and sc1[SC_GBEST_IDX] == g, 'gbest', 'not the first minimum of the improved costs', float(sc1[SC_GBEST]), float(m),
              float(sc1[SC_GBEST_IDX]), g)
        _need(same(b1['gbpos'], X[g]), 'gbest_position', 'not the row of the first minimum', g)
        if not reset and not same(b0['gbpos'], X[g]):
            rep['events'].add('gbest_moved')
    else:
        _need(_bits(sc1[SC_GBEST]) == _bits(gb0) and sc1[SC_GBEST_IDX] == sc0[SC_GBEST_IDX] and same(b1['gbpos'], b0['gbpos']), 'gbest', 'moved without an improvement',
              float(sc1[SC_GBEST]), float(gb0), float(sc1[SC_GBEST_IDX]), float(sc0[SC_GBEST_IDX]))
    _judge_exemplars(rep, b0, b1, t, cfg, reset, known)
    _judge_scalars(b0, b1, cfg, reset)
    _judge_outs(outs, blk1, cfg)
    return rep
